"""The cases of test_reward_reference_gpu.py (reward_fixture.py), checked without a device: the conditions the generator must
satisfy, K2's tile table, and that the bounds the kernels are held to tell wrong answers apart -- every mutant of the
oracle's inputs moves the reward or a c_info term by at least 100 x the bound, in both dtypes."""
import numpy as np
import pytest

import reward_fixture as RF
import tree_fixture as F
from oracle import humanoid as H
from oracle import reward as R

TILE_TABLE = {5: (16, 16, 64), 9: (8, 16, 64), 14: (4, 16, 64), 21: (3, 12, 60)}       # nbody -> envs per wave, one-pass, five-pass tile
EPS = np.finfo(float).eps


def test_tile_table_and_sizes():
    """A change of K2's layout (reward_envs_per_wave, reward_tile_envs, the threshold between the two forms) has to be restated in
    reward_fixture.py and here, or the sizes of the GPU comparison would miss a tile's edges unseen."""
    assert {len(F.skeleton(t).body_names) for t in F.TREES} == set(TILE_TABLE)
    for nb, (epw, one, five) in TILE_TABLE.items():
        assert (RF.envs_per_wave(nb), RF.tile_envs(nb, 1), RF.tile_envs(nb, 5)) == (epw, one, five)
        assert RF.k2_sizes(nb) == (1, one - 1, one, one + 1, 3 * one + 5)
        assert 4 * epw >= one and 20 * epw >= five                 # every env of a tile is covered by a pass that runs
    assert 4 * RF.envs_per_wave(5) > RF.tile_envs(5, 1) and 4 * RF.envs_per_wave(9) > RF.tile_envs(9, 1)      # the cap bites: waves skip
    assert 16 * RF.envs_per_wave(14) == RF.tile_envs(14, 5)       # chain33: the fifth pass is skipped whole
    assert RF.FIVE_PASS_N >= RF.FIVE_PASS_FROM and max(RF.k2_sizes(5)) < RF.FIVE_PASS_FROM
    assert RF.TAKE_OFF == tuple(np.concatenate([[0], np.cumsum(RF.TAKE_LENS)]))
    assert set(RF.BOUNDARY_FRAMES) == {o for o in RF.TAKE_OFF[:-1]} | {o - 1 for o in RF.TAKE_OFF[1:]}


def _all_cases(tree, coord):
    cs = [c for _, c in RF.k2_cases(tree, coord)] + RF.k7_cases(tree, coord)
    if coord == "heading" and tree in RF.FIVE_PASS_TREES:
        cs += [c for _, c in RF.five_pass_cases(tree)]
    if (tree, coord) == (RF.POSE_DIST_TREE, "heading"):
        cs.append(RF.pose_dist_case())
    return cs


@pytest.mark.parametrize("tree,coord", RF.TREE_COORDS)
def test_generator_conditions(tree, coord):
    """Every case the GPU module uses (one-pass, five-pass, K7, pose_dist) meets the generator's conditions one by one, but for
    "not saturated": that one is asserted per weight set on the ordinary rows pooled over the five one-pass sizes (n = 1 cannot
    meet it alone), and on each five-pass case by itself."""
    sk, bw = F.skeleton(tree), RF.gains(tree)["b_diffw"]
    nb = len(sk.body_names)
    assert len(set(bw.tolist())) == nb - 1 and 0.3 <= bw.min() and bw.max() <= 2.0 and sk.body_ndof[RF.neg_body(tree)] > 0
    tb = RF.table(tree)
    assert [len(t["qpos"]) for t in RF.takes(tree)] == list(RF.TAKE_LENS) and len(tb["qpos"]) == RF.N_FRAMES
    # unit quaternions, a defined heading: the expert's
    np.testing.assert_allclose(np.linalg.norm(tb["qpos"][:, 3:7], axis=1), 1.0, rtol=0, atol=4 * EPS)
    np.testing.assert_allclose(np.linalg.norm(tb["rq_rmh"], axis=1), 1.0, rtol=0, atol=8 * EPS)
    np.testing.assert_allclose(np.linalg.norm(tb["bquat"].reshape(RF.N_FRAMES, nb, 4), axis=2), 1.0, rtol=0, atol=8 * EPS)
    assert (tb["qpos"][:, 3] ** 2 + tb["qpos"][:, 6] ** 2).min() >= 0.05
    sign = np.ones((RF.N_FRAMES, nb, 1))
    sign[RF.NEG_FRAME, RF.neg_body(tree)] = -1.0
    assert (tb["bquat"] == (sign * H.body_quat(tb["qpos"], sk.body_qpos_start, sk.body_ndof).reshape(RF.N_FRAMES, nb, 4)).reshape(RF.N_FRAMES, -1)).all()
    seen_kinds = set()
    for c in _all_cases(tree, coord):
        n, kind, on = c["n"], c["kind"], c["active"] != 0
        why = "%s n=%d %s" % (tree, n, c["weights"])
        seen_kinds |= set(kind.tolist())
        # inputs: finite where active, NaN where not, frames in range, inactive rows on another valid frame
        assert np.isfinite(c["cur_qpos"][on]).all() and np.isnan(c["cur_qpos"][~on]).all() and np.isfinite(c["prev_qpos"]).all()
        assert (kind[~on] == RF.INACTIVE).all() and (kind[on] != RF.INACTIVE).all()
        assert c["frame"].min() >= 0 and c["frame"].max() < RF.N_FRAMES and c["t"].min() >= 1 and c["t"].max() <= RF.EPISODE_LEN
        assert (c["frame"][kind == RF.EXPERT_NEG] == RF.NEG_FRAME).all() and (c["frame"][kind != RF.EXPERT_NEG] != RF.NEG_FRAME).all()
        if (kind == RF.ORDINARY).sum() >= len(RF.BOUNDARY_FRAMES):
            assert set(RF.BOUNDARY_FRAMES) <= set(c["frame"][kind == RF.ORDINARY].tolist()), why
        # unit quaternions, a defined heading: the learner's
        for q in (c["cur_finite"][:, 3:7], c["prev_qpos"][:, 3:7]):
            np.testing.assert_allclose(np.linalg.norm(q, axis=1), 1.0, rtol=0, atol=4 * EPS)
            assert (q[:, 0] ** 2 + q[:, 3] ** 2).min() >= 0.05, why
        # away from the discontinuity of rotation_from_quaternion: still up to 4 ulp, or 1 - w >= 1e-6
        g = RF.one_minus_w(sk, c["cur_finite"], c["prev_qpos"])
        assert not RF.in_the_gap(g).any(), why
        assert (2.0 - g).min() >= RF.MOVING_MIN, why          # nor is any w that close to -1, where sqrt(1 - w^2) cancels as badly
        still =np.abs(g) <= RF.STILL_ULP * EPS
        assert still[kind == RF.STILL_ENV].all() and still[:, [l for l in range(1, nb) if sk.body_ndof[l] == 0]].all()
        assert (c["cur_finite"][kind == RF.STILL_ENV] == c["prev_qpos"][kind == RF.STILL_ENV]).all()
        moving = [l for l in range(1, nb) if sk.body_ndof[l] > 0]
        assert still[kind == RF.STILL_BODY][:, moving[-1]].all() and not still[kind == RF.STILL_BODY][:, 0].any()
        # the special rows do what they are there for
        qrel_w = 1.0 - g[:, 0]
        assert (qrel_w[kind == RF.ROOT_NEG] < 0).all() and (qrel_w[(kind != RF.ROOT_NEG)] > 0).all()       # the wrap, ang > pi
        assert ((1.0 - g[kind == RF.HINGE_2PI]).min(axis=1) < -0.9).all()             # a body turned by about 2 pi - 0.05: w near -1
        if (kind == RF.EXPERT_NEG).any():
            assert 0.05 < c["c_info"][kind == RF.EXPERT_NEG, 0].max() < 0.95            # half-angle near pi, and the pose term shows it
        assert (c["reward"][~on] == 0).all() and (c["c_info"][~on] == 0).all()
        assert n <= RF.ZERO_ROW or (kind[RF.ZERO_ROW] == RF.ORDINARY and (c["scale"][RF.ZERO_ROW] == 0).all())
    assert seen_kinds == set(range(7))
    # not saturated: per weight set, over the one-pass cases' ordinary rows
    for wn in RF.WEIGHT_SETS:
        ci = np.concatenate([c["c_info"][c["kind"] == RF.ORDINARY] for w, c in RF.k2_cases(tree, coord) if w == wn])
        frac = ((ci > 0.05) & (ci < 0.95)).mean(axis=0)
        assert frac.min() >= 0.2, "%s %s: fraction of ordinary rows with a term in (0.05, 0.95): %s" % (tree, wn, frac)
    for wn, c in (RF.five_pass_cases(tree) if coord == "heading" and tree in RF.FIVE_PASS_TREES else []):
        ci = c["c_info"][c["kind"] == RF.ORDINARY]
        assert ((ci > 0.05) & (ci < 0.95)).mean(axis=0).min() >= 0.2


def test_oracle_is_well_conditioned_on_the_cases():
    """A relative perturbation of 2e-16 on the inputs moves the oracle's c_info by far less than the float64 bound: the cases sit
    where acos is well conditioned, so 5e-10 is a statement about the kernel and not about the reference."""
    rng = np.random.RandomState(0)
    worst = 0.0
    for tree, coord in RF.TREE_COORDS:
        for wn, c in RF.k2_cases(tree, coord)[4::5]:                  # the largest size of every weight set
            jig = lambda a: a * (1.0 + 2e-16 * rng.choice([-1.0, 1.0], a.shape))
            r, ci = RF.oracle_reward(c, cur_qpos=jig(c["cur_qpos"]), prev_qpos=jig(c["prev_qpos"]), ee_wpos=jig(c["ee_wpos"]))
            worst = max(worst, float(np.abs(ci - c["c_info"]).max()))
    assert worst <= 5e-12, worst


def _mutants(c):
    """name -> overrides of oracle_reward; a mutant that cannot differ from the original on this case is left out."""
    ws, tree = R.resolve_weights(c["weights"]), c["tree"]
    ee = c["ee_wpos"].reshape(c["n"], 5, 3)[:, [1, 0, 2, 3, 4]].reshape(c["n"], 15)
    shifted = {k: v.copy() for k, v in RF.table(tree).items()}
    for k in shifted:
        for a, b in zip(RF.TAKE_OFF[1:-1], RF.TAKE_OFF[2:]):
            shifted[k][a:b] = np.roll(shifted[k][a:b], 1, axis=0)
    m = {"obs_coord swapped": dict(obs_coord="root" if c["obs_coord"] == "heading" else "heading"),
         "frame + 1": dict(frame=(c["frame"] + 1) % RF.N_FRAMES),
         "b_diffw rolled": dict(b_diffw=np.roll(c["b_diffw"], 1)),
         "two end effectors swapped": dict(ee_wpos=ee),
         "prev and cur swapped": dict(cur_qpos=np.where(np.isnan(c["cur_qpos"]), np.nan, c["prev_qpos"]), prev_qpos=c["cur_finite"]),
         "later takes' rows offset by one": dict(table=shifted)}
    if ws["v_ord"] != 2:
        m["v_ord taken as 2"] = dict(weights=dict(c["weights"], v_ord=2))
    if ws["decay"]:
        m["decay ignored"] = dict(weights=dict(c["weights"], decay=False))
    return m


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("tree,coord", RF.TREE_COORDS)
def test_bounds_tell_wrong_answers_apart(tree, coord, dt):
    """Per weight set, on the largest one-pass case of the GPU comparison: every mutant moves the reward or a c_info term of some
    row by >= 100 x the bound that row and column is held to (float32: against the oracle on the rounded inputs, as there)."""
    seen = set()
    for wn, c in RF.k2_cases(tree, coord)[4::5]:
        assert c["n"] == max(RF.k2_sizes(len(F.skeleton(tree).body_names)))
        want_r, want_c, b_r, b_c = RF.reward_bounds(c, dt)
        for why, over in _mutants(c).items():
            r, ci = RF.oracle_reward(c, rounded=dt == "f32", **over)
            m_c, m_r = (np.abs(ci - want_c) / b_c).max(), (np.abs(r - want_r) / b_r).max()
            print("MARGIN %s %s %s %s: c_info %.3g, reward %.3g" % (tree, dt, wn, why, m_c, m_r))
            assert max(m_c, m_r) >= 100.0, "%s %s, %s: only %.3g x the bound (c_info), %.3g x (reward)" % (tree, wn, why, m_c, m_r)
            seen.add(why)
    assert len(seen) == 8
