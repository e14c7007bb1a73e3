"""The imitation reward K2 (k_reward_quat_v3) and the pose features K7 (k_pose_features) of csrc/egp_reward.hip on the trees of
tree_fixture.py against float64 (oracle/reward.py, oracle/humanoid.py, oracle/quat.py) on the cases of reward_fixture.py: every
v_ord branch, tiles whose cap bites (nbody 5, 9, 14) and whose does not (21), 0- and 2-dof bodies, a non-uniform b_diffw, three
expert takes, the float32 and float64 five-pass forms, both obs_coord frames, and the quaternion branches recorded frames
barely touch (a body and an env that did not move, the root-angle wrap, a half-angle near pi, a hinge that jumps by almost
2 pi, inactive rows whose qpos is NaN). test_reward_reference_cpu.py checks the cases themselves and shows that a reward wrong
in one index, frame, weight or branch misses the bounds used here by a factor of 100 or more.

Bounds (reward_fixture.GATES): float64, the project's parity gate -- 5e-10 on c_info, rtol 1e-10 + atol 5e-10 on the reward, 1e-10
on quaternions and end effectors, 5e-9 on finite-difference velocities; float32, against the oracle on the float32-rounded
inputs and expert rows, max(the gate at float32's figures: 5e-5, 1e-5 + 5e-5, 1e-5, 5e-4; 8 s) with s the shift of the float64
oracle's own output under that rounding.

v_ord above 3 in float32: powf(|d|, v_ord) itself overflows only from |d|^v_ord > 3.4e38, which on the CPU is v_ord >= 17 at the
188 rad/s of the hinge-2pi row and v_ord >= 26 at 30 rad/s, so overflow was NOT confirmed for orders just above 3; they are
left out because no config uses them.

Every comparison prints `RATIO <tree> <what> <worst error / bound>` before it asserts (pytest -s shows them). Measured on an
MI355X when the file was written, worst over all tests of a tree:

    tree               dtype  K2 c_info  K2 reward  five-pass  K7 quat, ee  K7 velocities
    star4              f64    4.0e-4     3.1e-5     -          4.4e-6       0.036
    star4              f32    0.13       0.046      -          0.013        0.13
    welded             f64    6.6e-4     5.1e-5     7.6e-4     6.7e-6       3.1e-5
    welded             f32    0.13       0.053      0.13       0.020        0.13
    chain33            f64    7.9e-4     7.2e-5     8.7e-4     3.3e-6       0.021
    chain33            f32    0.13       0.052      0.13       0.015        0.12
    full64             f64    3.8e-4     3.1e-5     -          6.7e-6       0.018
    full64             f32    0.13       0.055      -          0.015        0.13
    other58            f64    6.6e-4     5.5e-5     -          3.3e-6       0.031
    other58            f32    0.13       0.073      -          0.014        0.13
    humanoid-topology  f64    5.2e-4     4.6e-5     7.6e-4     6.7e-6       0.21
    humanoid-topology  f32    0.13       0.054      0.13       0.017        0.13

No bound had to move and no kernel was wrong. float64's worst (1.1e-9 rad/s in 190) is the unwrapped root row of bangvel on a
root-negated row: w within 1.3e-5 of -1, where the reference's sqrt(1 - w^2) cancels, in the oracle as in the kernel (the
other kinds of row of that case agree to 5e-12). float32's 0.13 is rp_r and bangvel at about one input rounding (1 / 8 of 8 s).
pose_dist on welded: 1.3e-3 of 1e-12.
"""
import numpy as np
import pytest
import torch

import reward_fixture as RF
import tree_fixture as F
from oracle import reward as R

pytestmark = pytest.mark.gpu

TORCH = {"f64": torch.float64, "f32": torch.float32}


def dev(a, dt="f64"):
    return torch.as_tensor(np.array(a), dtype=TORCH[dt], device="cuda")            # (a copy: the cases' arrays are read-only)


def i32(a):
    return torch.as_tensor(np.array(a), dtype=torch.int32, device="cuda")


@pytest.fixture(scope="module")
def contexts():
    """(tree, obs_coord) -> its one context of this module, the tree's three expert takes resident."""
    made = {}

    def get(tree, coord="heading"):
        if (tree, coord) not in made:
            cx = F.context_for(F.skeleton(tree), F.SEEDS[tree], gains=RF.gains(tree), obs_options=dict(obs_coord=coord))
            assert cx.episode_len == RF.EPISODE_LEN and cx.frame_skip == RF.FRAME_SKIP
            cx.upload_experts(RF.takes(tree))
            assert cx.take_offset.tolist() == list(RF.TAKE_OFF)
            made[(tree, coord)] = cx
        return made[(tree, coord)]

    yield get
    for cx in made.values():
        cx.close()


def _report(tree, what, ratio):
    print("RATIO %s %s %.4g" % (tree, what, ratio))
    return ratio


def _run_reward(cx, c, dt, rows=slice(None)):
    """K2 on the case's rows -> (reward, c_info) as numpy; the outputs are pre-filled with NaN (every row must be written)."""
    n = len(c["frame"][rows])
    r = torch.full((n,), float("nan"), dtype=TORCH[dt], device="cuda")
    ci = torch.full((n, 5), float("nan"), dtype=TORCH[dt], device="cuda")
    cx.reward(dev(c["cur_qpos"][rows], dt), dev(c["prev_qpos"][rows], dt), dev(c["ee_wpos"][rows], dt), i32(c["t"][rows]),
              i32(c["frame"][rows]), i32(c["end"][rows]), RF.END_REWARD, active=i32(c["active"][rows]), reward_out=r, cinfo_out=ci)
    return r.cpu().numpy().astype(np.float64), ci.cpu().numpy().astype(np.float64)


def _check_reward(tree, tag, c, dt, r, ci):
    """Reward and the five c_info columns of every active row against the oracle, exact zeros on the inactive ones; prints the
    worst error / bound per column and per kind of row, then asserts. -> the worst ratio."""
    want_r, want_c, b_r, b_c = RF.reward_bounds(c, dt)
    on = c["active"] != 0
    assert r.shape == (c["n"],) and ci.shape == (c["n"], 5)
    assert (r[~on] == 0).all() and (ci[~on] == 0).all(), "%s %s: inactive rows must be exactly 0" % (tree, tag)
    ratio = np.c_[np.abs(ci - want_c) / b_c, np.abs(r - want_r) / b_r][on]
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)
    worst = {}
    for k, name in enumerate(("pose_r", "vel_r", "ee_r", "rp_r", "rv_r", "reward")):
        worst[name] = _report(tree, "%s %s/%s" % (dt, name, tag), float(ratio[:, k].max()))
    bad = np.where(ratio.max(axis=1) > 1.0)[0]
    kinds = sorted({RF.KIND_NAMES[k] for k in c["kind"][on][bad]})
    assert not len(bad), "%s %s %s: %d rows beyond the bound (kinds %s), worst %s" % (tree, dt, tag, len(bad), kinds, worst)
    return max(worst.values())


# ---------------------------------------------------------------------------------------------- a. K2, the one-pass form
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("tree,coord", RF.TREE_COORDS)
def test_reward_every_tree_every_weight_set(contexts, tree, coord, dt):
    """n in {1, tile - 1, tile, tile + 1, 3 tile + 5} x the four weight sets (v_ord 2, 1, 1.5 with decay, 3 with its own k_v and
    w_v): the t_pow path of both phases, the waves and passes beyond a capped tile, b_diffw read at the right body."""
    cx = contexts(tree, coord)
    before = dict(cx.reward_weights)
    try:
        for wn, c in RF.k2_cases(tree, coord):
            cx.set_reward_weights(c["weights"])
            r, ci = _run_reward(cx, c, dt)
            _check_reward(tree, "%s/%s/n=%d" % (coord, wn, c["n"]), c, dt, r, ci)
    finally:
        cx.set_reward_weights(before)


# ---------------------------------------------------------------------------------------------- b. K2, the five-pass form
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("tree", RF.FIVE_PASS_TREES)
def test_reward_five_pass_form(contexts, tree, dt):
    """n = 16384 + 77 launches the five-pass instantiation (tile capped at 64 on welded, the fifth pass skipped whole on chain33,
    tile 60 on the humanoid's tree): every row against the oracle, and bit-identical to the one-pass form on the same rows."""
    cx = contexts(tree)
    before = dict(cx.reward_weights)
    assert RF.FIVE_PASS_N >= RF.FIVE_PASS_FROM
    try:
        for wn, c in RF.five_pass_cases(tree):
            cx.set_reward_weights(c["weights"])
            r, ci = _run_reward(cx, c, dt)
            _check_reward(tree, "five-pass/%s" % wn, c, dt, r, ci)
            for a in range(0, c["n"], 8192):
                rows = slice(a, min(a + 8192, c["n"]))
                assert rows.stop - rows.start < RF.FIVE_PASS_FROM
                r1, c1 = _run_reward(cx, c, dt, rows)
                assert (r1 == r[rows]).all() and (c1 == ci[rows]).all(), "%s %s: the two forms differ in rows %d.." % (tree, wn, a)
    finally:
        cx.set_reward_weights(before)


# ---------------------------------------------------------------------------------------------- c. K7
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("tree,coord", RF.TREE_COORDS)
def test_pose_features_every_tree(contexts, tree, coord, dt):
    """n in {1, 8, 9, 65} (a workgroup holds eight envs), both conventions: all seven outputs, with the hinge entries of qvel at
    0- and 2-dof bodies and the root rows of bquat and bangvel (no wrap there: the negated root quaternion turns by > pi)."""
    cx, sk = contexts(tree, coord), F.skeleton(tree)
    nb = len(sk.body_names)
    for c in RF.k7_cases(tree, coord):
        n = c["n"]
        for conv in (False, True):
            out = cx.pose_features(dev(c["cur_finite"], dt), dev(c["prev_qpos"], dt), dev(c["ee_wpos"], dt), expert_convention=conv)
            worst = {}
            for k, (want, bound) in RF.feature_bounds(c, conv, dt).items():
                got = out[k].cpu().numpy().astype(np.float64)
                assert got.shape == want.shape == (n, dict(qvel=sk.nv, rlinv_local=3, rangv=3, rq_rmh=4, ee_pos=15, bquat=4 * nb, bangvel=3 * nb)[k])
                err = np.abs(got - want)
                worst[k] = _report(tree, "%s %s/%s/%s/n=%d" % (dt, k, coord, "expert" if conv else "learner", n),
                                   float(np.where(np.isfinite(err), err, np.inf).max() / bound))
            assert max(worst.values()) <= 1.0, "%s %s n=%d %s: %s" % (tree, dt, n, "expert" if conv else "learner", worst)
        if n > 5:
            assert abs(np.linalg.norm(c["features"][True]["bangvel"][5, :3]) * RF.dt_of(sk)) > np.pi      # row 5: the root turned by > pi, unwrapped


# ---------------------------------------------------------------------------------------------- d. pose_dist at nq != 59
def test_pose_dist_on_welded(contexts):
    """k_reward_simple takes the width of a pose from the context (nq = 18 here); inactive rows keep what the output held."""
    tree = RF.POSE_DIST_TREE
    cx, sk, c = contexts(tree), F.skeleton(tree), RF.pose_dist_case()
    assert sk.nq == 18
    on = c["active"] != 0
    want_r, want_d = np.full(c["n"], -7.0), np.full((c["n"], 1), -9.0)
    for i in np.where(on)[0]:
        want_r[i], want_d[i] = R.pose_dist(c["cur_qpos"][i], RF.table(tree)["qpos"][c["frame"][i]], c["end"][i] != 0, RF.END_REWARD)
    r, d = dev(np.full(c["n"], -7.0)), dev(np.full((c["n"], 1), -9.0))
    cx.reward_simple("pose_dist", dev(c["cur_qpos"]), i32(c["frame"]), i32(c["end"]), RF.END_REWARD, active=i32(c["active"]), reward_out=r, cinfo_out=d)
    r, d = r.cpu().numpy(), d.cpu().numpy()
    assert (r[~on] == -7.0).all() and (d[~on] == -9.0).all() and (~on).sum() >= 2
    _report(tree, "f64 pose_dist", float(max(np.abs(r - want_r).max(), np.abs(d - want_d).max()) / 1e-12))
    np.testing.assert_allclose(d, want_d, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r, want_r, rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------- e. the expert table's packing
@pytest.mark.parametrize("tree", ["star4", "chain33", "humanoid-topology"])
def test_three_takes_equal_one_concatenated_take(contexts, tree):
    """The rows of egp_upload_experts do not depend on how the frames are split into takes: the same 70 frames as one take give
    bit-identical rewards in both dtypes (and the three-take table itself is held to the oracle by the tests above)."""
    cx = contexts(tree)
    c = RF.k2_cases(tree, "heading")[4][1]
    try:
        three = {dt: _run_reward(cx, c, dt) for dt in ("f64", "f32")}
        cx.upload_experts([RF.one_take(tree)])
        assert cx.take_offset.tolist() == [0, RF.N_FRAMES]
        for dt in ("f64", "f32"):
            r, ci = _run_reward(cx, c, dt)
            assert (r == three[dt][0]).all() and (ci == three[dt][1]).all()
            _check_reward(tree, "one-take/n=%d" % c["n"], c, dt, r, ci)
    finally:
        cx.upload_experts(RF.takes(tree))


# ---------------------------------------------------------------------------------------------- f. v_ord that is not a number
def test_non_finite_v_ord_is_refused(contexts):
    """fill_reward refuses v_ord = inf (the reference's max-norm, which K2's pow(pow(|d|, inf), 0) = 1 is not) and NaN, at
    egp_create and at egp_set_reward_weights, and a refused call (v_ord < 1 as well) leaves the context's weights as they were:
    the next reward is bit-identical to the one before the refusal, and the binding's `reward_weights` has not moved."""
    tree = "star4"
    cx = contexts(tree)
    wn, c = RF.k2_cases(tree, "heading")[14]
    assert wn == "v1.5-decay"
    before = dict(cx.reward_weights)
    try:
        cx.set_reward_weights(c["weights"])
        kept = dict(cx.reward_weights)
        base = _run_reward(cx, c, "f64")
        for bad in (float("inf"), float("nan"), -float("inf"), 0.5):
            with pytest.raises(ValueError, match="v_ord"):
                cx.set_reward_weights(dict(v_ord=bad, k_v=1.0, w_p=7.0, decay=False))
            assert cx.reward_weights == kept
            again = _run_reward(cx, c, "f64")
            assert (again[0] == base[0]).all() and (again[1] == base[1]).all(), "a refused v_ord = %r changed the weights" % bad
        _check_reward(tree, "after-refusals/n=%d" % c["n"], c, "f64", *base)
    finally:
        cx.set_reward_weights(before)
    from egopose_amd.hip import EgpContext
    g, sk = RF.gains(tree), F.skeleton(tree)
    for bad in (float("inf"), float("nan")):
        with pytest.raises(ValueError, match="v_ord"):
            EgpContext(sk, g["jkp"], g["jkd"], g["a_ref"], g["a_scale"], g["torque_lim"], g["b_diffw"], reward_weights=dict(v_ord=bad))
