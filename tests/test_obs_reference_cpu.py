"""CPU, no kernel: the references, cases and bounds of obs_fixture.py that test_obs_reference_gpu.py holds K3 (observations), K4
(body quaternions) and K3 fused into K6 (the running filter on the drained state) to on the synthetic trees. The oracle is shape
generic and its generic path is the pinned one; the conditions the filter bounds rest on hold for every case the GPU file runs;
and each bound tells a kernel that shares rows, strides, columns or counts wrongly from a right one by a factor of at least 1 000,
on the very inputs the GPU file runs."""
import numpy as np
import pytest

import obs_fixture as F
import scan_fixture as S
import tree_fixture as TF
from conftest import load_golden

MARGIN = 1000.0


# ------------------------------------------------------------------------------------------------ the oracle on the trees
@pytest.mark.parametrize("name", F.TREE_NAMES)
def test_oracle_widths_are_obs_widths(name):
    sk = TF.skeleton(name)
    q, v, t = F.obs_states(name, 5)
    for o in F.OPTS[name]:
        assert F.ref_obs(o, q, v, t).shape == (5, F.obs_width(sk, o)), F.opt_id(o)
    assert F.ref_body_quat(name, q).shape == (5, 4 * len(sk.body_names))


def test_listed_widths_are_the_cases_widths():
    lo_hi = {"star4": (9, 21), "welded": (16, 35), "chain33": (37, 77), "full64": (63, 129), "other58": (57, 117), "humanoid-topology": (57, 117)}
    for name, (lo, hi) in lo_hi.items():
        sk = TF.skeleton(name)
        w = [F.obs_width(sk, o) for o in F.OPT_ALL]
        assert (min(w), max(w)) == (lo, hi), name
    for name, o, dim in F.ROWS_CASES + F.ZF_TREES + F.ZF_TWO_LEVEL[1]:
        assert F.obs_width(TF.skeleton(name), o) == dim, (name, F.opt_id(o))
    for name, o, H, dim in F.POLICY_CASES:
        assert F.obs_width(TF.skeleton(name), o) == dim
    assert len(F.OPT_ALL) == len(set(F.OPT_ALL)) == 48 and F.OPT_FEW[0] == F.DEFAULT


def test_generic_oracle_path_is_the_pinned_one():
    """full_obs / body_quat with the humanoid-topology tree's tables on the golden file's inputs give the golden file's outputs: the
    code the trees' references come from is the code the reference vectors pin."""
    g = load_golden("body_quat_obs.npz")
    sk = TF.skeleton("humanoid-topology")
    assert (sk.nq, sk.nv) == (g["qpos"].shape[1], g["qvel"].shape[1])
    np.testing.assert_allclose(F.ref_obs(F.DEFAULT, g["qpos"], g["qvel"], None), g["obs"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(F.ref_body_quat("humanoid-topology", g["qpos"]), g["bquat"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", ["welded", "chain33"])
def test_body_quat_of_a_welded_body_is_the_identity(name):
    sk = TF.skeleton(name)
    bq = F.ref_body_quat(name, F.bq_states(name, 130, True)).reshape(130, -1, 4)
    welded = [b for b in range(1, len(sk.body_ndof)) if sk.body_ndof[b] == 0]
    assert welded
    assert np.array_equal(bq[:, welded], np.broadcast_to([1.0, 0.0, 0.0, 0.0], (130, len(welded), 4)))


def test_states_are_what_the_cases_say():
    q, v, t = F.obs_states("full64", F.N_ROWS_KERNEL, F.NONUNIT_TAIL)
    nrm = np.linalg.norm(q[:, 3:7], axis=1)
    assert np.allclose(nrm[:-F.NONUNIT_TAIL], 1.0, atol=1e-15) and 0.3 <= nrm[-F.NONUNIT_TAIL:].min() < 0.4 and 2.9 < nrm[-F.NONUNIT_TAIL:].max() <= 3.0
    assert t.dtype == np.int32 and t.min() == 0 and t.max() == F.T_MAX - 1 and 0.5 < (t >= F.EPISODE_LEN).mean() < 0.7
    h = F.bq_states("welded", 130, True)[:, 7:]
    assert np.all(np.abs(h[0::2]) == 2 * np.pi) and np.abs(h[1::2]).max() < 2 * np.pi
    # the rotated root velocity straddles the wave boundary on full64 (63, 64, 65), sits behind it with the heading (64 .. 66)
    sk = TF.skeleton("full64")
    assert F.vel_cols(sk, F.DEFAULT) == [63, 64, 65] and F.vel_cols(sk, F.H_ONLY) == [64, 65, 66] and F.noise_col(F.H_ONLY) == 5


# ------------------------------------------------------------------------------------------------ the fixture's conditions
_ALL_ZF = sorted(set(F.ZF_CASES + F.SPLIT_CASES + [(nm, o, n) for nm, o, _, _ in F.POLICY_CASES for n in F.POLICY_ROWS]), key=F.case_id)


@pytest.mark.parametrize("name,o,n", _ALL_ZF, ids=[F.case_id(c) for c in _ALL_ZF])
def test_filter_cases_meet_the_conditions_of_their_bounds(name, o, n):
    """zf_case asserts them when it builds a case (the noise column below 1e-15, every other column spread by more than 0.1); here
    for every case of the GPU file, with the figures, and the mask and the clip have work to do."""
    c = F.zf_case(name, o, n)
    nz, rest = c["noise"], c["rest"]
    assert (nz is None) == o.keep and len(rest) == c["X"].shape[1] - (nz is not None)
    z = 0.0 if nz is None else max(np.abs(c["X"][:, nz]).max(), np.abs(c["X0"][:, nz]).max())
    print("%s: noise column max |z| %.3g, smallest spread of the others %.3g" % (F.case_id((name, o, n)), z, c["std"][rest].min()))
    assert z < F.NOISE_RAW and c["std"][rest].min() > F.MIN_SPREAD
    assert c["act"][0] == 1 and c["s1"][0] == 300 + c["act"].sum()
    if n >= 64:
        assert 0.6 < c["act"].mean() < 0.95
    # a raw error of 1e-12 stays 20 x under ZF_TOL["y"] at such a spread
    assert F.RAW_TOL["f64"] / c["std"][rest].min() <= S.ZF_TOL["y"] / 20
    # the oracle against itself: nothing but its own noise column, inside the absolute bounds
    own = F.zf_obs_excess(c["s1"], c["y"], c)
    assert own <= 0.5 and (own == 0.0 or nz is not None)


@pytest.mark.parametrize("name,o,n", F.ZF32_CASES, ids=[F.case_id(c) for c in F.ZF32_CASES])
def test_float32_filter_cases_meet_the_spread_condition(name, o, n):
    c = F.zf_case(name, o, n, "f32")
    assert c["std"][c["rest"]].min() > F.MIN_SPREAD
    assert np.array_equal(c["qpos"], c["qpos"].astype(np.float32).astype(np.float64))


def test_frozen_cases_leave_the_state_alone_and_the_clip_would_show():
    for name, o, n in F.ZF_FROZEN:
        c = F.zf_case(name, o, n, "f64", True)
        assert np.array_equal(c["s0"], c["s1"]) and c["act"].sum() == 0
        for frozen in (True, False):
            u = F.zf_case(name, o, n, "f64", frozen, 0.0)
            assert np.abs(u["y"][:, u["rest"]]).max() > F.ZF_CLIP, (n, frozen)      # (the clip would have shown)


# ------------------------------------------------------------------------------------------------ float32: the formula decides
@pytest.mark.parametrize("name", F.TREE_NAMES)
def test_float32_formula_sits_inside_the_raw_bound(name):
    """3e-6 was set on the humanoid. get_full_obs evaluated in numpy float32 on the GPU file's rows -- unit roots and roots of norm
    0.3 .. 3 -- stays below a quarter of it on every tree and option set, so 4 x the formula's own worst miss is inside the
    constant and the constant stays."""
    worst = 0.0
    for nonunit in (0, 257):
        q, v, t = F.obs_states(name, 257, nonunit)
        q, v = F.as_dtype((q, v), "f32")
        for o in F.OPTS[name]:
            worst = max(worst, F.raw_excess(F.obs_in_float32(o, q, v, t), F.ref_obs(o, q, v, t), "f32"))
    print("%s: numpy float32 get_full_obs at %.3g of the float32 bound" % (name, worst))
    assert worst <= 0.25


# ------------------------------------------------------------------------------------------------ the bounds against wrong kernels
def _show(what, margin):
    print("%-60s %.3g x the bound" % (what, margin))
    assert margin >= MARGIN, "%s: only %.3g x the bound" % (what, margin)


_CHUNK_CASES = [("star4", F.DEFAULT, 5), ("star4", F.DEFAULT, 64), ("welded", F.DEFAULT, 64), ("chain33", F.Opt(heading=True, vel="root", phase=True), 64),
                ("full64", F.DEFAULT, 64), ("full64", F.H_ONLY, 1025), ("full64", F.H_PHASE, 4100), ("other58", F.DEFAULT, 64)]


@pytest.mark.parametrize("name,o,n", _CHUNK_CASES, ids=[F.case_id(c) for c in _CHUNK_CASES])
def test_bounds_tell_wrongly_shared_rows_apart(name, o, n):
    """The lanes that de-head a row's quaternion and rotate its velocity hand their results to the wrong row of the 4-row chunk:
    the filtered rows and the statistics miss ZF_TOL, and the raw rows the raw bound, by 1 000 x."""
    c = F.zf_case(name, o, n)
    assert (name, o, n) in F.ZF_CASES
    for what, mut in (("velocity with the next row's quaternion", F.mut_vel_with_next_rows_quat), ("de-headed quaternion to the wrong row", F.mut_deheaded_to_wrong_row)):
        Xm = mut(name, o, c)
        _show("%s, %s, raw" % (F.case_id((name, o, n)), what), F.raw_excess(Xm, c["X"], "f64"))
        _show("%s, %s, filtered" % (F.case_id((name, o, n)), what), F.zf_obs_excess(*F.stats_of(Xm, c), c))
        # (the noise column takes the partner row's z: still rounding noise, still inside its absolute bounds -- the margin is the other columns')
    if o.phase:
        Xm = F.mut_phase_of_the_chunks_first_row(c["X"])
        _show("%s, phase of the chunk's first row, raw" % F.case_id((name, o, n)), F.raw_excess(Xm, c["X"], "f64"))
        _show("%s, phase of the chunk's first row, filtered" % F.case_id((name, o, n)), F.zf_obs_excess(*F.stats_of(Xm, c), c))


@pytest.mark.parametrize("n", [1, 5, 64, 1025, 4100, 16385])
def test_bounds_tell_a_lost_column_block_apart(n):
    """129 columns: column 128 is the second column block's only one. Left out of the statistics, or merged with the neighbouring
    row group's count (scan_fixture's wrong_group_count on the observation source), it misses ZF_TOL by 1 000 x; K6's tile
    structure done right, in numpy, passes."""
    name, o = "full64", F.H_PHASE
    c = F.zf_case(name, o, n)
    assert c["X"].shape[1] == 129
    _show("%d x 129, column 128 left out of the statistics" % n, F.zf_obs_excess(*F.mut_column_left_out(c), c))
    right = F.zf_obs_excess(*S.zf_tiled(c["X"], c["act"], c["s0"]), c)
    print("%d x 129, K6's tiles in numpy: %.3g x the bound" % (n, right))
    assert right <= 1.0
    if n >= 64:               # (fewer rows: one row group, no neighbour to take a count from)
        _show("%d x 129, column block 1 with the neighbouring group's count" % n,
              F.zf_obs_excess(*S.zf_tiled(c["X"], c["act"], c["s0"], mutant="wrong_group_count"), c))


def test_bounds_tell_a_dropped_last_chunk_apart():
    """n = 5: rows 4 .. 7 are a chunk of one row. Dropped from the statistics, the count is wrong wherever that row is active; where
    it is not, nothing was dropped -- at least one of the cases has it active."""
    seen = 0
    for name, o, _ in F.ZF_TREES:
        c = F.zf_case(name, o, 5)
        if c["act"][4]:
            seen += 1
            _show("%s, last partial chunk dropped" % F.case_id((name, o, 5)), F.zf_obs_excess(*F.stats_of(c["X"], c, rows=np.arange(4)), c))
    assert seen >= 4


@pytest.mark.parametrize("name", ["star4", "welded", "chain33", "full64"])
def test_bounds_tell_the_humanoids_strides_apart(name):
    sk = TF.skeleton(name)
    assert (sk.nq, sk.nv) != (59, 58)
    for n in (5, 257):
        q, v, t = F.obs_states(name, n)
        for o in F.OPTS[name][:4] if name in ("star4", "full64") else F.OPTS[name]:
            _show("%s %s n=%d, rows at strides 59 / 58" % (name, F.opt_id(o), n),
                  F.raw_excess(F.mut_strides_of_the_humanoid(name, o, q, v, t), F.ref_obs(o, q, v, t), "f64"))
    assert (TF.skeleton("other58").nq, TF.skeleton("other58").nv) == (59, 58)        # (there the strides are the humanoid's: the tables differ)


def test_bounds_tell_a_phase_taken_from_another_row_apart():
    for name, o, n in [("star4", F.Opt(heading=True, vel="no", phase=True), 5), ("full64", F.H_PHASE, 257), ("welded", F.Opt(vel="no", phase=True), 257)]:
        q, v, t = F.obs_states(name, n)
        X = F.ref_obs(o, q, v, t)
        _show("%s %s n=%d, phase of the chunk's first row" % (name, F.opt_id(o), n), F.raw_excess(F.mut_phase_of_the_chunks_first_row(X), X, "f64"))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", F.TREE_NAMES)
def test_bounds_tell_wrong_euler_slots_apart(name, dtype):
    """A 2-dof body's second angle in Euler slot 2, a 0-dof body with the preceding body's angles: 1 000 x the body quaternions' bound,
    the float32 one too, on every tree that has such bodies."""
    sk = TF.skeleton(name)
    nd = np.asarray(sk.body_ndof)[1:]
    for n in F.BQ_ROWS[1:]:
        q, = F.as_dtype((F.bq_states(name, n),), dtype)
        ref = F.ref_body_quat(name, q)
        for how, present in (("slot2", (nd == 2).any()), ("welded", (nd == 0).any())):
            w = F.raw_excess(F.mut_body_quat(name, q, how), ref, dtype)
            if present:
                _show("%s n=%d %s, body quaternions, %s" % (name, n, dtype, how), w)
            else:
                assert w == 0.0
    assert {k for nm in F.TREE_NAMES for k in np.asarray(TF.skeleton(nm).body_ndof)[1:]} == {0, 1, 2, 3}
