"""GPU: K3 (k_obs, k_obs_rows), K4 (k_body_quat) and K3 fused into K6 (k_zf_partial<T, true>, the rows form of k_zf_apply, the filter
prologue of the policy step) against the float64 oracle on the synthetic trees of tree_fixture.py -- strides and tables other
than the humanoid's 59 / 58 / 21, 0- and 2-dof bodies, rows narrower than a wave (star4) and wider than the 128-column block
(full64 with heading and phase: 129). Cases, references and bounds: obs_fixture.py; that the bounds would catch a kernel that
shares rows, strides, columns or counts wrongly: test_obs_reference_cpu.py.

What these cases execute that the humanoid's (obs_dim 57 .. 117) never do:
  129 columns     a second column block of zf_partial_body<T, true> (cl = min(c, dim - 1), the count kept by block 0 only), the flat
                  src.at() loop of k_zf_apply on the observation source, launch_obs staying with k_obs from 32 768 rows on, the
                  policy step's !own_col route (in0 = 128 + 129 > 256) on the observation source
  127, 128        the rotated root velocity in columns 63 .. 65 / 64 .. 66: across the wave boundary / in a wave that holds no
                  de-headed quaternion column
  9, 19           a row narrower than one wave; 75 (chain33): hinge columns of 0-, 2- and 3-dof bodies
Every test prints its worst excess as a multiple of the bound it asserts.
"""
import numpy as np
import pytest
import torch

import obs_fixture as F
import scan_fixture as S
import tree_fixture as TF

pytestmark = pytest.mark.gpu

TORCH = {"f64": torch.float64, "f32": torch.float32}
WORST = {}


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.array(a), dtype=dtype, device="cuda")          # (a copy: the fixture's arrays are read-only)


def host(t):
    return t.cpu().numpy().astype(np.float64)


def note(family, what, x):
    """Print one case's excess and keep the family's worst (printed when the module is done). A pair: (every column but the noise
    column against ZF_TOL, the noise column against its absolute bounds) -> the worse of the two."""
    if isinstance(x, tuple):
        print("%s %s: %.3g x the bound (noise column: %.3g x its absolute bounds)" % (family, what, x[0], x[1]))
        WORST[family + ", noise column"] = max(WORST.get(family + ", noise column", 0.0), x[1])
        WORST[family] = max(WORST.get(family, 0.0), x[0])
        return max(x)
    print("%s %s: %.3g x the bound" % (family, what, x))
    WORST[family] = max(WORST.get(family, 0.0), x)
    return x


@pytest.fixture(scope="module")
def ctxs():
    """(tree, options) -> its EgpContext, made once."""
    made = {}

    def get(name, o):
        if (name, o) not in made:
            made[(name, o)] = F.context(name, o)
        return made[(name, o)]
    yield get
    for cx in made.values():
        cx.close()
    print("worst excess per family:", {k: "%.3g" % v for k, v in sorted(WORST.items())})


def phase_kw(o, t, a=None, b=None):
    return dict(phase_t=dev(t[a:b], torch.int32)) if o.phase else {}


# ------------------------------------------------------------------------------------------------ K4
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", F.TREE_NAMES)
def test_body_quat_on_trees(ctxs, name, dtype):
    """k_body_quat with nbody 5, 9, 14 and 21 and bodies of 0, 1, 2 and 3 hinges, at 1, 63 and 130 rows and on a block of hinges at
    +-2 pi: against body_quat; a 0-dof body gives (1, 0, 0, 0) exactly; float64 quaternions have unit norm."""
    sk, cx = TF.skeleton(name), ctxs(name, F.DEFAULT)
    nb = len(sk.body_names)
    welded = [b for b in range(1, nb) if sk.body_ndof[b] == 0]
    bad = {}
    for n, two_pi in [(n, False) for n in F.BQ_ROWS] + [(F.BQ_ROWS[-1], True)]:
        q, = F.as_dtype((F.bq_states(name, n, two_pi),), dtype)
        ref = F.ref_body_quat(name, q)
        got = host(cx.body_quat(dev(q, TORCH[dtype])))
        assert got.shape == ref.shape == (n, 4 * nb)
        ex = note("body_quat " + dtype, "%s n=%d%s" % (name, n, " hinges at 2 pi" if two_pi else ""), F.raw_excess(got, ref, dtype))
        if not ex <= 1.0:
            bad[(n, two_pi)] = ex
        g = got.reshape(n, nb, 4)
        assert np.array_equal(g[:, welded], np.broadcast_to([1.0, 0.0, 0.0, 0.0], (n, len(welded), 4)))
        if dtype == "f64":
            assert np.abs(np.linalg.norm(g, axis=2) - 1.0).max() <= 1e-12
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ K3: k_obs
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", F.TREE_NAMES)
def test_observations_on_trees(name, dtype):
    """k_obs under the tree's option sets (star4, full64: the 24 switch combinations, with and without phase) at 1, 5 and 257 rows,
    unit roots and roots of norm 0.3 .. 3, against full_obs; float64: the phase column bit-equal to the reference's division."""
    bad, worst = {}, 0.0
    for o in F.OPTS[name]:
        cx = F.context(name, o)
        for n in F.OBS_ROWS:
            for nonunit in (0, n):
                q, v, t = F.obs_states(name, n, nonunit)
                q, v = F.as_dtype((q, v), dtype)
                ref = F.ref_obs(o, q, v, t)
                assert cx.obs_dim == ref.shape[1]
                got = host(cx.obs(dev(q, TORCH[dtype]), dev(v, TORCH[dtype]), **phase_kw(o, t)))
                ex = F.raw_excess(got, ref, dtype)
                worst = max(worst, ex)
                if not ex <= 1.0:
                    bad[(F.opt_id(o), n, nonunit)] = ex
                if o.phase and dtype == "f64":
                    assert np.array_equal(got[:, -1], ref[:, -1]), F.opt_id(o)
        cx.close()
    note("raw " + dtype, "%s, %d option sets" % (name, len(F.OPTS[name])), worst)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ K3: k_obs_rows and its guard
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,o,dim", F.ROWS_CASES, ids=[F.case_id(c) for c in F.ROWS_CASES])
def test_row_streaming_observation_kernel_on_trees(ctxs, name, o, dim, dtype):
    """32 768 + 37 rows: k_obs_rows at 9, 11, 19, 75, 127 and 128 columns, k_obs at 129 (launch_obs must refuse the 128-thread row
    there), the last 4 096 rows with roots of norm 0.3 .. 3: the whole output against full_obs, and bit for bit against the same
    rows pushed through calls of 9 000."""
    cx, n = ctxs(name, o), F.N_ROWS_KERNEL
    assert cx.obs_dim == dim
    q, v, t = F.obs_states(name, n, F.NONUNIT_TAIL)
    q, v = F.as_dtype((q, v), dtype)
    ref = F.ref_obs(o, q, v, t)
    qd, vd = dev(q, TORCH[dtype]), dev(v, TORCH[dtype])
    big = cx.obs(qd, vd, **phase_kw(o, t))
    parts = torch.cat([cx.obs(qd[a:a + F.CHUNK_ROWS], vd[a:a + F.CHUNK_ROWS], **phase_kw(o, t, a, a + F.CHUNK_ROWS)) for a in range(0, n, F.CHUNK_ROWS)], 0)
    assert big.shape == (n, dim)
    ex = note("rows " + dtype, "%s %s (%d columns)" % (name, F.opt_id(o), dim), F.raw_excess(host(big), ref, dtype))
    assert ex <= 1.0
    assert torch.equal(big, parts)


# ------------------------------------------------------------------------------------------------ K3 + K6, float64
def _fused(cx, o, c, dtype="f64", write_only_active=False, sentinel=None):
    """One call of egp_obs_zfilter_* on case `c` from its running state -> (state after, y, y2) as tensors; the state it started from
    must be untouched."""
    T = TORCH[dtype]
    n, dim = c["X"].shape
    st0 = dev(c["s0"])
    st1 = torch.full_like(st0, float("nan"))
    y = torch.full((n, dim), float("nan") if sentinel is None else sentinel, dtype=T, device="cuda")
    y2 = y.clone()
    cx.obs_zfilter(dev(c["qpos"], T), dev(c["qvel"], T), st0, st1, c["clip"], y, y2, active=dev(c["act"], torch.int32),
                   write_only_active=write_only_active, **phase_kw(o, c["t"]))
    assert np.array_equal(st0.cpu().numpy(), c["s0"])
    return st1, y, y2


def _raw_equals_k3(cx, o, c, dtype="f64"):
    """The fused call without a filter state (raw observations) is k_obs's output bit for bit -> that output."""
    T = TORCH[dtype]
    n, dim = c["X"].shape
    qd, vd = dev(c["qpos"], T), dev(c["qvel"], T)
    raw = torch.full((n, dim), float("nan"), dtype=T, device="cuda")
    cx.obs_zfilter(qd, vd, None, None, 0.0, raw, **phase_kw(o, c["t"]))
    assert torch.equal(raw, cx.obs(qd, vd, **phase_kw(o, c["t"])))
    return host(raw)


@pytest.mark.parametrize("name,o,n", F.ZF_CASES, ids=[F.case_id(c) for c in F.ZF_CASES])
def test_fused_observation_filter_on_trees(ctxs, name, o, n):
    """egp_obs_zfilter_f64 from a running state, 80 % of the rows active, clip 5, through every merge route (1, 5, 64, 1 024 rows: the
    apply kernel's own merge; 1 025, 4 100: one merge block; 16 385: two levels) at 9 .. 129 columns: the raw call is k_obs bit for
    bit, state and y against RunningStatOracle / zfilter_apply, out2 equals out, write_only_active leaves inactive rows alone."""
    cx, c = ctxs(name, o), F.zf_case(name, o, n)
    assert cx.obs_dim == c["X"].shape[1]
    raw = _raw_equals_k3(cx, o, c)
    assert F.raw_excess(raw, c["X"], "f64") <= 1.0
    if c["noise"] is not None:
        assert np.abs(raw[:, c["noise"]]).max() <= F.NOISE_RAW
    st, y, y2 = _fused(cx, o, c)
    ex = note("fused f64", F.case_id((name, o, n)), F.zf_obs_parts(st.cpu().numpy(), host(y), c))
    assert st[0].item() == c["s1"][0]
    assert ex <= 1.0
    assert torch.equal(y, y2)
    st_w, y_w, y2_w = _fused(cx, o, c, write_only_active=True, sentinel=-77.0)
    on = dev(c["act"], torch.bool)
    assert torch.equal(st_w, st) and torch.equal(y_w, y2_w)
    assert torch.equal(y_w[on], y[on]) and bool((y_w[~on] == -77.0).all())


@pytest.mark.parametrize("frozen,clip", [(True, F.ZF_CLIP), (True, 0.0), (False, 0.0)], ids=["frozen-clip", "frozen-noclip", "update-noclip"])
@pytest.mark.parametrize("name,o,n", F.ZF_FROZEN, ids=[F.case_id(c) for c in F.ZF_FROZEN])
def test_fused_filter_frozen_and_unclipped_at_129(ctxs, name, o, n, frozen, clip):
    """No row active (the statistics stay as they are: the fused call has no other way to freeze them) and clip 0, 129 columns wide."""
    cx, c = ctxs(name, o), F.zf_case(name, o, n, "f64", frozen, clip)
    if not clip:
        assert np.abs(c["y"][:, c["rest"]]).max() > F.ZF_CLIP          # (the clip would have shown)
    st, y, y2 = _fused(cx, o, c)
    ex = note("fused f64", "%s frozen=%s clip=%s" % (F.case_id((name, o, n)), frozen, clip), F.zf_obs_parts(st.cpu().numpy(), host(y), c))
    assert ex <= 1.0 and torch.equal(y, y2)
    if frozen:
        assert np.array_equal(st.cpu().numpy(), c["s0"])


# ------------------------------------------------------------------------------------------------ the split pair
@pytest.mark.parametrize("name,o,n", F.SPLIT_CASES, ids=[F.case_id(c) for c in F.SPLIT_CASES])
def test_split_statistics_and_apply_equal_the_fused_call(ctxs, name, o, n):
    cx, c = ctxs(name, o), F.zf_case(name, o, n)
    dim = cx.obs_dim
    st, y, y2 = _fused(cx, o, c)
    qd, vd, kw = dev(c["qpos"]), dev(c["qvel"]), phase_kw(o, c["t"])
    ws = torch.empty(int(cx.lib.egp_zfilter_workspace_bytes(n, dim)) // 8, dtype=torch.float64, device="cuda")
    st0 = dev(c["s0"])
    st_s = torch.full_like(st0, float("nan"))
    y_s, y2_s = torch.full_like(y, float("nan")), torch.full_like(y, float("nan"))
    cx.obs_zfilter_stats(qd, vd, ws, active=dev(c["act"], torch.int32), **kw)
    cx.obs_zfilter_apply(qd, vd, st0, st_s, c["clip"], y_s, y2_s, ws, **kw)
    assert torch.equal(st_s, st) and torch.equal(y_s, y) and torch.equal(y2_s, y)


# ------------------------------------------------------------------------------------------------ K3 + K6, float32
@pytest.mark.parametrize("name,o,n", F.ZF32_CASES, ids=[F.case_id(c) for c in F.ZF32_CASES])
def test_fused_observation_filter_float32_on_trees(ctxs, name, o, n):
    """egp_obs_zfilter_f32: float32 in and out, float64 statistics. The raw call is k_obs on the float32 inputs bit for bit (held
    to the oracle above); the state against RunningStatOracle over those float32 observations at the float64 tolerances, y at 2e-5."""
    cx, c = ctxs(name, o), F.zf_case(name, o, n, "f32")
    raw = _raw_equals_k3(cx, o, c, "f32")
    assert F.raw_excess(raw, c["X"], "f32") <= 1.0
    if c["noise"] is not None:
        assert np.abs(raw[:, c["noise"]]).max() <= F.RAW_TOL["f32"]
    s0, s1, y_ref, _ = F.zf_from_rows(c["X0"], raw, c["act"], c["clip"])
    st, y, y2 = _fused(cx, o, c, "f32")
    assert y.dtype == torch.float32 and st[0].item() == s1[0]
    ex = note("fused f32", F.case_id((name, o, n)), F.zf_obs_parts(st.cpu().numpy(), host(y), c, ytol=S.ZF_TOL["y32"], dtype="f32", s1=s1, y_ref=y_ref))
    assert ex <= 1.0 and torch.equal(y, y2)


# ------------------------------------------------------------------------------------------------ the policy step's prologue
@pytest.mark.parametrize("n", F.POLICY_ROWS)
@pytest.mark.parametrize("name,o,H,dim", F.POLICY_CASES, ids=[F.case_id(c) for c in F.POLICY_CASES])
def test_filter_prologue_of_the_policy_step_on_trees(ctxs, name, o, H, dim, n):
    """egp_obs_zfilter_stats_f64 + egp_policy_step_f32 (filter block) against egp_obs_zfilter_f64 + the plain step: filtered rows,
    statistics and actions bit for bit. 19 state columns in the wave behind the context; in0 = 256 = T exactly; in0 = 257: the
    !own_col route on the observation source; 129 state columns over three waves behind a 40-wide context. The first case's
    filtered rows against the oracle as well: bit-equality alone does not show that both sides are right."""
    from egopose_amd.nets import MLP, PolicyGaussian
    from egopose_amd import policy_step
    cx, c = ctxs(name, o), F.zf_case(name, o, n)
    Sd, Tn, nu = cx.obs_dim, 7, cx.nu
    assert Sd == dim
    torch.manual_seed(11)
    pol = PolicyGaussian(MLP(H + Sd, (300, 200), "relu"), nu, log_std=-2.3).cuda()
    fp = policy_step.FusedGaussianPolicy(pol, torch.device("cuda"))
    qp, qv, kw = dev(c["qpos"]), dev(c["qvel"]), phase_kw(o, c["t"])
    act = dev(c["act"], torch.int32)
    st_a = dev(c["s0"])
    st_b, st_d = torch.full_like(st_a, float("nan")), torch.full_like(st_a, float("nan"))
    v_out = torch.randn(n, Tn, H, device="cuda")
    t_idx = torch.randint(0, Tn, (n,), device="cuda")
    noise = torch.randn(n, nu, device="cuda")
    # reference: the two filter launches, then the plain step on the filtered rows
    y_ref, y2_ref = torch.empty(n, Sd, dtype=torch.float64, device="cuda"), torch.empty(n, Sd, dtype=torch.float64, device="cuda")
    cx.obs_zfilter(qp, qv, st_a, st_b, c["clip"], y_ref, y2_ref, active=act, **kw)
    a_ref = torch.empty(n, nu, dtype=torch.float64, device="cuda")
    fp(v_out, t_idx, y2_ref, a_ref, noise=noise)
    # the apply pass inside the policy step
    ws = torch.empty(int(cx.lib.egp_zfilter_workspace_bytes(n, Sd)) // 8, dtype=torch.float64, device="cuda")
    y1, y2 = torch.zeros_like(y_ref), torch.zeros_like(y_ref)
    a_f = torch.full_like(a_ref, float("nan"))
    cx.obs_zfilter_stats(qp, qv, ws, active=act, **kw)
    fp.with_filter(cx, v_out, t_idx, qp, qv, st_a, st_d, c["clip"], y1, y2, ws, a_f, noise=noise, **kw)
    assert torch.equal(st_d, st_b) and torch.equal(y1, y_ref) and torch.equal(y2, y2_ref)
    assert torch.equal(a_f, a_ref) and bool(torch.isfinite(a_f).all())
    ex = note("policy prologue", F.case_id((name, o, H, n)), F.zf_obs_parts(st_d.cpu().numpy(), host(y1), c))
    assert ex <= 1.0
