"""GPU: K5 (GAE, egp_gae_*) and K6 (the running filter, egp_zfilter_*) against high-precision references, at the gamma * tau,
masks and sizes that send K5's look to the right over several tiles and rounds, and at the widths and row counts that send K6
through every column-block, row-loop and merge route. Cases, references and bounds: scan_fixture.py; that the bounds would catch
a kernel with a wrong carry, order, stop or count: test_scan_reference_cpu.py.

What K5's cases execute that gamma = tau = 0.95 never does:
  1x1, 0.9999x1   `avail > 1` and `Aacc + Pacc * Aj` across tiles; a carry from up to 130 tiles away; `next += avail` and a second
                  and third round (65, 67, 131 tiles); the look ended by the batch's end, not by P
  0.99x0.95       the 2^-200 stop on a P that is not 0 (after two tiles)
  end@...         the look ended by an exact 0 at a chosen tile, on either side of a tile edge, and at the first tile of round two
  0.95x0.95       the control: one tile, as before
The path that gives up after two seconds without a neighbour's map is not exercised: nothing here keeps a map from coming.
"""
import numpy as np
import pytest
import torch

import scan_fixture as F
from conftest import load_golden

pytestmark = pytest.mark.gpu

L = np.longdouble
TORCH = {"f64": torch.float64, "f32": torch.float32}


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.array(a), dtype=dtype, device="cuda")          # (a copy: the fixture's arrays are read-only)


@pytest.fixture(scope="module")
def ctx(skel):
    from egopose_amd.hip import EgpContext
    c = load_golden("config_subject_03.npz")
    ws = dict(zip([str(k) for k in c["reward_keys"]], [float(v) for v in c["reward_vals"]]))
    cx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"],
                    reward_weights=ws, episode_len=int(c["env_episode_len"]))
    yield cx
    cx.close()


# ------------------------------------------------------------------------------------------------ K5
def _gae(ctx, inputs, gt, dtype):
    """One call of egp_gae_* and of egp_gae_standardize_* -> (adv, ret, stats, standardised adv) as tensors."""
    gamma, tau = F.GAMMA_TAU[gt]
    r, m, v = (dev(a, TORCH[dtype]) for a in inputs)
    adv, ret, stats = ctx.gae(r, m, v, gamma, tau)
    std = ctx.gae_standardize(adv.clone(), stats)
    return adv, ret, stats, std


def _excess(out, ref, dtype):
    """By how many times each output misses its bound: {adv, ret, stats, std} (pass: all <= 1)."""
    adv, ret, stats, std = (t.cpu().numpy() for t in out)
    st = np.abs(stats.astype(L) - ref["stats"]) / (L(F.STATS_RTOL) * np.abs(ref["stats"]))
    return dict(adv=F.worst(adv, ref["adv"], F.gae_bound(ref["adv"], dtype)), ret=F.worst(ret, ref["ret"], F.gae_bound(ref["ret"], dtype)),
                stats=float(np.where(np.isnan(st), np.inf, st).max()), std=F.worst(std, ref["std"], F.standardized_bound(ref, dtype)))


def _hold(ctx, n, mask, gt, dtype, salt=0):
    ex = _excess(_gae(ctx, F.gae_inputs(n, mask, salt), gt, dtype), F.gae_reference(n, mask, gt, dtype, salt), dtype)
    print("gae %s %s n=%d %s%s: x bound" % (dtype, gt, n, mask, " (salt %d)" % salt if salt else ""), {k: "%.3g" % x for k, x in ex.items()})
    return {k: x for k, x in ex.items() if not x <= 1.0}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("gt", list(F.GAMMA_TAU))
def test_gae_up_to_two_tiles(ctx, gt, dtype):
    """4, 5, 2 048, 2 049 and 4 096 samples -- a chunk and one more, whole tiles with no identity padding and one sample into the
    next -- under every mask: adv, ret, {n, mean, M2} and the standardised advantages against the long-double sweep."""
    bad = {}
    for n, mask in F.SMALL_CASES:
        miss = _hold(ctx, n, mask, gt, dtype)
        if miss:
            bad[(n, mask)] = miss
    assert not bad, bad


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("gt", list(F.GAMMA_TAU))
@pytest.mark.parametrize("n,mask", F.BIG_CASES, ids=["%d-%s" % c for c in F.BIG_CASES])
def test_gae_across_tiles_and_rounds(ctx, n, mask, gt, dtype):
    """64, 65, 67 and 131 tiles: one round of the look to the right exactly, one sample and well into the second, a third."""
    assert not _hold(ctx, n, mask, gt, dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gae_workspace_carries_nothing_over(ctx, dtype):
    """The map slots are armed again for every call: a second call of equal n with other data matches ITS reference, and so do a
    large, a small and again a large call on the one workspace (gamma tau = 1: every tile reads every map to its right)."""
    gt = "1x1"
    bad = {}
    for step, (n, mask, salt) in enumerate([(F.N_INTO_SECOND, "open1", 0), (F.N_INTO_SECOND, "open1", 1),
                                            (F.N_THIRD_ROUND, "open1", 0), (F.TILE + 1, "open0", 0), (F.N_THIRD_ROUND, "open1", 1)]):
        miss = _hold(ctx, n, mask, gt, dtype, salt)
        if miss:
            bad[(step, n, mask, salt)] = miss
    assert not bad, bad


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gae_is_bit_reproducible(ctx, dtype):
    """The order in which the maps are composed is fixed, whichever tiles have published when a tile looks: the same call twice
    gives the same bits, at 131 tiles with gamma tau = 1."""
    inputs = F.gae_inputs(F.N_THIRD_ROUND, "open1")
    a = _gae(ctx, inputs, "1x1", dtype)
    b = _gae(ctx, inputs, "1x1", dtype)
    for name, x, y in zip(("adv", "ret", "stats", "standardised"), a, b):
        assert torch.equal(x, y), name
    assert bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[2]).all())


# ------------------------------------------------------------------------------------------------ K6
def _zfilter(ctx, n, dim, dtype="f64", update=True, clip=F.ZF_CLIP):
    """One call of egp_zfilter_* from the case's running state -> (state after, y) as numpy; the state it started from must be untouched."""
    X0, X, act = F.zf_inputs(n, dim)
    s0 = F.zf_reference(n, dim, dtype, update, clip)[0]
    st0 = dev(s0)
    st1 = torch.full_like(st0, float("nan")) if update else None
    y = ctx.zfilter(dev(X, TORCH[dtype]), st0, st1, update=update, clip=clip, active=dev(act, torch.int32))
    assert np.array_equal(st0.cpu().numpy(), s0)
    return (st1.cpu().numpy() if update else s0), y.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("n,dim", F.ZF_CASES, ids=["%dx%d" % c for c in F.ZF_CASES])
def test_zfilter_widths_and_merge_routes(ctx, n, dim):
    """Widths on either side of the wave (63, 64) and of the 128-column block (127, 128, 129), one column, and three blocks (300),
    each through the apply kernel's own merge (1, 64, 1 024 rows), the one-block merge (1 025, 4 100) and, at 129 and 300, the
    two-level merge (16 385), from a running state, with a mask. Beyond 128 columns k_zf_apply takes its flat loop."""
    s0, s1, y_ref = F.zf_reference(n, dim)
    st, y = _zfilter(ctx, n, dim)
    ex = F.zf_excess(st, y, s1, y_ref)
    print("zfilter f64 %dx%d: %.3g x the tolerances" % (n, dim, ex))
    assert st[0] == s1[0]
    np.testing.assert_allclose(st[1:1 + dim], s1[1:1 + dim], rtol=F.ZF_TOL["mean"], atol=F.ZF_TOL["mean"])
    np.testing.assert_allclose(st[1 + dim:], s1[1 + dim:], rtol=F.ZF_TOL["S"])
    np.testing.assert_allclose(y, y_ref, rtol=F.ZF_TOL["y"], atol=F.ZF_TOL["y"])
    assert ex <= 1.0


@pytest.mark.parametrize("update,clip", [(False, F.ZF_CLIP), (False, 0.0), (True, 0.0)], ids=["frozen-clip", "frozen-noclip", "update-noclip"])
@pytest.mark.parametrize("n", [64, 1025])
def test_zfilter_frozen_and_unclipped_at_129(ctx, n, update, clip):
    dim = 129
    s0, s1, y_ref = F.zf_reference(n, dim, update=update, clip=clip)
    st, y = _zfilter(ctx, n, dim, update=update, clip=clip)
    if not clip:
        assert np.abs(y_ref).max() > F.ZF_CLIP          # (the clip would have shown)
    print("zfilter f64 %dx%d update=%s clip=%s: %.3g x the tolerances" % (n, dim, update, clip, F.zf_excess(st, y, s1, y_ref)))
    assert F.zf_excess(st, y, s1, y_ref) <= 1.0


@pytest.mark.parametrize("dim", [64, 129])
@pytest.mark.parametrize("n", [64, 4100])
def test_zfilter_float32_io(ctx, n, dim):
    """float32 in and out, float64 inside: the state against the oracle on the rounded rows at the float64 tolerances, y at 2e-5."""
    s0, s1, y_ref = F.zf_reference(n, dim, "f32")
    st, y = _zfilter(ctx, n, dim, "f32")
    ex = F.zf_excess(st, y, s1, y_ref, ytol=F.ZF_TOL["y32"])
    print("zfilter f32 %dx%d: %.3g x the tolerances" % (n, dim, ex))
    assert st[0] == s1[0]
    np.testing.assert_allclose(y, y_ref, rtol=F.ZF_TOL["y32"], atol=F.ZF_TOL["y32"])
    assert ex <= 1.0
