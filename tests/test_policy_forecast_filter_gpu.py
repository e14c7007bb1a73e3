"""The forecast policy step with the observation filter's apply pass in front (`egp_policy_step_f32` (`cell` + filter block),
FusedForecastPolicy.with_filter): bit for bit the chain egp_obs_zfilter_apply_f64 -> egp_policy_step_f32 (cell) in its merged
form, ZFilter(update=False) in its frozen form; in-place h / c, argument checks, graph capture."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda"
NU = 52


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _ctx(skel, **obs_options):
    from egopose_amd.hip import EgpContext
    c = load_golden("config_subject_03.npz")
    ws = dict(zip([str(k) for k in c["reward_keys"]], [float(v) for v in c["reward_vals"]]))
    return EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"], reward_weights=ws,
                      episode_len=int(c["env_episode_len"]), obs_options=obs_options or None)


@pytest.fixture(scope="module")
def ctxs(skel):
    out = {115: _ctx(skel), 116: _ctx(skel, obs_phase=True)}
    assert out[115].obs_dim == 115 and out[116].obs_dim == 116
    yield out
    for c in out.values():
        c.close()


def _nets(S, Hs=128, H=128, hidden=(300, 200), seed=11):
    from egopose_amd.nets import MLP, PolicyGaussian, VideoForecastNet
    torch.manual_seed(seed)
    vs = VideoForecastNet(16, S, H, 4, "lstm", None, Hs, "lstm", False).to(DEV)
    pol = PolicyGaussian(MLP(H + Hs, hidden, "relu"), NU, log_std=-0.7).to(DEV)
    with torch.no_grad():
        pol.action_mean.weight.mul_(10.0)
        pol.action_mean.bias.normal_()
        pol.action_log_std.normal_(std=0.3)
    return vs, pol


@pytest.fixture(scope="module")
def fused():
    from egopose_amd import policy_step
    out = {}
    for S in (115, 116):
        vs, pol = _nets(S)
        out[S] = policy_step.FusedForecastPolicy(pol, vs, torch.device(DEV))
    return out


def _case(ctx, n, seed, n_alloc=None):
    """Inputs of one tick for n rows (buffers of n_alloc rows): engine state, context, h / c, noise, a running filter state
    to continue from (test_hip_parity.py:938-941), an `active` mask with zeros, and the workspace."""
    S = ctx.obs_dim
    n_alloc = n if n_alloc is None else n_alloc
    rng = np.random.RandomState(1000 + seed)
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s, **k: torch.randn(*s, generator=g, device=DEV, **k)
    qpos = rng.normal(size=(n_alloc, 59)) * 0.4
    qpos[:, 3:7] = rng.normal(size=(n_alloc, 4))
    qpos[:, 3:7] /= np.linalg.norm(qpos[:, 3:7], axis=1, keepdims=True)
    d = dict(qpos=dev(qpos), qvel=dev(rng.normal(size=(n_alloc, 58))), ctx=r(n_alloc, 3, 128), t_idx=torch.randint(0, 3, (n_alloc,), generator=g, device=DEV),
             h=torch.tanh(r(n_alloc, 128)), c=r(n_alloc, 128), noise=r(n_alloc, NU))
    act = (rng.uniform(size=n_alloc) < 0.7).astype(np.int32)
    act[0] = 1
    if n > 1:
        act[1] = 0
    d["active"] = dev(act, torch.int32)
    d["phase_t"] = dev(rng.randint(0, 2 * ctx.episode_len, size=n_alloc), torch.int32) if ctx.obs_phase else None
    st0 = torch.zeros(1 + 2 * S, dtype=torch.float64, device=DEV)
    st_a = torch.empty_like(st0)
    pt = dev(rng.randint(0, 50, size=300), torch.int32) if ctx.obs_phase else None
    ctx.obs_zfilter(dev(rng.normal(size=(300, 59)) * 0.3 + np.r_[0, 0, 1, 1, 0, 0, 0, np.zeros(52)]), dev(rng.normal(size=(300, 58))), st0, st_a, 5.0,
                    torch.empty(300, S, dtype=torch.float64, device=DEV), phase_t=pt)
    d["st"] = st_a
    d["ws"] = torch.empty(int(ctx.lib.egp_zfilter_workspace_bytes(max(n, 1), S)) // 8, dtype=torch.float64, device=DEV)
    return d


def _pt(d, n):
    return None if d["phase_t"] is None else d["phase_t"][:n]


def _chain(ctx, fp, d, n, h, c, st_in, active, noise=True):
    """stats + apply + the unfiltered step on y2 -> (y, y2, zf_out, action, mean); h / c in place."""
    S = ctx.obs_dim
    y, y2 = (torch.full((n, S), -9.0, dtype=torch.float64, device=DEV) for _ in range(2))
    st_out = torch.empty_like(st_in)
    act, mean = torch.empty(n, NU, dtype=torch.float64, device=DEV), torch.empty(n, NU, device=DEV)
    ctx.obs_zfilter_stats(d["qpos"][:n], d["qvel"][:n], d["ws"], active=active, phase_t=_pt(d, n))
    ctx.obs_zfilter_apply(d["qpos"][:n], d["qvel"][:n], st_in, st_out, 5.0, y, y2, d["ws"], phase_t=_pt(d, n))
    fp(d["ctx"][:n], d["t_idx"][:n], y2, h, c, act, noise=d["noise"][:n] if noise else None, mean_out=mean)
    return y, y2, st_out, act, mean


def _fused(ctx, fp, d, n, h, c, st_in, active, noise=True, frozen=False, want_out=True):
    S = ctx.obs_dim
    y, y2 = (torch.full((n, S), -9.0, dtype=torch.float64, device=DEV) for _ in range(2))
    st_out = torch.full_like(st_in, -3.0) if want_out else None
    act, mean = torch.empty(n, NU, dtype=torch.float64, device=DEV), torch.empty(n, NU, device=DEV)
    ws = None
    if not frozen:
        ctx.obs_zfilter_stats(d["qpos"][:n], d["qvel"][:n], d["ws"], active=active, phase_t=_pt(d, n))
        ws = d["ws"]
    fp.with_filter(ctx, d["ctx"][:n], d["t_idx"][:n], d["qpos"][:n], d["qvel"][:n], st_in, st_out, 5.0, y, y2, ws, h, c, act,
                   noise=d["noise"][:n] if noise else None, mean_out=mean, phase_t=_pt(d, n))
    return y, y2, st_out, act, mean


NAMES = ("y", "y2", "zf_out", "action", "mean")


@pytest.mark.parametrize("S,n", [(115, 1), (115, 5), (115, 9), (115, 37), (116, 5)])
def test_merged_form_is_bit_identical_to_apply_then_forecast_step(ctxs, fused, S, n):
    """stats + with_filter(workspace) against stats + obs_zfilter_apply + FusedForecastPolicy.__call__ on y2: with R = 4 rows per
    workgroup a partial tile (1), a partial second (5) and third (9) tile, and ten workgroups (37); width 116 = the phase column."""
    ctx, fp = ctxs[S], fused[S]
    d = _case(ctx, n, seed=n + S)
    h_a, c_a, h_b, c_b = d["h"].clone(), d["c"].clone(), d["h"].clone(), d["c"].clone()
    ref = _chain(ctx, fp, d, n, h_a, c_a, d["st"], d["active"])
    got = _fused(ctx, fp, d, n, h_b, c_b, d["st"], d["active"])
    for name, a, b in zip(NAMES, ref, got):
        assert torch.equal(a, b), name
    assert torch.equal(h_a, h_b) and torch.equal(c_a, c_b)
    assert not torch.equal(h_b, d["h"]) and not torch.equal(ref[2], d["st"])
    assert (ref[3] != ref[4].double()).any()                       # (the noise took part)


def test_frozen_form_equals_a_merge_over_nothing_and_the_host_filter(ctxs, fused):
    from egopose_amd.zfilter import ZFilter
    S, n = 115, 9
    ctx, fp = ctxs[S], fused[S]
    d = _case(ctx, n, seed=77)
    none_active = torch.zeros(n, dtype=torch.int32, device=DEV)
    h_a, c_a, h_b, c_b, h_c, c_c = (d[k].clone() for k in ("h", "c", "h", "c", "h", "c"))
    ref = _fused(ctx, fp, d, n, h_a, c_a, d["st"], none_active)                 # merged form, no row counted
    got = _fused(ctx, fp, d, n, h_b, c_b, d["st"], None, frozen=True)
    for name, a, b in zip(NAMES, ref, got):
        assert torch.equal(a, b), name
    assert torch.equal(h_a, h_b) and torch.equal(c_a, c_b)
    assert torch.equal(got[2], d["st"])
    no_out = _fused(ctx, fp, d, n, h_c, c_c, d["st"], None, frozen=True, want_out=False)      # zf_out may be NULL
    assert torch.equal(no_out[0], got[0]) and torch.equal(no_out[3], got[3]) and torch.equal(h_c, h_b)
    zf = ZFilter((S,), clip=5)
    zf.from_device_state(d["st"])
    obs = ctx.obs(d["qpos"][:n], d["qvel"][:n]).cpu().numpy()
    want = np.stack([zf(o, update=False) for o in obs])
    np.testing.assert_allclose(got[0].cpu().numpy(), want, rtol=0, atol=1e-12)


def test_three_steps_with_a_reset_row_equal_the_two_launch_chain(ctxs, fused):
    S, n = 115, 9
    ctx, fp = ctxs[S], fused[S]
    d = _case(ctx, n, seed=31)
    h_a, c_a, h_b, c_b = d["h"].clone(), d["c"].clone(), d["h"].clone(), d["c"].clone()
    st_a = st_b = d["st"]
    g = torch.Generator(device=DEV).manual_seed(3)
    for step in range(3):
        if step == 1:
            for t in (h_a, c_a, h_b, c_b):
                t[n // 2] = 0
        d["qvel"] = d["qvel"] + 0.3 * torch.randn(d["qvel"].shape, generator=g, device=DEV, dtype=torch.float64)
        d["noise"] = torch.randn(d["noise"].shape, generator=g, device=DEV)
        ref = _chain(ctx, fp, d, n, h_a, c_a, st_a, d["active"])
        got = _fused(ctx, fp, d, n, h_b, c_b, st_b, d["active"])
        for name, a, b in zip(NAMES, ref, got):
            assert torch.equal(a, b), "%s, step %d" % (name, step)
        assert torch.equal(h_a, h_b) and torch.equal(c_a, c_b), "h / c, step %d" % step
        st_a, st_b = ref[2], got[2]


def test_rows_beyond_n_untouched_n_zero_and_bad_cell_width(ctxs, fused):
    from egopose_amd import _lib as L
    S, n, n_alloc = 115, 6, 11
    ctx, fp = ctxs[S], fused[S]
    d = _case(ctx, n, seed=9, n_alloc=n_alloc)
    h, c = d["h"].clone(), d["c"].clone()
    y = torch.full((n_alloc, S), -9.0, dtype=torch.float64, device=DEV)
    act = torch.full((n_alloc, NU), -9.0, dtype=torch.float64, device=DEV)
    fp.with_filter(ctx, d["ctx"][:n], d["t_idx"][:n], d["qpos"][:n], d["qvel"][:n], d["st"], None, 5.0, y[:n], None, None, h[:n], c[:n], act[:n])
    assert torch.equal(h[n:], d["h"][n:]) and torch.equal(c[n:], d["c"][n:]) and (y[n:] == -9.0).all() and (act[n:] == -9.0).all()
    assert (y[:n] != -9.0).all() and not torch.equal(h[:n], d["h"][:n])
    # n == 0: OK, nothing written
    before = (h.clone(), c.clone(), y.clone())
    fp.with_filter(ctx, d["ctx"][:0], d["t_idx"][:0], d["qpos"][:0], d["qvel"][:0], d["st"], None, 5.0, y[:0], None, None, h[:0], c[:0], act[:0])
    torch.cuda.synchronize()
    assert torch.equal(h, before[0]) and torch.equal(c, before[1]) and torch.equal(y, before[2])
    # a cell whose input width is not obs_dim + Hs: EGP_E_INVALID
    p = lambda t: t.data_ptr()
    bad = (L.MlpLayer * 1)()
    bad[0].wt, bad[0].bias = fp.cell_desc[0].wt, fp.cell_desc[0].bias
    bad[0].in_dim, bad[0].out_dim = fp.cell_desc[0].in_dim + 1, fp.cell_desc[0].out_dim
    pd = L.PolicyDesc()
    pd.n, pd.ctx_rows, pd.ctx_row_stride, pd.ctx_dim, pd.t_idx = n, p(d["ctx"]), d["ctx"].stride(0), 128, p(d["t_idx"])
    pd.ctx, pd.qpos, pd.qvel, pd.zf_in, pd.clip, pd.y = ctx.handle, p(d["qpos"]), p(d["qvel"]), p(d["st"]), 5.0, p(y)
    pd.layers, pd.n_layers, pd.activation, pd.log_std, pd.action = fp.desc, len(fp.layers), fp.act, p(fp.log_std), p(act)
    pd.cell, pd.h, pd.c, pd.hc_row_stride = bad, p(h), p(c), 128
    rc = fp.lib.egp_policy_step_f32(C.byref(pd), L.current_stream())
    assert rc == -1
    with pytest.raises(ValueError, match="egp_policy_step_f32") as err:
        L.check(rc, "egp_policy_step_f32")
    assert "cell: in_dim = state_dim + hidden size" in str(err.value)
    # merged statistics need zf_out
    with pytest.raises(ValueError):
        fp.with_filter(ctx, d["ctx"][:n], d["t_idx"][:n], d["qpos"][:n], d["qvel"][:n], d["st"], None, 5.0, y[:n], None, d["ws"], h[:n], c[:n], act[:n])
    with pytest.raises(ValueError):                                # the 116-wide model's context does not fit the 115-wide cell
        fp.with_filter(ctxs[116], d["ctx"][:n], d["t_idx"][:n], d["qpos"][:n], d["qvel"][:n], d["st"], None, 5.0, y[:n], None, None, h[:n], c[:n], act[:n])


def test_raw_observations_without_a_running_state(ctxs, fused):
    """zf_in=None (a checkpoint without running_state): y = the raw observation, then the unfiltered step."""
    S, n = 115, 5
    ctx, fp = ctxs[S], fused[S]
    d = _case(ctx, n, seed=4)
    h_a, c_a, h_b, c_b = d["h"].clone(), d["c"].clone(), d["h"].clone(), d["c"].clone()
    y = torch.empty(n, S, dtype=torch.float64, device=DEV)
    a_f, a_r = torch.empty(n, NU, dtype=torch.float64, device=DEV), torch.empty(n, NU, dtype=torch.float64, device=DEV)
    fp.with_filter(ctx, d["ctx"], d["t_idx"], d["qpos"], d["qvel"], None, None, 0.0, y, None, None, h_a, c_a, a_f)
    obs = ctx.obs(d["qpos"], d["qvel"])
    assert torch.equal(y, obs)
    fp(d["ctx"], d["t_idx"], obs, h_b, c_b, a_r)
    assert torch.equal(a_f, a_r) and torch.equal(h_a, h_b) and torch.equal(c_a, c_b)


def test_frozen_launch_replays_from_a_captured_graph(ctxs, fused):
    S, n = 115, 9
    ctx, fp = ctxs[S], fused[S]
    d = _case(ctx, n, seed=13)
    h0, c0 = d["h"].clone(), d["c"].clone()
    # eager: two consecutive steps
    h_e, c_e = h0.clone(), c0.clone()
    eager = []
    for _ in range(2):
        r = _fused(ctx, fp, d, n, h_e, c_e, d["st"], None, noise=False, frozen=True, want_out=False)
        eager.append((r[0].clone(), r[3].clone(), h_e.clone(), c_e.clone()))
    # captured: static buffers, one launch, replayed twice
    h_g, c_g = h0.clone(), c0.clone()
    y = torch.empty(n, S, dtype=torch.float64, device=DEV)
    act = torch.empty(n, NU, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fp.with_filter(ctx, d["ctx"], d["t_idx"], d["qpos"], d["qvel"], d["st"], None, 5.0, y, None, None, h_g, c_g, act)
    h_g.copy_(h0); c_g.copy_(c0)
    for k in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager[k][0]) and torch.equal(act, eager[k][1]), "replay %d" % k
        assert torch.equal(h_g, eager[k][2]) and torch.equal(c_g, eager[k][3]), "replay %d" % k
