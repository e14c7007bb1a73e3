"""Mini-batch PPO on the device (agents/agent_ppo.py:16-44): the epoch plan kernel and the fixed-shape loss kernel of
csrc/egp_update.hip on their own, then AgentPPO(use_mini_batch=True) against golden runs of the reference -- the plain path in
float64, the fused path in float32 and with float64 masters over float32 shadows."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from minibatch_fixture import FIXTURES, build_agent, run_update
from update_fixture import check_final

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kctx(skel):
    from egopose_amd.hip import EgpContext
    c = load_golden("config_subject_03.npz")
    ctx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"])
    yield ctx
    ctx.close()


def _columns(N, D, A, exps_mode, seed, offset_states=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    if offset_states:        # the same rows from a base one float past a 16-byte boundary
        states = rnd(N * D + 4)[1:1 + N * D].view(N, D)
        assert states.data_ptr() % 16 == 4
    else:
        states = rnd(N, D)
    exps = {"ones": torch.ones(N, device="cuda"), "zeros": torch.zeros(N, device="cuda"),
            "mixed": (torch.rand(N, device="cuda", generator=g) < 0.6).float()}[exps_mode]
    return [states, rnd(N, A), rnd(N, 1), rnd(N, 1), rnd(N, 1), exps]


def _check_plan(cols, B, seed):
    from egopose_amd import optim as O
    N = cols[0].shape[0]
    perm = np.random.RandomState(seed).permutation(N)
    perm_t = torch.from_numpy(perm).cuda()
    counts = torch.full(((N + B - 1) // B,), -7, dtype=torch.int32, device="cuda")         # not zeroed: the kernel writes every entry
    out, counts = O.minibatch_plan(*cols, perm_t, B, mb_n_exp=counts)
    for src, dst in zip(cols, out):
        assert dst.shape == src.shape and torch.equal(dst, src[perm_t])
    e = cols[5].cpu().numpy()[perm] != 0
    want = [int(e[i:i + B].sum()) for i in range(0, N, B)]
    assert counts.tolist() == want


@pytest.mark.parametrize("exps_mode", ["ones", "zeros", "mixed"])
@pytest.mark.parametrize("N,B,D,A", [(131, 64, 13, 5), (131, 64, 76, 52), (200, 200, 16, 17), (7, 1, 4, 1), (1000, 4096, 13, 5)])
def test_minibatch_plan_moves_rows_exactly_and_counts_exploration_rows(N, B, D, A, exps_mode):
    _check_plan(_columns(N, D, A, exps_mode, seed=N + D + A), B, seed=N + B)


def test_minibatch_plan_with_a_misaligned_states_base():
    _check_plan(_columns(131, 76, 52, "mixed", seed=5, offset_states=True), 64, seed=6)


def test_minibatch_plan_rejects_bad_arguments():
    from egopose_amd import optim as O
    cols = _columns(16, 4, 2, "ones", seed=1)
    perm = torch.arange(16, device="cuda")
    with pytest.raises(ValueError):
        O.minibatch_plan(*cols, perm.int(), 4)
    with pytest.raises(ValueError):
        O.minibatch_plan(*cols, perm, 0)
    with pytest.raises(ValueError):
        O.minibatch_plan(cols[0].double(), *cols[1:], perm, 4)
    with pytest.raises(ValueError):
        O.minibatch_plan(*cols, perm, 4, out=cols)


def _window(n, A, seed, exps=None):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    log_std = rnd(1, A) * 0.2 - 1.0
    actions = rnd(n, A) * 0.3
    mean0 = actions + rnd(n, A) * torch.exp(log_std)
    mean = mean0 + rnd(n, A) * 0.02                       # the policy has moved: ratios on both sides of the clip range
    pred, returns, adv = rnd(n, 1), rnd(n, 1), rnd(n, 1)
    z = (actions - mean0) * torch.exp(-log_std)
    fixed = (-0.5 * z * z - 0.5 * np.log(2 * np.pi) - log_std).sum(1)
    if exps is None:
        exps = (torch.rand(n, device="cuda", generator=g) < 0.6).float()
        exps[0] = 1.0
    return dict(pred=pred, returns=returns, mean=mean, actions=actions, log_std=log_std, adv=adv, fixed=fixed, exps=exps)


@pytest.mark.parametrize("A", [5, 17])
@pytest.mark.parametrize("n", [1, 3, 64, 200])
def test_ppo_losses_mb_matches_the_gathered_loss_kernel(n, A):
    """Same per-row device code as optim.ppo_losses on the gathered exploration rows: identical bits per row, float64 sums of
    the same float32 terms in another order."""
    from egopose_amd import optim as O
    w = _window(n, A, seed=100 * n + A)
    rows = w["exps"].nonzero().squeeze(1)
    cnt = torch.tensor([rows.numel()], dtype=torch.int32, device="cuda")
    losses, d_pred, d_mean, d_ls = O.ppo_losses_mb(w["pred"], w["returns"], w["mean"], w["actions"], w["log_std"], w["adv"], w["fixed"],
                                                   w["exps"], cnt, 0.2, want_d_log_std=True)
    l_ref, p_ref, m_ref, ls_ref = O.ppo_losses(w["pred"], w["returns"], w["mean"][rows].contiguous(), w["actions"], w["log_std"], w["adv"],
                                               w["fixed"][rows].contiguous(), False, 0.2, n, rows.numel(), rows=rows, want_d_log_std=True)
    assert torch.equal(d_pred, p_ref)
    assert torch.equal(d_mean[rows], m_ref)
    masked = (w["exps"] == 0).nonzero().squeeze(1)
    assert torch.equal(d_mean[masked], torch.zeros(masked.numel(), A, device="cuda"))
    assert not torch.signbit(d_mean[masked]).any()
    # |terms|: the float32 squared errors, and the float32 surrogate terms (their size from the float64 formulation)
    dv = (w["pred"] - w["returns"]).double()
    v_scale = float((dv * dv).sum()) / n
    zz = (w["actions"][rows].double() - w["mean"][rows].double()) * torch.exp(-w["log_std"].double())
    logp = (-0.5 * zz * zz - 0.5 * np.log(2 * np.pi) - w["log_std"].double()).sum(1)
    ratio = torch.exp(logp - w["fixed"][rows].double())
    ad = w["adv"].reshape(-1)[rows].double()
    s_scale = float(torch.min(ratio * ad, ratio.clamp(0.8, 1.2) * ad).abs().sum()) / rows.numel()
    got, ref = losses.tolist(), l_ref.tolist()
    print("n %d A %d: value loss %r vs %r, surrogate %r vs %r" % (n, A, got[0], ref[0], got[1], ref[1]))
    assert abs(got[0] - ref[0]) <= 1e-12 * v_scale
    assert abs(got[1] - ref[1]) <= 1e-12 * s_scale
    np.testing.assert_allclose(d_ls.cpu().numpy(), ls_ref.cpu().numpy(), rtol=2e-4, atol=1e-6)
    # the same call again: the same bits
    l2, _, m2, ls2 = O.ppo_losses_mb(w["pred"], w["returns"], w["mean"], w["actions"], w["log_std"], w["adv"], w["fixed"], w["exps"], cnt, 0.2,
                                     want_d_log_std=True)
    assert torch.equal(l2, losses) and torch.equal(m2, d_mean) and torch.equal(ls2, d_ls)


def test_ppo_losses_mb_on_a_window_without_exploration_rows():
    """What the reference's run recorded for such a window (tests/golden/ppo_minibatch.npz): a NaN surrogate loss and an all-zero
    policy gradient."""
    from egopose_amd import optim as O
    g = load_golden("ppo_minibatch.npz")
    e, i = (int(x) for x in g["empty_window"])
    assert np.isnan(g["surr_loss"][e, i]) and g["policy_grad_absmax"][e, i] == 0.0
    w = _window(3, 5, seed=9, exps=torch.zeros(3, device="cuda"))
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_mean = torch.full((3, 5), 7.0, device="cuda")
    losses, d_pred, d_mean, d_ls = O.ppo_losses_mb(w["pred"], w["returns"], w["mean"], w["actions"], w["log_std"], w["adv"], w["fixed"],
                                                   w["exps"], cnt, 0.2, d_mean=d_mean, want_d_log_std=True)
    got = losses.tolist()
    assert np.isnan(got[1]) and np.isfinite(got[0])
    assert torch.equal(d_mean, torch.zeros(3, 5, device="cuda")) and torch.equal(d_ls, torch.zeros(1, 5, device="cuda"))
    np.testing.assert_allclose(d_pred.cpu().numpy(), (2.0 / 3.0 * (w["pred"] - w["returns"])).cpu().numpy(), rtol=1e-6)


def test_ppo_losses_mb_rejects_bad_arguments():
    from egopose_amd import optim as O
    w = _window(4, 5, seed=3)
    a = [w["pred"], w["returns"], w["mean"], w["actions"], w["log_std"], w["adv"], w["fixed"], w["exps"]]
    cnt = torch.ones(1, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        O.ppo_losses_mb(*a, cnt.long(), 0.2)
    with pytest.raises(ValueError):
        O.ppo_losses_mb(*a[:3], w["actions"].double(), *a[4:], cnt, 0.2)
    with pytest.raises(ValueError):
        O.ppo_losses_mb(*a[:7], w["exps"][:3], cnt, 0.2)


# ------------------------------------------------------------------------------------------------ the agent
def _with_k5(agent, kctx):
    """K5 (GAE) through `kctx`: a plain AgentPPO has no rollout to take the kernel context from."""
    agent._kernel_ctx = lambda: kctx
    inner = agent._advantages

    def adv_fn(rewards, masks, values):
        adv, ret = inner(rewards, masks, values)
        agent._seen = (adv.double().cpu().numpy(), ret.double().cpu().numpy(), values.double().cpu().numpy())
        return adv, ret
    agent._advantages = adv_fn


def _count_calls(monkeypatch, module, name):
    calls = []
    inner = getattr(module, name)

    def wrapped(*a, **k):
        calls.append(name)
        return inner(*a, **k)
    monkeypatch.setattr(module, name, wrapped)
    return calls


@pytest.mark.parametrize("fixture", FIXTURES)
def test_minibatch_update_float64_on_device_matches_reference(kctx, fixture, monkeypatch):
    monkeypatch.setenv("EGP_NET_DTYPE", "float64")
    g = load_golden(fixture)
    torch.set_default_dtype(torch.float64)
    try:
        agent, mods = build_agent(g, device="cuda")
        assert agent.shadow is None and agent.cdtype == torch.float64 and not agent._fused_losses()
        _with_k5(agent, kctx)
        run_update(agent, g)
        a, r, v0 = agent._seen
        np.testing.assert_allclose(v0, g["values0"], rtol=1e-10, atol=1e-11)
        np.testing.assert_allclose(a, g["adv0"], rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(r, g["ret0"], rtol=1e-10, atol=1e-11)
        check_final(mods, g, rtol=1e-9, atol=1e-10)
    finally:
        torch.set_default_dtype(torch.float32)


def _fused_update(g, kctx, masters64, monkeypatch=None):
    from egopose_amd import optim as O
    counts = None
    if masters64:
        torch.set_default_dtype(torch.float64)
    try:
        agent, mods = build_agent(g, device="cuda", dtype=torch.float64 if masters64 else torch.float32)
        assert agent.cdtype == torch.float32 and (agent.shadow is not None) == masters64 and agent._fused_losses()
        _with_k5(agent, kctx)
        if monkeypatch is not None:
            counts = dict(plan=_count_calls(monkeypatch, O, "minibatch_plan"), loss=_count_calls(monkeypatch, O, "ppo_losses_mb"), nonzero=[])
            inner_update, inner_nonzero = agent.update_policy, torch.Tensor.nonzero

            def nonzero(*a, **k):
                counts["nonzero"].append("nonzero")
                return inner_nonzero(*a, **k)

            def update_policy(*a, **k):
                with monkeypatch.context() as m:
                    m.setattr(torch.Tensor, "nonzero", nonzero)
                    return inner_update(*a, **k)
            agent.update_policy = update_policy
        run_update(agent, g)
        torch.cuda.synchronize()
    finally:
        torch.set_default_dtype(torch.float32)
    return agent, mods, counts


@pytest.mark.parametrize("fixture", FIXTURES)
@pytest.mark.parametrize("mode", ["float32", "float64-masters"])
def test_minibatch_update_fused_float32_path_matches_reference(kctx, mode, fixture, monkeypatch):
    g = load_golden(fixture)
    masters64 = mode == "float64-masters"
    agent, mods, counts = _fused_update(g, kctx, masters64, monkeypatch)
    epochs, n_iter = g["surr_loss"].shape
    assert len(counts["plan"]) == epochs and len(counts["loss"]) == epochs * n_iter and counts["nonzero"] == []
    a, r, v0 = agent._seen
    np.testing.assert_allclose(v0, g["values0"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(r, g["ret0"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(a, g["adv0"], rtol=1e-4, atol=1e-4)
    # The plain path in float32 on the CPU against these fixtures (both of them, float32 modules and float64 masters over float32
    # shadows): 0 of 3 211 / 0 of 7 651 parameter elements miss (rtol 1e-4, atol 3e-6), largest miss 0. Hence the cap:
    # max(2 * 0, 8) elements, each within 2 * 0 -- with that bound on their size, no element may miss.
    check_final(mods, g, rtol=1e-4, atol=3e-6, max_outliers=8, outlier_atol=0.0)
    want = torch.float64 if masters64 else torch.float32
    assert all(v.dtype == want for m in mods.values() for v in m.state_dict().values())
    # per mini-batch losses, epoch by epoch; NaN exactly where the reference's window had no exploration row
    surr = np.array(agent.update_stats["surr_loss"]).reshape(epochs, n_iter)
    assert np.array_equal(np.isnan(surr), np.isnan(g["surr_loss"]))
    np.testing.assert_allclose(surr, g["surr_loss"], rtol=1e-3, atol=1e-5, equal_nan=True)
    assert len(agent.update_stats["value_loss"]) == epochs * n_iter


def test_minibatch_update_fused_is_deterministic(kctx):
    g = load_golden("ppo_minibatch.npz")
    _, mods_a, _ = _fused_update(g, kctx, False)
    _, mods_b, _ = _fused_update(g, kctx, False)
    for name in mods_a:
        for (k, va), vb in zip(mods_a[name].state_dict().items(), mods_b[name].state_dict().values()):
            assert torch.equal(va, vb), name + "." + k
