"""AgentVGAIL on the MI355X: the three kernels of csrc/egp_gail.hip against float64 torch on the same inputs, the fused
`update_discriminator` against golden runs of the reference's (tests/golden/vgail*.npz, tools/gen_golden_vgail.py) and against
the plain form, `update_params`, the discriminator as a reward, and two Trainer iterations with `gail={}`."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
import vgail_fixture as V
from update_fixture import check_final

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ------------------------------------------------------------------------------------------------ kernels alone
def _offset(shape, gen, off):
    """A float32 HIP tensor of `shape` whose base sits `off` floats past an allocation (off = 1: one float past a 16-byte boundary)."""
    n = int(np.prod(shape))
    buf = torch.empty(n + off, dtype=torch.float32, device=DEV)
    buf[off:] = torch.randn(n, generator=gen).to(DEV)
    return buf[off:].view(*shape)


def _rows_case(n, H, S, with_filter, off=0, seed=0):
    gen = torch.Generator().manual_seed(seed + n)
    R, T = n + 7, 97
    ctx = _offset((R, H), gen, off)
    x = _offset((n, S), gen, off)
    tab = _offset((T, S), gen, off)
    idx = torch.randperm(R, generator=gen)[:n].to(DEV)
    src = torch.randint(0, T, (n,), generator=gen).to(DEV)
    mean = _offset((S,), gen, off) if with_filter else None
    inv_std = _offset((S,), gen, off).abs_().add_(0.5) if with_filter else None          # (in place: the base stays where it is)
    return ctx, idx, x, tab, src, mean, inv_std


ROWS_SHAPES = [(1, 4, 1), (131, 16, 13), (131, 128, 76), (1000, 16, 115), (70001, 16, 13)]


@pytest.mark.parametrize("with_filter", [False, True])
@pytest.mark.parametrize("shape,off", [(s, 0) for s in ROWS_SHAPES] + [((131, 128, 76), 1)])
def test_gail_rows_forward_and_adjoint(shape, off, with_filter):
    """The kernels only move rows or add two floats: context and state columns exact, the normalised columns within 1 ulp of the
    float32 evaluation of (t - mean) * inv_std (one subtract, one multiply, in either contraction) and 2 ulp of the float64 one;
    the adjoint is one float32 add, exact."""
    from egopose_amd import optim as O
    n, H, S = shape
    ctx, idx, x, tab, src, mean, inv_std = _rows_case(n, H, S, with_filter, off)
    if off:
        assert ctx.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 4 and tab.data_ptr() % 16 == 4
        out = _offset((2 * n, H + S), torch.Generator().manual_seed(1), off)
        assert out.data_ptr() % 16 == 4
    else:
        out = None
    X = O.gail_rows(ctx, idx, x, tab, src, mean, inv_std, out=out, src_host=src.cpu().numpy())
    torch.cuda.synchronize()
    assert X.shape == (2 * n, H + S)
    g_ctx = ctx.double()[idx]
    np.testing.assert_array_equal(X[:n, :H].double().cpu().numpy(), g_ctx.cpu().numpy())
    np.testing.assert_array_equal(X[n:, :H].double().cpu().numpy(), g_ctx.cpu().numpy())
    np.testing.assert_array_equal(X[:n, H:].cpu().numpy(), x.cpu().numpy())
    got = X[n:, H:].cpu().numpy()
    if not with_filter:
        np.testing.assert_array_equal(got, tab[src].cpu().numpy())
    else:
        t32, m32, s32 = tab[src].cpu(), mean.cpu(), inv_std.cpu()
        ref32 = ((t32 - m32) * s32).numpy()
        ref64 = ((t32.double() - m32.double()) * s32.double()).numpy()
        ulp = np.spacing(np.abs(ref32))
        err32, err64 = np.abs(got - ref32) / ulp, np.abs(got.astype(np.float64) - ref64) / ulp
        print("normalised columns: max %.2f ulp against float32, %.2f ulp against float64" % (err32.max(), err64.max()))
        assert err32.max() <= 1.0 and err64.max() <= 2.0
    # the adjoint: dctx[idx[i]] = dout[i, :H] + dout[n + i, :H], zero elsewhere
    dout = torch.randn(2 * n, H + S, generator=torch.Generator().manual_seed(2)).to(DEV)
    if off:
        dout = _offset((2 * n, H + S), torch.Generator().manual_seed(2), off)
    dctx = O.gail_rows_bwd(dout, idx, tuple(ctx.shape))
    torch.cuda.synchronize()
    ref = torch.zeros(ctx.shape, dtype=torch.float64, device=DEV)
    ref[idx] = dout[:n, :H].double() + dout[n:, :H].double()
    np.testing.assert_array_equal(dctx.cpu().numpy(), ref.float().cpu().numpy())


def test_gail_rows_out_of_range_src_is_an_error_not_a_fault():
    from egopose_amd import optim as O
    n, H, S = 131, 16, 13
    ctx, idx, x, tab, src, mean, inv_std = _rows_case(n, H, S, True)
    for bad in (tab.shape[0], -1):
        src_bad = src.clone()
        src_bad[17] = bad
        with pytest.raises(ValueError, match="no row of the expert table"):
            O.gail_rows(ctx, idx, x, tab, src_bad, mean, inv_std, src_host=src_bad.cpu().numpy())
        # without the host copy the call cannot see the values: the device skips the row and reads nothing out of range
        out = torch.full((2 * n, H + S), 7.0, dtype=torch.float32, device=DEV)
        O.gail_rows(ctx, idx, x, tab, src_bad, mean, inv_std, out=out)
        torch.cuda.synchronize()
        good = O.gail_rows(ctx, idx, x, tab, src, mean, inv_std)
        keep = torch.ones(2 * n, dtype=torch.bool, device=DEV)
        keep[n + 17] = False
        assert torch.equal(out[keep], good[keep])
        assert torch.equal(out[n + 17, :H], good[n + 17, :H]) and bool((out[n + 17, H:] == 7.0).all())


def _softplus64(t):
    return torch.clamp(t, min=0) + torch.log1p(torch.exp(-t.abs()))


def _bce_reference(z, n, n_g, n_e):
    z64 = z.double().reshape(-1).cpu()
    g, e = z64[:n], z64[n:]
    losses = np.array([float(_softplus64(-g).sum() / n_g), float(_softplus64(e).sum() / n_e)])
    dz_scaled = torch.cat((torch.sigmoid(g) - 1.0, torch.sigmoid(e))).numpy()            # dz / inv_n
    return losses, dz_scaled, _softplus64(-g).numpy()


@pytest.mark.parametrize("n", [1, 131, 1000, 70001])
def test_bce_logits_against_float64(n):
    """expf and log1pf are good to a few ulp of 2^-23 ~ 1.2e-7, which leaves a factor of about 50 under rtol 1e-5."""
    from egopose_amd import optim as O
    gen = torch.Generator().manual_seed(100 + n)
    z = (4.0 * torch.randn(2 * n, 1, generator=gen)).clamp_(-12.0, 12.0).to(DEV)
    n_g, n_e = n + 3, 2 * n + 1                                   # global counts of their own: each half divides by its own
    losses, dz, score = O.bce_logits(z, n_g, n_e, want_score=True)
    losses2, _, _ = O.bce_logits(z, n_g, n_e, want_score=True)
    torch.cuda.synchronize()
    ref_l, ref_dz, ref_s = _bce_reference(z, n, n_g, n_e)
    np.testing.assert_allclose(losses.cpu().numpy(), ref_l, rtol=1e-5)
    got = dz.double().reshape(-1).cpu().numpy()
    got[:n] *= n_g
    got[n:] *= n_e
    np.testing.assert_allclose(got, ref_dz, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(score.double().cpu().numpy(), ref_s, rtol=1e-5, atol=1e-7)
    assert torch.equal(losses, losses2)                           # fixed-order float64 sums: two runs are bit-identical
    # dz = NULL: scores only
    l3, dz3, s3 = O.bce_logits(z, n_g, n_e, want_dz=False, want_score=True)
    assert dz3 is None and torch.equal(s3, score) and torch.equal(l3, losses)


def test_bce_logits_beyond_the_sigmoid_s_float32_range():
    """|z| = 30, 90: sigmoid(z) is exactly 0 or 1 in float32 and nn.BCELoss clamps its logarithm at -100; the kernel stays on
    the float64 softplus (~|z|)."""
    from egopose_amd import optim as O
    vals = torch.tensor([30.0, -30.0, 90.0, -90.0])
    z = torch.cat((vals, vals)).reshape(-1, 1).to(DEV)
    losses, dz, score = O.bce_logits(z, 4, 4, want_score=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(dz).all()) and bool(torch.isfinite(score).all())
    ref_l, ref_dz, ref_s = _bce_reference(z, 4, 4, 4)
    np.testing.assert_allclose(losses.cpu().numpy(), ref_l, rtol=1e-5)
    np.testing.assert_allclose(dz.double().reshape(-1).cpu().numpy() * 4, ref_dz, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(score.double().cpu().numpy(), ref_s, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(O.bce_scores(z[:4]).double().cpu().numpy(), ref_s, rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------------------------------------ the agent
def _count(monkeypatch, name):
    from egopose_amd import optim as O
    calls = []
    inner = getattr(O, name)

    def wrapped(*a, **k):
        calls.append(name)
        return inner(*a, **k)
    monkeypatch.setattr(O, name, wrapped)
    return calls


@pytest.mark.parametrize("fixture", V.FIXTURES)
@pytest.mark.parametrize("mode", ["float32", "float64-masters"])
def test_fused_update_discriminator_matches_reference(fixture, mode, monkeypatch):
    g = load_golden(fixture)
    rows_calls, bce_calls = _count(monkeypatch, "gail_rows"), _count(monkeypatch, "bce_logits")
    masters64 = mode == "float64-masters"
    if masters64:
        torch.set_default_dtype(torch.float64)
    try:
        agent, mods = V.build_agent(g, device=DEV, dtype=torch.float64 if masters64 else torch.float32)
        assert agent.cdtype == torch.float32 and (agent.shadow is not None) == masters64
        e_loss = V.run_update(agent, g, DEV, torch.float32)
        torch.cuda.synchronize()
        assert len(rows_calls) == 10 and len(bce_calls) == 10, "the fused form did not run: %r %r" % (rows_calls, bce_calls)
        assert agent._get_discrim_updater() is not None
        print("e_loss %.9g against %.9g" % (e_loss, float(g["e_loss"])))
        check_final(mods, g, **V.F32)
        np.testing.assert_allclose(e_loss, float(g["e_loss"]), rtol=1e-4)
        want = torch.float64 if masters64 else torch.float32
        assert all(v.dtype == want for m in mods.values() for v in m.state_dict().values())
        if masters64:
            for m, s in agent.shadow.pairs:
                assert torch.equal(s, m.float())
    finally:
        torch.set_default_dtype(torch.float32)


@pytest.mark.parametrize("fixture", V.FIXTURES)
def test_plain_update_discriminator_float64_on_device(fixture, monkeypatch):
    monkeypatch.setenv("EGP_NET_DTYPE", "float64")
    g = load_golden(fixture)
    rows_calls = _count(monkeypatch, "gail_rows")
    torch.set_default_dtype(torch.float64)
    try:
        agent, mods = V.build_agent(g, device=DEV)
        assert agent.shadow is None and agent.cdtype == torch.float64
        e_loss = V.run_update(agent, g, DEV)
        assert not rows_calls
        check_final(mods, g, rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(e_loss, float(g["e_loss"]), rtol=1e-9)
    finally:
        torch.set_default_dtype(torch.float32)


def _state(mods):
    return {"%s.%s" % (n, k): v.detach().clone() for n, m in mods.items() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("fixture", V.FIXTURES)
def test_fused_against_plain_with_a_binding_clip(fixture, monkeypatch):
    """discrim_grad_clip = 0.05 binds on every step (the unclipped norms are 0.1 .. 0.5): both forms clip discrim_net's
    gradient only, and agree under the float32 criterion."""
    g = load_golden(fixture)
    rows_calls = _count(monkeypatch, "gail_rows")
    out = {}
    for fused in (False, True):
        agent, mods = V.build_agent(g, device=DEV, dtype=torch.float32, discrim_grad_clip=0.05)
        agent.use_fused_discrim = fused
        n0 = len(rows_calls)
        V.run_update(agent, g, DEV, torch.float32)
        assert len(rows_calls) - n0 == (10 if fused else 0)
        st = agent.discrim_stats
        print("fused" if fused else "plain", st)
        assert st["grad_norm"] > 0.05 and st["clipped_norm"] <= 0.05 * (1 + 1e-5)
        out[fused] = _state(mods)
    bad, crit = 0, V.F32
    for k, ref in out[False].items():
        got, ref = out[True][k].double().cpu().numpy(), ref.double().cpu().numpy()
        miss = ~np.isclose(got, ref, rtol=crit["rtol"], atol=crit["atol"])
        if miss.any():
            assert np.abs(got - ref)[miss].max() <= crit["outlier_atol"], k
            bad += int(miss.sum())
    assert bad <= crit["max_outliers"], "%d elements differ between the fused and the plain form" % bad


@pytest.fixture(scope="module")
def kctx(skel):
    from egopose_amd.hip import EgpContext
    c = load_golden("config_subject_03.npz")
    ctx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"])
    yield ctx
    ctx.close()


def _full_agent(g, kctx, **kw):
    agent, mods = V.build_agent(g, device=DEV, dtype=torch.float32, **kw)
    agent._kernel_ctx = lambda: kctx
    ppo = dict(p=agent.policy_net, v=agent.value_net, p_vs=agent.policy_vs_net, v_vs=agent.value_vs_net)
    return agent, mods, ppo


def test_update_params_is_the_ppo_update_followed_by_the_discriminator_update(kctx):
    from egopose_amd.agent import AgentEgo
    g = load_golden("vgail.npz")
    batch = V.ppo_batch(g)
    a, a_d, a_ppo = _full_agent(g, kctx)
    t = a.update_params(batch)
    b, b_d, b_ppo = _full_agent(g, kctx)
    AgentEgo.update_params(b, batch)
    e_loss = V.run_update(b, g, DEV, torch.float32)
    torch.cuda.synchronize()
    assert t > 0 and a.last_e_loss == e_loss
    moved = 0
    for (k, va), vb in zip(_state(a_ppo).items(), _state(b_ppo).values()):
        assert torch.equal(va, vb), k
    for (k, va), vb in zip(_state(a_d).items(), _state(b_d).values()):
        assert torch.equal(va, vb), k
        moved += int((va.double().cpu().numpy() != g["init_" + k.replace(".", "__", 1)]).sum())
    assert moved > 0


def _spy_rewards(agent):
    seen = []
    inner = agent._advantages

    def adv_fn(rewards, masks, values):
        seen.append(rewards.detach().clone())
        return inner(rewards, masks, values)
    agent._advantages = adv_fn
    return seen


def _spy_scores(agent):
    calls = []
    inner = agent.discriminator_scores

    def scores(batch):
        calls.append(1)
        return inner(batch)
    agent.discriminator_scores = scores
    return calls


def test_discriminator_reward_weight(kctx):
    g = load_golden("vgail.npz")
    batch = V.ppo_batch(g)
    r = torch.as_tensor(np.asarray(batch.rewards), dtype=torch.float32, device=DEV)
    # w = 0.5: GAE sees the mixed rewards
    agent, mods, _ = _full_agent(g, kctx, discrim_reward_weight=0.5)
    scores = agent.discriminator_scores(batch)
    assert scores.shape == r.shape and scores.dtype == torch.float32
    states, masks, v_metas = V.inputs(g, DEV, torch.float32)
    with torch.no_grad():                                         # -log D(vs(s)) in torch ops, float64
        vs, dn = mods["d_vs"], mods["d"]
        vs.set_mode("train")
        vs.initialize((masks, agent.env.cnn_feat, v_metas))
        ref = -torch.log(dn(vs(states)).double()).reshape(-1)
    np.testing.assert_allclose(scores.double().cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-6)
    seen, calls = _spy_rewards(agent), _spy_scores(agent)
    agent.update_params(batch)
    assert len(seen) == 1 and len(calls) == 1
    np.testing.assert_allclose(seen[0].double().cpu().numpy(), (0.5 * r.double() + 0.5 * scores.double()).cpu().numpy(), rtol=0, atol=1e-6)
    # w = 0: the reward column as it is, and no discriminator pass before GAE
    agent0, _, _ = _full_agent(g, kctx)
    seen0, calls0 = _spy_rewards(agent0), _spy_scores(agent0)
    agent0.update_params(batch)
    assert len(seen0) == 1 and not calls0
    assert torch.equal(seen0[0], r)


def test_two_identical_updates_are_bit_identical():
    g = load_golden("vgail_wide.npz")
    runs = []
    for _ in range(2):
        agent, mods = V.build_agent(g, device=DEV, dtype=torch.float32)
        e_loss = V.run_update(agent, g, DEV, torch.float32)
        runs.append((e_loss, _state(mods)))
    assert runs[0][0] == runs[1][0]
    for k, v in runs[0][1].items():
        assert torch.equal(v, runs[1][1][k]), k


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def workspace(tmp_path_factory):
    from egopose_amd.bench_support import write_synthetic_dataset
    root = str(tmp_path_factory.mktemp("egp_vgail_ws"))
    write_synthetic_dataset(root, "subject_03", n_takes=3, n_frames=120, seed=4)
    return root


def test_trainer_with_gail_two_iterations_and_checkpoint(workspace, tmp_path):
    from egopose_amd.config import Config
    from egopose_amd.train import Trainer
    os.chdir(workspace)
    cfg = Config("subject_03", create_dirs=False)
    cfg.env_episode_len = 10
    cfg.num_optim_epoch = 1
    trainers = []
    try:
        tr = Trainer(cfg, torch.device("cuda", 0), torch.float32, num_envs=8, num_threads=2, num_groups=1, gail={})
        trainers.append(tr)
        from egopose_amd.agent import AgentVGAIL
        assert isinstance(tr.agent, AgentVGAIL)
        before = {k: v.detach().clone() for k, v in list(tr.discrim_net.state_dict().items()) + list(tr.discrim_vs_net.state_dict().items())}
        for it in range(2):
            log, _, _, n_steps = tr.iteration(it, 8 * 10)
            assert n_steps >= 80 and np.isfinite(log.avg_c_reward) and np.isfinite(tr.agent.last_e_loss)
            assert all(np.isfinite(v).all() for v in tr.agent.update_stats.values())
        after = {k: v.detach().clone() for k, v in list(tr.discrim_net.state_dict().items()) + list(tr.discrim_vs_net.state_dict().items())}
        assert all(bool(torch.isfinite(v).all()) for v in after.values())
        assert any(not torch.equal(before[k], after[k]) for k in before), "the discriminator's parameters did not move"
        path = str(tmp_path / "iter_0002.p")
        tr.save(path)
        for net in (tr.discrim_net, tr.discrim_vs_net):
            with torch.no_grad():
                for p in net.parameters():
                    p.zero_()
        tr.load(path)
        now = dict(list(tr.discrim_net.state_dict().items()) + list(tr.discrim_vs_net.state_dict().items()))
        for k in after:
            assert torch.equal(now[k], after[k]), k
        # the expert's rows: "reference" (gen_expert.py never sets qvel) has zero velocity columns, "fd" has not
        nq = tr.env.skel.nq
        rows_ref = np.concatenate(tr.agent._expert_obs_host()[0], 0)
        assert rows_ref.shape[1] == tr.env.obs_dim and not rows_ref[:, nq - 2:].any() and rows_ref[:, :nq - 2].any()
        tr.close()
        trainers.pop()
        tr_fd = Trainer(cfg, torch.device("cuda", 0), torch.float32, num_envs=8, num_threads=2, num_groups=1, gail=dict(expert_obs="fd"))
        trainers.append(tr_fd)
        rows_fd = np.concatenate(tr_fd.agent._expert_obs_host()[0], 0)
        assert rows_fd[:, nq - 2:].any()
        np.testing.assert_array_equal(rows_fd[:, :nq - 2], rows_ref[:, :nq - 2])
    finally:
        for tr in trainers:
            tr.close()
