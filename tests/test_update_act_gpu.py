"""The assembled update with tanh / sigmoid MLPs against a golden run of the reference's `AgentEgo.update_params` with a tanh
policy MLP and a sigmoid value MLP (tests/golden/ppo_update_act.npz, tools/gen_golden_act.py):

  * float64 on the CPU (the oracle's GAE standing in for K5)       -> the float64 tolerances of tests/test_update_gpu.py
  * float32 on the HIP path                                        -> that file's float32 criterion: rtol 1e-4, atol 3e-6, at
    most 8 parameter elements outside it, none beyond 1.3e-2; and no MLP layer's nn.Linear.forward is entered: every product
    of both heads runs in egp_gemm_f32, with the activation and its derivative in the epilogues
  * the other update forms once each with a tanh net, at the small shapes of minibatch_fixture.py / vgail_fixture.py: the fused
    mini-batch epochs (use_mini_batch=True) and the fused discriminator step -- finite numbers, no nn.Linear.forward either.
"""
import numpy as np
import pytest
import torch

import minibatch_fixture as MB
import vgail_fixture as V
from act_fixture import FIXTURE, build_agent, mlp_linears, watch_linears
from conftest import load_golden
from oracle.gae import estimate_advantages as oracle_gae
from update_fixture import batch_of, check_final

gpu = pytest.mark.gpu


def test_update_params_float64_on_the_cpu_matches_reference():
    g = load_golden(FIXTURE)
    assert (str(g["policy_htype"]), str(g["value_htype"])) == ("tanh", "sigmoid")
    torch.set_default_dtype(torch.float64)
    try:
        agent, mods = build_agent(g)
        assert mods["p"].net.activation is torch.tanh and mods["v"].net.activation is torch.sigmoid

        def adv_fn(rewards, masks, values):
            a, r, _ = oracle_gae(rewards.cpu().numpy(), masks.cpu().numpy(), values.cpu().numpy(), agent.gamma, agent.tau)
            agent._seen = (a, r, values.cpu().numpy())
            return torch.as_tensor(a), torch.as_tensor(r)
        agent._advantages = adv_fn
        agent.update_params(batch_of(g))
        a, r, v0 = agent._seen
        np.testing.assert_allclose(v0, g["values0"], rtol=1e-10, atol=1e-11)
        np.testing.assert_allclose(a, g["adv0"], rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(r, g["ret0"], rtol=1e-10, atol=1e-11)
        check_final(mods, g, rtol=1e-9, atol=1e-10)
    finally:
        torch.set_default_dtype(torch.float32)


@pytest.fixture(scope="module")
def kctx(skel):
    from egopose_amd.hip import EgpContext
    c = load_golden("config_subject_03.npz")
    ctx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"])
    yield ctx
    ctx.close()


def _with_k5(agent, kctx):
    agent._kernel_ctx = lambda: kctx
    inner = agent._advantages

    def adv_fn(rewards, masks, values):
        adv, ret = inner(rewards, masks, values)
        agent._seen = (adv.double().cpu().numpy(), ret.double().cpu().numpy(), values.double().cpu().numpy())
        return adv, ret
    agent._advantages = adv_fn


@gpu
def test_update_params_float32_hip_path_matches_reference(kctx, monkeypatch):
    from egopose_amd import gemm as G
    monkeypatch.setenv("EGP_GEMM", "hip")
    monkeypatch.setenv("EGP_GEMM_TERMS", "6")
    g = load_golden(FIXTURE)
    agent, mods = build_agent(g, device="cuda", dtype=torch.float32, fused_adam=True)
    assert agent.cdtype == torch.float32 and agent.shadow is None
    x = torch.zeros(4, mods["p"].net.affine_layers[0].in_features, device="cuda")
    assert G.mlp_head_available(x, mods["p"].net.affine_layers, mods["p"].action_mean, torch.tanh)
    assert G.mlp_head_available(x, mods["v"].net.affine_layers, mods["v"].value_head, torch.sigmoid)
    feats = [np.asarray(g["cnn_feat0"], np.float64), np.asarray(g["cnn_feat1"], np.float64)]
    table = torch.as_tensor(np.concatenate(feats, 0), dtype=torch.float32, device="cuda")
    for net in (agent.cn.policy_vs_net, agent.cn.value_vs_net):
        net.attach_feature_table(table, [0, feats[0].shape[0]])
    _with_k5(agent, kctx)
    entered = watch_linears(monkeypatch, mlp_linears(mods["p"], mods["v"], agent.cn.policy_net, agent.cn.value_net))
    agent.update_params(batch_of(g))
    torch.cuda.synchronize()
    assert entered == [], "the MLPs left the HIP path: nn.Linear.forward entered on %r" % (entered,)
    a, r, v0 = agent._seen
    np.testing.assert_allclose(v0, g["values0"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(r, g["ret0"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(a, g["adv0"], rtol=1e-4, atol=1e-4)
    bad = check_final(mods, g, rtol=1e-4, atol=3e-6, max_outliers=8, outlier_atol=1.3e-2)
    print("  %d parameter elements outside (rtol 1e-4, atol 3e-6)" % bad)


def _finite(mods):
    return all(bool(torch.isfinite(v).all()) for m in mods.values() for v in m.state_dict().values())


@gpu
def test_fused_minibatch_update_with_a_tanh_net(kctx, monkeypatch):
    from egopose_amd import optim as O
    monkeypatch.setenv("EGP_GEMM", "hip")
    g = load_golden(MB.FIXTURES[0])
    agent, mods = MB.build_agent(g, device="cuda", dtype=torch.float32)
    for m in mods.values():
        m.net.activation = torch.tanh
    before = {k: v.clone() for k, v in mods["p"].state_dict().items()}
    assert agent._fused_losses()
    _with_k5(agent, kctx)
    calls, inner = [], O.ppo_losses_mb
    monkeypatch.setattr(O, "ppo_losses_mb", lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    entered = watch_linears(monkeypatch, mlp_linears(mods["p"], mods["v"], agent.cn.policy_net, agent.cn.value_net))
    MB.run_update(agent, g)
    torch.cuda.synchronize()
    epochs, n_iter = g["surr_loss"].shape
    assert len(calls) == epochs * n_iter, "the fused mini-batch epochs did not run"
    assert entered == [], entered
    assert _finite(mods) and any(not torch.equal(v, before[k]) for k, v in mods["p"].state_dict().items())
    assert np.isfinite(np.asarray(agent.update_stats["value_loss"])).all()


@gpu
def test_fused_discriminator_step_with_a_tanh_trunk(monkeypatch):
    from egopose_amd import optim as O
    monkeypatch.setenv("EGP_GEMM", "hip")
    g = load_golden(V.FIXTURES[0])
    agent, mods = V.build_agent(g, device="cuda", dtype=torch.float32)
    mods["d"].net.activation = torch.tanh
    before = {k: v.clone() for k, v in mods["d"].state_dict().items()}
    calls, inner = [], O.bce_logits
    monkeypatch.setattr(O, "bce_logits", lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    entered = watch_linears(monkeypatch, mlp_linears(mods["d"], agent.cn.discrim_net))
    e_loss = V.run_update(agent, g, "cuda", torch.float32)
    torch.cuda.synchronize()
    assert len(calls) == int(g["hyper"][1]), "the fused discriminator step did not run"
    assert entered == [], entered
    assert np.isfinite(e_loss) and _finite(mods) and any(not torch.equal(v, before[k]) for k, v in mods["d"].state_dict().items())
