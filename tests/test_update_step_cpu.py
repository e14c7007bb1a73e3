"""The update-step protocol on the CPU: optim.TorchUpdater (zero_grad / collect_grads / all_reduce / step / grad_norm) against
the same sequence written out by hand, bit for bit, and the agent's one call of the `clip_policy_grad` hook per policy step."""
import pytest
import torch

from conftest import load_golden
from egopose_amd.agent import ShadowNets
from egopose_amd.optim import TorchUpdater
from oracle.gae import estimate_advantages as oracle_gae
from update_fixture import batch_of, build_agent, hyper

MAX_NORM = 0.1          # binds on every step (asserted below)


def _setup(shadowed):
    """Two Linear(3, 2) under one Adam each (float64), the nets that compute (themselves, or float32 shadows), data."""
    gen = torch.Generator().manual_seed(3)
    nets = [torch.nn.Linear(3, 2).double() for _ in range(2)]
    with torch.no_grad():
        for net in nets:
            for p in net.parameters():
                p.copy_(torch.randn(p.shape, generator=gen, dtype=torch.float64))
    opts = [torch.optim.Adam(net.parameters(), lr=1e-2) for net in nets]
    shadow = ShadowNets(dict(a=nets[0], b=nets[1]), torch.float32) if shadowed else None
    compute = [shadow.nets["a"], shadow.nets["b"]] if shadowed else nets
    dt = torch.float32 if shadowed else torch.float64
    x, y = torch.randn(7, 3, generator=gen, dtype=torch.float64).to(dt), torch.randn(7, 2, generator=gen, dtype=torch.float64).to(dt)
    loss = lambda: sum((net(x) - y).pow(2).sum() for net in compute)
    return nets, opts, shadow, loss


def _clip(net):
    return lambda: torch.nn.utils.clip_grad_norm_(net.parameters(), MAX_NORM)


def _everything(nets, opts, shadow):
    out = [p.detach().clone() for net in nets for p in net.parameters()]
    out += [opt.state[p][k].clone() for opt in opts for g in opt.param_groups for p in g["params"] for k in ("step", "exp_avg", "exp_avg_sq")]
    if shadow is not None:
        out += [s.detach().clone() for _, s in shadow.pairs]
    return out


@pytest.mark.parametrize("shadowed", [False, True])
def test_torch_updater_equals_the_sequence_written_out(shadowed):
    nets, opts, shadow, loss = _setup(shadowed)
    up = TorchUpdater(opts, shadow, {1: _clip(nets[1])})
    assert up.grad_norm(1) is None                      # no step yet
    got = []
    for _ in range(3):
        up.zero_grad()
        loss().backward()
        up.collect_grads()
        up.all_reduce()
        up.step()
        got.append(up.grad_norm(1).clone())
    up.rebind()
    nets_r, opts_r, shadow_r, loss_r = _setup(shadowed)
    want = []
    for _ in range(3):
        for opt in opts_r:
            opt.zero_grad()
        if shadowed:
            shadow_r.zero_grad()
        loss_r().backward()
        if shadowed:
            shadow_r.push_grads()
        opts_r[0].step()
        want.append(torch.nn.utils.clip_grad_norm_(nets_r[1].parameters(), MAX_NORM).clone())
        opts_r[1].step()
        if shadowed:
            shadow_r.pull()
    assert all(float(n) > MAX_NORM for n in want), "the clip must bind"
    assert all(n.dim() == 0 and torch.equal(n, w) for n, w in zip(got, want))
    a, b = _everything(nets, opts, shadow), _everything(nets_r, opts_r, shadow_r)
    assert len(a) == len(b) and all(t.dtype == r.dtype and torch.equal(t, r) for t, r in zip(a, b))
    if shadowed:
        assert all(m.dtype == torch.float64 and s.dtype == torch.float32 and torch.equal(s, m.float()) for m, s in shadow.pairs)


def test_step_steps_the_optimizers_named_in_which_only():
    nets, opts, _, loss = _setup(False)
    calls = []
    up = TorchUpdater(opts, None, {1: lambda: calls.append(1)})
    before = [p.detach().clone() for p in nets[1].parameters()]
    up.zero_grad()
    loss().backward()
    up.collect_grads((0,))
    up.all_reduce((0,))
    up.step((0,))
    assert calls == [] and len(opts[1].state) == 0 and len(opts[0].state) == 2
    assert all(torch.equal(p, b) for p, b in zip(nets[1].parameters(), before))
    first = [p.detach().clone() for p in nets[0].parameters()]
    up.step((1,))
    assert calls == [1] and len(opts[1].state) == 2
    assert all(torch.equal(p, b) for p, b in zip(nets[0].parameters(), first))
    assert not any(torch.equal(p, b) for p, b in zip(nets[1].parameters(), before))


def test_grad_norm_without_a_clip_is_none():
    nets, opts, _, loss = _setup(False)
    up = TorchUpdater(opts)
    up.zero_grad()
    loss().backward()
    up.step()
    assert up.grad_norm(1) is None and up.grad_norm(2) is None
    clipped = TorchUpdater(opts, None, {1: _clip(nets[1])})
    assert clipped.grad_norm(0) is None and clipped.grad_norm(2) is None


def test_agent_calls_the_clip_hook_once_per_policy_step():
    g = load_golden("ppo_update.npz")
    torch.set_default_dtype(torch.float64)
    try:
        agent, _ = build_agent(g)

        def adv_fn(rewards, masks, values):
            a, r, _ = oracle_gae(rewards.cpu().numpy(), masks.cpu().numpy(), values.cpu().numpy(), agent.gamma, agent.tau)
            return torch.as_tensor(a), torch.as_tensor(r)
        agent._advantages = adv_fn
        calls, inner = [], agent.clip_policy_grad
        agent.clip_policy_grad = lambda: (calls.append(1), inner())[1]
        agent.update_params(batch_of(g))
        assert len(calls) == agent.opt_num_epochs == hyper(g)["epochs"] > 1
        assert isinstance(agent._get_stepper(), TorchUpdater) and agent._get_updater() is None
    finally:
        torch.set_default_dtype(torch.float32)
