"""Shared set-up of the mini-batch PPO parity tests (CPU and GPU): rebuild the plain `AgentPPO` of a golden run of the
reference's `AgentPPO.update_params(use_mini_batch=True)` (tests/golden/ppo_minibatch*.npz, tools/gen_golden_minibatch.py)
from the fixture's initial parameters and hyper-parameters."""
import types

import numpy as np
import torch

from egopose_amd.agent import AgentPPO
from egopose_amd.nets import MLP, PolicyGaussian, Value
from oracle.gae import estimate_advantages as oracle_gae

FIXTURES = ("ppo_minibatch.npz", "ppo_minibatch_wide.npz")


def hyper(g):
    h = g["hyper"]
    return dict(lr_p=float(h[0]), lr_v=float(h[1]), clip=float(h[2]), epochs=int(h[3]), gamma=float(h[4]), tau=float(h[5]),
                eps=float(h[6]), log_std=float(h[7]))


def _sd(g, prefix, dtype):
    return {k[len(prefix):]: torch.as_tensor(np.asarray(g[k])).to(dtype) for k in g.files if k.startswith(prefix)}


def build_agent(g, device="cpu", dtype=torch.float64, net_dtype=None, **kw):
    sdim, adim, batch, h0, h1 = [int(x) for x in g["dims"]]
    hp = hyper(g)
    p_net = PolicyGaussian(MLP(sdim, [h0, h1], "relu"), adim, log_std=hp["log_std"], fix_std=False)
    v_net = Value(MLP(sdim, [h0, h1], "relu"))
    mods = dict(p=p_net, v=v_net)
    for name, mod in mods.items():
        mod.load_state_dict(_sd(g, "init_%s__" % name, dtype), strict=True)
        mod.to(dtype).to(device)
    p_params = list(p_net.parameters())
    args = dict(env=types.SimpleNamespace(cfg=types.SimpleNamespace(seed=1)), dtype=dtype, device=torch.device(device), running_state=None,
                custom_reward=None, mean_action=False, render=False, num_threads=1, policy_net=p_net, value_net=v_net,
                optimizer_policy=torch.optim.Adam(p_params, lr=hp["lr_p"]), optimizer_value=torch.optim.Adam(v_net.parameters(), lr=hp["lr_v"]),
                opt_num_epochs=hp["epochs"], gamma=hp["gamma"], tau=hp["tau"], clip_epsilon=hp["eps"],
                policy_grad_clip=[(p_params, hp["clip"])], opt_batch_size=batch, use_mini_batch=True, net_dtype=net_dtype)
    args.update(kw)
    return AgentPPO(**args), mods


def batch_of(g):
    f64 = lambda k: np.asarray(g[k], np.float64)
    return types.SimpleNamespace(states=f64("states"), actions=f64("actions"), rewards=f64("rewards"), masks=np.asarray(g["masks"]),
                                 exps=np.asarray(g["exps"]))


def with_oracle_gae(agent):
    """The GAE kernel is HIP-only: on the CPU the oracle's GAE stands in for K5 (test infrastructure, as in test_agent_update_cpu.py)."""
    def adv_fn(rewards, masks, values):
        a, r, _ = oracle_gae(rewards.cpu().numpy(), masks.cpu().numpy(), values.cpu().numpy(), agent.gamma, agent.tau)
        agent._seen = (a, r, values.cpu().numpy())
        return torch.as_tensor(a, device=rewards.device), torch.as_tensor(r, device=rewards.device)
    agent._advantages = adv_fn
    return agent


def run_update(agent, g):
    """update_params with NumPy's global generator seeded as the golden run's was."""
    np.random.seed(int(g["np_seed"]))
    agent.update_params(batch_of(g))


def misses(mods, g, rtol, atol):
    """(number of parameter elements outside the tolerance, the largest absolute difference among them, all elements)."""
    bad, worst, total = 0, 0.0, 0
    for name, mod in mods.items():
        for k, v in mod.state_dict().items():
            got, ref = v.detach().double().cpu().numpy(), g["final_%s__%s" % (name, k)]
            miss = ~np.isclose(got, ref, rtol=rtol, atol=atol)
            total += got.size
            if miss.any():
                bad += int(miss.sum())
                worst = max(worst, float(np.abs(got - ref)[miss].max()))
    return bad, worst, total
