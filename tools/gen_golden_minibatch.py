#!/usr/bin/env python3
"""Mini-batch PPO fixtures: the reference's AgentPPO.update_params with use_mini_batch=True, float64 on the CPU.

Imports the reference exactly as tools/gen_golden.py does (same stubs for the absent third-party modules, nothing copied)
and records one run of `AgentPPO.update_params` (agents/agent_pg.py:40-57 -> agents/agent_ppo.py:16-44) with plain MLP nets
(identity trans_policy / trans_value, learnable action_log_std):

    tests/golden/ppo_minibatch.npz        N = 131 rows in 3 episodes, opt_batch_size 64 (windows of 64, 64, 3), D = 13, A = 5.
                                          The shuffle seed is searched until one window of one epoch holds no exploration
                                          row (`empty_window` = epoch, window): what the reference does there -- NaN loss,
                                          all-zero policy gradient, an Adam step on it -- is part of the recorded run
    tests/golden/ppo_minibatch_wide.npz   N = 450, opt_batch_size 200 (200, 200, 50), D = 76, A = 17

Stored: the inputs (float32-representable), initial and final parameters of both nets, the permutation every epoch drew
(`perms`, from np.random.seed(`np_seed`)), values0 / adv0 / ret0, and per mini-batch the surrogate loss and the largest
absolute policy gradient the reference saw. Runs where the reference is available only. Own seeds.
"""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_golden as G          # noqa: E402  (stubs + workdir helpers)


def _windows_without_exploration(exps, perms, batch):
    """[(epoch, window)] whose rows all have exps == 0, following the reference's composition of the epochs' shuffles."""
    n, cur, out = exps.shape[0], np.arange(exps.shape[0]), []
    for e, perm in enumerate(perms):
        cur = cur[perm]
        for i in range((n + batch - 1) // batch):
            if not exps[cur[i * batch:(i + 1) * batch]].any():
                out.append((e, i))
    return out


def _draw_perms(seed, n, epochs):
    np.random.seed(seed)
    perms = []
    for _ in range(epochs):
        perm = np.arange(n)
        np.random.shuffle(perm)
        perms.append(perm)
    return perms


def main(out_name, ep_lens, sdim, adim, batch, seed_data, seed_torch, want_empty, epochs=3, hidden=(32, 32), p_zero=0.4,
         lr_p=1e-3, lr_v=2e-3, clip=0.5, gamma=0.95, tau=0.95, eps=0.2, log_std=-1.0):
    G.install_stubs()
    if G.REF not in sys.path:
        sys.path.insert(0, G.REF)
    G.enter_workdir()
    import torch
    torch.set_default_dtype(torch.float64)
    import utils as _ru          # noqa: F401  (reference utils: star exports the agents rely on)
    from core.common import estimate_advantages
    from core.policy_gaussian import PolicyGaussian
    from core.critic import Value
    from models.mlp import MLP
    from agents.agent_ppo import AgentPPO

    rng = np.random.RandomState(seed_data)
    torch.manual_seed(seed_torch)
    p_net = PolicyGaussian(MLP(sdim, list(hidden), 'relu'), adim, log_std=log_std, fix_std=False)
    v_net = Value(MLP(sdim, list(hidden), 'relu'))
    mods = [("p", p_net), ("v", v_net)]
    with torch.no_grad():        # initial parameters exactly representable in float32: both precisions start equal
        for _, mod in mods:
            for p in mod.parameters():
                p.copy_(p.float().double())
    init_np = {"init_%s__%s" % (a, k): v.numpy().astype(np.float32) for a, mod in mods for k, v in mod.state_dict().items()}
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    rows = dict(states=[], actions=[], masks=[], rewards=[], exps=[])
    for L_ep in ep_lens:
        for k in range(L_ep):
            rows['states'].append(f32(rng.normal(size=sdim)))
            rows['actions'].append(f32(rng.normal(size=adim) * 0.5))
            rows['masks'].append(0 if k == L_ep - 1 else 1)
            rows['rewards'].append(float(np.float32(rng.uniform(0, 1))))
            rows['exps'].append(0 if rng.uniform() < p_zero else 1)
    batch_np = types.SimpleNamespace(**{k: np.array(v) for k, v in rows.items()})
    n = len(batch_np.masks)
    np_seed, empty = 0, []
    while True:
        empty = _windows_without_exploration(batch_np.exps, _draw_perms(np_seed, n, epochs), batch)
        if empty or not want_empty:
            break
        np_seed += 1
    perms = _draw_perms(np_seed, n, epochs)

    p_params = list(p_net.parameters())
    agent = AgentPPO(env=None, dtype=torch.float64, device=torch.device('cpu'), running_state=None, custom_reward=None,
                     mean_action=False, render=False, num_threads=1, policy_net=p_net, value_net=v_net,
                     optimizer_policy=torch.optim.Adam(p_params, lr=lr_p), optimizer_value=torch.optim.Adam(v_net.parameters(), lr=lr_v),
                     opt_num_epochs=epochs, gamma=gamma, tau=tau, clip_epsilon=eps, policy_grad_clip=[(p_params, clip)],
                     opt_batch_size=batch, use_mini_batch=True)
    st_t, rw_t = torch.from_numpy(batch_np.states), torch.from_numpy(batch_np.rewards)
    mk_t = torch.from_numpy(batch_np.masks).to(torch.float64)
    with torch.no_grad():
        values0 = v_net(st_t)
        adv0, ret0 = estimate_advantages(rw_t, mk_t, values0, gamma, tau)
    # what the reference sees per mini-batch: its own ppo_loss / clip_policy_grad, observed from outside
    surr, gmax = [], []
    inner_loss, inner_clip = agent.ppo_loss, agent.clip_policy_grad

    def ppo_loss(*a, **k):
        out = inner_loss(*a, **k)
        surr.append(float(out.detach()))
        return out

    def clip_policy_grad():
        gmax.append(max(float(p.grad.abs().max()) for p in p_params))
        return inner_clip()
    agent.ppo_loss, agent.clip_policy_grad = ppo_loss, clip_policy_grad
    np.random.seed(np_seed)
    agent.update_params(batch_np)
    final_np = {"final_%s__%s" % (a, k): v.detach().numpy().copy() for a, mod in mods for k, v in mod.state_dict().items()}
    n_iter = (n + batch - 1) // batch
    assert len(surr) == epochs * n_iter == len(gmax)
    for e, i in empty:
        print("window without exploration rows: epoch %d window %d -> surr_loss %r, max |policy grad| %r" % (e, i, surr[e * n_iter + i], gmax[e * n_iter + i]))
    out = os.path.join(G.OUT, out_name)
    np.savez_compressed(
        out, states=batch_np.states.astype(np.float32), actions=batch_np.actions.astype(np.float32), masks=batch_np.masks,
        rewards=batch_np.rewards.astype(np.float32), exps=batch_np.exps, perms=np.stack(perms), np_seed=np.array(np_seed),
        empty_window=np.array(empty[0] if empty else (-1, -1)), surr_loss=np.array(surr).reshape(epochs, n_iter),
        policy_grad_absmax=np.array(gmax).reshape(epochs, n_iter),
        values0=values0.numpy(), adv0=adv0.numpy(), ret0=ret0.numpy(),
        dims=np.array([sdim, adim, batch, hidden[0], hidden[1]]), hyper=np.array([lr_p, lr_v, clip, epochs, gamma, tau, eps, log_std]),
        **init_np, **final_np)
    print("wrote", out, "%.0f kB" % (os.path.getsize(out) / 1e3), "N =", n, "np_seed =", np_seed, "exps == 0: %.0f %%" % (100 * (1 - batch_np.exps.mean())))


if __name__ == "__main__":
    main("ppo_minibatch.npz", ep_lens=[50, 47, 34], sdim=13, adim=5, batch=64, seed_data=3101, seed_torch=31, want_empty=True)
    main("ppo_minibatch_wide.npz", ep_lens=[150, 180, 120], sdim=76, adim=17, batch=200, seed_data=3102, seed_torch=32, want_empty=False)
