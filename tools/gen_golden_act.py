#!/usr/bin/env python3
"""PPO update fixture with the two activations the shipped configs do not use: the reference's AgentEgo.update_params with a
tanh policy MLP and a sigmoid value MLP, float64 on the CPU.

Imports the reference exactly as tools/gen_golden.py does (same stubs for the absent third-party modules, nothing copied) and
records one run of `AgentEgo.update_params` (ego_pose/core/agent_ego.py:34-57 -> agents/agent_ppo.py:16-65) with
`PolicyGaussian(MLP(., [12, 10], 'tanh'))` and `Value(MLP(., [12, 10], 'sigmoid'))` (models/mlp.py:12-17) behind two
VideoStateNets, at about the dims of tests/golden/ppo_update.npz (tools/gen_golden.py, G9):

    tests/golden/ppo_update_act.npz   70 rows in 10 ragged episodes, 9 state columns, 4 actions, cnn_feat_dim 6, v_hdim 8,
                                      margin 2; the layout of ppo_update.npz (inputs, values0 / adv0 / ret0 / logp0, `dims`,
                                      initial and final parameters) + `hyper` + `policy_htype` / `value_htype`

Inputs and initial parameters are float32-representable (stored as float32), so that a float32 run starts from the same numbers.

Before the fixture is written the same reference code runs in float32 on the CPU and must stay inside the float32 criterion
the GPU test uses (tests/test_update_act_gpu.py: at most 8 parameter elements outside rtol 1e-4 / atol 3e-6, none beyond
1.3e-2): a criterion the reference itself does not meet in float32 would test nothing. The count found is printed; a run
outside it refuses to write (choose another seed). With the seeds below the float32 reference misses on 0 elements.
Runs where the reference is available only. Own seeds.
"""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_golden as G          # noqa: E402  (stubs + workdir helpers)

CRITERION = dict(rtol=1e-4, atol=3e-6, max_outliers=8, outlier_atol=1.3e-2)
MODS = ("p_vs", "v_vs", "p", "v")


def _run(torch, dtype, data, init, dims, hidden, htypes, hp):
    """One update_params of the reference in `dtype` from the initial parameters `init` (None: freshly initialised ones,
    rounded to float32) -> (init, final, the quantities before the update)."""
    from core.common import estimate_advantages
    from core.critic import Value
    from core.policy_gaussian import PolicyGaussian
    from ego_pose.core.agent_ego import AgentEgo
    from models.mlp import MLP
    from models.video_state_net import VideoStateNet
    import copy
    sdim, adim, cdim, hdim, margin, T_ep = dims
    torch.set_default_dtype(dtype)
    p_vs = VideoStateNet(cdim, hdim, margin, 'lstm', None, False)
    v_vs = VideoStateNet(cdim, hdim, margin, 'lstm', None, False)
    p_net = PolicyGaussian(MLP(sdim + hdim, list(hidden), htypes[0]), adim, log_std=hp["log_std"], fix_std=True)
    v_net = Value(MLP(sdim + hdim, list(hidden), htypes[1]))
    mods = list(zip(MODS, (p_vs, v_vs, p_net, v_net)))
    if init is not None:
        for name, mod in mods:
            pre = "init_%s__" % name
            mod.load_state_dict({k[len(pre):]: torch.as_tensor(v).to(dtype) for k, v in init.items() if k.startswith(pre)})
    else:
        with torch.no_grad():        # initial parameters exactly representable in float32: both precisions start equal
            for _, mod in mods:
                for p in mod.parameters():
                    p.copy_(p.float().to(dtype))
        init = {"init_%s__%s" % (a, k): v.numpy().astype(np.float32) for a, mod in mods for k, v in mod.state_dict().items()}
    p_params = list(p_net.parameters()) + list(p_vs.parameters())
    v_params = list(v_net.parameters()) + list(v_vs.parameters())
    cnn_feat = [c.astype(np.float64) for c in data["cnn_feat"]]
    agent = AgentEgo(env=types.SimpleNamespace(cnn_feat=cnn_feat), dtype=dtype, device=torch.device('cpu'), running_state=None,
                     custom_reward=None, mean_action=False, render=False, num_threads=1,
                     policy_net=p_net, policy_vs_net=p_vs, value_net=v_net, value_vs_net=v_vs,
                     optimizer_policy=torch.optim.Adam(p_params, lr=hp["lr_p"]), optimizer_value=torch.optim.Adam(v_params, lr=hp["lr_v"]),
                     opt_num_epochs=hp["epochs"], gamma=hp["gamma"], tau=hp["tau"], clip_epsilon=hp["eps"],
                     policy_grad_clip=[(p_params, hp["clip"])])
    batch = types.SimpleNamespace(**{k: data[k] for k in ("states", "actions", "masks", "rewards", "exps", "v_metas")})
    s_p_vs, s_v_vs, s_p, s_v = copy.deepcopy((p_vs, v_vs, p_net, v_net))
    st_t, ac_t = torch.from_numpy(batch.states).to(dtype), torch.from_numpy(batch.actions).to(dtype)
    mk_t, rw_t = torch.from_numpy(batch.masks).to(dtype), torch.from_numpy(batch.rewards).to(dtype)
    for m in (s_p_vs, s_v_vs):
        m.set_mode('train')
        m.initialize((mk_t, cnn_feat, batch.v_metas))
    with torch.no_grad():
        values0 = s_v(s_v_vs(st_t))
        adv0, ret0 = estimate_advantages(rw_t, mk_t, values0, hp["gamma"], hp["tau"])
        logp0 = s_p.get_log_prob(s_p_vs(st_t), ac_t)
    agent.update_params(batch)
    final = {"final_%s__%s" % (a, k): v.detach().double().numpy().copy() for a, mod in mods for k, v in mod.state_dict().items()}
    before = dict(values0=values0.double().numpy(), adv0=adv0.double().numpy(), ret0=ret0.double().numpy(), logp0=logp0.double().numpy())
    return init, final, before


def _misses(final, ref, rtol, atol):
    bad, worst = 0, 0.0
    for k, v in ref.items():
        miss = ~np.isclose(final[k], v, rtol=rtol, atol=atol)
        if miss.any():
            bad += int(miss.sum())
            worst = max(worst, float(np.abs(final[k] - v)[miss].max()))
    return bad, worst


def main(out_name="ppo_update_act.npz", htypes=("tanh", "sigmoid"), seed_np=5101, seed_torch=51):
    G.install_stubs()
    if G.REF not in sys.path:
        sys.path.insert(0, G.REF)
    G.enter_workdir()
    import torch
    import utils as _ru          # noqa: F401  (reference utils: star exports the agents rely on)
    rng = np.random.RandomState(seed_np)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    dims = sdim, adim, cdim, hdim, margin, T_ep = 9, 4, 6, 8, 2, 10
    hidden = (12, 10)
    hp = dict(lr_p=5e-3, lr_v=3e-3, clip=0.5, epochs=3, gamma=0.95, tau=0.95, eps=0.2, log_std=-1.0)
    cnn_feat = [f32(rng.normal(size=(40, cdim))), f32(rng.normal(size=(36, cdim)))]
    ep_lens = [10, 4, 7, 10, 2, 10, 5, 10, 9, 3]
    rows = dict(states=[], actions=[], masks=[], rewards=[], exps=[], v_metas=[])
    for L_ep in ep_lens:
        e_ind = int(rng.randint(2))
        s_ind = int(rng.randint(margin, cnn_feat[e_ind].shape[0] - T_ep - margin))
        for k in range(L_ep):
            rows['states'].append(f32(rng.normal(size=sdim)))
            rows['actions'].append(f32(rng.normal(size=adim) * 0.5))
            rows['masks'].append(0 if k == L_ep - 1 else 1)
            rows['rewards'].append(float(np.float32(rng.uniform(0, 1))))
            rows['exps'].append(1 if rng.uniform() < 0.8 else 0)
            rows['v_metas'].append([e_ind, s_ind])
    data = {k: np.array(v) for k, v in rows.items()}
    data["cnn_feat"] = cnn_feat
    torch.manual_seed(seed_torch)
    init, final, before = _run(torch, torch.float64, data, None, dims, hidden, htypes, hp)
    _, final32, _ = _run(torch, torch.float32, data, init, dims, hidden, htypes, hp)
    torch.set_default_dtype(torch.float64)
    bad, worst = _misses(final32, final, CRITERION["rtol"], CRITERION["atol"])
    print("%s: the reference in float32 misses (rtol %g, atol %g) on %d parameter elements, worst |diff| %.3g"
          % (out_name, CRITERION["rtol"], CRITERION["atol"], bad, worst))
    if bad > CRITERION["max_outliers"] or worst > CRITERION["outlier_atol"]:
        raise SystemExit("%s: the float32 reference run is outside the tests' float32 criterion -- not written, choose another seed" % out_name)
    out = os.path.join(G.OUT, out_name)
    np.savez_compressed(
        out, cnn_feat0=cnn_feat[0].astype(np.float32), cnn_feat1=cnn_feat[1].astype(np.float32),
        states=data["states"].astype(np.float32), actions=data["actions"].astype(np.float32), masks=data["masks"],
        rewards=data["rewards"].astype(np.float32), exps=data["exps"], v_metas=data["v_metas"],
        dims=np.array(dims), hyper=np.array([hp[k] for k in ("lr_p", "lr_v", "clip", "epochs", "gamma", "tau", "eps", "log_std")]),
        policy_htype=np.array(htypes[0]), value_htype=np.array(htypes[1]), **before, **init, **final)
    print("wrote", out, "%.0f kB" % (os.path.getsize(out) / 1e3), "N =", len(data["masks"]), "episodes =", len(ep_lens))


if __name__ == "__main__":
    main()
