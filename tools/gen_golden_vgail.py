#!/usr/bin/env python3
"""GAIL discriminator fixtures: the reference's AgentVGAIL.update_discriminator, float64 on the CPU.

Imports the reference exactly as tools/gen_golden.py does (same stubs for the absent third-party modules, nothing copied) and
records one run of `AgentVGAIL.update_discriminator` (ego_pose/core/agent_vgail.py:54-88) with the reference's VideoStateNet
(bi-LSTM) and a discriminator module written HERE (the reference ships none): the reference's MLP (relu) + Linear(., 1) +
sigmoid, under nn.BCELoss() and Adam, discrim_num_update = 10, a ZFilter with a non-trivial mean and std, `obs` tables present.

    tests/golden/vgail.npz        three takes of 70 .. 90 frames, N = 131 rows in 3 episodes (50, 47, 34), S = 13,
                                  cnn_feat_dim 8, v_hdim 16, margin 2, MLP [24, 12]
    tests/golden/vgail_wide.npz   episodes of 150, 180, 120 rows, S = 76, v_hdim 128, MLP [64, 32]

Stored: the inputs (float32-representable), the filter's (n, M, S), initial and final parameters of both nets,
`expert_states` as the reference's get_expert_states returned them (rows `expert_states_rows` of them: all rows, or -- the
wide fixture, to stay below the size limit of a committed file -- every episode's first and last row and every third row;
the final parameters depend on every row), and `e_loss`.

Before a fixture is written the same reference code runs in float32 on the CPU and must stay inside the float32 criterion
of the tests (at most 8 parameter elements outside rtol 1e-4 / atol 3e-6, none beyond 1.3e-2): a criterion the reference
itself does not meet in float32 would test nothing. The count found is printed; a run outside it refuses to write (choose
another seed). Runs where the reference is available only. Own seeds.
"""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_golden as G          # noqa: E402  (stubs + workdir helpers)

CRITERION = dict(rtol=1e-4, atol=3e-6, max_outliers=8, outlier_atol=1.3e-2)


def _discriminator(torch, MLP, in_dim, hidden):
    nn = torch.nn

    class Discriminator(nn.Module):
        """MLP trunk -> one logit -> sigmoid; state-dict keys net.affine_layers.i.*, logic.* (nets.Discriminator's)."""

        def __init__(self):
            super().__init__()
            self.net = MLP(in_dim, list(hidden), 'relu')
            self.logic = nn.Linear(hidden[-1], 1)
            self.logic.weight.data.mul_(0.1)
            self.logic.bias.data.mul_(0.0)

        def forward(self, x):
            return torch.sigmoid(self.logic(self.net(x)))

    return Discriminator()


def _run(torch, dtype, data, init, dims, lr, steps):
    """One update_discriminator of the reference in `dtype` from the initial parameters `init` -> (final params, expert_states, e_loss)."""
    from models.mlp import MLP
    from models.video_state_net import VideoStateNet
    from utils.zfilter import ZFilter
    from ego_pose.core.agent_vgail import AgentVGAIL
    S, cdim, hdim, margin, h0, h1 = dims
    torch.set_default_dtype(dtype)
    vs = VideoStateNet(cdim, hdim, margin, 'lstm', None, False)
    dn = _discriminator(torch, MLP, S + hdim, (h0, h1))
    mods = [("d_vs", vs), ("d", dn)]
    if init is not None:
        for name, mod in mods:
            mod.load_state_dict({k[len("init_%s__" % name):]: torch.as_tensor(v).to(dtype) for k, v in init.items() if k.startswith("init_%s__" % name)})
    else:
        with torch.no_grad():        # initial parameters exactly representable in float32: both precisions start equal
            for _, mod in mods:
                for p in mod.parameters():
                    p.copy_(p.float().to(dtype))
        init = {"init_%s__%s" % (a, k): v.numpy().astype(np.float32) for a, mod in mods for k, v in mod.state_dict().items()}
    zf = ZFilter((S,), clip=5)
    zf.rs._n, zf.rs._M, zf.rs._S = int(data["zf_n"]), data["zf_M"].copy(), data["zf_S"].copy()
    env = types.SimpleNamespace(cnn_feat=data["cnn_feat"], expert_arr=[dict(obs=o) for o in data["obs"]])
    params = list(vs.parameters()) + list(dn.parameters())
    agent = AgentVGAIL(env=env, dtype=dtype, device=torch.device('cpu'), running_state=zf, custom_reward=None, mean_action=False,
                       render=False, num_threads=1, policy_net=None, value_net=None, policy_vs_net=None, value_vs_net=None,
                       optimizer_policy=None, optimizer_value=None, discrim_net=dn, discrim_vs_net=vs, discrim_criterion=torch.nn.BCELoss(),
                       optimizer_discrim=torch.optim.Adam(params, lr=lr), discrim_num_update=steps)
    states = torch.from_numpy(data["states"]).to(dtype)
    masks = torch.from_numpy(data["masks"]).to(dtype)
    expert_states = agent.get_expert_states(data["v_metas"], masks)
    e_loss = agent.update_discriminator(states, masks, data["v_metas"])
    final = {"final_%s__%s" % (a, k): v.detach().double().numpy().copy() for a, mod in mods for k, v in mod.state_dict().items()}
    return init, final, expert_states.double().numpy(), e_loss


def _misses(final, ref, rtol, atol):
    bad, worst = 0, 0.0
    for k, v in ref.items():
        miss = ~np.isclose(final[k], v, rtol=rtol, atol=atol)
        if miss.any():
            bad += int(miss.sum())
            worst = max(worst, float(np.abs(final[k] - v)[miss].max()))
    return bad, worst


def main(out_name, take_lens, ep_lens, S, hdim, hidden, seed_data, seed_torch, cdim=8, margin=2, lr=2e-3, steps=10, thin_expert_rows=False):
    G.install_stubs()
    if G.REF not in sys.path:
        sys.path.insert(0, G.REF)
    G.enter_workdir()
    import torch
    import utils as _ru          # noqa: F401  (reference utils: star exports the agents rely on)
    rng = np.random.RandomState(seed_data)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    cnn_feat = [f32(rng.normal(size=(L, cdim))) for L in take_lens]
    scale, shift = rng.uniform(0.5, 2.0, size=S), rng.normal(size=S)
    obs = [f32(rng.normal(size=(L, S)) * scale + shift) for L in take_lens]
    max_len = max(ep_lens)
    v_metas, states, masks = [], [], []
    for e, L_ep in enumerate(ep_lens):
        take = e % len(take_lens)
        start = int(rng.randint(margin, take_lens[take] - max_len - margin + 1))
        for k in range(L_ep):
            v_metas.append([take, start])
            states.append(f32(rng.normal(size=S)))
            masks.append(0 if k == L_ep - 1 else 1)
    hist = rng.normal(size=(40, S)) * scale * 1.3 + shift * 0.7          # what the filter has seen: a mean and std of its own
    mean = hist.mean(0)
    data = dict(cnn_feat=cnn_feat, obs=obs, states=np.array(states), masks=np.array(masks), v_metas=np.array(v_metas, dtype=np.int64),
                zf_n=np.array(hist.shape[0]), zf_M=f32(mean), zf_S=f32(((hist - mean) ** 2).sum(0)))
    dims = (S, cdim, hdim, margin, hidden[0], hidden[1])
    torch.manual_seed(seed_torch)
    init, final, expert_states, e_loss = _run(torch, torch.float64, data, None, dims, lr, steps)
    _, final32, _, e_loss32 = _run(torch, torch.float32, data, init, dims, lr, steps)
    torch.set_default_dtype(torch.float64)
    bad, worst = _misses(final32, final, CRITERION["rtol"], CRITERION["atol"])
    print("%s: the reference in float32 misses (rtol %g, atol %g) on %d parameter elements, worst |diff| %.3g; e_loss %.9g (float64) %.9g (float32)"
          % (out_name, CRITERION["rtol"], CRITERION["atol"], bad, worst, e_loss, e_loss32))
    if bad > CRITERION["max_outliers"] or worst > CRITERION["outlier_atol"] or abs(e_loss32 - e_loss) > 1e-4 * abs(e_loss):
        raise SystemExit("%s: the float32 reference run is outside the tests' float32 criterion -- not written, choose another seed" % out_name)
    keep = np.arange(len(masks))
    if thin_expert_rows:
        ends = np.nonzero(data["masks"] == 0)[0]
        keep = np.unique(np.concatenate((keep[::3], ends, np.insert(ends[:-1] + 1, 0, 0))))
    expert_states = expert_states[keep]
    out = os.path.join(G.OUT, out_name)
    np.savez_compressed(
        out, states=data["states"].astype(np.float32), masks=data["masks"], v_metas=data["v_metas"],
        zf_n=data["zf_n"], zf_M=data["zf_M"], zf_S=data["zf_S"], expert_states=expert_states, expert_states_rows=keep, e_loss=np.array(e_loss),
        dims=np.array(dims), hyper=np.array([lr, steps]), ep_lens=np.array(ep_lens),
        **{"cnn_feat%d" % i: c.astype(np.float32) for i, c in enumerate(cnn_feat)}, **{"obs%d" % i: o.astype(np.float32) for i, o in enumerate(obs)},
        **init, **final)
    print("wrote", out, "%.0f kB" % (os.path.getsize(out) / 1e3), "N =", len(masks))


if __name__ == "__main__":
    main("vgail.npz", take_lens=[83, 70, 90], ep_lens=[50, 47, 34], S=13, hdim=16, hidden=(24, 12), seed_data=4101, seed_torch=41)
    main("vgail_wide.npz", take_lens=[200, 190, 210], ep_lens=[150, 180, 120], S=76, hdim=128, hidden=(64, 32), seed_data=4102, seed_torch=42, thin_expert_rows=True)
