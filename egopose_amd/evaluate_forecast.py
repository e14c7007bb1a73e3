"""Evaluation driver of the ego_forecast policy: every forecast window of every take, batched onto lockstep env slots.

Restates the save mode of ego_pose/ego_forecast_eval.py:95-204 and the `--mode stats` part of ego_pose/eval_forecast.py:29-114.
The reference evaluates the windows `start = m, 2m, 3m, ... while start + test_len <= take_len` (m = cfg.fr_margin,
test_len = cfg.env_episode_len) of every take one after another; a window is a fixed-length episode that never breaks on
`fail`, has no reset inside, no exploration noise and a frozen observation filter (`running_state(x, update=False)`). So the
windows run here as the slots of `env.batched(N)` in strict lockstep, in passes of N; a tick is

    record qpos -> [observation -> frozen normalisation -> state-LSTM cell -> MLP -> mean action] -> env-step

with the bracket one launch (`FusedForecastPolicy.with_filter(..., workspace=None)`, egp_policy_step_f32 (cell + filter block)). The pass
around it -- slots, frozen filter state, records, env-step and timed wait -- is `lockstep_eval.LockstepPass`, shared with the
ego_mimic evaluation; the plan, the launch with its LSTM state and the `failed` log are here.

A window starts from the expert's state (`gt_init`) or from the ego_mimic result of the same take (ego_forecast_eval.py:107-120,
`window_init_state`). The value nets are NOT evaluated: the reference only logs their output, which does not enter the results.
Rendering (`--render`, `--mode vis`, `--show-noise`) and the per-step reward log (`--verbose`) are out of scope.

Feature-only takes (ego_forecast_eval_wild.py): the window plan (`wild_window_plan`: `window_plan` from another first start) and the
seat / history rows (`wild_window_init_state`) are here, `ForecastEvaluator(..., cnn_feat_dict=...)` runs them -- the feature
table comes from the pickle, seat and history from the wild ego_mimic result, there is no expert, no `sync_traj`, no `traj_orig` and no per-take head bound (`failed` is
only logged against the env's `fix_head_lb`, if set) -- and `--mode wild-stats` scores the saved results with the 2D keypoint
metric (`egopose_amd.pose2d`). `--test-feat NAME` selects this path.

`--mode stats` scores the SAVED result of `--data` at `--horizon` without running anything. `--physical [--contacts FILE]
[--contact-height H] [--ground-z Z]` adds foot skate, ground penetration and floating (`egopose_amd.plausibility`) in every mode;
with MoCap also the `mocap` row, what MoCap itself reaches.
"""
from __future__ import annotations

import pickle

import numpy as np

from . import metrics
from .lockstep_eval import LockstepPass, Timing, check_frozen_filter


# ---------------------------------------------------------------------- ego_forecast_eval.py:185-196
def window_plan(take_lens, fr_margin, test_len, first_start=None):
    """(take_ind[W], start_ind[W]) of every evaluated window: per take start = m, 2m, ... while start + test_len <= take_len
    (`first_start`: another first start than m)."""
    m, test_len = int(fr_margin), int(test_len)
    take_ind, start_ind = [], []
    for i, take_len in enumerate(take_lens):
        start = m if first_start is None else int(first_start)
        while start + test_len <= int(take_len):
            take_ind.append(i)
            start_ind.append(start)
            start += m
    return np.asarray(take_ind, dtype=np.int64), np.asarray(start_ind, dtype=np.int64)


# ---------------------------------------------------------------------- ego_forecast_eval.py:107-133
def window_init_state(expert_qpos, expert_qvel, start, fr_margin, test_len, em_traj=None, em_vel=None, em_off=0):
    """Seat state and history rows of the window starting at frame `start` of a take -> (qpos, qvel, history[m, nq], miss_len).

    em_traj is None (`gt_init`): the expert's state at `start`, history = the expert's rows [start - m, start).
    Otherwise em_traj / em_vel are the ego_mimic result of the take (its row i is take frame i + em_off, em_off = the ego_mimic
    config's fr_margin): the slice [max(0, start - m - em_off), start + test_len - em_off) of it, synced to the expert's pose at
    frame start - m when it reaches back that far (`sync_traj`); `miss_len` rows are missing from it (at its front for an early
    window; the reference's arithmetic treats a slice cut short at the take's end the same way, and so does this). The seat
    state is row m - miss_len, history row t the expert's for t < miss_len and slice row t - miss_len after that."""
    m, start, test_len = int(fr_margin), int(start), int(test_len)
    history = np.array(expert_qpos[start - m:start], dtype=np.float64, copy=True)
    if em_traj is None:
        return np.array(expert_qpos[start], float, copy=True), np.array(expert_qvel[start], float, copy=True), history, 0
    lo = start - m - int(em_off)
    state_pred = np.asarray(em_traj, float)[max(0, lo):start + test_len - int(em_off)]
    vel_pred = np.asarray(em_vel, float)[max(0, lo):start + test_len - int(em_off)]
    miss_len = m + test_len - state_pred.shape[0]
    if lo >= 0:
        state_pred, vel_pred = metrics.sync_traj(state_pred, vel_pred, expert_qpos[start - m])
    ind = m - miss_len
    qpos, qvel = state_pred[ind].copy(), vel_pred[ind].copy()
    for t in range(m):
        if not t < miss_len:
            history[t] = state_pred[t - miss_len]
    return qpos, qvel, history, miss_len


# ---------------------------------------------------------------------- ego_forecast_eval_wild.py:160-170
def wild_window_plan(take_lens, fr_margin, em_margin, test_len):
    """(take_ind[W], start_ind[W]) of the windows of feature-only takes: per take start = m + em_m, m + em_m + m, ... while
    start + test_len <= take_len (take_len = rows of the take's feature array, em_m = the ego_mimic config's fr_margin)."""
    return window_plan(take_lens, fr_margin, test_len, int(fr_margin) + int(em_margin))


# ---------------------------------------------------------------------- ego_forecast_eval_wild.py:102-120
def wild_window_init_state(em_traj, em_vel, start, fr_margin, em_margin, test_len):
    """Seat state and history rows of the window starting at feature row `start` of a feature-only take, from the take's wild
    ego_mimic result (its row i is feature row i + em_m) -> (qpos, qvel, history[m, nq]): the slice
    [start - m - em_m, start + test_len - em_m) of it, seat = its row m, history = its rows 0..m-1. No expert, no sync_traj. (The result has take_len - 2 em_m rows, so the slice of a window at
    the take's end comes up short, as the reference's does; only its first m + 1 rows are read.)"""
    m, em_m, start, test_len = int(fr_margin), int(em_margin), int(start), int(test_len)
    if start < m + em_m:
        raise ValueError("window start %d before fr_margin + the ego_mimic margin" % start)        # the reference's assert
    lo, hi = start - m - em_m, start + test_len - em_m
    state_pred, vel_pred = np.asarray(em_traj, float)[lo:hi], np.asarray(em_vel, float)[lo:hi]
    if state_pred.shape[0] <= m:      # the mimic result ends em_m rows before the features do: a window at the take's end needs test_len > em_m
        raise ValueError("window at %d: the ego_mimic result has no row for its start (%d rows from %d)" % (start, state_pred.shape[0], lo))
    return state_pred[m].copy(), vel_pred[m].copy(), state_pred[:m].copy()


def result_path(cfg, it, data="test", gt_init=False):
    return "%s/iter_%04d_%s%s.p" % (cfg.result_dir, it, data, "_gt" if gt_init else "")


class ForecastEvaluator:
    """`run()` -> (results, meta) in the reference's pickle layout: results = {'traj_pred': {take: [n_win, m + test_len, nq]},
    'traj_orig': ...}, meta = {'algo': 'ego_forecast'}. `em_res` (+ `em_off`): the ego_mimic results the windows start from
    unless `gt_init`. `keep_trace`: `self.trace` keeps per window the actions, the filtered states the policy saw, the qvel that
    goes with each recorded qpos, and the plan (take_ind, start_ind). `self.timing`: wall seconds of the last run, split into
    the wait for the host physics and the rest.
    `cnn_feat_dict` = {take: features} (ego_forecast_eval_wild.py): feature-only takes on an env without experts; `em_res` is then the
    wild ego_mimic result, and results = {'traj_pred': {take: [n_win, m + test_len, nq]}} alone."""

    CTX_BATCH = 1024         # windows per launch of the video net

    def __init__(self, cfg, env, policy_net, policy_vs_net, running_state=None, gt_init=False, em_res=None, em_off=0, num_envs=1024,
                 device_index=0, n_threads=None, keep_trace=False, logger=None, cnn_feat_dict=None):
        if cnn_feat_dict is not None and (gt_init or env.expert_list is not None):
            raise ValueError("feature-only takes have no expert: no gt_init, and an env without experts")
        if not gt_init and em_res is None:
            raise ValueError("ego_mimic results (em_res) are needed unless gt_init")
        check_frozen_filter(running_state)
        self.cfg, self.env = cfg, env
        self.policy_net, self.policy_vs_net = policy_net, policy_vs_net
        self.running_state = running_state
        self.gt_init, self.em_res, self.em_off = bool(gt_init), em_res, int(em_off)
        self.num_envs, self.device_index, self.n_threads = int(num_envs), int(device_index), n_threads
        self.keep_trace, self.logger = bool(keep_trace), logger
        self.trace, self.timing = None, {}
        self.wild = cnn_feat_dict is not None
        self.take_names = list(cnn_feat_dict.keys()) if self.wild else None
        self.cnn_feat = [np.asarray(cnn_feat_dict[take]) for take in self.take_names] if self.wild else None
        for net in (policy_net, policy_vs_net):
            net.eval()
        policy_vs_net.set_mode("test")

    # ------------------------------------------------------------------ host side of a run: plan, seat states, history rows
    def _names_and_features(self):
        return (self.take_names, self.cnn_feat) if self.wild else (self.env.expert_list, self.env.cnn_feat)

    def _window_state(self, e, s, m, T):
        """(qpos, qvel, history, miss_len) of the window at frame `s` of take `e`."""
        if self.wild:
            take = self.take_names[e]
            return wild_window_init_state(self.em_res["traj_pred"][take], self.em_res["vel_pred"][take], s, m, self.em_off, T) + (0,)
        env = self.env
        ex, take = env.expert_arr[e], env.expert_list[e]
        if s + T > ex["qpos"].shape[0]:
            raise ValueError("take %s: the expert has fewer frames than the features" % take)
        em_t, em_v = (None, None) if self.gt_init else (self.em_res["traj_pred"][take], self.em_res["vel_pred"][take])
        return window_init_state(ex["qpos"], ex["qvel"], s, m, T, em_t, em_v, self.em_off)

    def plan(self, takes=None):
        m, T = int(self.cfg.fr_margin), int(self.cfg.env_episode_len)
        names, feats = self._names_and_features()
        take_ind, start_ind = window_plan([c.shape[0] if takes is None or names[i] in takes else 0 for i, c in enumerate(feats)], m, T,
                                          m + self.em_off if self.wild else None)
        W = len(take_ind)
        nq, nv = self.env.skel.nq, self.env.skel.nv
        qpos0, qvel0, hist = np.empty((W, nq)), np.empty((W, nv)), np.empty((W, m, nq))
        miss = np.zeros(W, np.int64)
        for w, (e, s) in enumerate(zip(take_ind, start_ind)):
            qpos0[w], qvel0[w], hist[w], miss[w] = self._window_state(e, s, m, T)
        return take_ind, start_ind, qpos0, qvel0, hist, miss

    # ------------------------------------------------------------------ ego_forecast_eval.py:95-204, batched
    def run(self, takes=None):
        """Evaluate every window of every take of the env's expert list (or of `takes`) -> (results, meta)."""
        import torch
        from . import policy_step
        cfg, env = self.cfg, self.env
        m, T = int(cfg.fr_margin), int(cfg.env_episode_len)
        tm = Timing()
        take_ind, start_ind, qpos0, qvel0, hist, miss = self.plan(takes)
        W = tm["windows"] = len(take_ind)
        N = self.num_envs
        lp = LockstepPass(env, N, self.device_index, self.n_threads, self.running_state, T, tm, record_qvel=self.keep_trace)
        ctx, eng, dev, ex = lp.ctx, lp.eng, lp.dev, lp.sim.experts
        if self.wild:
            from .expert import ExpertSet
            ex = ExpertSet.features_only(self.cnn_feat)
        names = self._names_and_features()[0]
        vs = self.policy_vs_net
        if not policy_step.supported_forecast(self.policy_net, vs):
            raise NotImplementedError("the forecast evaluation needs the HIP policy step: a float32 PolicyGaussian over an MLP behind a "
                                      "VideoForecastNet with an LSTMCell state net")
        nq, nv, nu, od = ctx.nq, ctx.nv, ctx.nu, ctx.obs_dim
        pred = np.empty((W, m + T, nq))
        orig = None if self.wild else np.empty((W, m + T, nq))
        for w, (e, s) in enumerate(zip(take_ind, start_ind)):
            if orig is not None:
                orig[w] = env.expert_arr[e]["qpos"][s - m:s + T]
        pred[:, :m] = hist
        failed = np.zeros(W, bool)
        tr_act, tr_st, tr_qv = (np.empty((W, T, nu)), np.empty((W, T, od)), np.empty((W, T, nv))) if self.keep_trace else (None, None, None)
        with torch.no_grad(), torch.cuda.device(dev):
            fused = policy_step.FusedForecastPolicy(self.policy_net, vs, dev)
            vs.attach_feature_table(ex.cnn_table(dev, torch.float32), ex.cnn_offset)
            vs.check_windows(take_ind, start_ind, 0)
            v_out = torch.zeros(N, 1, vs.v_hdim, dtype=torch.float32, device=dev)
            h = torch.zeros(N, vs.s_hdim, dtype=torch.float32, device=dev)
            c = torch.zeros_like(h)
            t_idx = torch.zeros(N, dtype=torch.int64, device=dev)
            lb = ex.head_height_lb            # (feature-only takes: None)
            fix_lb = getattr(env, "fix_head_lb", None) if self.wild else None
            # the windows' video contexts, as LockstepRollout._draw_episodes computes them for forecast episodes: in batches whose
            # size does not follow the slot count (the LSTM kernels' tiling follows the batch size, and a window's forecast must
            # not depend on how many slots it was evaluated with)
            ctx_all = torch.empty(W, vs.v_hdim, dtype=torch.float32, device=dev)
            for w0 in range(0, W, self.CTX_BATCH):
                sl = slice(w0, min(W, w0 + self.CTX_BATCH))
                e_d, s_d = torch.as_tensor(take_ind[sl], device=dev), torch.as_tensor(start_ind[sl], device=dev)
                ctx_all[sl] = vs.context(vs.window_features(e_d, s_d))

            def launch(t, k):
                fused.with_filter(ctx, v_out[:k], t_idx[:k], eng.qpos[:k], eng.qvel[:k], lp.zf_in, None, lp.clip, lp.states[t, :k], None, None,
                                  h[:k], c[:k], lp.actions[t, :k], phase_t=lp.phase_t(t))

            for w0 in range(0, W, N):
                k = min(N, W - w0)
                sl = slice(w0, w0 + k)
                lp.seat(qpos0[sl], qvel0[sl])
                h.zero_(); c.zero_()
                v_out[:k, 0] = ctx_all[sl]
                for t in range(T):
                    lp.tick(t, launch)
                    if lb is not None:
                        failed[sl] |= np.asarray(eng.head_z[:k]) < lb[take_ind[sl]] - 0.1      # (logged only: the window runs on)
                    elif fix_lb is not None:
                        failed[sl] |= np.asarray(eng.head_z[:k]) < fix_lb
                if self.keep_trace:
                    pred[sl, m:], tr_act[sl], tr_st[sl], tr_qv[sl] = lp.copy_out(T, "traj", "actions", "states", "qvel")
                else:
                    pred[sl, m:], = lp.copy_out(T, "traj")
        if self.logger is not None:
            for w in np.nonzero(failed)[0]:
                self.logger.info("fail - expert_ind: %d, start_ind %d" % (take_ind[w], start_ind[w]))
        traj_pred, traj_orig = {}, {}
        for i, take in enumerate(names):
            sel = take_ind == i
            if sel.any():                          # (a take too short for one window has no entry)
                traj_pred[take] = pred[sel]
                if orig is not None:
                    traj_orig[take] = orig[sel]
        self.failed = failed
        self.miss_len = miss
        if self.keep_trace:
            self.trace = dict(actions=tr_act, states=tr_st, qvel=tr_qv, take_ind=take_ind, start_ind=start_ind)
        tm.close()
        self.timing = tm
        if self.wild:
            return {"traj_pred": traj_pred}, {"algo": "ego_forecast"}
        return {"traj_pred": traj_pred, "traj_orig": traj_orig}, {"algo": "ego_forecast"}

    def save(self, results, meta, it, data="test"):
        return metrics.save_results(result_path(self.cfg, it, data, self.gt_init), results, meta)


def build_parser():
    import argparse
    ap = argparse.ArgumentParser(prog="python -m egopose_amd.evaluate_forecast")
    ap.add_argument("--cfg", default="subject_03")
    ap.add_argument("--iter", type=int, default=0)
    ap.add_argument("--data", default="test")
    ap.add_argument("--gt-init", action="store_true")
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--gpu-index", type=int, default=0)
    ap.add_argument("--mode", default="eval", choices=["eval", "wild-stats", "stats"],
                    help="wild-stats: 2D keypoint statistics of saved --test-feat results; stats: the statistics of saved --data results at --horizon")
    ap.add_argument("--test-feat", default=None, help="forecast on the feature-only takes of features/cnn_feat_<NAME>.p, from the wild ego_mimic result iter_<N>_<NAME>.p")
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--host", action="store_true", help="wild-stats, --joint-pos: the per-frame numpy loop instead of the GPU kernel")
    ap.add_argument("--joint-pos", action="store_true", help="eval: also the joint-position metrics at each horizon (egopose_amd.pose3d)")
    ap.add_argument("--keep-hands", action="store_true", help="--joint-pos: count the hands too (left out by default)")
    from . import plausibility
    plausibility.add_arguments(ap)                 # --physical [--contacts FILE] [--contact-height H] [--ground-z Z]: stats, wild-stats
    return ap


def _wild_stats(cfg, args):
    """eval_forecast_wild.py --mode stats on the saved forecast results of feature-only takes."""
    from . import pose2d
    meta, pose_ctx, loader = pose2d.wild_stats_front(cfg, args.test_feat)
    with open("%s/iter_%04d_%s.p" % (cfg.result_dir, args.iter, args.test_feat), "rb") as f:
        res, _ = pickle.load(f)
    out = pose2d.eval_forecast_wild_stats(res, meta, loader, cfg, horizon=args.horizon, backend="host" if args.host else "hip",
                                          pose_ctx=pose_ctx, verbose=True, device_index=args.gpu_index)
    if args.physical:                              # the only 3D figures of takes without MoCap
        out["physical"] = _physical(res, cfg, args, args.horizon, which=("traj_pred",))
    return out


def _physical(stats, cfg, args, horizon, which=("traj_pred", "traj_orig")):
    """The `--physical` line(s) of one horizon: foot skate, ground penetration and floating (egopose_amd.plausibility) over frames
    [m, m + horizon) of every window; with MoCap also the `mocap` row."""
    from . import plausibility
    return plausibility.from_args(stats, cfg, args, "ego forecast", which=which, forecast=(cfg.fr_margin, horizon),
                                  what="all - horizon: %d" % horizon)


def _stats(cfg, args):
    """eval_forecast.py --mode stats on the SAVED forecast result of --data at --horizon; `--joint-pos` and `--physical` add their lines."""
    import copy
    with open(result_path(cfg, args.iter, args.data, args.gt_init), "rb") as f:
        saved, _ = pickle.load(f)
    stats = copy.deepcopy({k: saved[k] for k in ("traj_pred", "traj_orig")})
    metrics.remove_noisy_hands(stats)
    out = metrics.compute_forecast_metrics(stats, cfg.fr_margin, args.horizon, verbose=True)
    if args.joint_pos:
        out["joint_pos"] = _joint_pos(stats, cfg, args, args.horizon)
    if args.physical:
        out["physical"] = _physical(stats, cfg, args, args.horizon)
    return out


def _joint_pos(stats, cfg, args, horizon, ctx=None):
    """The `--joint-pos` line of one horizon: the joint-position metrics (egopose_amd.pose3d) over frames [m, m + horizon) of every window."""
    from . import pose3d
    from .skeleton import load_skeleton
    skel = load_skeleton()
    out = pose3d.compute_forecast_joint_metrics(stats, skel, cfg.fr_margin, horizon, backend="host" if args.host else "hip", ctx=ctx, cfg=cfg,
                                                mask=pose3d.body_mask(skel, () if args.keep_hands else pose3d.HANDS),
                                                device_index=args.gpu_index)
    print(pose3d.format_line([out[k] for k in pose3d.FIGURES], "all - horizon: %d" % horizon))
    return out


def main(argv=None):
    """`python -m egopose_amd.evaluate_forecast --cfg subject_03 --iter N --data test [--gt-init] [--num-envs 1024] [--gpu-index 0]
    [--joint-pos [--keep-hands] [--host]]`: ego_forecast_eval.py in save mode (checkpoint loading: :57-79) followed by the statistics
    of eval_forecast.py (--mode stats); `--joint-pos` adds the joint-position line of each horizon."""
    import copy
    import torch
    from .config import Config as EgoMimicConfig, ForecastConfig
    from .env import HumanoidEnv
    from .evaluate_wild import cli_takes
    from .nets import MLP, PolicyGaussian, VideoForecastNet
    from .zfilter import load_reference_pickle
    args = build_parser().parse_args(argv)
    cfg = ForecastConfig(args.cfg, create_dirs=False)
    if args.mode == "wild-stats":
        return _wild_stats(cfg, args)
    if args.mode == "stats":
        return _stats(cfg, args)
    if args.gt_init and args.test_feat is not None:
        raise SystemExit("--gt-init needs MoCap: not with --test-feat")
    if args.joint_pos and args.test_feat is not None:
        raise SystemExit("--joint-pos needs MoCap: not with --test-feat")
    cfg.random_cur_t = False
    cfg.env_init_noise = 0.0
    dev = torch.device("cuda", args.gpu_index)
    env = HumanoidEnv(cfg)
    env.seed(cfg.seed)
    cnn_feat_dict, cnn_dim = cli_takes(cfg, env, args.data, args.test_feat)
    data = args.data if args.test_feat is None else args.test_feat
    sd, ad = env.observation_space.shape[0], env.action_space.shape[0]
    policy_vs = VideoForecastNet(cnn_dim, sd, cfg.policy_v_hdim, cfg.fr_margin, cfg.policy_v_net, cfg.policy_v_net_param, cfg.policy_s_hdim,
                                 cfg.policy_s_net, cfg.policy_dyn_v)
    policy = PolicyGaussian(MLP(policy_vs.out_dim, cfg.policy_hsize, cfg.policy_htype), ad, log_std=cfg.log_std, fix_std=cfg.fix_std)
    with open("%s/iter_%04d.p" % (cfg.model_dir, args.iter), "rb") as f:
        cp = load_reference_pickle(f)
    policy.load_state_dict(cp["policy_dict"])
    policy_vs.load_state_dict(cp["policy_vs_dict"])
    for net in (policy, policy_vs):
        net.to(dev, torch.float32)
    em_res, em_off = None, 0
    if not args.gt_init:
        em_cfg = EgoMimicConfig(cfg.ego_mimic_cfg, create_dirs=False)
        with open("%s/iter_%04d_%s.p" % (em_cfg.result_dir, cfg.ego_mimic_iter, data), "rb") as f:
            em_res, _ = pickle.load(f)
        em_off = em_cfg.fr_margin
    ev = ForecastEvaluator(cfg, env, policy, policy_vs, running_state=cp["running_state"], gt_init=args.gt_init, em_res=em_res, em_off=em_off,
                           num_envs=args.num_envs, device_index=args.gpu_index, cnn_feat_dict=cnn_feat_dict)
    results, meta = ev.run()
    path = ev.save(results, meta, args.iter, data)
    print("saved results to %s (%d windows, %.2f s, %.2f s of it waiting for the physics)"
          % (path, ev.timing["windows"], ev.timing["total"], ev.timing["phys_wait"]))
    if cnn_feat_dict is not None:                  # (no MoCap to compare with: `--mode wild-stats` scores the file)
        env.close()
        return
    stats = copy.deepcopy(results)
    metrics.remove_noisy_hands(stats)
    for horizon in (30, 90):
        metrics.compute_forecast_metrics(stats, cfg.fr_margin, horizon, verbose=True)
        if args.joint_pos:
            _joint_pos(stats, cfg, args, horizon)
        if args.physical:
            _physical(stats, cfg, args, horizon)
    env.close()


if __name__ == "__main__":
    main()
