#!/usr/bin/env python3
"""The two figures profiles/forecast_eval.md asks for, one JSON line:

  (a) per-launch time of FusedForecastPolicy.with_filter (frozen and merged form) at 512 rows against the two-launch pair
      obs_zfilter_apply + egp_policy_step_f32 (cell) (the merged form's and the pair's statistics pass is launched once, outside
      the timed loops: all three read the same workspace), HIP events over `--launches` launches after `--warm` warm-up launches;
  (b) wall time of ForecastEvaluator.run on a synthetic dataset at `--slots` slots, split into host physics wait and the rest.

    python tools/forecast_eval_probe.py [--rows 512] [--launches 400] [--slots 1024] [--takes 8] [--frames 2000]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def launch_times(tr, n, launches, warm):
    from egopose_amd import policy_step
    dev = torch.device("cuda", 0)
    sim = tr.env.batched(max(n, 8), 0, 2, 1)
    ctx = sim.ctx
    S, nu = ctx.obs_dim, ctx.nu
    fp = policy_step.FusedForecastPolicy(tr.policy_net, tr.policy_vs_net, dev)
    ex = tr.env.expert_arr[0]
    rows = np.arange(n) % (ex["qpos"].shape[0] - 1)
    qp = torch.as_tensor(ex["qpos"][rows], device=dev)
    qv = torch.as_tensor(ex["qvel"][rows], device=dev)
    v_out = torch.randn(n, 1, tr.policy_vs_net.v_hdim, device=dev)
    t_idx = torch.zeros(n, dtype=torch.int64, device=dev)
    h, c = torch.zeros(n, fp.Hs, device=dev), torch.zeros(n, fp.Hs, device=dev)
    y, y2 = torch.empty(n, S, dtype=torch.float64, device=dev), torch.empty(n, S, dtype=torch.float64, device=dev)
    act = torch.empty(n, nu, dtype=torch.float64, device=dev)
    st = tr.running_state.to_device_state(dev)
    st_out = torch.empty_like(st)
    ws = torch.empty(int(ctx.lib.egp_zfilter_workspace_bytes(n, S)) // 8, dtype=torch.float64, device=dev)
    pt = torch.zeros(n, dtype=torch.int32, device=dev) if ctx.obs_phase else None
    ctx.obs_zfilter_stats(qp, qv, ws, phase_t=pt)

    def pair():
        ctx.obs_zfilter_apply(qp, qv, st, st_out, 5.0, y, y2, ws, phase_t=pt)
        fp(v_out, t_idx, y2, h, c, act)

    forms = {"pair_apply_then_forecast": pair,
             "with_filter_merged": lambda: fp.with_filter(ctx, v_out, t_idx, qp, qv, st, st_out, 5.0, y, y2, ws, h, c, act, phase_t=pt),
             "with_filter_frozen": lambda: fp.with_filter(ctx, v_out, t_idx, qp, qv, st, None, 5.0, y, None, None, h, c, act, phase_t=pt)}
    out = {}
    for rep in range(3):                                  # the forms in turn, three rounds: drift shows as spread
        for name, fn in forms.items():
            for _ in range(warm):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            torch.cuda.synchronize()
            out.setdefault(name, []).append(round(a.elapsed_time(b) * 1e3 / launches, 3))
    return {k: {"us_per_call_runs": v, "us_per_call_median": float(np.median(v))} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--warm", type=int, default=50)
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--takes", type=int, default=8)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--threads", type=int, default=None)
    args = ap.parse_args()
    from egopose_amd.bench_support import write_synthetic_dataset
    from egopose_amd.config import ForecastConfig
    from egopose_amd.evaluate_forecast import ForecastEvaluator
    from egopose_amd.train import Trainer
    root = tempfile.mkdtemp(prefix="egp_feval_")
    write_synthetic_dataset(root, "subject_03", n_takes=args.takes, n_frames=args.frames, seed=4)
    os.chdir(root)
    cfg = ForecastConfig("subject_03", create_dirs=False)
    tr = Trainer(cfg, torch.device("cuda", 0), torch.float32, num_envs=64, num_threads=2, num_groups=1)
    tr.pre_iter_update(0)
    tr.agent.sample(64 * cfg.env_episode_len)             # real filter statistics
    res = {"rows": args.rows, "launches": args.launches, "launch_us": launch_times(tr, args.rows, args.launches, args.warm)}
    ev = ForecastEvaluator(cfg, tr.env, tr.policy_net, tr.policy_vs_net, running_state=tr.running_state, gt_init=True, num_envs=args.slots,
                           n_threads=args.threads)
    runs = []
    for _ in range(3):
        ev.run()
        runs.append({k: (round(v, 4) if isinstance(v, float) else v) for k, v in ev.timing.items()})
    res["evaluate"] = {"slots": args.slots, "takes": args.takes, "frames": args.frames, "episode_len": int(cfg.env_episode_len),
                       "host_threads": tr.env.batched(args.slots, 0, args.threads, 1).engine.n_threads, "runs": runs}
    tr.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
