#!/usr/bin/env python
"""Time of the joint-position metrics (profiles/pose3d.md): `python tools/pose3d_time.py [takes] [frames]` -> one JSON line.

The workload is `takes` x `frames` pairs of random humanoid poses (default 8 x 3000). `kernel_ms`: one launch of egp_pose3d_f64 with
every optional output, HIP events, the median of 20 launches after a warm-up of 5 launches and 30 ms; `kernel_lean_ms`: the same with
per_frame alone. `hip_path_s`: wall clock of `compute_joint_metrics(backend='hip')`, the launch with its uploads, downloads and the host
acceleration error. `host_path_s`: wall clock of `backend='host'`, once (a Python forward kinematics per row)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    from egopose_amd import pose3d
    from egopose_amd.hip import EgpContext
    from egopose_amd.presets import config_params
    from egopose_amd.skeleton import load_skeleton
    takes = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
    sk = load_skeleton()
    p = config_params("subject_03")
    ctx = EgpContext(sk, p["jkp"], p["jkd"], p["a_ref"], p["a_scale"], p["torque_lim"], p["b_diffw"])
    rng = np.random.RandomState(0)

    def rows(n):
        q = np.zeros((n, sk.nq))
        q[:, :3] = rng.normal(size=(n, 3))
        q[:, 3:7] = rng.normal(size=(n, 4))
        q[:, 3:7] /= np.linalg.norm(q[:, 3:7], axis=1, keepdims=True)
        q[:, 7:] = rng.uniform(sk.joint_range[:, 0], sk.joint_range[:, 1], size=(n, sk.nq - 7))
        return q
    res = {"traj_pred": {"t%d" % i: rows(frames) for i in range(takes)}, "traj_orig": {"t%d" % i: rows(frames) for i in range(takes)}}
    mask = pose3d.body_mask(sk, pose3d.HANDS)
    n = takes * frames
    qp = torch.as_tensor(np.concatenate(list(res["traj_pred"].values())), device="cuda")
    qg = torch.as_tensor(np.concatenate(list(res["traj_orig"].values())), device="cuda")
    out = ctx.pose3d(qp, qg, body_mask=mask, want_err=True, want_xpos=True)

    def median_ms(fn):
        t0 = time.perf_counter()
        done = 0
        while done < 5 or time.perf_counter() - t0 < 0.03:
            fn()
            torch.cuda.synchronize()
            done += 1
        ts = []
        for _ in range(20):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts)), float(min(ts)), float(max(ts))
    full = median_ms(lambda: ctx.pose3d(qp, qg, body_mask=mask, out=out))
    lean = median_ms(lambda: ctx.pose3d(qp, qg, body_mask=mask, out=dict(per_frame=out["per_frame"])))
    pose3d.compute_joint_metrics(res, sk, mask=mask, backend="hip", ctx=ctx)
    t0 = time.perf_counter()
    a = pose3d.compute_joint_metrics(res, sk, mask=mask, backend="hip", ctx=ctx)
    hip_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    b = pose3d.compute_joint_metrics(res, sk, mask=mask, backend="host")
    host_s = time.perf_counter() - t0
    ctx.close()
    print(json.dumps(dict(takes=takes, frames=frames, pairs=n, kernel_ms=full[0], kernel_ms_min_max=full[1:], kernel_lean_ms=lean[0],
                          kernel_lean_ms_min_max=lean[1:], hip_path_s=hip_s, host_path_s=host_s,
                          max_abs_diff_m={k: abs(a[k] - b[k]) for k in ("g_mpjpe", "mpjpe", "pa_mpjpe", "root_err")},
                          mpjpe_mm=1e3 * a["mpjpe"], pa_mpjpe_mm=1e3 * a["pa_mpjpe"])))


if __name__ == "__main__":
    main()
