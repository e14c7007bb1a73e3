#!/usr/bin/env python
"""Time of the plausibility figures (profiles/contact.md): `python tools/contact_time.py [takes] [frames]` -> one JSON line.

The workload is `takes` x `frames` rows of random humanoid poses (default 8 x 3000) with the feet near the ground, every row followed
by the next row of its take, the feet's 16 box corners as the contact set. `kernel_ms`: one launch of egp_contact_f64 with `points`,
HIP events, the median of 20 launches after a warm-up of 5 launches and 30 ms; `kernel_lean_ms`: the same with per_frame alone.
`hip_path_s`: wall clock of `compute_plausibility(backend='hip')` for the predictions, the launch with its uploads, downloads and the
host means. `host_path_s`: wall clock of `backend='host'`, once (a Python forward kinematics per row)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    from egopose_amd import plausibility
    from egopose_amd.hip import EgpContext
    from egopose_amd.presets import config_params
    from egopose_amd.skeleton import load_skeleton
    takes = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
    sk = load_skeleton()
    p = config_params("subject_03")
    ctx = EgpContext(sk, p["jkp"], p["jkd"], p["a_ref"], p["a_scale"], p["torque_lim"], p["b_diffw"])
    cs = plausibility.ContactSet.feet(sk)
    rng = np.random.RandomState(0)

    def rows(n):
        q = np.zeros((n, sk.nq))
        q[:, :2] = rng.normal(size=(n, 2))
        q[:, 2] = rng.uniform(0.84, 0.92, size=n)
        yaw = rng.uniform(-np.pi, np.pi, size=n)
        q[:, 3], q[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
        q[:, 7:] = rng.normal(size=(n, sk.nq - 7)) * 0.1
        return q
    res = {"traj_pred": {"t%d" % i: rows(frames) for i in range(takes)}}
    n = takes * frames
    nxt = np.arange(1, n + 1, dtype=np.int64)
    nxt[frames - 1::frames] = -1
    q, nx = torch.as_tensor(np.concatenate(list(res["traj_pred"].values())), device="cuda"), torch.as_tensor(nxt, device="cuda")
    ctx.set_contact_points(cs)
    out = ctx.contact(q, nx, want_points=True)

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
    full = median_ms(lambda: ctx.contact(q, nx, out=out, validate=False))              # (validate=True adds a reduction and a sync)
    lean = median_ms(lambda: ctx.contact(q, nx, out=dict(per_frame=out["per_frame"]), validate=False))
    plausibility.compute_plausibility(res, sk, backend="hip", ctx=ctx)
    t0 = time.perf_counter()
    a = plausibility.compute_plausibility(res, sk, backend="hip", ctx=ctx)
    hip_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    b = plausibility.compute_plausibility(res, sk, backend="host")
    host_s = time.perf_counter() - t0
    ctx.close()
    fig = lambda d: {k: d["traj_pred"][k] for k in plausibility.FIGURES}
    print(json.dumps(dict(takes=takes, frames=frames, rows=n, points=cs.K, kernel_ms=full[0], kernel_ms_min_max=full[1:], kernel_lean_ms=lean[0],
                          kernel_lean_ms_min_max=lean[1:], hip_path_s=hip_s, host_path_s=host_s,
                          max_abs_diff={k: abs(fig(a)[k] - fig(b)[k]) for k in plausibility.FIGURES}, figures=fig(a))))


if __name__ == "__main__":
    main()
