#!/usr/bin/env python3
"""Time `update_params` with tanh MLPs on the HIP update path against the library fallback it replaces, interleaved in one
process (record: profiles/gemm_act_epilogue.md).

Two modes alternate from iteration to iteration on the same agent:
    hip       the code as it stands: gemm.mlp_head_available accepts tanh / sigmoid, MlpHead / GatherMlpHead run every product
    fallback  gemm.mlp_head_available answers as it did before the tanh / sigmoid epilogues existed (relu only), so both heads
              take nets.py's other branch: materialised input, bucket_rows padding, nn.Linear + element-wise autograd kernels

    shipped   the ego_mimic trainer at the shipped widths (300, 200) with policy_htype = value_htype = tanh on the synthetic
              dataset bench.py uses: whole iterations (rollout + update), the update's wall time taken (it ends in a device sync)
    fixture   tests/golden/ppo_update_act.npz (70 rows, MLP (12, 10), tanh policy / sigmoid value): update_params alone

    python tools/time_update_act.py [--pairs 6] [--warmup 2] [--envs 1024] [--min-batch 0]
Prints one JSON line per workload: both medians, min / max of each mode, the per-iteration times.
"""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def _med(xs):
    s = sorted(xs)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def _summary(what, times):
    out = {"workload": what}
    for mode, ts in times.items():
        out[mode] = {"median_ms": round(_med(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "ms": [round(t, 3) for t in ts]}
    print(json.dumps(out), flush=True)


class _Mode:
    """Switches gemm.mlp_head_available between the present predicate and the relu-only one."""

    def __init__(self):
        import torch
        from egopose_amd import gemm
        self.gemm, self.inner, self.relu = gemm, gemm.mlp_head_available, torch.relu

    def set(self, mode):
        inner, relu = self.inner, self.relu
        self.gemm.mlp_head_available = inner if mode == "hip" else (lambda x, layers, head, act: act is relu and inner(x, layers, head, act))


def shipped(args):
    import torch
    from egopose_amd.bench_support import write_synthetic_dataset
    from egopose_amd.config import Config
    from egopose_amd.physics import default_threads
    from egopose_amd.train import Trainer
    root = tempfile.mkdtemp(prefix="egp_time_act_")
    write_synthetic_dataset(root, "subject_03")
    os.chdir(root)
    cfg = Config("subject_03", create_dirs=False)
    cfg.policy_htype = cfg.value_htype = "tanh"
    tr = Trainer(cfg, torch.device("cuda", 0), torch.float32, num_envs=args.envs, num_threads=max(2, default_threads(share=1, device_index=0)), num_groups=2)
    assert tr.agent.policy_net.net.activation is torch.tanh and list(cfg.policy_hsize) == [300, 200]
    mode, it, times = _Mode(), 0, {"fallback": [], "hip": []}
    min_batch = args.min_batch or cfg.min_batch_size
    for rep in range(args.warmup + args.pairs):
        for m in ("fallback", "hip"):
            mode.set(m)
            _, _, tu, n = tr.iteration(it, min_batch)
            it += 1
            if rep >= args.warmup:
                times[m].append(tu * 1e3)
    mode.set("hip")
    tr.close()
    _summary("shipped widths (300, 200), tanh, %d envs, %d env-steps per iteration" % (args.envs, min_batch), times)


def fixture(args):
    import numpy as np
    import torch
    from act_fixture import FIXTURE, build_agent
    from egopose_amd.hip import EgpContext
    from egopose_amd.skeleton import load_skeleton
    from update_fixture import batch_of
    golden = os.path.join(REPO, "tests", "golden")
    g, c = np.load(os.path.join(golden, FIXTURE)), np.load(os.path.join(golden, "config_subject_03.npz"))
    kctx = EgpContext(load_skeleton(), c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"])
    agent, _ = build_agent(g, device="cuda", dtype=torch.float32, fused_adam=True)
    agent._kernel_ctx = lambda: kctx
    batch = batch_of(g)
    mode, times = _Mode(), {"fallback": [], "hip": []}
    for rep in range(args.warmup + 5 * args.pairs):
        for m in ("fallback", "hip"):
            mode.set(m)
            torch.cuda.synchronize()
            t0 = time.time()
            agent.update_params(batch)
            torch.cuda.synchronize()
            if rep >= args.warmup:
                times[m].append((time.time() - t0) * 1e3)
    mode.set("hip")
    kctx.close()
    _summary("ppo_update_act.npz (70 rows, MLP (12, 10), tanh / sigmoid)", times)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--min-batch", type=int, default=0)
    ap.add_argument("--only", choices=["shipped", "fixture"], default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_update_act.py needs an MI355X (a timing on the CPU says nothing)")
    if a.only != "shipped":
        fixture(a)
    if a.only != "fixture":
        shipped(a)
