#!/usr/bin/env python3
"""Time one `AgentEgo.update_params` at the bench's batch with the update monitor off, with diagnostics on and with
target_kl = inf, and the monitor's launch alone.

    python tools/update_monitor_probe.py [rows] [--commit ID] [--out FILE]

Builds the bench's set-up (subject_03's nets over the synthetic dataset, 1 024 env slots), samples one batch of at least `rows`
rows (default: the config's min_batch_size, which the bench's rollout turns into ~134 k rows) and times the update on it with HIP
events in the three modes, alternating, after warm-up updates of each:
  off          the defaults: no monitor launch, no host read
  diagnostics  update_diagnostics=True: one `egp_ppo_stats_f32` call per epoch, records read with the losses at the end
  target_kl    target_kl=inf: the same launches + the per-epoch device-to-host copy of the record before the backward pass
(every update moves the weights, so the three modes do not see the same weights -- the work per update is the same). The monitor's
own launch is timed on the tensors of the last epoch's shapes. The next rollout's set-up, which `update_params` otherwise starts
behind the last epoch, is switched off for all modes. Writes a markdown record to --out and prints it."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MODES = (("off", {}), ("diagnostics", dict(update_diagnostics=True)), ("target_kl", dict(target_kl=float("inf"))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rows", nargs="?", type=int, default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    out = os.path.abspath(args.out) if args.out else None        # (before the chdir into the workspace)
    if not torch.cuda.is_available():
        raise SystemExit("update_monitor_probe times the MI355X: no ROCm device visible")
    from egopose_amd import optim as O
    from egopose_amd.bench_support import write_synthetic_dataset
    from egopose_amd.config import Config
    from egopose_amd.physics import default_threads
    from egopose_amd.train import Trainer
    root = tempfile.mkdtemp(prefix="egp_update_monitor_probe_")
    write_synthetic_dataset(root, "subject_03")
    os.chdir(root)
    cfg = Config("subject_03", create_dirs=False)
    tr = Trainer(cfg, torch.device("cuda", 0), torch.float32, num_envs=1024, num_threads=max(2, default_threads(share=1, device_index=0)),
                 num_groups=2)
    agent = tr.agent
    agent.prefetch_rollout = False
    tr.pre_iter_update(0)
    batch, _ = agent.sample(args.rows or cfg.min_batch_size)
    n = len(batch)
    n_pol = int(np.asarray(batch.exps).sum()) if batch.device_column("exps") is None else int(batch.device_column("exps").sum().item())

    def set_mode(kw):
        agent.target_kl, agent.update_diagnostics, agent.stop_on_nonfinite = kw.get("target_kl"), kw.get("update_diagnostics", False), False

    def one(kw):
        set_mode(kw)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        agent.update_params(batch)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for _ in range(args.warmup):
        for _, kw in MODES:
            one(kw)
    ms = {name: [] for name, _ in MODES}
    t0 = time.time()
    for _ in range(args.repeats):                       # alternating: the modes see the same neighbours on the box
        for name, kw in MODES:
            ms[name].append(one(kw))
    wall = time.time() - t0
    last = dict(agent.update_stats)
    set_mode({})

    # ---- the monitor's launch alone, on tensors of the epoch's shapes
    A = agent.cn.policy_net.action_log_std.shape[1]
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev)
    pred, ret, adv, actions, mean, fixed = rnd(n, 1), rnd(n), rnd(n), rnd(n, A), rnd(n_pol, A), rnd(n_pol) - 70.0
    rows = torch.randperm(n, device=dev)[:n_pol].sort().values if n_pol < n else None
    log_std = agent.cn.policy_net.action_log_std.detach()
    rec = torch.empty(len(O.L.PPO_STATS_FIELDS), dtype=torch.float64, device=dev)
    call = lambda: O.ppo_stats(pred, ret, mean, actions, log_std, adv, fixed, agent.clip_epsilon, rows=rows, out=rec)
    for _ in range(5):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(50)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        call()
        b.record()
    torch.cuda.synchronize()
    launch = [a.elapsed_time(b) for a, b in ev]
    bytes_moved = 4.0 * (2 * n_pol * A + 3 * n + 3 * n_pol) + 8.0 * n_pol * (rows is not None)

    load = os.getloadavg()
    fmt = lambda v: "median %.2f ms (quartiles %.2f / %.2f, min %.2f, max %.2f, n = %d)" % (
        np.median(v), np.percentile(v, 25), np.percentile(v, 75), min(v), max(v), len(v))
    base = float(np.median(ms["off"]))
    rel = lambda k: "%+.2f %%" % (100.0 * (np.median(ms[k]) - base) / base)
    lines = [
        "# update_monitor_probe: one update_params of %d epochs" % agent.opt_num_epochs,
        "",
        "- commit: %s" % args.commit,
        "- device: %s; host load average (1 / 5 / 15 min): %.1f / %.1f / %.1f on %d CPUs" % ((torch.cuda.get_device_name(0),) + load + (os.cpu_count(),)),
        "- batch: %d rows, %d exploration rows, %d action dimensions" % (n, n_pol, A),
        "- timing: HIP events around the whole call (it ends with a device synchronise), %d warm-up updates of each mode, then %d of each, "
        "alternating (%.1f s in all); next-rollout set-up off" % (args.warmup, args.repeats, wall),
        "",
        "| mode | T_update | against off |",
        "|---|---|---|",
        "| off (defaults) | %s | |" % fmt(ms["off"]),
        "| diagnostics (`update_diagnostics=True`) | %s | %s |" % (fmt(ms["diagnostics"]), rel("diagnostics")),
        "| target_kl (`target_kl=inf`: + one host read per epoch) | %s | %s |" % (fmt(ms["target_kl"]), rel("target_kl")),
        "",
        "The monitor's launch alone (`optim.ppo_stats`, two kernels; 50 calls between HIP events): median %.1f us (min %.1f, max %.1f); "
        "%.1f MB read per call -> %.0f GB/s at the median." % (1e3 * np.median(launch), 1e3 * min(launch), 1e3 * max(launch), bytes_moved / 1e6,
                                                              bytes_moved / (1e6 * np.median(launch))),
        "",
        "Last update (target_kl = inf): epochs_run %s, approx_kl %s, clip_frac %s" % (
            last.get("epochs_run"), ["%.3g" % v for v in last.get("approx_kl", [])], ["%.3g" % v for v in last.get("clip_frac", [])]),
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
    tr.close()


if __name__ == "__main__":
    main()
