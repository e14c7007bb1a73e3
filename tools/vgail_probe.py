#!/usr/bin/env python3
"""Time one `AgentVGAIL.update_discriminator` (discrim_num_update = 10) at the update's own batch, both forms.

    python tools/vgail_probe.py [rows] [--commit ID] [--out FILE]

Builds the bench's set-up (subject_03's nets over the synthetic dataset, 1 024 env slots) with `Trainer(gail={})`, samples one
batch of at least `rows` rows (default: the config's min_batch_size, which the bench's rollout turns into ~134 k rows) and times
the discriminator update on it with HIP events: the fused form (one sweep per step, one stacked block, HIP loss tail, fused clip +
Adam) and the reference-structured plain float32 torch form (`use_fused_discrim = False`), alternating, after warm-up updates of
both. Writes a markdown record (both medians, their spread, the commit, the box's load) to --out and prints it."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rows", nargs="?", type=int, default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    out = os.path.abspath(args.out) if args.out else None        # (before the chdir into the workspace)
    if not torch.cuda.is_available():
        raise SystemExit("vgail_probe times the MI355X: no ROCm device visible")
    from egopose_amd.bench_support import write_synthetic_dataset
    from egopose_amd.config import Config
    from egopose_amd.physics import default_threads
    from egopose_amd.train import Trainer
    root = tempfile.mkdtemp(prefix="egp_vgail_probe_")
    write_synthetic_dataset(root, "subject_03")
    os.chdir(root)
    cfg = Config("subject_03", create_dirs=False)
    tr = Trainer(cfg, torch.device("cuda", 0), torch.float32, num_envs=1024, num_threads=max(2, default_threads(share=1, device_index=0)),
                 num_groups=2, gail={})
    agent = tr.agent
    tr.pre_iter_update(0)
    batch, _ = agent.sample(args.rows or cfg.min_batch_size)
    c = agent._load_batch(batch)
    v_metas = agent._v_metas_of(batch)
    n = c["states"].shape[0]
    n_ep = int((c["masks"] == 0).sum())

    def one(fused):
        agent.use_fused_discrim = fused
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        e_loss = agent.update_discriminator(c["states"], c["masks"], v_metas)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), e_loss

    for _ in range(args.warmup):
        one(True), one(False)
    ms = {True: [], False: []}
    t0 = time.time()
    for _ in range(args.repeats):                       # alternating: both forms see the same neighbours on the box
        for fused in (True, False):
            ms[fused].append(one(fused)[0])
    wall = time.time() - t0
    load = os.getloadavg()
    fmt = lambda v: "median %.2f ms (min %.2f, max %.2f, n = %d)" % (np.median(v), min(v), max(v), len(v))
    vs, dn = agent.cn.discrim_vs_net, agent.cn.discrim_net
    lines = [
        "# vgail_probe: one update_discriminator of %d steps" % agent.discrim_num_update,
        "",
        "- commit: %s" % args.commit,
        "- device: %s; host load average (1 / 5 / 15 min): %.1f / %.1f / %.1f on %d CPUs" % ((torch.cuda.get_device_name(0),) + load + (os.cpu_count(),)),
        "- batch: %d rows in %d episodes; state width %d, context width %d, CNN feature width %d, margin %d; MLP %s"
        % (n, n_ep, c["states"].shape[1], vs.v_hdim, vs.cnn_feat_dim, vs.v_margin, [l.out_features for l in dn.net.affine_layers]),
        "- timing: HIP events around the whole call (it ends with the host reading e_loss), %d warm-up updates of each form, then %d of each, "
        "alternating (%.1f s in all)" % (args.warmup, args.repeats, wall),
        "",
        "| form | time per update |",
        "|---|---|",
        "| fused (`use_fused_discrim = True`, the default) | %s |" % fmt(ms[True]),
        "| plain float32 torch, the reference's structure (`use_fused_discrim = False`) | %s |" % fmt(ms[False]),
        "",
        "fused / plain = %.2f" % (np.median(ms[True]) / np.median(ms[False])),
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
