#!/usr/bin/env python3
"""One mini-batch PPO update (AgentPPO(use_mini_batch=True).update_policy) on both of its paths, in one process:

  fused   optim.minibatch_plan per epoch + optim.ppo_losses_mb and one clip + Adam step per mini-batch, no host read inside
  plain   the reference's formulation (agents/agent_ppo.py:24-44) in torch ops on the same nets and the same fused optimizer:
          column gathers per epoch, nonzero() + index gathers + the element-wise losses + two optimizer steps per mini-batch

at N = 50 000 rows, opt_batch_size 64, D = 76, A = 52, hidden (300, 200). HIP events bracket update_policy; the kernel launches of
a short run (10 mini-batches) are counted with torch.profiler. Prints a text report (profiles/minibatch_probe.txt).

    python tools/probes/minibatch_probe.py [--rows 50000] [--batch 64] [--epochs 1] [--commit HASH]
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from egopose_amd.agent import AgentPPO                       # noqa: E402
from egopose_amd.nets import MLP, PolicyGaussian, Value       # noqa: E402


def make_agent(D, A, hidden, batch, epochs, fused):
    torch.manual_seed(0)
    p_net = PolicyGaussian(MLP(D, list(hidden), "relu"), A, log_std=-1.0, fix_std=False).cuda()
    v_net = Value(MLP(D, list(hidden), "relu")).cuda()
    p_params = list(p_net.parameters())
    agent = AgentPPO(env=types.SimpleNamespace(cfg=types.SimpleNamespace(seed=1)), dtype=torch.float32, device=torch.device("cuda", 0),
                     running_state=None, custom_reward=None, policy_net=p_net, value_net=v_net,
                     optimizer_policy=torch.optim.Adam(p_params, lr=5e-5), optimizer_value=torch.optim.Adam(v_net.parameters(), lr=3e-4),
                     opt_num_epochs=epochs, clip_epsilon=0.2, policy_grad_clip=[(p_params, 40.0)], opt_batch_size=batch, use_mini_batch=True)
    agent.use_fused_loss = fused
    assert agent._fused_losses() == fused
    return agent


def columns(N, D, A, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    exps = (torch.rand(N, device="cuda", generator=g) < 0.85).float()
    return rnd(N, D), rnd(N, A) * 0.3, rnd(N, 1), rnd(N, 1), exps


def timed_update(agent, cols):
    np.random.seed(0)
    torch.cuda.synchronize()
    ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev[0].record()
    agent.update_policy(*cols)
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def launches_per_minibatch(agent, cols, n_mb):
    """Device kernels + memcpy / memset nodes per mini-batch of a run of `n_mb` mini-batches (one epoch), or None."""
    try:
        from torch.profiler import ProfilerActivity, profile
        np.random.seed(0)
        agent.update_policy(*cols)              # same shapes once before: no first-call work in the count
        torch.cuda.synchronize()
        np.random.seed(0)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            agent.update_policy(*cols)
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n / float(n_mb) if n else None
    except Exception as e:                      # the profiler is a convenience here; the timings do not depend on it
        print("# launch count unavailable: %r" % (e,))
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    D, A, hidden = 76, 52, (300, 200)
    n_mb = -(-args.rows // args.batch) * args.epochs
    print("minibatch_probe: commit %s, %s, load average %.2f %.2f %.2f" % ((args.commit, torch.cuda.get_device_name(0)) + os.getloadavg()))
    print("N = %d, opt_batch_size = %d, D = %d, A = %d, hidden %s, epochs = %d -> %d mini-batches per update" %
          (args.rows, args.batch, D, A, hidden, args.epochs, n_mb))
    cols = columns(args.rows, D, A)
    short = columns(10 * args.batch, D, A, seed=1)
    result = {}
    for name, fused in (("fused", True), ("plain", False)):
        agent = make_agent(D, A, hidden, args.batch, args.epochs, fused)
        timed_update(agent, short)              # warm-up: library handles, the flat optimizer buffers, allocator blocks
        ms = [timed_update(agent, cols) for _ in range(args.repeats)]
        short_agent = make_agent(D, A, hidden, args.batch, 1, fused)
        per_mb = launches_per_minibatch(short_agent, short, 10)
        result[name] = min(ms)
        print("%-5s  update_policy %s ms (min %.1f ms, %.1f us per mini-batch), device launches per mini-batch: %s" %
              (name, " ".join("%.1f" % m for m in ms), min(ms), 1e3 * min(ms) / n_mb, "%.1f" % per_mb if per_mb else "n/a"))
    print("fused / plain = %.3f" % (result["fused"] / result["plain"]))


if __name__ == "__main__":
    main()
