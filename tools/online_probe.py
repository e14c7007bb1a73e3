"""Cost of the online (`--causal`) evaluation's policy contexts and of the evaluation itself:
`python tools/online_probe.py <len> [<takes>] [<num_envs>]` prints one JSON line.

1. One take of <len> synthetic frames through the config's policy video net (subject_03: 128 -> 128 bi-LSTM, margin 10):
   `VideoStateNet.online_contexts` against the loop it replaces, `initialize(x[:t + 2m + 1]); v_out[t]` for every tick
   (ego_pose/ego_mimic_eval.py:143-145). HIP events around each, after a warm-up of both; the median of the repeats, and their
   spread. The largest difference of the two tables is printed next to the times.
2. <takes> (default 8) synthetic takes of <len> frames: `BatchedOnlineEvaluator` on <num_envs> (default 8) slots against
   `Evaluator(causal=True)`, the take-by-take path that is all the parent commit has. Wall seconds of run(), each after a warm-up run on one take;
   untrained nets, the value head scaled as in the tests so that `valuefs` re-seats now and then."""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, repeats):
    """Milliseconds of fn() by HIP events, `repeats` times -> (median, min, max)."""
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def contexts(n_frames, cfg, loop_repeats=3, repeats=9):
    from egopose_amd import lstm as hl
    from egopose_amd.nets import VideoStateNet
    torch.manual_seed(cfg.seed)
    net = VideoStateNet(128, cfg.policy_v_hdim, cfg.fr_margin, cfg.policy_v_net, cfg.policy_v_net_param, cfg.causal).cuda()
    net.eval()
    net.set_mode("test")
    m = cfg.fr_margin
    x = torch.as_tensor(np.random.RandomState(2).normal(size=(n_frames, 128)), dtype=torch.float32, device="cuda")
    T = n_frames - 2 * m

    @torch.no_grad()
    def loop():
        rows = []
        for t in range(T):
            net.initialize(x[:t + 2 * m + 1])
            rows.append(net.v_out[t])
        return torch.stack(rows, 0)

    n0 = hl.WINDOW_CALLS
    a, b = net.online_contexts(x), loop()                      # warm-up of both, and the comparison
    out = {"frames": n_frames, "ticks": T, "v_net": cfg.policy_v_net, "window_launches_per_call": hl.WINDOW_CALLS - n0,
           "max_abs_diff": float((a - b).abs().max())}
    out["online_contexts_ms"], out["online_contexts_ms_min"], out["online_contexts_ms_max"] = _timed(lambda: net.online_contexts(x), repeats)
    out["prefix_loop_ms"], out["prefix_loop_ms_min"], out["prefix_loop_ms_max"] = _timed(loop, loop_repeats)
    out["ratio"] = out["prefix_loop_ms"] / out["online_contexts_ms"]
    return out


def evaluation(n_frames, n_takes, num_envs, cfg_id="subject_03", fail_safe="valuefs"):
    from egopose_amd.bench_support import write_synthetic_dataset
    from egopose_amd.config import Config
    from egopose_amd.evaluate import BatchedOnlineEvaluator, Evaluator
    from egopose_amd.nets import VideoRegNet
    from egopose_amd.train import Trainer
    root = tempfile.mkdtemp(prefix="egp_online_")
    write_synthetic_dataset(root, cfg_id, n_takes=n_takes, n_frames=n_frames, seed=4)
    os.chdir(root)
    cfg = Config(cfg_id, create_dirs=False)
    tr = Trainer(cfg, torch.device("cuda", 0), torch.float32, num_envs=64, num_threads=4, num_groups=1)
    tr.agent.sample(64 * 20)
    env = tr.env
    torch.manual_seed(11)
    state_net = VideoRegNet(115, 128, env.cnn_feat[0].shape[-1]).cuda()
    ex, m = env.expert_arr[0], cfg.fr_margin
    mean, std = np.concatenate([ex["qpos"][m:, 2:], ex["qvel"][m:]], 1).mean(0), np.full(115, 0.02)
    with torch.no_grad():
        tr.value_net.value_head.weight.mul_(30.0)
    args = (cfg, env, tr.policy_net, tr.policy_vs_net, tr.value_net, tr.value_vs_net, state_net, mean, std)
    out = {"takes": n_takes, "frames": n_frames, "num_envs": num_envs, "fail_safe": fail_safe}
    first = env.expert_list[:1]
    Evaluator(*args, running_state=tr.running_state, fail_safe=fail_safe, causal=True).run(takes=first)        # kernels, libraries warm
    seq = Evaluator(*args, running_state=tr.running_state, fail_safe=fail_safe, causal=True)
    torch.cuda.synchronize()
    t0 = time.time()
    _, meta = seq.run()
    torch.cuda.synchronize()
    out["sequential_s"], out["sequential_resets"] = time.time() - t0, meta["num_reset"]
    BatchedOnlineEvaluator(*args, running_state=tr.running_state, fail_safe=fail_safe, num_envs=num_envs).run(takes=first)
    bat = BatchedOnlineEvaluator(*args, running_state=tr.running_state, fail_safe=fail_safe, num_envs=num_envs)
    torch.cuda.synchronize()
    t0 = time.time()
    _, meta = bat.run()
    torch.cuda.synchronize()
    out["batched_online_s"], out["batched_online_resets"] = time.time() - t0, meta["num_reset"]
    out["batched_online_timing"] = dict(bat.timing)
    out["speedup"] = out["sequential_s"] / out["batched_online_s"]
    tr.close()
    return out, cfg


def main(n_frames, n_takes=8, num_envs=8):
    ev, cfg = evaluation(n_frames, n_takes, num_envs)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "contexts": contexts(n_frames, cfg), "evaluation": ev}, default=float))


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(*(int(a) for a in sys.argv[1:4]))
