"""Wall time of the ego_mimic evaluation on one synthetic dataset, take by take (`Evaluator`) and side by side
(`BatchedEvaluator`): `python tools/mimic_eval_compare.py [n_takes] [n_frames] [num_envs]` prints one JSON line.
Untrained nets; the value head is scaled as in the tests so that `valuefs` re-seats now and then."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(n_takes=8, n_frames=2000, num_envs=8, fail_safe="valuefs"):
    from egopose_amd.bench_support import write_synthetic_dataset
    from egopose_amd.config import Config
    from egopose_amd.evaluate import BatchedEvaluator, Evaluator
    from egopose_amd.nets import VideoRegNet
    from egopose_amd.train import Trainer
    root = tempfile.mkdtemp(prefix="egp_meval_")
    write_synthetic_dataset(root, "subject_03", n_takes=n_takes, n_frames=n_frames, seed=4)
    os.chdir(root)
    cfg = Config("subject_03", create_dirs=False)
    tr = Trainer(cfg, torch.device("cuda", 0), torch.float32, num_envs=64, num_threads=4, num_groups=1)
    tr.agent.sample(64 * 20)
    env = tr.env
    torch.manual_seed(11)
    state_net = VideoRegNet(115, 128, env.cnn_feat[0].shape[-1]).cuda()
    ex = env.expert_arr[0]
    m = cfg.fr_margin
    mean, std = np.concatenate([ex["qpos"][m:, 2:], ex["qvel"][m:]], 1).mean(0), np.full(115, 0.02)
    with torch.no_grad():
        tr.value_net.value_head.weight.mul_(30.0)
    args = (cfg, env, tr.policy_net, tr.policy_vs_net, tr.value_net, tr.value_vs_net, state_net, mean, std)
    out = {"n_takes": n_takes, "n_frames": n_frames, "num_envs": num_envs, "fail_safe": fail_safe}
    seq = Evaluator(*args, running_state=tr.running_state, fail_safe=fail_safe)
    t0 = time.time()
    _, meta = seq.run()
    out["sequential_s"], out["sequential_resets"] = time.time() - t0, meta["num_reset"]
    bat = BatchedEvaluator(*args, running_state=tr.running_state, fail_safe=fail_safe, num_envs=num_envs)
    bat.run(takes=env.expert_list[:1])                      # engine, kernels and pinned buffers warm
    bat = BatchedEvaluator(*args, running_state=tr.running_state, fail_safe=fail_safe, num_envs=num_envs)
    _, meta = bat.run()
    out["batched_s"], out["batched_resets"], out["batched_timing"] = bat.timing["total"], meta["num_reset"], bat.timing
    print(json.dumps(out))
    tr.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    main(*(int(x) for x in a[:3]), *(a[3:4]))
