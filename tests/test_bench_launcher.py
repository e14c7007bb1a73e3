"""bench.py --gpus N starts its own ranks (one process per GPU) when it is not under torchrun; here with the
gloo backend and no GPU work (--dry-run): rendezvous, barrier-bracketed timing, sum / max aggregation over ranks and
the rank-0-only JSON line. A mismatch between --gpus and the environment must be refused, never reported as n_gpus 1."""
import json
import os
import subprocess
import sys

from conftest import REPO

BENCH = os.path.join(REPO, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_PORT")}
    env.update(HIP_VISIBLE_DEVICES="", EGP_DIST_BACKEND="gloo", **kw)
    return env


def test_bench_launches_its_own_ranks():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run", "--steps", "3"], env=_env(), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line (rank 0): %r" % out.stdout
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["steps"] == 3 and r["scaling"] == "weak" and r["dry_run"] is True
    assert r["env_steps"] == 100 * 3 * (1 + 2)                      # sum over ranks
    assert r["ms_per_step"] * 3 >= 40.0 * 0.9                         # max over ranks (rank 1 sleeps 40 ms)
    assert abs(r["value"] - r["env_steps"] / (r["ms_per_step"] * 3e-3)) < 1e-6 * r["value"]


def test_bench_refuses_a_world_size_mismatch():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--dry-run"], env=_env(WORLD_SIZE="1"), capture_output=True,
                         text=True, timeout=120)
    assert out.returncode != 0 and "WORLD_SIZE=1" in out.stderr and "{" not in out.stdout
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--dry-run"], env=_env(WORLD_SIZE="2", RANK="0", MASTER_PORT="1"),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "{" not in out.stdout


def test_bench_refuses_more_ranks_than_gpus():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "8"], env=_env(), capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "GPU(s)" in out.stderr and "{" not in out.stdout


def test_a_failing_rank_stops_the_launch():
    """Rank 1 dies before the rendezvous (bad MASTER_PORT handling is not needed: an argparse error is enough)."""
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run", "--steps", "x"], env=_env(), capture_output=True,
                         text=True, timeout=120)
    assert out.returncode != 0 and "{" not in out.stdout


import pytest


@pytest.mark.gpu
def test_two_ranks_through_the_launcher_on_a_gpu():
    """The whole multi-rank path on real hardware: bench.py starts two ranks itself; with one GPU on the box they share it
    and exchange through gloo (EGP_BENCH_SHARE_GPU=1: a self-test, not a measurement) -- env shards per rank, advantage /
    filter / logger moments merged, one flat gradient all-reduce per epoch, rank-0 line with the summed env-steps."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_PORT")}
    env.update(EGP_BENCH_SHARE_GPU="1", EGP_DIST_BACKEND="gloo")
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "1", "--envs", "128", "--min-batch", "2048",
                          "--threads", "3", "--full"], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["config"]["parallelism"] == "dp2" and r["scaling"] == "weak"
    assert r["env_steps"] >= 2 * 2048 and r["value"] > 0 and r["roofline"] is not None
    assert "legs" not in r and "cpu_baseline" not in r          # 1-GPU extras only


def test_dump_outputs_writes_float_arrays_and_samples_past_the_limit(tmp_path, monkeypatch):
    """bench.dump_outputs on a stand-in trainer: one .npy per state_dict entry (float32 stays float32, anything else becomes
    float64), the observation filter and every sampling statistic; past the byte limit a fixed seeded sample of each array."""
    import numpy as np
    import torch
    import bench
    from egopose_amd.rl_core import LoggerRL

    class Filter:
        def to_device_state(self, device):
            return np.arange(231, dtype=np.float64)

    class Trainer:
        nets = {"policy_dict": torch.nn.Linear(300, 200), "value_dict": torch.nn.Linear(40, 1).double()}
        running_state = Filter()

    torch.manual_seed(0)
    log = LoggerRL()
    log.step(None, 1.0, 0.5, np.full(5, 0.2))
    log.end_episode(None)
    log.end_sampling()
    n, size = bench.dump_outputs(str(tmp_path / "all"), Trainer, log)
    files = sorted(os.listdir(tmp_path / "all"))
    assert n == len(files) == 4 + 1 + 12 and "running_state.npy" in files and "log.avg_c_info.npy" in files
    w = np.load(tmp_path / "all" / "policy_dict.weight.npy")
    assert w.dtype == np.float32 and w.shape == (200, 300) and np.array_equal(w, Trainer.nets["policy_dict"].weight.detach().numpy())
    assert np.load(tmp_path / "all" / "value_dict.bias.npy").dtype == np.float64
    assert np.load(tmp_path / "all" / "log.avg_c_info.npy").shape == (5,)
    assert size == sum(np.load(tmp_path / "all" / f).nbytes for f in files)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", size // 4)
    for d in ("a", "b"):
        _, small = bench.dump_outputs(str(tmp_path / d), Trainer, log)
        assert small <= size // 4
    a = np.load(tmp_path / "a" / "policy_dict.weight.npy")
    assert a.ndim == 1 and a.size < w.size and np.isin(a, w).all()
    for f in files:            # the sample is fixed: two dumps of the same state agree
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f


@pytest.mark.gpu
def test_dump_outputs_are_the_same_on_every_run(tmp_path):
    """bench.py --dump-outputs twice with the same arguments: the same files, float32 / float64 only, under 64 MB, and the
    same bits (seeded inputs, and a timed path without run-to-run float reordering); --steps sets the timed steps."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_PORT")}
    dumps = []
    for run in ("a", "b"):
        d = tmp_path / run
        out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--envs", "128", "--min-batch", "2048",
                              "--threads", "3", "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
        r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        assert r["steps"] == 2 and r["ms_per_step"] > 0 and r["dump_outputs"]["arrays"] == len(os.listdir(d))
        dumps.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = dumps
    assert sorted(a) == sorted(b) and "running_state.npy" in a and "log.num_steps.npy" in a
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for f in a:
        assert a[f].dtype in (np.float32, np.float64), f
        assert np.array_equal(a[f], b[f]), f
