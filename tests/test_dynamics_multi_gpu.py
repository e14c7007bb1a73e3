"""Device dynamics with two envs per resident wave (k_pd_server_tree58_multi_dyn<2>: K8 inside the multi-env resident K1).
The comparisons and their tolerances are those of test_dynamics.py (engine == host loop with the oracle's M, C of the PREVIOUS
substep's state: 1e-9) and test_hip_parity.py (forms of the env-step agree: 1e-9), at sizes and schedules that make a wave serve
two envs: ragged and packed workgroups, envs that sit out an env-step, resets next to a running wave-mate, 'torque' actions,
2 048 slots through the rollout, a CU mask."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import dynamics as D
from oracle import humanoid as H


@pytest.fixture(scope="module")
def ctx(skel):
    from conftest import load_golden
    from egopose_amd.hip import EgpContext
    c = load_golden("config_subject_03.npz")
    cx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"])
    yield cx
    cx.close()


def _schedule(n, rng, g, steps=3, reset_before=None, inactive=None):
    """One dict per env-step: the actions, the envs reset before it (ids, qpos, qvel) and the envs that sit it out."""
    sched = []
    used = n
    for k in range(steps):
        ids = np.array(sorted((reset_before or {}).get(k, [])), dtype=np.int64)
        rq, rv = g["qpos"][used:used + len(ids)], g["qvel"][used:used + len(ids)] * 0.1
        used += len(ids)
        out = sorted((inactive or {}).get(k, []))
        mask = None
        if out:
            mask = np.ones(n, np.int32)
            mask[out] = 0
        sched.append(dict(action=rng.normal(size=(n, 52)) * 0.2, reset=(ids, rq, rv), mask=mask))
    return sched


def _run_engine(ctx, skel, n, qpos0, qvel0, sched, expect_substeps, expect_ke, n_threads=2, n_groups=1):
    """The engine with device dynamics on a backend that is only asked for qpos / qvel and whose reported bias is poison."""
    from conftest import VaryingInertiaBackend
    from egopose_amd.physics import RolloutEngine
    be = VaryingInertiaBackend(skel, n)
    got_qM = []
    orig_drain = be._drain

    def spy_drain(env, qpos, qvel, qM, bias, xpos):
        got_qM.append(qM is not None)
        orig_drain(env, qpos, qvel, qM, bias, xpos)
        bias[:] = 1e9                                  # whatever the backend reports as bias must be ignored

    be._drain = spy_drain
    eng = RolloutEngine(ctx, be, n, n_threads=n_threads, n_groups=n_groups, device_dynamics=True)
    try:
        assert eng.substeps_per_launch == expect_substeps, (eng.substeps_per_launch, eng.envs_per_wave)
        assert eng.envs_per_wave == expect_ke, eng.envs_per_wave
        eng.reset(np.arange(n), qpos0, qvel0)
        for st in sched:
            ids, rq, rv = st["reset"]
            if len(ids):
                eng.reset(ids, rq, rv)
            ad = torch.as_tensor(st["action"], device="cuda")
            torch.cuda.synchronize()
            for gi in range(n_groups):
                eng.step_async(gi, ad, active_host=st["mask"])
            for gi in range(n_groups):
                eng.wait(gi)
            torch.cuda.synchronize()
        assert not be.physics.errors and not any(got_qM)
        return eng.qpos.cpu().numpy(), eng.qvel.cpu().numpy(), [np.array(t) for t in be.torques]
    finally:
        eng.close()
        be.close()


def _check_against_host_loop(skel, envs, qpos0, qvel0, sched, got_q, logged):
    """test_dynamics.py's host loop: the oracle's stable PD fed the oracle's M, C of the previous substep's state (fresh after a
    reset only); an env that sits an env-step out is not touched. Returns how far fresh M, C would have moved a torque."""
    from conftest import load_golden
    from egopose_amd.physics import SurrogatePhysics
    c = load_golden("config_subject_03.npz")
    ref = SurrogatePhysics(skel, 1)
    fresh_err = 0.0
    for e in envs:
        ref.reset(0, qpos0[e], qvel0[e])
        M, C, _ = D.crba_rne_spatial(skel, qpos0[e], qvel0[e])             # sim.forward() of the reset
        row = 0
        for st in sched:
            ids, rq, rv = st["reset"]
            if e in ids:
                j = int(np.where(ids == e)[0][0])
                ref.reset(0, rq[j], rv[j])
                M, C, _ = D.crba_rne_spatial(skel, rq[j], rv[j])
            if st["mask"] is not None and st["mask"][e] == 0:
                continue
            a = st["action"]
            for s in range(15):
                q, v, _, _, _ = ref.drain(0, want_xpos=False)
                _, tc = H.pd_torque(q, v, a[e], M, C, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], skel.timestep)
                np.testing.assert_allclose(logged[e][row], tc[0], rtol=1e-9, atol=1e-9, err_msg="env %d substep %d" % (e, row))
                M_now, C_now, _ = D.crba_rne_spatial(skel, q, v)          # what this substep's mj_step leaves behind
                if row > 0:
                    _, tf = H.pd_torque(q, v, a[e], M_now, C_now, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], skel.timestep)
                    fresh_err = max(fresh_err, float(np.abs(tf[0] - tc[0]).max()))
                M, C = M_now, C_now
                ref.step(0, tc[0])
                row += 1
        assert len(logged[e]) == row, "env %d was stepped %d times, the schedule says %d" % (e, len(logged[e]), row)
        q, *_ = ref.drain(0, want_xpos=False)
        np.testing.assert_allclose(got_q[e], q, rtol=1e-9, atol=1e-9, err_msg="final qpos of env %d" % e)
    ref.close()
    return fresh_err


@pytest.mark.gpu
@pytest.mark.parametrize("n", [13, 16])               # two workgroups: ragged (some waves serve one env) and packed
def test_engine_device_dynamics_two_envs_per_wave_matches_host_loop(ctx, skel, n, monkeypatch):
    """The body of test_engine_device_dynamics_matches_host_loop with a resident wave serving two envs in turn: 3 env-steps, a
    partial reset before the third, every logged torque and the final qpos == the host loop with the reference's stale timing."""
    from conftest import load_golden
    monkeypatch.setenv("EGP_SERVER_KE", "2")
    g = load_golden("body_quat_obs.npz")
    rng = np.random.RandomState(2)
    qpos0, qvel0 = g["qpos"][:n], g["qvel"][:n] * 0.2
    sched = _schedule(n, rng, g, steps=3, reset_before={2: [0, 6, 9]})
    got_q, _, logged = _run_engine(ctx, skel, n, qpos0, qvel0, sched, 15, 2)
    fresh_err = _check_against_host_loop(skel, [0, 3, 4, 6, 9, n - 1], qpos0, qvel0, sched, got_q, logged)
    assert fresh_err > 1e-6, "the test cannot tell stale from fresh M, C (%g)" % fresh_err


@pytest.mark.gpu
def test_two_envs_per_wave_across_launches_and_partial_activity(ctx, skel, monkeypatch):
    """n = 13 packed by EGP_SERVER_KE=2: workgroup 0 has the envs 0-5 (waves: {0, 4}, {1, 5}, {2}, {3}), workgroup 1 the envs 6-12
    ({6, 10}, {7, 11}, {8, 12}, {9}). Env-step 2 runs without env 4 (a wave's second env), env 6 (a wave's first env) and env 9 (alone
    in its wave); before env-step 3 the envs 0 and 10 are reset while their wave-mates 4 and 6 run on. An env that sat out finds its
    HBM inertia / bias rows as its last substep left them: neither advanced nor overwritten."""
    from conftest import load_golden
    monkeypatch.setenv("EGP_SERVER_KE", "2")
    g = load_golden("body_quat_obs.npz")
    n = 13
    rng = np.random.RandomState(5)
    qpos0, qvel0 = g["qpos"][:n], g["qvel"][:n] * 0.2
    sched = _schedule(n, rng, g, steps=4, reset_before={2: [0, 10]}, inactive={1: [4, 6, 9]})
    got_q, _, logged = _run_engine(ctx, skel, n, qpos0, qvel0, sched, 15, 2)
    fresh_err = _check_against_host_loop(skel, [0, 4, 6, 9, 10, 12], qpos0, qvel0, sched, got_q, logged)
    assert fresh_err > 1e-6, "the test cannot tell stale from fresh M, C (%g)" % fresh_err


@pytest.mark.gpu
def test_device_dynamics_forms_agree(ctx, skel, monkeypatch):
    """The same inputs through the one-env resident kernel, the two-env one and the per-substep launch pairs."""
    from conftest import load_golden
    g = load_golden("body_quat_obs.npz")
    n = 21
    qpos0, qvel0 = g["qpos"][:n], g["qvel"][:n] * 0.2
    sched = _schedule(n, np.random.RandomState(11), g, steps=3, reset_before={1: [2, 7, 20]}, inactive={2: [5, 13]})
    res = {}
    for name, env, sub, ke in [("ke1", {"EGP_SERVER_KE": "1"}, 15, 1), ("ke2", {"EGP_SERVER_KE": "2"}, 15, 2), ("per-substep", {"EGP_SERVER": "0"}, 1, 0)]:
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            q, v, _ = _run_engine(ctx, skel, n, qpos0, qvel0, sched, sub, ke, n_threads=3, n_groups=2)
        res[name] = (q, v)
    for a, b in [("ke1", "ke2"), ("ke2", "per-substep"), ("ke1", "per-substep")]:
        np.testing.assert_allclose(res[a][0], res[b][0], rtol=1e-9, atol=1e-9, err_msg="qpos %s vs %s" % (a, b))
        np.testing.assert_allclose(res[a][1], res[b][1], rtol=1e-9, atol=1e-9, err_msg="qvel %s vs %s" % (a, b))


@pytest.mark.gpu
def test_torque_actions_through_the_two_env_device_dynamics_kernel(skel, monkeypatch):
    """cfg.action_type = 'torque' (humanoid_v1.py:167-172) through k_pd_server_tree58_multi_dyn: the clipped control itself, no solve,
    no K8 -- against the host loop with the oracle's control law."""
    from conftest import load_golden
    from egopose_amd.hip import EgpContext
    from egopose_amd.physics import SurrogatePhysics, RolloutEngine
    monkeypatch.setenv("EGP_SERVER_KE", "2")
    c = load_golden("config_subject_03.npz")
    g = load_golden("body_quat_obs.npz")
    cx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"], obs_options=dict(action_type="torque"))
    n = 23
    rng = np.random.RandomState(19)
    qpos0, qvel0 = g["qpos"][:n], g["qvel"][:n] * 0.2
    action = rng.normal(size=(n, 52)) * 40.0                 # some beyond the limits (50 ... 200)
    ph = SurrogatePhysics(skel, n)
    eng = RolloutEngine(cx, ph, n, n_threads=3, n_groups=2, device_dynamics=True)
    assert eng.substeps_per_launch == 15 and eng.envs_per_wave == 2
    eng.reset(np.arange(n), qpos0, qvel0)
    act_d = torch.as_tensor(action, device="cuda")
    torch.cuda.synchronize()
    for gi in range(2):
        eng.step_async(gi, act_d)
    for gi in range(2):
        eng.wait(gi)
    torch.cuda.synchronize()
    got_q, got_v = eng.qpos.cpu().numpy(), eng.qvel.cpu().numpy()
    eng.close()
    ph.close()
    cx.close()
    ref = SurrogatePhysics(skel, n)
    _, tc = H.control_torque("torque", None, None, action, None, None, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], skel.timestep)
    assert (np.abs(tc) == c["torque_lim"]).any()
    for e in range(n):
        ref.reset(e, qpos0[e], qvel0[e])
        for s in range(15):
            ref.step(e, tc[e])
        q, v, _, _, _ = ref.drain(e)
        np.testing.assert_allclose(got_q[e], q, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(got_v[e], v, rtol=1e-12, atol=1e-12)
    ref.close()


@pytest.mark.gpu
def test_2048_slots_device_dynamics_take_the_resident_form_and_replay(tmp_path_factory, skel, monkeypatch):
    """EGP_DEVICE_DYNAMICS=1 with more slots than the chip holds one-env waves for: the engine keeps the resident env-step with two
    envs per wave; a sample of the episodes -- first / last slots of both groups, in-batch restarts -- replays on the oracle env
    with device dynamics and does NOT replay with the backend's constant inertia."""
    from egopose_amd.bench_support import write_synthetic_dataset
    from egopose_amd.config import Config
    from egopose_amd.physics import default_threads
    from egopose_amd.train import Trainer
    from test_rollout_gpu import _replay_episodes
    monkeypatch.setenv("EGP_DEVICE_DYNAMICS", "1")
    root = str(tmp_path_factory.mktemp("egp_2048_dyn"))
    write_synthetic_dataset(root, "subject_03", n_takes=4, n_frames=600)
    os.chdir(root)
    cfg = Config("subject_03", create_dirs=False)
    cfg.num_optim_epoch = 1
    cfg.env_episode_len = 12
    n_threads = max(2, default_threads(share=1, device_index=0))
    tr = Trainer(cfg, torch.device("cuda", 0), torch.float32, num_envs=2048, num_threads=n_threads, num_groups=2)
    tr.pre_iter_update(0)
    tr.agent.running_state = None
    tr.env.end_reward = 0.9
    batch, log = tr.agent.sample(2048 * 20)
    eng = tr.agent._get_rollout().engine
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert eng.device_dynamics
    assert eng.substeps_per_launch == 15, "2 048 device-dynamics slots must keep the resident env-step"
    assert eng.envs_per_wave == 2 or 4 * cus >= 2048
    assert 2048 // (4 * eng.envs_per_wave) <= eng.resident_capacity
    ends = np.where(batch.masks == 0)[0]
    n_ep = len(ends)
    assert len(batch) >= 2048 * 20 and ends[-1] == len(batch) - 1
    sample = sorted({0, 1, n_ep // 4, n_ep // 2 - 1, n_ep // 2, n_ep - 2, n_ep - 1})
    _replay_episodes(tr, cfg, skel, batch, sample, 0.9, device_dynamics=True)
    with pytest.raises(AssertionError):
        _replay_episodes(tr, cfg, skel, batch, sample[:1], 0.9, device_dynamics=False)
    tr.close()


@pytest.mark.gpu
def test_device_dynamics_keeps_the_resident_form_when_cus_are_masked():
    """1 024 device-dynamics slots with 16 CUs masked off: the probe counts what is there, a wave serves two envs instead of the
    engine dropping to one launch pair per substep, and two env-steps equal the unmasked run. The mask must be set before HIP
    starts: subprocesses, each under its own timeout."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(repo, "tools", "cu_mask_check.py"), "--envs", "1024", "--step", "--device-dynamics"]

    def run(extra):
        out = subprocess.run(cmd, env=dict(os.environ, **extra), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads(out.stdout.strip().splitlines()[-1])
    full = run({})
    assert full["device_dynamics"] is True
    cus = full["cus_reported"]
    if cus < 64:
        pytest.skip("needs a chip with >= 64 CUs")
    keep = cus - 16
    masked = run({"ROC_GLOBAL_CU_MASK": "0x" + "f" * (keep // 4)})
    assert masked["device_dynamics"] is True
    assert full["substeps_per_launch"] == 15 and masked["substeps_per_launch"] == 15
    assert full["envs_per_wave"] == 1 or full["resident_capacity"] < 256
    assert masked["resident_capacity"] <= keep, "the probe must not count more workgroups than CUs were left: %r" % (masked,)
    if 4 * masked["resident_capacity"] < 1024:
        assert masked["envs_per_wave"] == 2
    assert masked["qpos_abs_sum"] == pytest.approx(full["qpos_abs_sum"], rel=1e-9)
    np.testing.assert_allclose(masked["qpos_probe"], full["qpos_probe"], rtol=1e-9, atol=1e-9)


@pytest.mark.gpu
def test_four_envs_per_wave_with_device_dynamics_falls_back_to_per_substep(ctx, skel, monkeypatch):
    """There is no four-env device-dynamics kernel (its float64 factor rows do not fit the LDS next to the K8 scratch):
    EGP_SERVER_KE=4 ends in the per-substep form, without an error, and steps correctly."""
    from conftest import load_golden
    monkeypatch.setenv("EGP_SERVER_KE", "4")
    g = load_golden("body_quat_obs.npz")
    n = 13
    rng = np.random.RandomState(2)
    qpos0, qvel0 = g["qpos"][:n], g["qvel"][:n] * 0.2
    sched = _schedule(n, rng, g, steps=2, reset_before={1: [3]})
    got_q, _, logged = _run_engine(ctx, skel, n, qpos0, qvel0, sched, 1, 0)
    _check_against_host_loop(skel, [0, 3, 12], qpos0, qvel0, sched, got_q, logged)
