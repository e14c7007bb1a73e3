"""The ego_mimic evaluation with the takes side by side: the actor + critic step (`egp_policy_step_f32` (`vlayers`),
FusedActorCritic) against the policy step it shares its code with and against float64 chains, and BatchedEvaluator
(egopose_amd/evaluate.py) replayed by the oracle's CPU env, its `valuefs` decisions against the sequential statistic, its
independence of the slot count, its pickle and the forecast evaluation that starts from it."""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

S_, NU_ = 115, 52
FAIL_SAFES = ("naivefs", "valuefs", "none")


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


# ====================================================================================================== the kernel
@pytest.fixture(scope="module")
def ctx(skel):
    from egopose_amd.hip import EgpContext
    c = load_golden("config_subject_03.npz")
    cx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"])
    yield cx
    cx.close()


def _rows(rng, n):
    qpos = rng.normal(size=(n, 59)) * 0.4
    qpos[:, 3:7] = rng.normal(size=(n, 4))
    qpos[:, 3:7] /= np.linalg.norm(qpos[:, 3:7], axis=1, keepdims=True)
    return dev(qpos), dev(rng.normal(size=(n, 58)))


def _frozen_stats(ctx, rng):
    """Running statistics of 300 observation rows: what an evaluation freezes."""
    st0 = torch.zeros(1 + 2 * S_, dtype=torch.float64, device="cuda")
    st = torch.empty_like(st0)
    q, v = _rows(rng, 300)
    ctx.obs_zfilter(q, v, st0, st, 5.0, torch.empty(300, S_, dtype=torch.float64, device="cuda"))
    return st


def _nets(Hp=128, Hv=128, seed=11):
    from egopose_amd.nets import MLP, PolicyGaussian, Value
    torch.manual_seed(seed)
    pol = PolicyGaussian(MLP(Hp + S_, (300, 200), "relu"), NU_, log_std=-2.3).cuda()
    val = Value(MLP(Hv + S_, (300, 200), "relu")).cuda()
    with torch.no_grad():
        val.value_head.weight.mul_(30.0)
        val.value_head.bias.fill_(1.0)
    return pol, val


def _value64(val, vctx, t_idx, y):
    v64 = copy.deepcopy(val).double()
    x = torch.cat((vctx[torch.arange(vctx.shape[0], device="cuda"), t_idx].double(), y), 1)
    with torch.no_grad():
        return v64.value_head(v64.net(x)).reshape(-1).cpu().numpy()


def test_actor_is_bit_identical_to_the_policy_step_and_values_match_float64(ctx):
    """5 rows (the 4-row tile does not divide them), the config's 128 + 115 -> 300 -> 200 -> 52 / 1 nets, frozen statistics."""
    from egopose_amd import policy_step
    n, T = 5, 7
    rng = np.random.RandomState(3)
    pol, val = _nets()
    assert policy_step.supported(pol) and policy_step.supported_value(val)
    fac = policy_step.FusedActorCritic(pol, val, torch.device("cuda"))
    fp = policy_step.FusedGaussianPolicy(pol, torch.device("cuda"))
    st = _frozen_stats(ctx, rng)
    qp, qv = _rows(rng, n)
    pctx, vctx = torch.randn(n, T, 128, device="cuda"), torch.randn(n, T, 128, device="cuda")
    t_idx = torch.randint(0, T, (n,), device="cuda")
    for noise in (None, torch.randn(n, NU_, device="cuda")):
        y_r, y2_r = torch.zeros(n, S_, dtype=torch.float64, device="cuda"), torch.zeros(n, S_, dtype=torch.float64, device="cuda")
        a_r, m_r = torch.zeros(n, NU_, dtype=torch.float64, device="cuda"), torch.zeros(n, NU_, device="cuda")
        fp.with_filter(ctx, pctx, t_idx, qp, qv, st, None, 5.0, y_r, y2_r, None, a_r, noise=noise, mean_out=m_r)
        y, y2, a, m = torch.zeros_like(y_r), torch.zeros_like(y_r), torch.zeros_like(a_r), torch.zeros_like(m_r)
        v = torch.zeros(n, device="cuda")
        fac.with_filter(ctx, pctx, t_idx, qp, qv, st, None, 5.0, y, y2, None, a, vctx, v, noise=noise, mean_out=m)
        assert torch.equal(a, a_r) and torch.equal(y, y_r) and torch.equal(y2, y2_r) and torch.equal(m, m_r)
        assert a.abs().max() > 1e-3 and y.abs().max() > 0.1 and y.abs().max() <= 5.0
        np.testing.assert_allclose(v.cpu().numpy(), _value64(val, vctx, t_idx, y), rtol=2e-4, atol=2e-4)
    # the frozen filter is running_state(x, update=False) of the same statistics
    raw = ctx.obs(qp, qv).cpu().numpy()
    s = st.cpu().numpy()
    want = np.clip((raw - s[1:1 + S_]) / (np.sqrt(s[1 + S_:] / (s[0] - 1)) + 1e-8), -5, 5)
    np.testing.assert_allclose(y.cpu().numpy(), want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("n,Hv,filtered", [(1, 128, True), (70, 128, False), (6, 64, True)])
def test_values_rows_widths_and_canaries(ctx, n, Hv, filtered):
    """1 row; 70 rows (18 workgroups per net) without a filter; a value context narrower than the policy's. The outputs are
    allocated for n + 3 rows, canary-filled: rows >= n stay untouched."""
    from egopose_amd import policy_step
    T = 5
    rng = np.random.RandomState(10 + n)
    pol, val = _nets(128, Hv)
    fac = policy_step.FusedActorCritic(pol, val, torch.device("cuda"))
    st = _frozen_stats(ctx, rng) if filtered else None
    qp, qv = _rows(rng, n)
    pctx, vctx = torch.randn(n, T, 128, device="cuda"), torch.randn(n, T, Hv, device="cuda")
    t_idx = torch.randint(0, T, (n,), device="cuda")
    y = torch.full((n + 3, S_), -7.0, dtype=torch.float64, device="cuda")
    a = torch.full((n + 3, NU_), -7.0, dtype=torch.float64, device="cuda")
    v = torch.full((n + 3,), -7.0, device="cuda")
    fac.with_filter(ctx, pctx, t_idx, qp, qv, st, None, 5.0, y[:n], None, None, a[:n], vctx, v[:n])
    assert (y[n:] == -7.0).all() and (a[n:] == -7.0).all() and (v[n:] == -7.0).all()
    assert (a[:n] != -7.0).all() and (v[:n] != -7.0).all()
    if not filtered:
        assert torch.equal(y[:n], ctx.obs(qp, qv))
    np.testing.assert_allclose(v[:n].cpu().numpy(), _value64(val, vctx, t_idx, y[:n]), rtol=2e-4, atol=2e-4)
    p64 = copy.deepcopy(pol).double()
    with torch.no_grad():
        mean, _ = p64.mean_std(torch.cat((pctx[torch.arange(n, device="cuda"), t_idx].double(), y[:n]), 1))
    np.testing.assert_allclose(a[:n].cpu().numpy(), mean.cpu().numpy(), rtol=2e-4, atol=2e-4)
    with pytest.raises(ValueError):
        fac.with_filter(ctx, pctx, t_idx, qp, qv, st, None, 5.0, y[:n], None, None, a[:n], torch.randn(n, T, Hv + 1, device="cuda"), v[:n])


# ====================================================================================================== the driver
@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """3 takes of 60 frames (test_len 40), take 1 cut to 45 (test_len 25); a trainer whose running filter has seen a sampling
    pass; a state regressor; the value head scaled so that `valuefs` fires now and then."""
    from egopose_amd.bench_support import write_synthetic_dataset
    from egopose_amd.config import Config
    from egopose_amd.nets import VideoRegNet
    from egopose_amd.train import Trainer
    root = str(tmp_path_factory.mktemp("egp_ws_meval"))
    write_synthetic_dataset(root, "subject_03", n_takes=3, n_frames=60, seed=6)
    os.chdir(root)
    cfg = Config("subject_03", create_dirs=False)
    cfg.env_episode_len = 15
    cfg.num_optim_epoch = 2
    tr = Trainer(cfg, torch.device("cuda", 0), torch.float32, num_envs=8, num_threads=2, num_groups=1)
    cfg.env_init_noise = 0.0
    tr.agent.sample(8 * 20)
    assert tr.running_state.rs.n > 100
    env = tr.env
    assert env.cnn_feat[0].shape[0] == 60 and cfg.fr_margin == 10
    env.cnn_feat[1] = env.cnn_feat[1][:45]
    env.expert_arr[1] = {k: (v[:45] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == 60 else v) for k, v in env.expert_arr[1].items()}
    if "len" in env.expert_arr[1]:
        env.expert_arr[1]["len"] = 45
    torch.manual_seed(11)
    state_net = VideoRegNet(115, 128, env.cnn_feat[0].shape[-1]).cuda()
    ex = env.expert_arr[0]
    obs_like = np.concatenate([ex["qpos"][10:, 2:], ex["qvel"][10:]], 1)
    with torch.no_grad():
        tr.value_net.value_head.weight.mul_(30.0)
        tr.value_net.value_head.bias.fill_(1.0)
    out = dict(tr=tr, cfg=cfg, env=env, root=root, state_net=state_net, mean=obs_like.mean(0), std=np.full(115, 0.02))
    # ... and, the head being linear, moved to mean 1 / standard deviation 1 over a run without fail-safe: a good part of the
    # values, not all, then lies below 0.6 x the running mean
    from egopose_amd.evaluate import BatchedEvaluator
    ev = BatchedEvaluator(cfg, env, tr.policy_net, tr.policy_vs_net, tr.value_net, tr.value_vs_net, state_net, out["mean"], out["std"],
                          running_state=tr.running_state, fail_safe="none", keep_trace=True, num_envs=3, n_threads=2)
    ev.run()
    v = np.concatenate([ev.trace[t]["values"] for t in env.expert_list])
    print("value head before calibration: mean %.4f std %.4f" % (v.mean(), v.std()))
    with torch.no_grad():
        head = tr.value_net.value_head
        head.bias.copy_(1.0 + (head.bias - float(v.mean())) / float(v.std()))
        head.weight.div_(float(v.std()))
    yield out
    tr.close()


_RUNS = {}


def _run(setup, fail_safe, n_slots):
    """One BatchedEvaluator run per (fail_safe, slot count), shared by the tests (a fresh evaluator: a fresh value statistic)."""
    from egopose_amd.evaluate import BatchedEvaluator
    key = (fail_safe, n_slots)
    if key not in _RUNS:
        tr = setup["tr"]
        ev = BatchedEvaluator(setup["cfg"], setup["env"], tr.policy_net, tr.policy_vs_net, tr.value_net, tr.value_vs_net, setup["state_net"],
                              setup["mean"], setup["std"], running_state=tr.running_state, fail_safe=fail_safe, keep_trace=True,
                              num_envs=n_slots, n_threads=2)
        results, meta = ev.run()
        _RUNS[key] = (ev, results, meta)
    return _RUNS[key]


@pytest.mark.parametrize("fail_safe", ["naivefs", "valuefs"])
def test_takes_replayed_by_the_oracle_env(setup, skel, fail_safe):
    """3 takes on 2 slots (one full pass, one partial): the oracle's CPU env driven with the traced actions, re-seated where the
    trace says so on the traced state_pred, reproduces every frame (tolerances of test_eval_driver_replayed_by_oracle_env)."""
    from egopose_amd import metrics as M
    from egopose_amd.physics import SurrogatePhysics
    from oracle.cpu_env import OracleHumanoidEnv
    from oracle import humanoid as H
    ev, results, meta = _run(setup, fail_safe, 2)
    env, cfg = setup["env"], copy.copy(setup["cfg"])
    m = cfg.fr_margin
    assert ev.timing["takes"] == 3 and ev.timing["passes"] >= 2 and ev.timing["ticks"] >= 40 + 40
    assert list(results["traj_pred"]) == list(env.expert_list) and set(results) == {"traj_pred", "traj_orig", "vel_pred"}
    assert meta == {"algo": "ego_mimic", "num_reset": sum(len(ev.trace[t]["resets"]) for t in env.expert_list)}
    ph = SurrogatePhysics(skel, 1)
    for i, take in enumerate(env.expert_list):
        test_len = 25 if i == 1 else 40
        pred, orig, vel = results["traj_pred"][take], results["traj_orig"][take], results["vel_pred"][take]
        assert pred.shape == orig.shape == (test_len, 59) and vel.shape == (test_len, 58)          # the short take ends at its own length
        ex = env.expert_arr[i]
        np.testing.assert_array_equal(orig, ex["qpos"][m:m + test_len])
        trc = ev.trace[take]
        assert trc["actions"].shape == (test_len, 52) and trc["values"].shape == (test_len,) and trc["state_pred"].shape == (test_len, 115)
        cfg.env_episode_len = test_len
        ref = OracleHumanoidEnv(skel, cfg, ph, env.expert_arr, env.cnn_feat)
        ref.expert_ind, ref.start_ind, ref.cur_t = i, m, 0

        def seat(state, ref_qpos):
            qpos = ref_qpos.copy()
            qpos[2:] = state[:57]
            qvel = state[57:].copy()
            M.align_human_state(qpos, qvel, ref_qpos)
            ph.reset(0, qpos, qvel)
            ref._drain(True)
            ref.bquat = H.body_quat(ref.qpos, skel.body_qpos_start, skel.body_ndof)[0]

        seat(trc["state_pred"][0], ex["qpos"][m])
        resets = set(trc["resets"])
        for t in range(test_len):
            np.testing.assert_allclose(pred[t], ref.qpos, rtol=1e-7, atol=1e-7, err_msg="take %d frame %d" % (i, t))
            np.testing.assert_allclose(vel[t], ref.qvel, rtol=1e-6, atol=1e-6, err_msg="take %d frame %d" % (i, t))
            _, _, _, info = ref.step(trc["actions"][t])
            if info["end"]:
                assert t == test_len - 1 and t not in resets
                break
            if fail_safe == "naivefs":
                assert info["fail"] == (t in resets)
            if t in resets:
                seat(trc["state_pred"][t + 1], ref.qpos)
    ph.close()


def test_valuefs_decisions_are_the_sequential_statistic_s(setup):
    from egopose_amd.zfilter import RunningStat
    ev, results, meta = _run(setup, "valuefs", 2)
    stat = RunningStat(1)
    n_reset = n_kept = 0
    for take in setup["env"].expert_list:
        trc = ev.trace[take]
        want = []
        for t, v in enumerate(trc["values"]):
            stat.push(np.array([float(v)]))
            if t == len(trc["values"]) - 1:
                break
            if v < 0.6 * stat.mean[0]:
                want.append(t)
            else:
                n_kept += 1
        assert want == list(trc["resets"]), take
        n_reset += len(want)
    print("valuefs: %d re-seats, %d decisions without, scheduler passes %s" % (n_reset, n_kept, ev.timing["fs_pass_takes"]))
    assert meta["num_reset"] == n_reset and n_reset >= 1 and n_kept >= 1
    assert ev.value_stat.n == stat.n == 105 and ev.value_stat.mean[0] == stat.mean[0]
    assert 1 <= ev.timing["fs_passes"] <= 3 and ev.timing["fs_pass_takes"][0] == 3


@pytest.mark.parametrize("fail_safe", ["valuefs", "none"])
def test_traced_values_and_actions_against_float64_chains(setup, fail_safe):
    ev, results, meta = _run(setup, fail_safe, 2)
    tr, env = setup["tr"], setup["env"]
    pol64, val64 = copy.deepcopy(tr.policy_net).double(), copy.deepcopy(tr.value_net).double()
    for i, take in enumerate(env.expert_list):
        trc = ev.trace[take]
        feat = torch.as_tensor(env.cnn_feat[i], dtype=torch.float32, device="cuda")
        st = dev(trc["states"])
        assert np.abs(trc["states"]).max() <= 5.0
        with torch.no_grad():
            tr.policy_vs_net.initialize(feat)
            tr.value_vs_net.initialize(feat)
            mean, _ = pol64.mean_std(torch.cat((tr.policy_vs_net.v_out.double(), st), 1))
            value = val64.value_head(val64.net(torch.cat((tr.value_vs_net.v_out.double(), st), 1))).reshape(-1)
        np.testing.assert_allclose(trc["actions"], mean.cpu().numpy(), rtol=2e-4, atol=2e-4, err_msg=take)
        np.testing.assert_allclose(trc["values"], value.cpu().numpy(), rtol=2e-4, atol=2e-4, err_msg=take)
        assert np.abs(trc["actions"]).max() > 1e-3


@pytest.mark.parametrize("fail_safe", FAIL_SAFES)
def test_results_do_not_depend_on_the_slot_count(setup, fail_safe):
    ev2, r2, m2 = _run(setup, fail_safe, 2)
    ev3, r3, m3 = _run(setup, fail_safe, 3)
    ev5, r5, m5 = _run(setup, fail_safe, 5)            # more slots than takes: the first pass leaves two slots without a take
    assert m2 == m3 == m5 and ev3.timing["passes"] < ev2.timing["passes"]
    if fail_safe == "none":
        assert m2["num_reset"] == 0
    for evn, rn in ((ev3, r3), (ev5, r5)):
        for take in setup["env"].expert_list:
            for k in ("traj_pred", "vel_pred", "traj_orig"):
                np.testing.assert_array_equal(r2[k][take], rn[k][take])
            a, b = ev2.trace[take], evn.trace[take]
            np.testing.assert_array_equal(a["actions"], b["actions"])
            np.testing.assert_array_equal(a["values"], b["values"])
            np.testing.assert_array_equal(a["states"], b["states"])
            assert list(a["resets"]) == list(b["resets"])


@pytest.mark.parametrize("fail_safe", ["valuefs", "naivefs"])
def test_save_metrics_and_the_forecast_evaluation_on_top(setup, fail_safe):
    from egopose_amd.evaluate import Evaluator, compute_metrics
    ev, results, meta = _run(setup, fail_safe, 2)
    cfg = copy.copy(setup["cfg"])
    cfg.result_dir = os.path.join(setup["root"], "results_meval")
    ev_cfg, ev.cfg = ev.cfg, cfg
    try:
        path = ev.save(results, meta, 7, data="test")
    finally:
        ev.cfg = ev_cfg
    assert path.endswith("iter_0007_test%s.p" % ("" if fail_safe == "valuefs" else "_naivefs"))
    assert type(ev).save is Evaluator.save
    r2, m2 = pickle.load(open(path, "rb"))
    assert m2 == meta and set(r2) == {"traj_pred", "traj_orig", "vel_pred"} and set(m2) == {"algo", "num_reset"}
    for take in setup["env"].expert_list:
        np.testing.assert_array_equal(r2["traj_pred"][take], results["traj_pred"][take])
    out = compute_metrics(r2)
    assert np.isfinite([out["pose_dist"], out["vel_dist"], out["accels"]]).all() and out["pose_dist"] > 0
    if fail_safe == "valuefs":
        from egopose_amd.config import ForecastConfig
        from egopose_amd.evaluate_forecast import ForecastEvaluator
        from egopose_amd.train import Trainer
        os.chdir(setup["root"])
        fcfg = ForecastConfig("subject_03", create_dirs=False)
        fcfg.env_episode_len = 10
        ftr = Trainer(fcfg, torch.device("cuda", 0), torch.float32, num_envs=4, num_threads=2, num_groups=1)
        try:
            ftr.env.set_experts(setup["env"].expert_list, setup["env"].expert_arr, setup["env"].cnn_feat)
            fev = ForecastEvaluator(fcfg, ftr.env, ftr.policy_net, ftr.policy_vs_net, running_state=None, gt_init=False, em_res=r2,
                                    em_off=setup["cfg"].fr_margin, num_envs=5, n_threads=2)
            fres, fmeta = fev.run()
            assert fmeta == {"algo": "ego_forecast"} and set(fres["traj_pred"]) == set(setup["env"].expert_list)
            assert all(np.isfinite(v).all() for v in fres["traj_pred"].values())
        finally:
            ftr.close()


def test_refusals_and_the_selection_helper(setup):
    from egopose_amd.evaluate import BatchedEvaluator, Evaluator, select_evaluator
    tr = setup["tr"]
    args = (setup["cfg"], setup["env"], tr.policy_net, tr.policy_vs_net, tr.value_net, tr.value_vs_net, setup["state_net"], setup["mean"], setup["std"])
    with pytest.raises(NotImplementedError, match="Evaluator"):
        BatchedEvaluator(*args, causal=True)
    with pytest.raises(NotImplementedError, match="Evaluator"):
        BatchedEvaluator(*args, show_noise=True)
    assert select_evaluator(tr.policy_net, tr.value_net, num_envs=4) == (BatchedEvaluator, None)
    assert select_evaluator(tr.policy_net, tr.value_net, num_envs=1) == (Evaluator, None)
    assert select_evaluator(tr.policy_net, tr.value_net, num_envs=4, sequential=True) == (Evaluator, None)
    cls, why = select_evaluator(tr.policy_net, copy.deepcopy(tr.value_net).double(), num_envs=4)
    assert cls is Evaluator and "float32" in why
    cls, why = select_evaluator(tr.policy_net, tr.value_net, num_envs=4, causal=True)
    assert cls is Evaluator and why
    with pytest.raises(NotImplementedError, match="Evaluator"):
        BatchedEvaluator(*args[:4], copy.deepcopy(tr.value_net).double(), *args[5:])
