"""ForecastEvaluator (egopose_amd/evaluate_forecast.py): the sliding-window forecasts of ego_forecast_eval.py batched onto lockstep
env slots -- layout and expert rows, the oracle's CPU env replaying windows from the traced actions, the frozen filter, the
actions against a float64 chain, independence of the slot count, ego_mimic-based starts, save + statistics, the phase column."""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M_, T_ = 30, 12          # fr_margin of the shipped config, the tests' episode length


@pytest.fixture(scope="module")
def workspace(tmp_path_factory):
    from egopose_amd.bench_support import write_synthetic_dataset
    root = str(tmp_path_factory.mktemp("egp_ws_feval"))
    write_synthetic_dataset(root, "subject_03", n_takes=3, n_frames=300, seed=4)
    return root


def _forecast_trainer(workspace, n_env, episode_len, obs_phase=False, **kw):
    from egopose_amd.config import ForecastConfig
    from egopose_amd.train import Trainer
    os.chdir(workspace)
    cfg = ForecastConfig("subject_03", create_dirs=False)
    cfg.env_episode_len = episode_len
    cfg.num_optim_epoch = 2
    if obs_phase:
        cfg.obs_phase = True
    return Trainer(cfg, torch.device("cuda", 0), torch.float32, num_envs=n_env, **kw), cfg


def _evaluator(tr, cfg, n_slots, **kw):
    from egopose_amd.evaluate_forecast import ForecastEvaluator
    return ForecastEvaluator(cfg, tr.env, tr.policy_net, tr.policy_vs_net, running_state=tr.running_state, num_envs=n_slots, n_threads=2,
                             keep_trace=True, **kw)


@pytest.fixture(scope="module")
def run8(workspace):
    """One trainer (a sampling pass first: the running filter has real statistics) and the gt_init run on 8 slots that the
    tests below share: 27 windows in 4 passes, the last with 3 slots."""
    tr, cfg = _forecast_trainer(workspace, 8, T_, num_threads=2, num_groups=1)
    assert cfg.fr_margin == M_
    tr.pre_iter_update(0)
    tr.agent.sample(8 * 24)
    assert tr.running_state.rs.n > 100
    ev = _evaluator(tr, cfg, 8, gt_init=True)
    results, meta = ev.run()
    assert ev.timing["passes"] == 4 and ev.timing["windows"] == 27
    yield tr, cfg, ev, results, meta
    tr.close()


def test_gt_init_layout_and_expert_rows(run8):
    tr, cfg, ev, results, meta = run8
    env = tr.env
    assert meta == {"algo": "ego_forecast"} and set(results) == {"traj_pred", "traj_orig"}
    assert list(results["traj_pred"]) == list(env.expert_list)
    assert ev.trace["take_ind"].tolist() == sorted(ev.trace["take_ind"].tolist()) and len(ev.trace["take_ind"]) == 27
    for i, take in enumerate(env.expert_list):
        pred, orig = results["traj_pred"][take], results["traj_orig"][take]
        assert pred.shape == orig.shape == (9, M_ + T_, 59)
        qpos = env.expert_arr[i]["qpos"]
        for w in range(9):
            s = M_ * (w + 1)
            np.testing.assert_array_equal(orig[w], qpos[s - M_:s + T_])
            np.testing.assert_array_equal(pred[w, :M_], qpos[s - M_:s])
            np.testing.assert_array_equal(pred[w, M_], qpos[s])               # seated on the expert's state, no init noise
        assert np.abs(pred[:, M_ + 1:] - orig[:, M_ + 1:]).max() > 1e-6       # (the windows were simulated, not copied)


def test_windows_replayed_by_the_oracle_env(run8, skel):
    """6 windows spread over the 4 passes (24 .. 26 are the partial pass): the oracle's CPU env seated on the window's start state
    and driven with the traced actions reproduces every frame (tolerances of test_eval_driver_replayed_by_oracle_env)."""
    from egopose_amd.physics import SurrogatePhysics
    from oracle.cpu_env import OracleHumanoidEnv
    from oracle import humanoid as H
    tr, cfg, ev, results, meta = run8
    env, trc = tr.env, ev.trace
    ph = SurrogatePhysics(skel, 1)
    ref = OracleHumanoidEnv(skel, cfg, ph, env.expert_arr, env.cnn_feat)
    for w in (0, 7, 8, 13, 23, 25):
        e, s = int(trc["take_ind"][w]), int(trc["start_ind"][w])
        ref.expert_ind, ref.start_ind, ref.cur_t = e, s, 0
        ph.reset(0, env.expert_arr[e]["qpos"][s], env.expert_arr[e]["qvel"][s])
        ref._drain(True)
        ref.bquat = H.body_quat(ref.qpos, skel.body_qpos_start, skel.body_ndof)[0]
        pred = results["traj_pred"][env.expert_list[e]][s // M_ - 1]
        for t in range(T_):
            np.testing.assert_allclose(pred[M_ + t], ref.qpos, rtol=1e-7, atol=1e-7, err_msg="window %d frame %d" % (w, t))
            np.testing.assert_allclose(trc["qvel"][w, t], ref.qvel, rtol=1e-6, atol=1e-6, err_msg="window %d frame %d" % (w, t))
            ref.step(trc["actions"][w, t])
    ph.close()


def test_traced_states_are_the_frozen_filter_of_the_observations(run8):
    tr, cfg, ev, results, meta = run8
    trc = ev.trace
    sim = tr.env.batched(8, 0, 2, 1)
    rs = tr.running_state
    n_before = rs.rs.n
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    pred = np.concatenate([results["traj_pred"][t] for t in tr.env.expert_list])[:, M_:]          # [27, T, 59], window order
    obs = sim.ctx.obs(dev(pred.reshape(-1, 59)), dev(trc["qvel"].reshape(-1, 58))).cpu().numpy()
    want = np.stack([rs(o, update=False) for o in obs]).reshape(27, T_, -1)
    np.testing.assert_allclose(trc["states"], want, rtol=1e-9, atol=1e-9)
    assert rs.rs.n == n_before and np.abs(want).max() <= 5.0


def test_traced_actions_against_a_float64_chain(run8):
    """float64 LSTMCell carried from zero over the traced states, float64 policy mean over [context | h], the context from
    policy_vs_net in float64 over the window's margin frames; 2e-4 = the bound of
    test_forecast_rollout_matches_train_mode_nets_and_oracle_env for the same float32 kernels."""
    tr, cfg, ev, results, meta = run8
    trc = ev.trace
    pol64 = copy.deepcopy(tr.policy_net).double()
    cell64, vcell64 = copy.deepcopy(tr.policy_vs_net.s_net.rnn_f).double(), copy.deepcopy(tr.policy_vs_net.v_net.rnn_f).double()
    W = len(trc["take_ind"])
    win = np.stack([tr.env.cnn_feat[e][s - M_:s] for e, s in zip(trc["take_ind"], trc["start_ind"])], 1)      # (m, W, D)
    with torch.no_grad():
        x = torch.as_tensor(win, dtype=torch.float64, device="cuda")
        hv = torch.zeros(W, vcell64.hidden_size, dtype=torch.float64, device="cuda")
        cv = torch.zeros_like(hv)
        for f in range(M_):                        # VideoForecastNet.context: the causal LSTM's last output
            hv, cv = vcell64(x[f], (hv, cv))
        ctx = hv
        h = torch.zeros(W, cell64.hidden_size, dtype=torch.float64, device="cuda")
        c = torch.zeros_like(h)
        for t in range(T_):
            st = torch.as_tensor(trc["states"][:, t], dtype=torch.float64, device="cuda")
            h, c = cell64(st, (h, c))
            mean, _ = pol64.mean_std(torch.cat((ctx, h), 1))
            np.testing.assert_allclose(trc["actions"][:, t], mean.cpu().numpy(), rtol=2e-4, atol=2e-4, err_msg="tick %d" % t)
    assert np.abs(trc["actions"]).max() > 1e-3


def test_results_do_not_depend_on_the_slot_count(run8):
    tr, cfg, ev, results, meta = run8
    ev5 = _evaluator(tr, cfg, 5, gt_init=True)
    r5, _ = ev5.run()
    assert ev5.timing["passes"] == 6
    ev32 = _evaluator(tr, cfg, 32, gt_init=True)       # more slots than windows: the one pass leaves five slots without a window
    r32, _ = ev32.run()
    assert ev32.timing["passes"] == 1
    for evn, rn in ((ev5, r5), (ev32, r32)):
        for take in results["traj_pred"]:
            np.testing.assert_array_equal(rn["traj_pred"][take], results["traj_pred"][take])
            np.testing.assert_array_equal(rn["traj_orig"][take], results["traj_orig"][take])
        np.testing.assert_array_equal(evn.trace["actions"], ev.trace["actions"])
        np.testing.assert_array_equal(evn.trace["states"], ev.trace["states"])


def test_ego_mimic_based_start(run8):
    """em results = the expert's own trajectory (rows [em_off, L - em_off)): every window starts where gt_init starts it, up to
    sync_traj's rounding; the first window of a take lacks em_off rows of history, which come from the expert (:128-131)."""
    tr, cfg, ev, results, meta = run8
    env = tr.env
    em_off = 10
    em = {"traj_pred": {}, "vel_pred": {}}
    for take, ex in zip(env.expert_list, env.expert_arr):
        L = ex["qpos"].shape[0]
        em["traj_pred"][take], em["vel_pred"][take] = ex["qpos"][em_off:L - em_off], ex["qvel"][em_off:L - em_off]
    ev_em = _evaluator(tr, cfg, 8, gt_init=False, em_res=em, em_off=em_off)
    r_em, meta_em = ev_em.run()
    assert meta_em == meta
    miss = ev_em.miss_len.reshape(3, 9)
    assert (miss[:, 0] == em_off).all() and (miss[:, 1:8] == 0).all()
    assert (miss[:, 8] == 0).all()                                  # the last window ends at frame 282 <= 290 = the em result's end
    for i, take in enumerate(env.expert_list):
        np.testing.assert_allclose(r_em["traj_pred"][take][:, M_:], results["traj_pred"][take][:, M_:], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(r_em["traj_pred"][take][:, :M_], results["traj_pred"][take][:, :M_], rtol=1e-12, atol=1e-12)
        np.testing.assert_array_equal(r_em["traj_pred"][take][0, :em_off], env.expert_arr[i]["qpos"][:em_off])
        np.testing.assert_array_equal(r_em["traj_orig"][take], results["traj_orig"][take])


def test_save_and_statistics_round_trip(run8, workspace):
    from egopose_amd import metrics as M
    tr, cfg, ev, results, meta = run8
    cfg.result_dir = os.path.join(workspace, "results_feval")
    path = ev.save(results, meta, 3, data="test")
    assert path.endswith("iter_0003_test_gt.p")
    r2, m2 = pickle.load(open(path, "rb"))
    assert m2 == {"algo": "ego_forecast"}
    out = M.compute_forecast_metrics(r2, cfg.fr_margin, 10)
    assert np.isfinite([out["pose_dist"], out["vel_dist"], out["accels"]]).all() and out["pose_dist"] > 0
    take = tr.env.expert_list[1]
    pred, orig = r2["traj_pred"][take], r2["traj_orig"][take]
    want = np.mean([M.get_mean_dist(M.get_joint_angles(pred[w, M_:M_ + 10]), M.get_joint_angles(orig[w, M_:M_ + 10])) for w in range(9)])
    np.testing.assert_allclose(out["per_take"][take][0], want, rtol=1e-12)
    full = M.compute_forecast_metrics(r2, cfg.fr_margin, T_)
    assert np.isfinite(list(full["per_take"][take])).all()
    assert M.forecast_err_vs_horizon(r2, cfg.fr_margin, T_, step=5).shape == (2,)


def test_phase_observation(workspace):
    """cfg.obs_phase: state width 116, the last column of the filtered state is the frozen filter of min(t / 12, 1); without a
    running state (as test_forecast_rollout_with_phase_observation_and_random_cur_t runs it) it is that number itself."""
    tr, cfg = _forecast_trainer(workspace, 4, T_, obs_phase=True, num_threads=2, num_groups=1)
    assert tr.env.observation_space.shape[0] == 116
    tr.running_state = None
    ev = _evaluator(tr, cfg, 4, gt_init=True)
    results, _ = ev.run(takes=[tr.env.expert_list[0]])
    assert list(results["traj_pred"]) == [tr.env.expert_list[0]] and results["traj_pred"][tr.env.expert_list[0]].shape == (9, M_ + T_, 59)
    st = ev.trace["states"]
    assert st.shape == (9, T_, 116) and ev.timing["passes"] == 3
    for t in range(T_):
        np.testing.assert_array_equal(st[:, t, -1], np.full(9, min(t / 12.0, 1.0)))
    tr.close()
