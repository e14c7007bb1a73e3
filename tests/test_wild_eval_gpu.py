"""ego_mimic on feature-only takes (egopose_amd/evaluate_wild.py): the env without experts, BatchedWildEvaluator's independence of the
slot count, its `valuefs` decisions against the sequential statistic (the last tick's included), the take-by-take WildEvaluator, and
the saved result scored by the 2D keypoint kernel; ForecastEvaluator's feature-only mode on top of that result; both CLIs end to end."""
import os
import pickle
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S_, NU_, FEAT = 115, 52, 32
LENS = {"wild_c": 24, "wild_a": 31, "wild_b": 40}           # feature rows; test_len = 4, 11, 20 with the config's margin of 10


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """Three feature-only takes, random nets (the value head scaled so that `valuefs` fires), a frozen filter that has seen 300
    observation-like rows, an env that never loads an expert."""
    from egopose_amd.bench_support import write_synthetic_dataset
    from egopose_amd.config import Config
    from egopose_amd.env import HumanoidEnv
    from egopose_amd.nets import MLP, PolicyGaussian, Value, VideoRegNet, VideoStateNet
    from egopose_amd.zfilter import ZFilter
    root = str(tmp_path_factory.mktemp("egp_ws_wild"))
    write_synthetic_dataset(root, "subject_03", n_takes=1, n_frames=60, seed=6)       # (the config wants its meta file; no take of it is used)
    os.chdir(root)
    cfg = Config("subject_03", create_dirs=False)
    assert cfg.fr_margin == 10
    cfg.result_dir = os.path.join(root, "results_wild")
    rng = np.random.RandomState(21)
    feats = {take: rng.normal(size=(n, FEAT)) for take, n in LENS.items()}
    env = HumanoidEnv(cfg)
    env.seed(cfg.seed)
    torch.manual_seed(5)
    pol_vs, val_vs = VideoStateNet(FEAT, 128, 10, "lstm"), VideoStateNet(FEAT, 128, 10, "lstm")
    pol = PolicyGaussian(MLP(128 + S_, (300, 200), "relu"), NU_, log_std=-2.3)
    val = Value(MLP(128 + S_, (300, 200), "relu"))
    state_net = VideoRegNet(S_, 128, FEAT)
    with torch.no_grad():
        val.value_head.weight.mul_(30.0)
        val.value_head.bias.fill_(1.0)
    for net in (pol_vs, val_vs, pol, val, state_net):
        net.cuda()
    rest = env.rest_qpos()
    mean = np.concatenate([rest[2:], np.zeros(58)])
    mean[0] = 0.9
    zf = ZFilter((S_,), clip=5.0)
    for _ in range(300):
        zf(mean + rng.normal(size=S_) * 0.3)
    out = dict(cfg=cfg, env=env, feats=feats, nets=(pol, pol_vs, val, val_vs, state_net, mean, np.full(S_, 0.02)), zf=zf, root=root)
    # ... and, the head being linear, moved to mean 1 / standard deviation 1 over a run in which the rule never fired (the values
    # of the head as built lie close to its bias): a good part of the values, not all, then lies below 0.6 x the running mean
    from egopose_amd.evaluate_wild import BatchedWildEvaluator
    ev = BatchedWildEvaluator(cfg, env, feats, *out["nets"], running_state=zf, keep_trace=True, num_envs=3, n_threads=2)
    ev.run()
    assert ev.num_reset == 0
    v = np.concatenate([ev.trace[t]["values"] for t in LENS])
    print("wild value head before calibration: mean %.4f std %.4f" % (v.mean(), v.std()))
    with torch.no_grad():
        val.value_head.bias.copy_(1.0 + (val.value_head.bias - float(v.mean())) / float(v.std()))
        val.value_head.weight.div_(float(v.std()))
    yield out
    env.close()


_RUNS = {}


def _batched(setup, n_slots):
    from egopose_amd.evaluate_wild import BatchedWildEvaluator
    if n_slots not in _RUNS:
        ev = BatchedWildEvaluator(setup["cfg"], setup["env"], setup["feats"], *setup["nets"], running_state=setup["zf"], keep_trace=True,
                                  num_envs=n_slots, n_threads=2)
        _RUNS[n_slots] = (ev,) + ev.run()
    return _RUNS[n_slots]


def test_env_without_experts_resets_to_the_rest_pose(setup, skel):
    """humanoid_v1.py:227-230: rest pose with qpos[2] += 1, zero velocity, cur_t = 0; step() and batched(N) work without experts."""
    env = setup["env"]
    assert env.expert_list is None
    obs = env.reset()
    want = np.zeros(59)
    want[:3], want[3] = skel.body_pos[0], 1.0
    want[2] += 1.0
    np.testing.assert_array_equal(env.data.qpos, want)
    np.testing.assert_array_equal(env.data.qvel, np.zeros(58))
    assert env.cur_t == 0 and obs.shape == (S_,)
    _, _, done, info = env.step(np.zeros(NU_))
    assert info["fail"] is False and env.cur_t == 1
    assert env.batched(2, 0, 2, 1).experts is None


def test_results_do_not_depend_on_the_slot_count(setup):
    ev2, r2, m2 = _batched(setup, 2)
    ev3, r3, m3 = _batched(setup, 3)
    ev5, r5, m5 = _batched(setup, 5)                   # more slots than takes: the first pass leaves two slots without a take
    assert m2 == m3 == m5 == {"algo": "ego_mimic"} and set(r2) == {"traj_pred", "vel_pred"}
    assert list(r2["traj_pred"]) == list(LENS) and ev3.timing["passes"] < ev2.timing["passes"]
    for take, n in LENS.items():
        assert r2["traj_pred"][take].shape == (n - 20, 59) and r2["vel_pred"][take].shape == (n - 20, 58)
        for evn, rn in ((ev3, r3), (ev5, r5)):
            for k in ("traj_pred", "vel_pred"):
                np.testing.assert_array_equal(r2[k][take], rn[k][take])
            a, b = ev2.trace[take], evn.trace[take]
            for k in ("actions", "values", "states"):
                np.testing.assert_array_equal(a[k], b[k])
            assert list(a["resets"]) == list(b["resets"])
    # the first seat: state_pred[0] on the rest pose's position and heading
    first = r2["traj_pred"]["wild_c"][0]
    np.testing.assert_array_equal(first[:2], setup["env"].rest_qpos()[:2])
    np.testing.assert_allclose(first[2:3], ev2.trace["wild_c"]["state_pred"][0, :1], rtol=0, atol=0)


def test_valuefs_decisions_are_the_sequential_statistic_s(setup):
    """A RunningStat replay of the traced values in take order; the decision is also taken on a take's last tick. (With the
    calibrated head: 17 of the 35 decisions re-seat.)"""
    from egopose_amd.zfilter import RunningStat
    ev, results, meta = _batched(setup, 2)
    stat = RunningStat(1)
    n_reset = n_kept = 0
    for take in LENS:
        trc = ev.trace[take]
        want = []
        for t, v in enumerate(trc["values"]):
            stat.push(np.array([float(v)]))
            if v < 0.6 * stat.mean[0]:
                want.append(t)
            else:
                n_kept += 1
        assert want == list(trc["resets"]), take
        n_reset += len(want)
    print("wild valuefs: %d decisions to re-seat, %d without, scheduler passes %s" % (n_reset, n_kept, ev.timing["fs_pass_takes"]))
    assert ev.num_reset == n_reset and n_kept >= 1
    assert any(t + 1 < LENS["wild_b"] - 20 for t in ev.trace["wild_b"]["resets"])          # a re-seat inside the long take
    assert ev.value_stat.n == stat.n == 35 and ev.value_stat.mean[0] == stat.mean[0]


def test_sequential_wild_evaluator_against_the_batched_one(setup):
    """Float32 torch nets take by take against the fused step: actions / values at the tolerance test_mimic_eval_batched_gpu.py uses
    between the fused step and float64 chains (2e-4), on the ticks before the first decision that differs; a take whose first such
    decision is a near-tie (|value - 0.6 mean| below that tolerance) is skipped from there on -- at most one of the three.
    Measured on an MI355X with these seeds: the sequential path's smallest margins are 7.3e-2 (wild_c), 2.2e-1 (wild_a) and
    1.0e-1 (wild_b), no decision differs between the two paths, and their traj_pred rows differ by at most 2.6e-9."""
    from egopose_amd.evaluate_wild import WildEvaluator
    tol = 2e-4
    evb, rb, _ = _batched(setup, 2)
    ev = WildEvaluator(setup["cfg"], setup["env"], setup["feats"], *setup["nets"], running_state=setup["zf"], keep_trace=True)
    rs, ms = ev.run()
    assert ms == {"algo": "ego_mimic"} and list(rs["traj_pred"]) == list(LENS)
    from egopose_amd.zfilter import RunningStat
    stat, skipped = RunningStat(1), 0
    for take, n in LENS.items():
        a, b = ev.trace[take], evb.trace[take]
        margins = []
        for v in a["values"]:
            stat.push(np.array([v]))
            margins.append(abs(v - 0.6 * stat.mean[0]))
        print("take %s: smallest margin |value - 0.6 mean| of the sequential path %.3e" % (take, min(margins)))
        assert min(margins) > tol                  # the seeds were chosen so that the sequential path alone has no near-tie
        T = n - 20
        assert rs["traj_pred"][take].shape == (T, 59) and len(a["values"]) == T
        ra, rb_ = set(a["resets"]), set(b["resets"])
        diff = sorted(t for t in range(T) if (t in ra) != (t in rb_))
        upto = T if not diff else diff[0] + 1
        if diff:
            skipped += 1
            print("take %s: decisions differ first at tick %d (values %.6f / %.6f)" % (take, diff[0], a["values"][diff[0]], b["values"][diff[0]]))
        np.testing.assert_allclose(np.array(a["values"])[:upto], b["values"][:upto], rtol=tol, atol=tol, err_msg=take)
        np.testing.assert_allclose(np.array(a["actions"])[:upto], b["actions"][:upto], rtol=tol, atol=tol, err_msg=take)
        np.testing.assert_allclose(rs["traj_pred"][take][0], rb["traj_pred"][take][0], rtol=1e-9, atol=1e-9, err_msg=take)    # the same seat
        d_traj = np.abs(rs["traj_pred"][take][:upto] - rb["traj_pred"][take][:upto])
        print("take %s: largest |traj_pred difference| over rows [:%d] %.3e" % (take, upto, d_traj.max()))
        np.testing.assert_allclose(rs["traj_pred"][take][:upto], rb["traj_pred"][take][:upto], rtol=tol, atol=tol, err_msg=take)
    assert skipped <= 1


def test_saved_result_scored_by_the_kernel(setup, skel):
    from egopose_amd.pose2d import Pose2DContext, eval_pose_wild_stats
    ev, results, meta = _batched(setup, 3)
    path = ev.save(results, meta, 7, data="wild_xx")
    assert path.endswith("iter_0007_wild_xx.p")
    r2, m2 = pickle.load(open(path, "rb"))
    assert m2 == {"algo": "ego_mimic"} and set(r2) == {"traj_pred", "vel_pred"}
    pctx = Pose2DContext(skel)
    b2 = pctx.body2id

    def loader(take, gt_fr):
        r = np.random.RandomState(gt_fr)
        gt = np.zeros((12, 3))
        gt[:, 0], gt[:, 1], gt[:, 2] = r.uniform(400, 1500, 12), np.sort(r.uniform(100, 1000, 12)), r.uniform(0.2, 1.0, 12)
        if gt_fr % 4 == 0:
            gt[b2["RightUpLeg"], 2] = gt[b2["LeftUpLeg"], 2] = 0.0
        return gt
    tpv = {"traj_ub": {"wild_b": 15}, "tpv_offset": {"wild_a": -2}, "tpv_flip": {"wild_c": True}}
    sim = setup["env"].batched(3, 0, 2, 1)
    out = eval_pose_wild_stats(r2, tpv, loader, setup["cfg"], backend="hip", ctx=sim.ctx, pose_ctx=pctx)
    host = eval_pose_wild_stats(r2, tpv, loader, setup["cfg"], backend="host", pose_ctx=pctx)
    assert np.isfinite([out["pose_dist"], out["accels"]]).all() and out["pose_dist"] > 0
    np.testing.assert_allclose(out["pose_dist"], host["pose_dist"], rtol=1e-12)


def test_main_round_trip_on_a_data_dir(setup, capsys):
    """`evaluate --test-feat NAME` on a data dir with a features file, a checkpoint and a state regressor writes the pickle;
    `--mode wild-stats` scores it against keypoint files with the kernel, and agrees with the host loop."""
    import json
    from egopose_amd import evaluate
    from egopose_amd.zfilter import dump_reference_pickle
    cfg = setup["cfg"]
    pol, pol_vs, val, val_vs, state_net, sn_mean, sn_std = setup["nets"]
    os.chdir(setup["root"])
    rng = np.random.RandomState(8)
    feats = {"rt_a": rng.normal(size=(24, FEAT)), "rt_b": rng.normal(size=(27, FEAT))}           # test_len 4 and 7
    os.makedirs("%s/features" % cfg.data_dir, exist_ok=True)
    with open("%s/features/cnn_feat_wild_rt.p" % cfg.data_dir, "wb") as f:
        pickle.dump((feats, {}), f)
    cpu = lambda net: {k: v.cpu() for k, v in net.state_dict().items()}
    with open("%s/iter_0003.p" % cfg.model_dir, "wb") as f:
        dump_reference_pickle(dict(policy_dict=cpu(pol), policy_vs_dict=cpu(pol_vs), value_dict=cpu(val), value_vs_dict=cpu(val_vs),
                                   running_state=setup["zf"]), f)
    sn_cfg = types.SimpleNamespace(v_hdim=128, cnn_type="resnet", mlp_dim=(300, 200), v_net="lstm", v_net_param=None, causal=False)
    os.makedirs(os.path.dirname(cfg.state_net_model), exist_ok=True)
    with open(cfg.state_net_model, "wb") as f:
        pickle.dump(({"state_net_dict": cpu(state_net)}, {"cfg": sn_cfg, "mean": sn_mean, "std": sn_std}), f)
    with open("%s/meta/meta_wild_rt.yml" % cfg.data_dir, "w") as f:
        f.write("traj_ub: {rt_b: 7}\ntpv_offset: {rt_a: 12}\ntpv_flip: {rt_b: true}\n")
    for take in feats:
        os.makedirs("%s/tpv/poses/%s" % (cfg.data_dir, take), exist_ok=True)
        for fr in range(0, 30):
            kp = np.zeros((25, 3))
            kp[:, 0], kp[:, 1], kp[:, 2] = rng.uniform(400, 1500, 25), rng.uniform(100, 1000, 25), rng.uniform(0.2, 1.0, 25)
            with open("%s/tpv/poses/%s/%05d_keypoints.json" % (cfg.data_dir, take, fr), "w") as f:
                json.dump({"people": [{"pose_keypoints_2d": kp.reshape(-1).tolist()}]}, f)
    args = ["--cfg", "subject_03", "--iter", "3", "--test-feat", "wild_rt"]
    evaluate.main(args + ["--num-envs", "2"])
    assert "iter_0003_wild_rt.p" in capsys.readouterr().out
    results, meta = pickle.load(open("results/egomimic/subject_03/results/iter_0003_wild_rt.p", "rb"))
    assert meta == {"algo": "ego_mimic"} and list(results["traj_pred"]) == ["rt_a", "rt_b"]
    assert results["traj_pred"]["rt_a"].shape == (4, 59) and results["vel_pred"]["rt_b"].shape == (7, 58)
    assert all(np.isfinite(results[k][t]).all() for k in results for t in feats)
    out = evaluate.main(args + ["--mode", "wild-stats"])["ego mimic"]
    host = evaluate.main(args + ["--mode", "wild-stats", "--host"])["ego mimic"]
    assert set(out["takes"]) == set(feats)
    assert np.isfinite([out["pose_dist"], out["accels"]]).all() and out["pose_dist"] > 0
    np.testing.assert_allclose(out["pose_dist"], host["pose_dist"], rtol=1e-12)
    # ... and the forecast on top of it: `evaluate_forecast --test-feat` reads that result, writes its own; `--mode wild-stats` scores it.
    # (A config of the data dir's own: the packaged one with the margin and horizon of the `forecast` fixture below.)
    import yaml
    from egopose_amd import evaluate_forecast
    from egopose_amd.config import ForecastConfig
    from egopose_amd.env import HumanoidEnv
    from egopose_amd.nets import MLP, PolicyGaussian, VideoForecastNet
    os.makedirs("config/egoforecast", exist_ok=True)
    try:
        fdict = yaml.safe_load(open(os.path.join(os.path.dirname(evaluate.__file__), "assets", "config", "egoforecast", "subject_03.yml")))
        fdict.update(fr_margin=M_F, env_episode_len=T_F, ego_mimic_cfg="subject_03", ego_mimic_iter=3)
        with open("config/egoforecast/wild_small.yml", "w") as f:
            yaml.safe_dump(fdict, f)
        fcfg = ForecastConfig("wild_small", create_dirs=False)
        fenv = HumanoidEnv(fcfg)
        sd, ad = fenv.observation_space.shape[0], fenv.action_space.shape[0]
        fenv.close()
        torch.manual_seed(13)
        fvs = VideoForecastNet(FEAT, sd, fcfg.policy_v_hdim, fcfg.fr_margin, fcfg.policy_v_net, fcfg.policy_v_net_param, fcfg.policy_s_hdim,
                               fcfg.policy_s_net, fcfg.policy_dyn_v)
        fpol = PolicyGaussian(MLP(fvs.out_dim, fcfg.policy_hsize, fcfg.policy_htype), ad, log_std=fcfg.log_std, fix_std=fcfg.fix_std)
        with open("%s/iter_0002.p" % fcfg.model_dir, "wb") as f:
            dump_reference_pickle(dict(policy_dict=fpol.state_dict(), policy_vs_dict=fvs.state_dict(), running_state=None), f)
        fargs = ["--cfg", "wild_small", "--iter", "2", "--test-feat", "wild_rt"]
        evaluate_forecast.main(fargs + ["--num-envs", "2"])
        assert "iter_0002_wild_rt.p (3 windows" in capsys.readouterr().out
        fres, fmeta = pickle.load(open("%s/iter_0002_wild_rt.p" % fcfg.result_dir, "rb"))
        assert fmeta == {"algo": "ego_forecast"} and set(fres) == {"traj_pred"}
        assert fres["traj_pred"]["rt_a"].shape == (1, M_F + T_F, 59) and fres["traj_pred"]["rt_b"].shape == (2, M_F + T_F, 59)
        np.testing.assert_array_equal(fres["traj_pred"]["rt_b"][1, :M_F + 1], results["traj_pred"]["rt_b"][3:3 + M_F + 1])    # window at 16
        fout = evaluate_forecast.main(fargs + ["--mode", "wild-stats", "--horizon", "5"])
        fhost = evaluate_forecast.main(fargs + ["--mode", "wild-stats", "--horizon", "5", "--host"])
        assert set(fout["takes"]) == set(feats) and np.isfinite([fout["pose_dist"], fout["accels"]]).all() and fout["pose_dist"] > 0
        np.testing.assert_allclose(fout["pose_dist"], fhost["pose_dist"], rtol=1e-12)
    finally:
        if os.path.exists("config/egoforecast/wild_small.yml"):
            os.remove("config/egoforecast/wild_small.yml")


M_F, T_F = 3, 11


@pytest.fixture(scope="module")
def forecast(setup):
    """The wild ego_mimic result under ForecastEvaluator's feature-only mode at 2 and 5 slots, random forecast nets, no filter.
    The forecast config's own margin is 30 and the first window starts at m + em_m = 40 rows, the longest take's length, so at the
    config's m these takes have no window: m is set to 3. T = 11 is the smallest horizon at which every planned window has its seat row
    in the mimic result (that result ends em_m = 10 rows before the features do, so start + T <= take_len reaches it only for T > em_m)."""
    from egopose_amd.config import ForecastConfig
    from egopose_amd.env import HumanoidEnv
    from egopose_amd.evaluate_forecast import ForecastEvaluator
    from egopose_amd.nets import MLP, PolicyGaussian, VideoForecastNet
    os.chdir(setup["root"])
    fcfg = ForecastConfig("subject_03", create_dirs=False)
    fcfg.fr_margin, fcfg.env_episode_len, fcfg.random_cur_t, fcfg.env_init_noise = M_F, T_F, False, 0.0
    fcfg.result_dir = os.path.join(setup["root"], "results_wild_forecast")
    env = HumanoidEnv(fcfg)
    env.seed(fcfg.seed)
    sd, ad = env.observation_space.shape[0], env.action_space.shape[0]
    torch.manual_seed(9)
    vs = VideoForecastNet(FEAT, sd, fcfg.policy_v_hdim, fcfg.fr_margin, fcfg.policy_v_net, fcfg.policy_v_net_param, fcfg.policy_s_hdim,
                          fcfg.policy_s_net, fcfg.policy_dyn_v).cuda()
    pol = PolicyGaussian(MLP(vs.out_dim, fcfg.policy_hsize, fcfg.policy_htype), ad, log_std=fcfg.log_std, fix_std=fcfg.fix_std).cuda()
    _, em_res, _ = _batched(setup, 2)
    runs = {}
    for n_slots in (2, 5):
        ev = ForecastEvaluator(fcfg, env, pol, vs, running_state=None, em_res=em_res, em_off=setup["cfg"].fr_margin, num_envs=n_slots,
                               n_threads=2, keep_trace=True, cnn_feat_dict=setup["feats"])
        runs[n_slots] = (ev,) + ev.run()
    yield dict(cfg=fcfg, env=env, em_res=em_res, runs=runs)
    env.close()


def test_wild_forecast_windows_follow_the_plan_and_start_from_the_mimic_result(setup, forecast):
    from egopose_amd.evaluate_forecast import wild_window_plan
    em_m = setup["cfg"].fr_margin
    take_ind, start_ind = wild_window_plan(list(LENS.values()), M_F, em_m, T_F)
    assert [int((take_ind == i).sum()) for i in range(3)] == [1, 3, 6]            # wild_c: its one window ends on the take's last row
    assert start_ind[0] + T_F == LENS["wild_c"]
    ev, res, meta = forecast["runs"][2]
    assert meta == {"algo": "ego_forecast"} and set(res) == {"traj_pred"} and list(res["traj_pred"]) == list(LENS)
    assert ev.timing["windows"] == 10 and ev.timing["passes"] == 5 and forecast["runs"][5][0].timing["passes"] == 2
    assert not ev.failed.any()                                                    # no head bound without experts or fix_head_lb
    for i, take in enumerate(LENS):
        wins, starts = res["traj_pred"][take], start_ind[take_ind == i]
        assert wins.shape == (len(starts), M_F + T_F, 59) and np.isfinite(wins).all()
        em = forecast["em_res"]["traj_pred"][take]
        for w, s in zip(wins, starts):
            np.testing.assert_array_equal(w[:M_F], em[s - M_F - em_m:s - em_m])   # the history rows
            np.testing.assert_array_equal(w[M_F], em[s - em_m])                   # the seat, recorded before the first step
        assert np.abs(wins[:, M_F + 1:] - wins[:, M_F:-1]).max() > 0               # ... and the humanoid moves after it


def test_wild_forecast_does_not_depend_on_the_slot_count(forecast):
    (ev2, r2, _), (ev5, r5, _) = forecast["runs"][2], forecast["runs"][5]
    for take in LENS:
        np.testing.assert_array_equal(r2["traj_pred"][take], r5["traj_pred"][take])
    for k in ("actions", "states", "qvel", "take_ind", "start_ind"):
        np.testing.assert_array_equal(ev2.trace[k], ev5.trace[k])


def test_wild_forecast_result_saved_and_scored_by_the_kernel(setup, forecast, skel):
    from egopose_amd.pose2d import Pose2DContext, eval_forecast_wild_stats
    ev, res, meta = forecast["runs"][5]
    path = ev.save(res, meta, 4, data="wild_xx")
    assert path.endswith("iter_0004_wild_xx.p")
    r2, m2 = pickle.load(open(path, "rb"))
    assert m2 == {"algo": "ego_forecast"} and set(r2) == {"traj_pred"}
    pctx = Pose2DContext(skel)

    def loader(take, gt_fr):
        r = np.random.RandomState(gt_fr)
        gt = np.zeros((12, 3))
        gt[:, 0], gt[:, 1], gt[:, 2] = r.uniform(400, 1500, 12), np.sort(r.uniform(100, 1000, 12)), r.uniform(0.2, 1.0, 12)
        if gt_fr % 4 == 0:
            gt[pctx.body2id["RightUpLeg"], 2] = gt[pctx.body2id["LeftUpLeg"], 2] = 0.0
        return gt
    tpv = {"traj_ub": {"wild_b": 20}, "tpv_offset": {"wild_a": -2}, "tpv_flip": {"wild_c": True}}     # cuts wild_b's last window to 2 frames
    sim = setup["env"].batched(3, 0, 2, 1)
    out = eval_forecast_wild_stats(r2, tpv, loader, forecast["cfg"], horizon=5, backend="hip", ctx=sim.ctx, pose_ctx=pctx)
    host = eval_forecast_wild_stats(r2, tpv, loader, forecast["cfg"], horizon=5, backend="host", pose_ctx=pctx)
    assert set(out["takes"]) == set(LENS) and np.isfinite([out["pose_dist"], out["accels"]]).all() and out["pose_dist"] > 0
    np.testing.assert_allclose(out["pose_dist"], host["pose_dist"], rtol=1e-12)
    with pytest.raises(ValueError, match="wild_b, window 5"):          # a bound that leaves a window (rows from 18) without a frame
        eval_forecast_wild_stats(r2, dict(tpv, traj_ub={"wild_b": 17}), loader, forecast["cfg"], horizon=5, backend="host", pose_ctx=pctx)
