"""Host side of the ego_forecast evaluation (egopose_amd/evaluate_forecast.py, egopose_amd/metrics.py): the window plan, the
seat-state arithmetic of ego_forecast_eval.py:107-133, sync_traj and the forecast statistics against vectors recorded from the
reference (tools/gen_golden_forecast_eval.py), result paths and the command line."""
import pickle
import types

import numpy as np
import pytest

from conftest import load_golden

from egopose_amd import metrics as M
from egopose_amd import evaluate_forecast as EF


def test_window_plan():
    for L, want in ((29, []), (41, []), (42, [30]), (300, list(range(30, 271, 30)))):
        e, s = EF.window_plan([L], 30, 12)
        assert s.tolist() == want and e.tolist() == [0] * len(want) and e.dtype == s.dtype == np.int64
    e, s = EF.window_plan([29, 41, 42, 300], 30, 12)
    assert e.tolist() == [2] + [3] * 9 and s.tolist() == [30] + list(range(30, 271, 30))


def test_sync_traj_matches_the_reference():
    """float64, the same dozen operations per frame as the reference's loop: 1e-12."""
    g = load_golden("forecast_eval.npz")
    qpos, qvel = M.sync_traj(g["sync_qpos"], g["sync_qvel"], g["sync_ref"])
    np.testing.assert_allclose(qpos, g["sync_out_qpos"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(qvel, g["sync_out_qvel"], rtol=1e-12, atol=1e-12)
    assert np.abs(qpos - g["sync_qpos"]).max() > 0.1 and qpos is not g["sync_qpos"]
    np.testing.assert_allclose(qpos[0, :2], g["sync_ref"][:2], rtol=0, atol=1e-12)          # the first frame lands on ref's xy


def test_forecast_statistics_match_the_reference():
    """compute_metrics / compute_err_vs_h of eval_forecast.py, executed from the reference's file when the fixture was made
    (tolerance: test_oracle_golden.py's for the same metric functions on metrics.npz, 1e-10)."""
    g = load_golden("forecast_eval.npz")
    takes = ["take_a", "take_b"]
    res = {"traj_pred": {t: g["fm_pred"][i] for i, t in enumerate(takes)}, "traj_orig": {t: g["fm_orig"][i] for i, t in enumerate(takes)}}
    m = int(g["fm_margin"])
    for h in (10, 20):
        out = M.compute_forecast_metrics(res, m, h)
        np.testing.assert_allclose([out["pose_dist"], out["vel_dist"], out["accels"]], g["fm_h%d" % h], rtol=1e-10, atol=1e-10)
        assert set(out["per_take"]) == set(takes)
        np.testing.assert_allclose(np.mean([out["per_take"][t] for t in takes], 0), g["fm_h%d" % h], rtol=1e-10, atol=1e-10)
    err = M.forecast_err_vs_horizon(res, m, int(g["fm_err_horizon"]), step=int(g["fm_err_step"]))
    np.testing.assert_allclose(err, g["fm_err_vs_h"], rtol=1e-10, atol=1e-10)
    assert err.shape == (4,)


def test_forecast_statistics_print_the_reference_format(capsys):
    g = load_golden("forecast_eval.npz")
    res = {"traj_pred": {"take_a": g["fm_pred"][0]}, "traj_orig": {"take_a": g["fm_orig"][0]}}
    out = M.compute_forecast_metrics(res, 4, 10, verbose=True)
    text = capsys.readouterr().out
    assert "=" * 10 + " ego forecast " + "=" * 10 in text
    assert "take_a - horizon: 10, pose dist: %.4f, vel dist: %.4f, accels: %.4f" % tuple(out["per_take"]["take_a"]) in text
    assert "all - horizon: 10, pose dist: %.4f, vel dist: %.4f, accels: %.4f" % (out["pose_dist"], out["vel_dist"], out["accels"]) in text


def test_remove_noisy_hands_zeroes_the_wrist_columns_only():
    rng = np.random.RandomState(2)
    res = {"traj_pred": {"a": rng.normal(size=(3, 16, 59)) + 5.0}, "traj_orig": {"a": rng.normal(size=(3, 16, 59)) + 5.0}}
    before = {k: v["a"].copy() for k, v in res.items()}
    M.remove_noisy_hands(res)
    zero = np.zeros(59, bool)
    zero[32:35] = zero[42:45] = True
    for k in res:
        assert (res[k]["a"][..., zero] == 0).all()
        np.testing.assert_array_equal(res[k]["a"][..., ~zero], before[k][..., ~zero])


def _take(L=120, seed=3):
    rng = np.random.RandomState(seed)
    qpos = rng.normal(size=(L, 59)) * 0.3
    qpos[:, :2] = np.cumsum(rng.normal(size=(L, 2)) * 0.02, 0)
    qpos[:, 2] = 0.9 + 0.01 * rng.normal(size=L)
    qpos[:, 3:7] = np.array([1.0, 0, 0, 0]) + 0.2 * rng.normal(size=(L, 4))
    qpos[:, 3:7] /= np.linalg.norm(qpos[:, 3:7], axis=1, keepdims=True)
    return qpos, rng.normal(size=(L, 58))


def _yawed(qpos, qvel, angle, shift):
    """The trajectory turned about z by `angle` (about the origin) and moved by `shift` in xy: what sync_traj undoes."""
    q = np.array([np.cos(angle / 2), 0.0, 0.0, np.sin(angle / 2)])
    R = M._rot_matrix(q)
    out_q, out_v = qpos.copy(), qvel.copy()
    out_q[:, :3] = qpos[:, :3] @ R.T
    out_q[:, :2] += shift
    out_q[:, 3:7] = M._qmul(q, qpos[:, 3:7])
    out_v[:, :3] = qvel[:, :3] @ R.T
    return out_q, out_v


def test_init_state_from_ego_mimic_results():
    """ego_forecast_eval.py:107-133 on a hand-built ego_mimic result (its row i = take frame i + em_off)."""
    m, T, em_off, L = 10, 12, 5, 120
    qpos, qvel = _take(L)
    # gt_init
    q0, v0, hist, miss = EF.window_init_state(qpos, qvel, 40, m, T)
    np.testing.assert_array_equal(q0, qpos[40]); np.testing.assert_array_equal(v0, qvel[40])
    np.testing.assert_array_equal(hist, qpos[30:40])
    assert miss == 0
    # (a) em = the expert's own trajectory
    em_q, em_v = qpos[em_off:L - em_off], qvel[em_off:L - em_off]
    for start, want_miss in ((m, em_off), (40, 0)):
        q0, v0, hist, miss = EF.window_init_state(qpos, qvel, start, m, T, em_q, em_v, em_off)
        assert miss == want_miss
        np.testing.assert_allclose(q0, qpos[start], rtol=0, atol=1e-12)
        np.testing.assert_allclose(v0, qvel[start], rtol=0, atol=1e-12)
        np.testing.assert_allclose(hist, qpos[start - m:start], rtol=0, atol=1e-12)
    # (b) em = the same, yawed and shifted
    ym_q, ym_v = _yawed(em_q, em_v, 0.8, np.array([0.4, -0.7]))
    q0, v0, hist, miss = EF.window_init_state(qpos, qvel, 40, m, T, ym_q, ym_v, em_off)          # reaches back: synced
    assert miss == 0
    np.testing.assert_allclose(q0, qpos[40], rtol=0, atol=1e-12)
    np.testing.assert_allclose(v0, qvel[40], rtol=0, atol=1e-12)
    np.testing.assert_allclose(hist, qpos[30:40], rtol=0, atol=1e-12)
    q0, v0, hist, miss = EF.window_init_state(qpos, qvel, m, m, T, ym_q, ym_v, em_off)           # first window: not synced
    assert miss == em_off
    np.testing.assert_array_equal(q0, ym_q[m - em_off]); np.testing.assert_array_equal(v0, ym_v[m - em_off])
    np.testing.assert_array_equal(hist[:miss], qpos[:miss])                                    # rows the em result lacks: the expert's
    np.testing.assert_array_equal(hist[miss:], ym_q[:m - miss])
    # the em result cut short at the take's end: the reference's arithmetic counts the missing rows at the front all the same
    short_q, short_v = em_q[:-3], em_v[:-3]
    start = L - T                                                                              # slice end start + T - em_off = 115 > 107 rows
    q0, v0, hist, miss = EF.window_init_state(qpos, qvel, start, m, T, short_q, short_v, em_off)
    sl_q, sl_v = M.sync_traj(short_q[start - m - em_off:], short_v[start - m - em_off:], qpos[start - m])
    assert miss == m + T - sl_q.shape[0] and 0 < miss < m
    np.testing.assert_array_equal(q0, sl_q[m - miss]); np.testing.assert_array_equal(v0, sl_v[m - miss])
    np.testing.assert_array_equal(hist[:miss], qpos[start - m:start - m + miss])
    np.testing.assert_array_equal(hist[miss:], sl_q[:m - miss])


def _tiny_evaluator(tmp_path, gt_init):
    import torch
    from egopose_amd.nets import MLP, PolicyGaussian, VideoForecastNet
    torch.manual_seed(0)
    vs = VideoForecastNet(4, 115, 8, 10, "lstm", None, 8, "lstm", False)
    pol = PolicyGaussian(MLP(16, (8,), "relu"), 52, log_std=-1.0)
    cfg = types.SimpleNamespace(result_dir=str(tmp_path / "results"), fr_margin=10, env_episode_len=12)
    return EF.ForecastEvaluator(cfg, None, pol, vs, gt_init=gt_init, em_res={} if not gt_init else None, em_off=5)


def test_save_paths_meta_and_command_line(tmp_path):
    res = {"traj_pred": {"a": np.zeros((2, 22, 59))}, "traj_orig": {"a": np.ones((2, 22, 59))}}
    meta = {"algo": "ego_forecast"}
    for gt_init, tail in ((True, "iter_0007_test_gt.p"), (False, "iter_0007_test.p")):
        ev = _tiny_evaluator(tmp_path, gt_init)
        path = ev.save(res, meta, 7, data="test")
        assert path.endswith("/results/" + tail)
        r2, m2 = pickle.load(open(path, "rb"))
        assert m2 == {"algo": "ego_forecast"} and set(r2) == {"traj_pred", "traj_orig"}
        np.testing.assert_array_equal(r2["traj_orig"]["a"], res["traj_orig"]["a"])
    with pytest.raises(ValueError):
        EF.ForecastEvaluator(types.SimpleNamespace(), None, ev.policy_net, ev.policy_vs_net, gt_init=False)      # no ego_mimic results
    ap = EF.build_parser()
    args = ap.parse_args(["--cfg", "subject_01", "--iter", "12", "--gt-init", "--num-envs", "64"])
    assert (args.cfg, args.iter, args.data, args.gt_init, args.num_envs, args.gpu_index) == ("subject_01", 12, "test", True, 64, 0)
    for flag in (["--render"], ["--mode", "vis"], ["--show-noise"], ["--verbose"]):
        with pytest.raises(SystemExit):
            ap.parse_args(flag)
