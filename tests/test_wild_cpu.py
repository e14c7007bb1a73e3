"""In-the-wild evaluation, host side: the numpy restatement of the 2D keypoint metric against the reference's own numbers
(tests/golden/pose2d.npz, tools/gen_golden_pose2d.py), the window plan of feature-only takes against a literal loop, the state
regressor on stored features against integrating its output by hand, and the two `--mode stats` loops against per-frame loops."""
import types

import numpy as np
import pytest
import torch

from conftest import load_golden


@pytest.fixture(scope="module")
def pctx():
    from egopose_amd.pose2d import Pose2DContext
    return Pose2DContext()


# ====================================================================================================== Pose2DContext
def test_pose2d_restatement_against_the_reference(pctx):
    """Same float64 numpy arithmetic as the reference's: p, dist, valid at 1e-12, on every branch the fixture holds."""
    g = load_golden("pose2d.npz")
    assert list(g["body_names"]) == pctx.body_names and pctx.nbody == 12
    b2 = pctx.body2id
    valid, gt, flip = g["valid"], g["gt"], g["flip"]
    seen = gt[:, :, 2] > 0.1
    lu, ru = seen[:, b2["LeftUpLeg"]], seen[:, b2["RightUpLeg"]]
    # the branches: left pair, right pair only (knee / shoulder), one hip only (each side), flip on and off, invalid frames
    assert (valid & lu & seen[:, b2["LeftLeg"]]).any() and (valid & lu & ~seen[:, b2["LeftLeg"]]).any()
    assert (valid & lu & ~seen[:, b2["LeftArm"]]).any() and (valid & ~lu).any() and (valid & ~ru).any()
    assert (flip[valid] == 1).any() and (flip[valid] == 0).any() and (~valid).sum() >= 8
    np.testing.assert_array_equal(valid, lu | ru)
    for i in range(len(valid)):
        np.testing.assert_array_equal(pctx.gt_from_keypoints(g["keypoints"][i]), gt[i])
        x = g["xpos"][i][pctx.body_filter]
        np.testing.assert_array_equal(x, g["xpos"][i][pctx.body_index])
        assert pctx.check_gt(gt[i]) == bool(valid[i])
        np.testing.assert_allclose(pctx.project_xpos(x, flip[i]), g["p_proj"][i], rtol=1e-12, atol=1e-12)
        if valid[i]:
            p = pctx.align_xpos(x, gt[i], flip=bool(flip[i]))
            np.testing.assert_allclose(p, g["p"][i], rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(pctx.get_pose_dist(p, gt[i]), g["dist"][i], rtol=1e-12, atol=1e-12)


def test_load_gt_pose_reads_openpose_json(pctx, tmp_path):
    import json
    g = load_golden("pose2d.npz")
    f = tmp_path / "00003_keypoints.json"
    f.write_text(json.dumps({"people": [{"pose_keypoints_2d": g["keypoints"][3].tolist()}]}))
    np.testing.assert_array_equal(pctx.load_gt_pose(str(f)), g["gt"][3])


def test_kernel_tables(pctx, skel):
    body, roles = pctx.kernel_tables()
    assert [skel.body_names[b] for b in body] == pctx.body_names
    assert [pctx.body_names[r] for r in roles] == ["LeftUpLeg", "RightUpLeg", "LeftLeg", "RightLeg", "LeftArm", "RightArm"]


# ====================================================================================================== window plan
@pytest.mark.parametrize("m,em_m,T", [(10, 10, 12), (10, 5, 30), (4, 10, 13)])
def test_wild_window_plan_and_init_state_against_a_literal_loop(m, em_m, T):
    """ego_forecast_eval_wild.py:94-120,160-170 written out; take lengths with 0, 1 and several windows, one exactly start + T."""
    from egopose_amd.evaluate_forecast import wild_window_init_state, wild_window_plan
    rng = np.random.RandomState(5)
    take_lens = [m + em_m + T - 1, m + em_m + T, m + em_m + T + 1, m + em_m + 3 * m + T, m + em_m + 2 * m + T + m - 1, 3]
    em_traj = [rng.normal(size=(max(0, n - 2 * em_m), 59)) for n in take_lens]
    em_vel = [rng.normal(size=(max(0, n - 2 * em_m), 58)) for n in take_lens]
    take_ind, start_ind = wild_window_plan(take_lens, m, em_m, T)
    want = []
    for i, take_len in enumerate(take_lens):
        start = m + em_m
        while start + T <= take_len:
            want.append((i, start))
            start += m
    assert [(int(a), int(b)) for a, b in zip(take_ind, start_ind)] == want
    assert [sum(1 for w in want if w[0] == i) for i in range(len(take_lens))] == [0, 1, 1, 4, 3, 0]
    for i, start in want:
        state_pred = em_traj[i][start - m - em_m: start + T - em_m]
        vel_pred = em_vel[i][start - m - em_m: start + T - em_m]
        qpos, qvel, hist = wild_window_init_state(em_traj[i], em_vel[i], start, m, em_m, T)
        np.testing.assert_array_equal(qpos, state_pred[m])
        np.testing.assert_array_equal(qvel, vel_pred[m])
        np.testing.assert_array_equal(hist, np.vstack([state_pred[t + m] for t in range(-m, 0)]))
        assert m < state_pred.shape[0] <= m + T             # (the mimic result ends em_m rows before the features: the slice may be short)
    with pytest.raises(ValueError):
        wild_window_init_state(em_traj[3], em_vel[3], m + em_m - 1, m, em_m, T)
    # a horizon no longer than the mimic margin: the last window of a take has no mimic row to start from (the reference: IndexError)
    short = rng.normal(size=(m + em_m + em_m - 2 * em_m, 59))
    with pytest.raises(ValueError):
        wild_window_init_state(short, short[:, :58], m + em_m, m, em_m, em_m)


# ====================================================================================================== state_reg --test-feat
def test_statereg_test_features_against_integration_by_hand():
    from egopose_amd import statereg as SR
    m, fdim, traj_dim = 4, 16, 115
    cfg = types.SimpleNamespace(fr_margin=m, v_hdim=32, cnn_fdim=fdim, cnn_type="resnet", mlp_dim=(24, 20), v_net="lstm", v_net_param=None,
                                causal=False, pose_only=False, lr=1e-4)
    rng = np.random.RandomState(2)
    ds = types.SimpleNamespace(traj_dim=traj_dim, dt=1 / 30.0, mean=rng.normal(size=traj_dim), std=rng.uniform(0.5, 1.5, size=traj_dim))
    torch.manual_seed(3)
    tr = SR.StateRegTrainer(cfg, ds, "cpu", torch.float64, no_cnn=True)
    feats = {"wild_b": rng.normal(size=(2 * m + 9, fdim)), "wild_a": rng.normal(size=(2 * m + 1, fdim))}
    results, meta = tr.test_features(feats)
    assert list(results) == ["traj_pred"] and list(results["traj_pred"]) == ["wild_b", "wild_a"]
    assert meta == {"algo": "state_reg", "num_sample": 10}
    for take, f in feats.items():
        with torch.no_grad():
            sp = tr.net(torch.as_tensor(f).unsqueeze(1)).squeeze(1)[m:-m].numpy()
        sp = sp * ds.std[None] + ds.mean[None]
        want = SR.get_traj_from_state_pred(sp, np.zeros(2), np.array([1.0, 0, 0, 0]), ds.dt, traj_dim)
        got = results["traj_pred"][take]
        assert got.shape == (f.shape[0] - 2 * m, 59)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
        np.testing.assert_array_equal(got[0, :2], 0.0)      # from position (0, 0) and heading (1, 0, 0, 0)
        np.testing.assert_allclose(got[0, 2:], sp[0, :57], rtol=1e-12, atol=1e-12)


# ====================================================================================================== --mode stats loops
def _wild_case(pctx, skel, seed=7):
    """Two takes + synthetic keypoints: traj_ub cuts take 'a', take 'b' has a negative tpv_offset and is flipped; every 5th keypoint
    frame has both hips unseen."""
    rng = np.random.RandomState(seed)

    def traj(n):
        q = np.zeros((n, skel.nq))
        q[:, :2] = np.cumsum(rng.normal(size=(n, 2)) * 0.02, 0)
        q[:, 2] = 0.9
        yaw = np.cumsum(rng.normal(size=n) * 0.05) + rng.uniform(-3, 3)
        q[:, 3], q[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
        q[:, 7:] = np.cumsum(rng.normal(size=(n, skel.nq - 7)) * 0.02, 0)
        return q

    trajs = {"a": traj(14), "b": traj(9)}
    meta = {"traj_ub": {"a": 11}, "tpv_offset": {"b": -3}, "tpv_flip": {"b": True}}
    b2 = pctx.body2id

    def loader(take, gt_fr):
        r = np.random.RandomState(1000 * (take == "b") + gt_fr)
        gt = np.zeros((12, 3))
        gt[:, 0], gt[:, 1] = r.uniform(400, 1500, 12), np.sort(r.uniform(100, 1000, 12))
        gt[:, 2] = r.uniform(0.0, 1.0, 12)
        gt[b2["RightUpLeg"], 2] = 0.8
        if gt_fr % 5 == 0:
            gt[b2["RightUpLeg"], 2] = gt[b2["LeftUpLeg"], 2] = 0.05
        return gt
    return trajs, meta, loader


def test_eval_pose_wild_stats_against_a_literal_loop(pctx, skel):
    from egopose_amd import metrics as M
    from egopose_amd.pose2d import eval_pose_wild_stats
    trajs, meta, loader = _wild_case(pctx, skel)
    cfg = types.SimpleNamespace(fr_margin=10)
    out = eval_pose_wild_stats({"traj_pred": trajs}, meta, loader, cfg, backend="host", pose_ctx=pctx)
    dt, g_d, g_s, n_invalid = 1 / 30.0, 0, 0, 0
    for take in trajs:
        traj_pred = trajs[take][:meta["traj_ub"].get(take, trajs[take].shape[0])]
        tpv_offset, flip = meta["tpv_offset"].get(take, cfg.fr_margin), meta["tpv_flip"].get(take, False)
        pose_dist, valid_num = 0, 0
        for fr in range(max(0, -tpv_offset), traj_pred.shape[0]):
            gt_p = loader(take, fr + tpv_offset)
            if not pctx.check_gt(gt_p):
                n_invalid += 1
                continue
            valid_num += 1
            pose_dist += pctx.get_pose_dist(pctx.align_qpos(traj_pred[fr], gt_p, flip=flip), gt_p)
        pose_dist /= valid_num
        smooth = M.get_mean_abs(M.get_joint_accels(M.get_joint_vels(traj_pred, dt), dt))
        np.testing.assert_allclose(out["takes"][take], (pose_dist, smooth), rtol=1e-12)
        g_d += pose_dist
        g_s += smooth
    assert n_invalid >= 2
    np.testing.assert_allclose([out["pose_dist"], out["accels"]], [g_d / 2, g_s / 2], rtol=1e-12)
    # the take cut by traj_ub and the negative offset change the numbers
    other = eval_pose_wild_stats({"traj_pred": trajs}, dict(meta, traj_ub={}, tpv_offset={}), loader, cfg, backend="host", pose_ctx=pctx)
    assert other["takes"]["a"] != out["takes"]["a"] and other["takes"]["b"] != out["takes"]["b"]
    with pytest.raises(ValueError):
        eval_pose_wild_stats({"traj_pred": trajs}, meta, loader, cfg, backend="eager", pose_ctx=pctx)


def test_eval_forecast_wild_stats_against_a_literal_loop(pctx, skel):
    from egopose_amd import metrics as M
    from egopose_amd.pose2d import eval_forecast_wild_stats
    trajs, meta, loader = _wild_case(pctx, skel, seed=8)
    m, horizon = 3, 5
    cfg = types.SimpleNamespace(fr_margin=m)
    wins = {"a": np.stack([trajs["a"][s:s + m + 6] for s in (0, 2, 5)]), "b": np.stack([trajs["b"][s:s + m + 6] for s in (0,)])}
    keep = {k: v.copy() for k, v in wins.items()}
    out = eval_forecast_wild_stats({"traj_pred": wins}, meta, loader, cfg, horizon=horizon, backend="host", pose_ctx=pctx)
    for k in wins:
        np.testing.assert_array_equal(wins[k], keep[k])        # (the wrists are zeroed on a copy)
    res = {"traj_pred": {k: v.copy() for k, v in wins.items()}}
    M.remove_noisy_hands(res)
    dt, g_d, g_s, cut = 1 / 30.0, 0, 0, 0
    for take, tp in res["traj_pred"].items():
        t_d, t_s = 0, 0
        for i in range(tp.shape[0]):
            traj, start_fr = tp[i, m:m + horizon], (i + 1) * m
            traj_ub, tpv_offset, flip = meta["traj_ub"].get(take, None), meta["tpv_offset"].get(take, m), meta["tpv_flip"].get(take, False)
            pose_dist, valid_num = 0, 0
            for fr in range(traj.shape[0]):
                if traj_ub is not None and start_fr + fr >= traj_ub:
                    cut += 1
                    break
                gt_p = loader(take, start_fr + fr + tpv_offset)
                if not pctx.check_gt(gt_p):
                    continue
                valid_num += 1
                pose_dist += pctx.get_pose_dist(pctx.align_qpos(traj[fr], gt_p, flip=flip), gt_p)
            t_d += pose_dist / valid_num
            t_s += M.get_mean_abs(M.get_joint_accels(M.get_joint_vels(traj, dt), dt))
        np.testing.assert_allclose(out["takes"][take], (t_d / tp.shape[0], t_s / tp.shape[0]), rtol=1e-12)
        g_d += t_d / tp.shape[0]
        g_s += t_s / tp.shape[0]
    assert cut >= 1
    np.testing.assert_allclose([out["pose_dist"], out["accels"]], [g_d / 2, g_s / 2], rtol=1e-12)


# ====================================================================================================== fail-safe on the last tick
def test_speculative_failsafe_decides_on_the_last_tick_when_asked():
    from egopose_amd.failsafe import SpeculativeValueFailSafe, decisions
    from egopose_amd.zfilter import RunningStat
    values = {0: np.array([1.0, 1.0, 0.1]), 1: np.array([1.0, 0.2])}

    def run_pass(ids, prefixes):
        return [(values[i], decisions(values[i], -1, st)[0]) for i, st in zip(ids, prefixes)]

    fs = SpeculativeValueFailSafe(decide_on_end=True)
    out = fs.run([0, 1], run_pass)
    assert out[0][1].tolist() == [False, False, True] and out[1][1].tolist() == [False, True] and fs.stat.n == 5
    assert decisions(values[0], 2, RunningStat(1))[0].tolist() == [False, False, False]     # the default: the end step decides nothing
