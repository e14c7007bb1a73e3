"""The host path of the joint-position metrics (egopose_amd/pose3d.py): definitions on cases with known answers, the proper-rotation
rule on mirrored bodies, the body mask, the acceleration error, the aggregation loops and `evaluate --mode stats`."""
import pickle

import numpy as np
import pytest

import pose3d_fixture as PF

DT = 1.0 / 30.0
FIGS = ("g_mpjpe", "mpjpe", "pa_mpjpe", "root_err", "accel_err")


def _bodies(skel, n, seed):
    """Body positions [n][nbody][3] of random poses."""
    q = PF.poses(skel, n, np.random.RandomState(seed))
    return q, np.stack([skel.body_xpos(r) for r in q])


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def test_identical_trajectories_score_exactly_zero(skel):
    from egopose_amd import pose3d
    q = PF.two_takes(skel)["traj_orig"]
    out = pose3d.compute_joint_metrics({"traj_pred": {k: v.copy() for k, v in q.items()}, "traj_orig": q}, skel, dt=DT, backend="host")
    assert [out[k] for k in FIGS] == [0.0] * 5
    assert (out["per_body"] == 0.0).all() and all((row == 0.0).all() for row in out["per_take"].values())


def test_root_translation_moves_only_the_global_figures(skel):
    from egopose_amd import pose3d
    q, _ = _bodies(skel, 6, 1)
    t = np.array([0.3, -0.2, 0.1])
    g = q.copy()
    g[:, :3] += t
    r = pose3d.score_host(skel, q, g)
    assert np.abs(r["mpjpe"]).max() <= 1e-12 and np.abs(r["pa_mpjpe"]).max() <= 1e-12
    np.testing.assert_allclose(r["g_mpjpe"], np.linalg.norm(t), rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["root_err"], np.linalg.norm(t), rtol=0, atol=1e-12)


def test_similarity_of_positions_is_undone(skel):
    from egopose_amd import pose3d
    rng = np.random.RandomState(2)
    _, Y = _bodies(skel, 5, 2)
    X = np.stack([1.3 * y @ _rotation(rng).T + rng.normal(size=3) for y in Y])
    r = pose3d.score_xpos(X, Y)
    assert r["pa_mpjpe"].max() <= 1e-12
    assert r["mpjpe"].min() > 0.05                      # bodies tens of centimetres from the root, scaled by 1.3 and turned


def test_mirrored_bodies_are_not_matched_by_a_reflection(skel):
    from egopose_amd import pose3d
    _, Y = _bodies(skel, 8, 3)
    X = Y * np.array([1.0, -1.0, 1.0])
    r = pose3d.score_xpos(X, Y)
    for i in range(len(Y)):
        proper, free = PF.procrustes(X[i], Y[i]), PF.procrustes(X[i], Y[i], correct=False)
        assert free <= 1e-12                            # a reflection would match the mirrored body exactly
        np.testing.assert_allclose(r["pa_mpjpe"][i], proper, rtol=1e-12, atol=1e-15)
        assert r["pa_mpjpe"][i] > free and r["pa_mpjpe"][i] > 1e-3


def test_mask_means_and_err_rows(skel):
    from egopose_amd import pose3d
    names = list(skel.body_names)
    pred, gt = PF.pairs(skel, 5, 4)
    mask = pose3d.body_mask(skel, pose3d.HANDS)
    assert mask == sum(1 << b for b, n in enumerate(names) if n not in ("LeftHand", "RightHand")) and bin(mask).count("1") == len(names) - 2
    assert pose3d.body_mask(skel) == (1 << len(names)) - 1
    r_all, r = pose3d.score_host(skel, pred, gt), pose3d.score_host(skel, pred, gt, mask)
    for i in range(len(pred)):
        X, Y = skel.body_xpos(pred[i]), skel.body_xpos(gt[i])
        g = rel = 0.0
        keep = []
        for b, n in enumerate(names):
            d_rel = np.linalg.norm((X[b] - X[0]) - (Y[b] - Y[0]))
            if n in ("LeftHand", "RightHand"):
                assert r["err"][i, b] == 0.0 and abs(r_all["err"][i, b] - d_rel) <= 1e-15
                continue
            keep.append(b)
            g += np.linalg.norm(X[b] - Y[b])
            rel += d_rel
            assert abs(r["err"][i, b] - d_rel) <= 1e-15
        np.testing.assert_allclose([r["g_mpjpe"][i], r["mpjpe"][i]], [g / len(keep), rel / len(keep)], rtol=1e-13)
        np.testing.assert_allclose(r["pa_mpjpe"][i], PF.procrustes(X[keep], Y[keep]), rtol=1e-10, atol=1e-14)
    assert not np.allclose(r["mpjpe"][[0, 1]], r_all["mpjpe"][[0, 1]])
    with pytest.raises(ValueError):
        pose3d.score_host(skel, pred, gt, 0b101)
    with pytest.raises(ValueError):
        pose3d.score_host(skel, pred, gt, 1 << len(names))
    with pytest.raises(ValueError):
        pose3d.body_mask(skel, ("NoSuchBody",))


def test_accel_err(skel):
    from egopose_amd import pose3d
    q, Y = _bodies(skel, 7, 5)
    t = np.arange(7)[:, None, None] * DT
    v, a = np.array([0.4, -0.3, 0.2]), np.array([1.5, -2.0, 0.5])
    assert pose3d.accel_err(Y + v * t, Y, DT) <= 1e-9            # (rounding of metres, over dt^2 = 1 / 900)
    moved = q.copy()
    moved[:, :3] += (0.5 * a * t * t)[:, 0]                      # the root displaced: the whole body follows
    X = np.stack([skel.body_xpos(r) for r in moved])
    assert abs(pose3d.accel_err(X, Y, DT) - np.linalg.norm(a)) <= 1e-9
    only_root = Y.copy()
    only_root[:, 0] = X[:, 0]                                    # one of three counted bodies
    assert abs(pose3d.accel_err(only_root, Y, DT, 0b111) - np.linalg.norm(a) / 3) <= 1e-9
    assert np.isnan(pose3d.accel_err(Y[:2], Y[:2] + 0.1, DT))
    res = PF.two_takes(skel)
    res["traj_pred"]["c"], res["traj_orig"]["c"] = res["traj_pred"]["a"][:2], res["traj_orig"]["a"][:2]
    out = pose3d.compute_joint_metrics(res, skel, dt=DT, backend="host")
    assert np.isnan(out["per_take"]["c"][4]) and np.isfinite(out["accel_err"])
    np.testing.assert_allclose(out["accel_err"], np.mean([out["per_take"][k][4] for k in ("a", "b")]), rtol=1e-15)
    np.testing.assert_allclose(out["mpjpe"], np.mean([out["per_take"][k][1] for k in ("a", "b", "c")]), rtol=1e-15)


def _take_row(skel, pred, gt, sel, dt):
    """The five figures and the per-body row of one trajectory, frame by frame."""
    X, Y = np.stack([skel.body_xpos(r) for r in pred]), np.stack([skel.body_xpos(r) for r in gt])
    rows, errs = zip(*[PF.figures_of_positions(X[t], Y[t], sel) for t in range(len(pred))])
    acc = [np.linalg.norm((X[t - 1, b] - 2 * X[t, b] + X[t + 1, b]) - (Y[t - 1, b] - 2 * Y[t, b] + Y[t + 1, b])) / dt ** 2
           for t in range(1, len(pred) - 1) for b in np.nonzero(sel)[0]]
    return np.append(np.mean(rows, 0), np.mean(acc)), np.mean(errs, 0)


def test_compute_joint_metrics_against_a_per_take_loop(skel):
    from egopose_amd import pose3d
    res = PF.two_takes(skel)
    mask = pose3d.body_mask(skel, pose3d.HANDS)
    sel = pose3d.mask_bits(mask, len(skel.body_names))
    out = pose3d.compute_joint_metrics(res, skel, dt=DT, mask=mask, backend="host")
    want = {k: _take_row(skel, res["traj_pred"][k], res["traj_orig"][k], sel, DT) for k in ("a", "b")}
    for k in ("a", "b"):
        np.testing.assert_allclose(out["per_take"][k], want[k][0], rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose([out[f] for f in FIGS], np.mean([want[k][0] for k in ("a", "b")], 0), rtol=1e-9)
    np.testing.assert_allclose(out["per_body"], np.mean([want[k][1] for k in ("a", "b")], 0), rtol=1e-12)
    assert out["per_body"][~sel].tolist() == [0.0, 0.0] and out["mpjpe"] > 1e-3
    bad = {"traj_pred": {"a": res["traj_pred"]["a"][:-1]}, "traj_orig": {"a": res["traj_orig"]["a"]}}
    with pytest.raises(ValueError):
        pose3d.compute_joint_metrics(bad, skel, backend="host")
    with pytest.raises(ValueError):
        pose3d.compute_joint_metrics(res, skel, backend="eager")


def test_compute_forecast_joint_metrics_against_a_per_window_loop(skel):
    from egopose_amd import pose3d
    res = PF.two_takes(skel)
    win = lambda d: {"a": np.stack([d["a"][s:s + 9] for s in (0, 2, 5)]), "b": d["b"][None]}
    wins = {"traj_pred": win(res["traj_pred"]), "traj_orig": win(res["traj_orig"])}
    assert wins["traj_pred"]["a"].shape == (3, 9, skel.nq)
    m, horizon = 3, 5
    sel = np.ones(len(skel.body_names), bool)
    out = pose3d.compute_forecast_joint_metrics(wins, skel, m, horizon, dt=DT, backend="host")
    want = {}
    for k in ("a", "b"):
        per = [_take_row(skel, wins["traj_pred"][k][i, m:m + horizon], wins["traj_orig"][k][i, m:m + horizon], sel, DT)
               for i in range(wins["traj_pred"][k].shape[0])]
        want[k] = (np.mean([p[0] for p in per], 0), np.mean([p[1] for p in per], 0))
        np.testing.assert_allclose(out["per_take"][k], want[k][0], rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose([out[f] for f in FIGS], np.mean([want[k][0] for k in ("a", "b")], 0), rtol=1e-9)
    np.testing.assert_allclose(out["per_body"], np.mean([want[k][1] for k in ("a", "b")], 0), rtol=1e-12)


def test_mode_stats_scores_saved_results_of_both_algorithms(skel, tmp_path, monkeypatch, capsys):
    import yaml
    from egopose_amd import evaluate, metrics, pose3d
    monkeypatch.chdir(tmp_path)
    (tmp_path / "datasets" / "meta").mkdir(parents=True)
    with open("datasets/meta/meta_subject_03.yml", "w") as f:
        yaml.safe_dump({"train": ["x"], "test": ["a", "b"]}, f)
    em = PF.two_takes(skel, seed=11)
    sr = PF.two_takes(skel, seed=12)
    assert np.abs(em["traj_pred"]["a"][:, 32:35]).min() > 0
    em_file = dict(em, vel_pred={k: np.zeros((len(v), skel.nv)) for k, v in em["traj_pred"].items()})     # the ego_mimic layout has more keys
    paths = {"em": "results/egomimic/subject_03/results/iter_0003_test.p", "sr": "results/statereg/subject_03/results/iter_0100_test.p"}
    metrics.save_results(paths["em"], em_file, {"algo": "ego_mimic", "num_reset": 0})
    metrics.save_results(paths["sr"], sr, {"algo": "state_reg", "num_sample": 23, "epoch_loss": 0.1})
    before = {k: open(p, "rb").read() for k, p in paths.items()}
    out = evaluate.main(["--cfg", "subject_03", "--iter", "3", "--data", "test", "--statereg-cfg", "subject_03", "--statereg-iter", "100",
                         "--mode", "stats", "--joint-pos", "--host"])
    text = capsys.readouterr().out
    assert {k: open(p, "rb").read() for k, p in paths.items()} == before
    assert (pickle.load(open(paths["em"], "rb"))[0]["traj_pred"]["a"][:, 32:35] != 0).all()
    mask = pose3d.body_mask(skel, pose3d.HANDS)
    for algo, res in (("ego mimic", em), ("state reg", sr)):
        clean = {k: {t: v.copy() for t, v in res[k].items()} for k in ("traj_pred", "traj_orig")}
        metrics.remove_noisy_hands(clean)
        three, joint = metrics.compute_metrics(clean), pose3d.compute_joint_metrics(clean, skel, mask=mask, backend="host")
        raw = metrics.compute_metrics(res)
        assert raw["pose_dist"] != three["pose_dist"]                               # the hands were zeroed for the printed numbers
        assert out[algo]["pose_dist"] == three["pose_dist"] and out[algo]["joint_pos"]["pa_mpjpe"] == joint["pa_mpjpe"]
        assert "=" * 10 + " %s " % algo + "=" * 10 in text
        assert "all - pose dist: %.4f, vel dist: %.4f, accels: %.4f" % (three["pose_dist"], three["vel_dist"], three["accels"]) in text
        assert pose3d.format_line([joint[k] for k in FIGS]) in text
        assert "mpjpe: %.2f mm" % (1e3 * joint["mpjpe"]) in text
    assert text.count("LeftHand") == 2 and "RightFoot" in text                       # the per-body table, once per algorithm
    # --keep-hands counts them; without --joint-pos nothing of the 3D part is printed
    kept = evaluate.main(["--cfg", "subject_03", "--iter", "3", "--mode", "stats", "--joint-pos", "--keep-hands", "--host"])
    assert set(kept) == {"ego mimic"} and kept["ego mimic"]["joint_pos"]["per_body"][list(skel.body_names).index("LeftHand")] > 0
    capsys.readouterr()
    evaluate.main(["--cfg", "subject_03", "--iter", "3", "--mode", "stats"])
    assert "mpjpe" not in capsys.readouterr().out
