"""The host path of the plausibility figures (egopose_amd/plausibility.py): the feet's inertia boxes, cases with known answers through
`score_host`, `Skeleton.body_frames` against the oracle, the aggregation loops with their nan rule, and the `--physical` command lines."""
import itertools
import pickle

import numpy as np
import pytest

import contact_fixture as CF
import pose3d_fixture as PF
import tree_fixture as F

FIGS = ("pen_mean", "pen_max", "gap_mean", "contact_ratio", "skate_mean")
TALL = 0.07          # a contact height above the feet's 0.06 m thick boxes: all 16 corners of two flat feet count, not the 8 of the soles


def _box_inertia(m, h):
    return m / 3.0 * np.diag([h[1] ** 2 + h[2] ** 2, h[0] ** 2 + h[2] ** 2, h[0] ** 2 + h[1] ** 2])


def _check_box(sk, name):
    """The corners of `name`'s box: centred on the COM, edges along three orthogonal axes, and a solid box of these half sizes and the
    body's mass has the body's inertia."""
    from egopose_amd.plausibility import ContactSet
    cs = ContactSet.feet(sk, bodies=(name,))
    b = list(sk.body_names).index(name)
    assert cs.K == 8 and (cs.body == b).all() and (cs.group == 0).all()
    centre = sk.body_com[b] - sk.body_pos[b]
    np.testing.assert_allclose(cs.offset.mean(0), centre, atol=1e-15)
    c = cs.offset - centre                                      # corner c has the signs of product((-1, 1), repeat=3): bit 2, 1, 0 = axis 0, 1, 2
    axes = [0.5 * (c[4] - c[0]), 0.5 * (c[2] - c[0]), 0.5 * (c[1] - c[0])]
    h = np.array([np.linalg.norm(a) for a in axes])
    V = np.stack([a / np.linalg.norm(a) for a in axes], axis=1)
    np.testing.assert_allclose(V.T @ V, np.eye(3), atol=1e-12)
    signs = np.array(list(itertools.product((-1.0, 1.0), repeat=3)))
    np.testing.assert_allclose(c, (signs * h) @ V.T, atol=1e-14)
    np.testing.assert_allclose(V @ _box_inertia(sk.body_mass[b], h) @ V.T, sk.body_inertia[b], atol=1e-12, rtol=0)
    return h, V


def test_feet_are_the_inertia_boxes_of_the_humanoid(skel):
    from egopose_amd.plausibility import ContactSet
    for name in ("LeftFoot", "RightFoot"):
        h, V = _check_box(skel, name)
        along = np.abs(V.T) @ h                                 # half sizes along x, y, z (the feet's inertias are diagonal)
        np.testing.assert_allclose(along, [0.062, 0.100, 0.030], atol=5e-4)
    cs = ContactSet.feet(skel)
    assert cs.K == 16 and cs.group.tolist() == [0] * 8 + [1] * 8
    names = list(skel.body_names)
    assert cs.body.tolist() == [names.index("LeftFoot")] * 8 + [names.index("RightFoot")] * 8
    # the soles lie 0.8606 m below the asset's origin in the zero pose, level across both feet
    low = (skel.body_pos[cs.body] + cs.offset)[:, 2]
    assert abs(low.min() + 0.8606) < 5e-5 and np.sum(np.abs(low - low.min()) < 1e-12) == 8


@pytest.mark.parametrize("name", list(F.TREES))
def test_inertia_boxes_on_the_trees(name):
    """Rotated inertias. The generator draws principal moments freely, so some bodies violate the triangle inequality (no solid box,
    no solid body at all, has such an inertia): those are refused, every other body's box reproduces its inertia."""
    from egopose_amd.plausibility import ContactSet
    sk = F.skeleton(name)
    good = 0
    for b, body in enumerate(sk.body_names):
        lam = np.linalg.eigvalsh(sk.body_inertia[b])
        if (lam.sum() - 2.0 * lam).min() > 1e-6:
            _check_box(sk, body)
            good += 1
        elif (lam.sum() - 2.0 * lam).min() < -1e-6:
            with pytest.raises(ValueError):
                ContactSet.feet(sk, bodies=(body,))
    assert good >= 2


def test_contact_set_refuses_bad_input(skel, tmp_path):
    from egopose_amd.plausibility import ContactSet
    nb = len(skel.body_names)
    zero = np.zeros((1, 3))
    for args in (([], np.zeros((0, 3))), ([0] * 33, np.zeros((33, 3))), ([-1], zero), ([0], [[0.0, np.nan, 0.0]]), ([0], [[np.inf, 0.0, 0.0]]),
                 ([0], np.zeros((2, 3))), ([0.5], zero), ([[0]], zero)):
        with pytest.raises(ValueError):
            ContactSet(*args)
    with pytest.raises(ValueError):
        ContactSet([nb], zero, nbody=nb)
    with pytest.raises(ValueError):
        ContactSet([nb], zero).check(skel)
    with pytest.raises(ValueError):
        ContactSet([0], zero, group=[0, 1])
    with pytest.raises(ValueError):
        ContactSet.feet(skel, bodies=("LeftFoot", "Tail"))
    flat = F.mutate(skel, body_inertia=np.array([np.diag([1.0, 0.1, 0.1])] * nb))       # lam_0 > lam_1 + lam_2: h_0^2 < 0
    with pytest.raises(ValueError):
        ContactSet.feet(flat)
    assert ContactSet([nb - 1] * 32, np.zeros((32, 3)), nbody=nb).K == 32
    # the file format is the three arrays, and a round trip keeps every bit
    cs = ContactSet.feet(skel)
    cs.to_file(tmp_path / "feet.json")
    back = ContactSet.from_file(tmp_path / "feet.json")
    assert (back.body == cs.body).all() and (back.offset == cs.offset).all() and (back.group == cs.group).all()
    (tmp_path / "bad.json").write_text('{"body": [0], "offset": [[0, 0, 0]]}')
    with pytest.raises(ValueError):
        ContactSet.from_file(tmp_path / "bad.json")


def _standing(skel, z=None, n=1):
    """Zero pose rows with the soles exactly on the ground (or the root at height z)."""
    from egopose_amd.plausibility import ContactSet
    cs = ContactSet.feet(skel)
    sole = (skel.body_pos[cs.body] + cs.offset)[:, 2].min() - skel.body_pos[0, 2]        # sole height relative to the root body
    q = np.zeros((n, skel.nq))
    q[:, 3] = 1.0
    q[:, 2] = -sole if z is None else z
    return cs, q, -sole


def test_known_answers_standing(skel):
    """Standing on the ground, 5 mm lower, 0.1 m higher. The soles are 0.8606 m below the asset's ORIGIN; qpos[2] is the height of the
    root body, which the asset puts 5.4 mm above its origin, so the feet touch the ground with the root at 0.8660 m and sink 5.4 mm at
    0.8606 m (row 3 pins that). With the default contact height of 0.02 m the 8 sole corners are in contact (the boxes are 0.06 m
    thick); all 16 corners are with a contact height above that (TALL)."""
    from egopose_amd import plausibility as P
    cs, q, z0 = _standing(skel, n=4)
    assert abs(z0 - (0.8606 + skel.body_pos[0, 2])) < 5e-5      # the root body sits 5.4 mm above the asset's origin
    q[1, 2] -= 0.005
    q[2, 2] += 0.1
    q[3, 2] = 0.8606                                            # the root AT 0.8606 m: the soles 5.4 mm under the ground
    none = np.full(4, -1)
    r = P.score_host(skel, cs, q, none)
    np.testing.assert_allclose(r["pen"], [0.0, 0.005, 0.0, skel.body_pos[0, 2]], atol=1e-15)
    np.testing.assert_allclose(r["gap"], [0.0, 0.0, 0.1, 0.0], atol=1e-15)
    assert r["n_contact"].tolist() == [8, 8, 0, 8]              # the soles' corners; the boxes' upper corners are 0.06 m above them
    assert P.score_host(skel, cs, q, none, contact_height=TALL)["n_contact"].tolist() == [16, 16, 0, 16]
    for k in ("n_skate", "skate", "skate_max"):                 # no following row: zero skate outputs
        assert (r[k] == 0).all()
    # the ground elsewhere: the same figures from the same poses lifted with it
    q2 = q.copy()
    q2[:, 2] += 0.25
    r2 = P.score_host(skel, cs, q2, none, ground_z=0.25)
    np.testing.assert_allclose(r2["pen"], r["pen"], atol=1e-15)
    assert r2["n_contact"].tolist() == [8, 8, 0, 8]


def test_known_answers_sliding_and_turning(skel):
    from egopose_amd import plausibility as P
    cs, q, _ = _standing(skel, n=4)
    d = np.array([0.03, -0.04])
    q[1, :2] += d                                               # row 0 -> row 1: a slide by |d| = 0.05 with both feet down
    a = 0.2
    q[3, 3], q[3, 6] = np.cos(a / 2), np.sin(a / 2)             # row 2 -> row 3: a turn about the vertical through the root
    nxt = np.array([1, -1, 3, -1])
    for h, cnt in ((0.02, 8), (TALL, 16)):
        r = P.score_host(skel, cs, q, nxt, contact_height=h)
        assert r["n_skate"].tolist() == [cnt, 0, cnt, 0]
        np.testing.assert_allclose([r["skate"][0], r["skate_max"][0]], [0.05, 0.05], atol=1e-15)
        assert r["skate"][1] == 0.0 and r["skate_max"][1] == 0.0 and r["skate"][3] == 0.0
        # each corner moves along an arc about the root's axis: chord = 2 r sin(a / 2), r its horizontal distance from the axis
        rel = skel.body_pos[cs.body] + cs.offset - skel.body_pos[0]
        sel = rel[:, 2] - rel[:, 2].min() <= h
        chord = 2.0 * np.hypot(rel[sel, 0], rel[sel, 1]) * np.sin(a / 2)
        np.testing.assert_allclose([r["skate"][2], r["skate_max"][2]], [chord.mean(), chord.max()], atol=1e-15)
    assert chord.max() > 1.2 * chord.min()


def test_a_raised_leg_leaves_the_other_foot(skel):
    from egopose_amd import plausibility as P
    cs, q, _ = _standing(skel, n=2)
    names = list(skel.joint_names)
    q[:, 7 + names.index("LeftUpLeg_x")] = -1.0                 # the left thigh swung a radian about x: the foot well off the ground
    q[1, :2] += [0.0, 0.02]
    r = P.score_host(skel, cs, q, np.array([1, -1]), contact_height=TALL)
    left = list(skel.body_names).index("LeftFoot")
    assert (r["points"][0][cs.body == left][:, 2] > 0.1).all()
    assert r["n_contact"].tolist() == [8, 8] and r["n_skate"].tolist() == [8, 0]
    np.testing.assert_allclose([r["pen"][0], r["gap"][0], r["skate"][0], r["skate_max"][0]], [0.0, 0.0, 0.02, 0.02], atol=1e-15)
    per_foot = P.score_points(r["points"][:, cs.group == 0], np.array([1, -1]), contact_height=TALL)
    assert per_foot["n_contact"].tolist() == [0, 0] and per_foot["gap"][0] > 0.1 and per_foot["skate"][0] == 0.0


def test_body_frames_against_the_oracle(skel):
    from oracle import dynamics as D
    cases = [(skel, PF.poses(skel, 6, np.random.RandomState(3)))]
    cases += [(F.skeleton(name), F.rand_state(F.skeleton(name), np.random.RandomState(5), 3)[0]) for name in F.TREES]
    for sk, qs in cases:
        for q in qs:
            R, p = sk.body_frames(q)
            Ro, po = D.fk(sk, q)[:2]
            np.testing.assert_allclose(R, Ro, atol=1e-14)
            np.testing.assert_allclose(p, po, atol=1e-14)
            assert (sk.body_xpos(q) == p).all()                 # body_xpos keeps its behaviour: the positions of the same pass


def test_score_host_against_the_yardstick(skel):
    """The product's vectorised host path against the point-by-point loops of the fixture, on the random cases the kernel gets."""
    from egopose_amd import plausibility as P
    cs = P.ContactSet.feet(skel)
    c = CF.case(skel, cs.body, cs.offset, 41, seed=5)
    N = len(c["qpos"])
    nxt = np.concatenate([c["nxt"], np.full(N - 41, -1)])
    want, pts = CF.yardstick(c["points"], None, nxt)
    r = P.score_host(skel, cs, c["qpos"], nxt)
    got = np.stack([r[k] for k in P.COLS], axis=1)
    np.testing.assert_array_equal(got[:, 2:4], want[:, 2:4])
    np.testing.assert_allclose(got, want, atol=1e-14, rtol=0)
    np.testing.assert_allclose(r["points"], pts, atol=1e-14, rtol=0)
    assert (want[:41, 0] > 0).sum() >= 5 and (want[:41, 1] > 0).sum() >= 5 and (want[:41, 3] > 0).sum() >= 5     # all three regimes occur
    with pytest.raises(ValueError):
        P.score_host(skel, cs, c["qpos"], nxt[:-1])
    with pytest.raises(ValueError):
        P.score_host(skel, cs, c["qpos"], np.where(np.arange(N) == 1, N, nxt))
    with pytest.raises(ValueError):
        P.score_host(skel, cs, c["qpos"], nxt, contact_height=np.nan)


def _traj_row(skel, cs, traj, h=0.02, gz=0.0):
    """The five figures of one trajectory, frame by frame through the yardstick."""
    pts = CF.points_of(skel, cs.body, cs.offset, traj)
    T = len(traj)
    rows = np.stack([CF.figures_of_points(pts[t], pts[t + 1] if t + 1 < T else None, gz, h) for t in range(T)])
    skated = rows[:, 3] > 0
    return np.array([rows[:, 0].mean(), rows[:, 0].max(), rows[:, 1].mean(), (rows[:, 2] > 0).mean(), rows[skated, 4].mean() if skated.any() else np.nan])


def _nanmean_rows(rows):
    rows = np.array(rows)
    return np.append(rows[:, :4].mean(0), np.nanmean(rows[:, 4]) if (~np.isnan(rows[:, 4])).any() else np.nan)


def test_compute_plausibility_against_a_per_take_loop(skel):
    from egopose_amd import plausibility as P
    res = CF.two_takes(skel)
    res["traj_pred"]["c"] = res["traj_pred"]["a"][:1].copy()                  # one frame: nothing follows, skate_mean is nan
    res["traj_orig"]["c"] = res["traj_orig"]["a"][:1].copy()
    fly = res["traj_pred"]["b"].copy()
    fly[:, 2] += 1.0                                                          # floating throughout: no contact, nan again
    res["traj_pred"]["d"], res["traj_orig"]["d"] = fly, res["traj_orig"]["b"].copy()
    cs = P.ContactSet.feet(skel)
    out = P.compute_plausibility(res, skel, backend="host", contact_height=0.03)
    assert out["ground_z"] == 0.0 and out["contact_height"] == 0.03
    for key in ("traj_pred", "traj_orig"):
        want = {k: _traj_row(skel, cs, res[key][k], h=0.03) for k in "abcd"}
        for k in "abcd":
            np.testing.assert_allclose(out[key]["per_take"][k], want[k], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose([out[key][f] for f in FIGS], _nanmean_rows(list(want.values())), rtol=1e-12)
        assert np.isnan(want["c"][4]) and not np.isnan(out[key]["skate_mean"]) and out[key]["skate_mean"] > 1e-4
        assert set(out[key]["per_group"]) == {0, 1}
    assert np.isnan(out["traj_pred"]["per_take"]["d"][4]) and out["traj_pred"]["per_take"]["d"][3] == 0.0
    assert out["traj_pred"]["per_take"]["d"][2] > 0.9 and 0.0 < out["traj_pred"]["contact_ratio"] < 1.0
    # a single foot as the contact set is that foot's group row
    left = P.ContactSet(cs.body[:8], cs.offset[:8])
    one = P.compute_plausibility(res, skel, contacts=left, which=("traj_pred",), backend="host", contact_height=0.03)
    np.testing.assert_allclose(out["traj_pred"]["per_group"][0], [one["traj_pred"][f] for f in FIGS], rtol=1e-12)
    # results without MoCap score the prediction alone; a trajectory that is all nan gives nan
    wild = P.compute_plausibility({"traj_pred": {"c": res["traj_pred"]["c"]}}, skel, backend="host")
    assert "traj_orig" not in wild and np.isnan(wild["traj_pred"]["skate_mean"])
    with pytest.raises(ValueError):
        P.compute_plausibility(res, skel, backend="eager")
    with pytest.raises(ValueError):
        P.compute_plausibility(res, skel, backend="hip")                      # neither a context nor a config: nothing falls back
    with pytest.raises(ValueError):
        P.compute_plausibility({"traj_pred": {}}, skel, backend="host")


def test_compute_forecast_plausibility_against_a_per_window_loop(skel):
    from egopose_amd import plausibility as P
    res = CF.two_takes(skel)
    win = lambda d: {"a": np.stack([d["a"][s:s + 9] for s in (0, 2, 5)]), "b": d["b"][None]}
    wins = {"traj_pred": win(res["traj_pred"]), "traj_orig": win(res["traj_orig"])}
    m, horizon = 3, 5
    cs = P.ContactSet.feet(skel)
    out = P.compute_forecast_plausibility(wins, skel, m, horizon, backend="host", contact_height=0.03)
    for key in ("traj_pred", "traj_orig"):
        want = {k: _nanmean_rows([_traj_row(skel, cs, w[m:m + horizon], h=0.03) for w in wins[key][k]]) for k in "ab"}
        for k in "ab":
            np.testing.assert_allclose(out[key]["per_take"][k], want[k], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose([out[key][f] for f in FIGS], _nanmean_rows(list(want.values())), rtol=1e-12)
    # the following row stays inside the window: a horizon of one frame has no skate at all
    assert np.isnan(P.compute_forecast_plausibility(wins, skel, m, 1, backend="host", contact_height=0.03)["traj_pred"]["skate_mean"])
    with pytest.raises(ValueError):
        P.compute_forecast_plausibility(res, skel, m, horizon, backend="host")          # trajectories, not windows


def _saved(skel, tmp_path, monkeypatch):
    import yaml
    from egopose_amd import metrics
    monkeypatch.chdir(tmp_path)
    (tmp_path / "datasets" / "meta").mkdir(parents=True)
    with open("datasets/meta/meta_subject_03.yml", "w") as f:
        yaml.safe_dump({"train": ["x"], "test": ["a", "b"]}, f)
    em, sr = CF.two_takes(skel, seed=11), CF.two_takes(skel, seed=12)
    sr["traj_orig"] = {k: v.copy() for k, v in em["traj_orig"].items()}                 # both algorithms ran on the same takes
    metrics.save_results("results/egomimic/subject_03/results/iter_0003_test.p", em, {"algo": "ego_mimic", "num_reset": 0})
    metrics.save_results("results/statereg/subject_03/results/iter_0100_test.p", sr, {"algo": "state_reg"})
    return em, sr


def test_mode_stats_physical_on_the_host(skel, tmp_path, monkeypatch, capsys):
    from egopose_amd import evaluate, metrics, plausibility as P
    em, sr = _saved(skel, tmp_path, monkeypatch)
    argv = ["--cfg", "subject_03", "--iter", "3", "--statereg-cfg", "subject_03", "--mode", "stats", "--host"]
    P.ContactSet.feet(skel, bodies=("RightFoot",)).to_file("right.json")
    out = evaluate.main(argv + ["--physical", "--contact-height", "0.03"])
    text = capsys.readouterr().out
    for algo, res in (("ego mimic", em), ("state reg", sr)):
        want = P.compute_plausibility(res, skel, backend="host", contact_height=0.03)
        got = out[algo]["physical"]
        assert got["contact_height"] == 0.03 and got["ground_z"] == 0.0
        assert [got["traj_pred"][f] for f in FIGS] == [want["traj_pred"][f] for f in FIGS]
        assert P.format_line([want["traj_pred"][f] for f in FIGS], algo, 0.0, 0.03) in text
    assert "traj_orig" not in out["ego mimic"]["physical"] and "traj_orig" in out["state reg"]["physical"]
    assert text.count("mocap - pen:") == 1 and P.format_line([want["traj_orig"][f] for f in FIGS], "mocap", 0.0, 0.03) in text
    assert "contact height: 30.0 mm" in text and "ground z: 0.0 mm" in text
    # another contact set, another ground; alone, the one algorithm gets the mocap row; without the flag nothing of it is printed
    one = evaluate.main(argv[:4] + ["--mode", "stats", "--host", "--physical", "--contacts", "right.json", "--ground-z", "0.01"])
    right = P.compute_plausibility(em, skel, contacts=P.ContactSet.from_file("right.json"), backend="host", ground_z=0.01)
    assert one["ego mimic"]["physical"]["traj_pred"]["pen_mean"] == right["traj_pred"]["pen_mean"] != out["ego mimic"]["physical"]["traj_pred"]["pen_mean"]
    assert one["ego mimic"]["physical"]["traj_orig"]["gap_mean"] == right["traj_orig"]["gap_mean"]
    assert "ground z: 10.0 mm" in capsys.readouterr().out
    evaluate.main(argv)
    assert "pen:" not in capsys.readouterr().out


def test_forecast_mode_stats_physical_on_the_host(skel, tmp_path, monkeypatch, capsys):
    import yaml
    from egopose_amd import evaluate_forecast, metrics, plausibility as P
    from egopose_amd.config import ForecastConfig
    em, _ = _saved(skel, tmp_path, monkeypatch)
    cfg = ForecastConfig("subject_03", create_dirs=False)
    m = cfg.fr_margin
    long = {k: {t: np.concatenate([v] * (1 + (m + 6) // len(v)))[:m + 6] for t, v in em[k].items()} for k in em}     # windows of m + 6 frames
    wins = {k: {t: np.stack([v, v[::-1]]) for t, v in long[k].items()} for k in long}
    metrics.save_results(evaluate_forecast.result_path(cfg, 2, "test"), wins, {"algo": "ego_forecast"})
    out = evaluate_forecast.main(["--cfg", "subject_03", "--iter", "2", "--mode", "stats", "--horizon", "5", "--physical", "--host"])
    text = capsys.readouterr().out
    want = P.compute_forecast_plausibility(wins, skel, m, 5, backend="host")
    for key, what in (("traj_pred", "all - horizon: 5"), ("traj_orig", "mocap")):
        assert [out["physical"][key][f] for f in FIGS] == [want[key][f] for f in FIGS]
        assert P.format_line([want[key][f] for f in FIGS], what) in text
    assert "pose_dist" in out and "pose dist" in text


def test_wild_stats_physical_on_the_host(skel, tmp_path, monkeypatch, capsys):
    """Takes without MoCap: the pickles hold traj_pred alone, and the plausibility row is their only 3D figure."""
    import json
    from egopose_amd import evaluate, evaluate_forecast, metrics, plausibility as P
    from egopose_amd.config import Config, ForecastConfig
    em, sr = _saved(skel, tmp_path, monkeypatch)
    cfg, fcfg = Config("subject_03", create_dirs=False), ForecastConfig("subject_03", create_dirs=False)
    with open("%s/meta/meta_wild_x.yml" % cfg.data_dir, "w") as f:
        f.write("tpv_offset: {a: 0, b: 0}\n")
    rng = np.random.RandomState(4)
    for take in "ab":
        (tmp_path / cfg.data_dir / "tpv" / "poses" / take).mkdir(parents=True)
        for fr in range(fcfg.fr_margin * 2 + 12):
            kp = np.stack([rng.uniform(400, 1500, 25), rng.uniform(100, 1000, 25), rng.uniform(0.2, 1.0, 25)], axis=1)
            with open("%s/tpv/poses/%s/%05d_keypoints.json" % (cfg.data_dir, take, fr), "w") as f:
                json.dump({"people": [{"pose_keypoints_2d": kp.reshape(-1).tolist()}]}, f)
    metrics.save_results("%s/iter_0003_wild_x.p" % cfg.result_dir, {"traj_pred": em["traj_pred"]}, {"algo": "ego_mimic"})
    out = evaluate.main(["--cfg", "subject_03", "--iter", "3", "--test-feat", "wild_x", "--mode", "wild-stats", "--physical", "--host"])
    text = capsys.readouterr().out
    want = P.compute_plausibility({"traj_pred": em["traj_pred"]}, skel, backend="host")
    got = out["ego mimic"]["physical"]
    assert "traj_orig" not in got and [got["traj_pred"][f] for f in FIGS] == [want["traj_pred"][f] for f in FIGS]
    assert P.format_line([want["traj_pred"][f] for f in FIGS], "ego mimic") in text and "mocap" not in text
    m = fcfg.fr_margin
    wins = {t: np.concatenate([v] * (1 + (m + 6) // len(v)))[None, :m + 6] for t, v in em["traj_pred"].items()}
    metrics.save_results("%s/iter_0002_wild_x.p" % fcfg.result_dir, {"traj_pred": wins}, {"algo": "ego_forecast"})
    fout = evaluate_forecast.main(["--cfg", "subject_03", "--iter", "2", "--test-feat", "wild_x", "--mode", "wild-stats", "--horizon", "5",
                                   "--physical", "--host"])
    fwant = P.compute_forecast_plausibility({"traj_pred": wins}, skel, m, 5, backend="host")
    assert [fout["physical"]["traj_pred"][f] for f in FIGS] == [fwant["traj_pred"][f] for f in FIGS]
    assert P.format_line([fwant["traj_pred"][f] for f in FIGS], "all - horizon: 5") in capsys.readouterr().out
