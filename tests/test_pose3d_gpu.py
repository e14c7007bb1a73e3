"""egp_pose3d_f64 (csrc/egp_pose3d.hip) against float64 forward kinematics of the oracle (oracle/dynamics.py: fk) and the numpy SVD with
the determinant correction (pose3d_fixture.py) -- never against the product's host path, never against the kernel."""
import functools

import numpy as np
import pytest
import torch

import pose3d_fixture as PF
import tree_fixture as F
from conftest import load_golden

pytestmark = pytest.mark.gpu

# Bounds on the absolute error against the yardstick, in metres: 10 x the largest error seen on the first run on an MI355X (FMA
# contraction and reduction order), per output, over n = 1, 63, 130 on the humanoid, the three masks and the six trees; anything above
# 1e-8 would be wrong rather than loose. MEASURED holds what was seen; every test prints its figures before it asserts.
#   largest, where: g_mpjpe 2.665e-15 (mask of three bodies, n = 63), mpjpe 9.391e-16 (the same), pa_mpjpe 3.143e-15 (n = 130),
#   root_err 1.776e-15 (n = 130), err 2.706e-15 (n = 63), xpos 3.553e-15 (n = 63; roots up to ~10 m from the origin, 2 ulp there).
#   The six trees stayed below 2e-15 everywhere (root at ~1 m); backend='hip' against 'host' on the two takes: at most 5.6e-17 m
#   in the figures and 5.7e-14 m/s^2 in accel_err.
MEASURED = dict(g_mpjpe=2.665e-15, mpjpe=9.391e-16, pa_mpjpe=3.143e-15, root_err=1.776e-15, err=2.706e-15, xpos=3.553e-15)
BOUND = {k: 10.0 * v for k, v in MEASURED.items()}
COLS = ("g_mpjpe", "mpjpe", "pa_mpjpe", "root_err")


def dev(a):
    return torch.as_tensor(np.array(a, order="C"), device="cuda")          # (a copy: the shared cases are read-only)


@pytest.fixture(scope="module")
def ctx(skel):
    from egopose_amd.hip import EgpContext
    c = load_golden("config_subject_03.npz")
    cx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"])
    yield cx
    cx.close()


@functools.lru_cache(maxsize=None)
def _case(n):
    """Pairs of the five kinds on the humanoid and their oracle positions, computed once per n."""
    from egopose_amd.skeleton import load_skeleton
    from oracle import dynamics as D
    sk = load_skeleton()
    pred, gt = PF.pairs(sk, n, seed=70 + n)
    X, Y = np.stack([D.fk(sk, q)[1] for q in pred]), np.stack([D.fk(sk, q)[1] for q in gt])
    for a in (pred, gt, X, Y):
        a.setflags(write=False)
    return pred, gt, X, Y


def _figures(X, Y, mask, nb):
    sel = np.array([(mask >> b) & 1 == 1 for b in range(nb)])
    rows, errs = zip(*[PF.figures_of_positions(X[i], Y[i], sel) for i in range(len(X))])
    return np.stack(rows), np.stack(errs)


def _run(cx, pred, gt, mask, nb, canaries=3):
    """Launch with every optional output (buffers with canary rows behind n) and with none -> numpy outputs of the first launch."""
    n = len(pred)
    shapes = dict(per_frame=(4,), err=(nb,), xpos_pred=(nb, 3), xpos_gt=(nb, 3))
    buf = {k: torch.full((n + canaries,) + s, -7.0, dtype=torch.float64, device="cuda") for k, s in shapes.items()}
    cx.pose3d(dev(pred), dev(gt), body_mask=mask, out={k: v[:n] for k, v in buf.items()})
    torch.cuda.synchronize()
    for k, v in buf.items():
        assert (v[n:] == -7.0).all(), "%s: rows behind n were written" % k
    out = {k: v[:n].cpu().numpy() for k, v in buf.items()}
    lean_buf = torch.full((n + canaries, 4), -7.0, dtype=torch.float64, device="cuda")
    lean = cx.pose3d(dev(pred), dev(gt), body_mask=mask, out=dict(per_frame=lean_buf[:n]))
    torch.cuda.synchronize()
    assert set(lean) == {"per_frame"} and (lean_buf[n:] == -7.0).all()
    np.testing.assert_array_equal(lean["per_frame"].cpu().numpy(), out["per_frame"])          # bit for bit
    return out


def _compare(tag, out, X, Y, mask, nb):
    rows, errs = _figures(X, Y, mask, nb)
    seen = {c: float(np.abs(out["per_frame"][:, i] - rows[:, i]).max()) for i, c in enumerate(COLS)}
    seen["err"] = float(np.abs(out["err"] - errs).max())
    seen["xpos"] = float(max(np.abs(out["xpos_pred"] - X).max(), np.abs(out["xpos_gt"] - Y).max()))
    print("POSE3D %s: " % tag + ", ".join("%s %.3e" % kv for kv in seen.items()))
    assert np.isfinite(out["per_frame"]).all()
    for k, v in seen.items():
        assert v <= BOUND[k], "%s %s: %.3e above the bound %.3e" % (tag, k, v, BOUND[k])
    return rows


@pytest.mark.parametrize("n", [1, 63, 130])
def test_kernel_against_the_yardstick(ctx, skel, n):
    """One frame; a ragged last workgroup (63 = 15 x 4 + 3 waves); more than one workgroup and the five kinds many times over."""
    pred, gt, X, Y = _case(n)
    nb = len(skel.body_names)
    mask = (1 << nb) - 1
    rows = _compare("n=%d" % n, _run(ctx, pred, gt, mask, nb), X, Y, mask, nb)
    if n >= 5:                                   # the kinds are what they claim: identical, translated and turned pairs align to ~0
        assert rows[0, 2] > 1e-3 and rows[1, 2] > 1e-2 and rows[2].max() <= 1e-12
        assert rows[3, 1] <= 1e-12 and rows[3, 2] <= 1e-12 and rows[3, 0] > 1e-2
        assert rows[4, 2] <= 1e-12 and rows[4, 1] > 1e-2


@pytest.mark.parametrize("which", ["all", "no-hands", "three"])
def test_masks(ctx, skel, which):
    from egopose_amd import pose3d
    names = list(skel.body_names)
    nb = len(names)
    mask = {"all": None, "no-hands": pose3d.body_mask(skel, pose3d.HANDS),
            "three": 1 | 1 << names.index("LeftFoot") | 1 << names.index("RightHand")}[which]
    pred, gt, X, Y = _case(63)
    out = _run(ctx, pred, gt, mask, nb)
    mask = (1 << nb) - 1 if mask is None else mask
    _compare("mask=%s" % which, out, X, Y, mask, nb)
    clear = [b for b in range(nb) if not (mask >> b) & 1]
    assert (out["err"][:, clear] == 0.0).all()


@pytest.fixture(scope="module")
def contexts():
    """name -> the tree's context, made as test_dynamics_reference_gpu.py makes it."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = F.context_for(F.skeleton(name), F.SEEDS[name], gains=F.pd_case(name)["gains"])
        return made[name]

    yield get
    for cx in made.values():
        cx.close()


@pytest.mark.parametrize("name", list(F.TREES))
def test_trees(contexts, name):
    """star4 has 5 bodies and full64 has 64 dofs: the ends of the lane reductions and of the LDS budget."""
    from oracle import dynamics as D
    sk, cx = F.skeleton(name), contexts(name)
    nb = len(sk.body_names)
    pred, gt = PF.pairs(sk, 5, F.SEEDS[name] + 3, gen=lambda s, n, rng: F.rand_state(s, rng, n)[0])
    X, Y = np.stack([D.fk(sk, q)[1] for q in pred]), np.stack([D.fk(sk, q)[1] for q in gt])
    mask = (1 << nb) - 1
    _compare("tree=%s" % name, _run(cx, pred, gt, mask, nb), X, Y, mask, nb)


def test_compute_joint_metrics_on_the_kernel_matches_the_host_loop(ctx, skel):
    from egopose_amd import pose3d
    res = PF.two_takes(skel)
    mask = pose3d.body_mask(skel, pose3d.HANDS)
    a = pose3d.compute_joint_metrics(res, skel, mask=mask, backend="hip", ctx=ctx)
    b = pose3d.compute_joint_metrics(res, skel, mask=mask, backend="host")
    win = lambda d: {"a": np.stack([d["a"][s:s + 9] for s in (0, 2, 5)]), "b": d["b"][None]}
    wins = {"traj_pred": win(res["traj_pred"]), "traj_orig": win(res["traj_orig"])}
    c = pose3d.compute_forecast_joint_metrics(wins, skel, 3, 5, mask=mask, backend="hip", ctx=ctx)
    d = pose3d.compute_forecast_joint_metrics(wins, skel, 3, 5, mask=mask, backend="host")
    for tag, x, y in (("takes", a, b), ("windows", c, d)):
        seen = {k: abs(x[k] - y[k]) for k in COLS}
        seen["err"] = float(np.abs(x["per_body"] - y["per_body"]).max())
        acc = abs(x["accel_err"] - y["accel_err"])
        print("POSE3D joint-metrics %s: " % tag + ", ".join("%s %.3e" % kv for kv in seen.items()) + ", accel_err %.3e" % acc)
        assert x["mpjpe"] > 1e-3 and set(x["per_take"]) == {"a", "b"}
        for k, v in seen.items():
            assert v <= BOUND[k]
        assert acc <= 4.0 * BOUND["xpos"] * 900.0              # a second difference of positions (|1| + |-2| + |1|) over dt^2 = 1 / 900


def test_command_line_on_the_kernel(skel, tmp_path, monkeypatch, capsys):
    """`--mode stats --joint-pos` without --host makes its own context from the config and agrees with --host; the `--joint-pos` hooks
    of the two eval modes print their line from a result in memory."""
    import types
    import yaml
    from egopose_amd import evaluate, evaluate_forecast, metrics, pose3d
    from egopose_amd.config import Config, ForecastConfig
    monkeypatch.chdir(tmp_path)
    (tmp_path / "datasets" / "meta").mkdir(parents=True)
    with open("datasets/meta/meta_subject_03.yml", "w") as f:
        yaml.safe_dump({"train": ["x"], "test": ["a", "b"]}, f)
    em, sr = PF.two_takes(skel, seed=11), PF.two_takes(skel, seed=12)
    metrics.save_results("results/egomimic/subject_03/results/iter_0003_test.p", em, {"algo": "ego_mimic", "num_reset": 0})
    metrics.save_results("results/statereg/subject_03/results/iter_0100_test.p", sr, {"algo": "state_reg"})
    argv = ["--cfg", "subject_03", "--iter", "3", "--statereg-cfg", "subject_03", "--mode", "stats", "--joint-pos"]
    hip = evaluate.main(argv)
    text = capsys.readouterr().out
    host = evaluate.main(argv + ["--host"])
    for algo in ("ego mimic", "state reg"):
        a, b = hip[algo]["joint_pos"], host[algo]["joint_pos"]
        assert a["mpjpe"] > 1e-3 and pose3d.format_line([a[k] for k in pose3d.FIGURES]) in text
        for k in COLS:
            assert abs(a[k] - b[k]) <= BOUND[k]
        assert np.abs(a["per_body"] - b["per_body"]).max() <= BOUND["err"]
    capsys.readouterr()
    args = types.SimpleNamespace(host=False, keep_hands=True, gpu_index=0)
    one = evaluate._joint_pos(em, Config("subject_03"), args, "ego_mimic", table=False)
    win = lambda d: {"a": np.stack([d["a"][s:s + 9] for s in (0, 2, 5)]), "b": d["b"][None]}
    fcfg = ForecastConfig("subject_03")
    fcfg.fr_margin = 3                                      # windows of 9 frames: 3 of margin, a horizon of 5
    two = evaluate_forecast._joint_pos({k: win(em[k]) for k in em}, fcfg, args, 5)
    lines = capsys.readouterr().out.strip().split("\n")
    assert lines == [pose3d.format_line([one[k] for k in pose3d.FIGURES]), pose3d.format_line([two[k] for k in pose3d.FIGURES], "all - horizon: 5")]
    assert one["per_body"][list(skel.body_names).index("LeftHand")] > 0 and two["pa_mpjpe"] > 1e-4


def test_argument_errors_launch_nothing(ctx, skel):
    from egopose_amd import _lib as L
    nb = len(skel.body_names)
    pred, gt, _, _ = _case(1)
    qp, qg = dev(np.repeat(pred, 2, 0)), dev(np.repeat(gt, 2, 0))
    assert torch.isfinite(ctx.pose3d(qp, qg)["per_frame"]).all()           # (the tree is uploaded: the refusals below are about the arguments)
    pf = torch.full((2, 4), -7.0, dtype=torch.float64, device="cuda")
    bad = [dict(body_mask=0b11), dict(body_mask=1 << nb | 0b111), dict(body_mask=-1)]
    for kw in bad:
        with pytest.raises(ValueError):
            ctx.pose3d(qp, qg, out=dict(per_frame=pf), **kw)
    for a, b, out in ((qp[:, :-1].contiguous(), qg, {}), (qp, qg[:1], {}), (qp.float(), qg, {}), (qp, qg.cpu(), {}),
                      (qp, qg, dict(per_frame=pf[:1])), (qp, qg, dict(per_frame=pf, err=torch.zeros(2, nb + 1, dtype=torch.float64, device="cuda"))),
                      (qp, qg, dict(per_frame=pf.float())), (qp, qg, dict(per_frame=pf, p=pf))):
        with pytest.raises(ValueError):
            ctx.pose3d(a, b, out=dict(out))
    # the C entry refuses the same on its own (EGP_E_INVALID = -1), and n = 0 is fine
    p = lambda t: L.C.c_void_p(t.data_ptr())
    null = L.C.c_void_p(0)
    call = lambda mask, q=p(qp), o=p(pf), n=2: ctx.lib.egp_pose3d_f64(ctx.handle, q, p(qg), mask, o, null, null, null, n, L.current_stream())
    assert call(0b11) == -1 and call(1 << nb | 0b111) == -1 and call(0b111, q=null) == -1 and call(0b111, o=null) == -1
    assert call(0b111, n=-1) == -1 and call(0b111, n=0) == 0
    torch.cuda.synchronize()
    assert (pf == -7.0).all()
    ctx.pose3d(qp, qg, out=dict(per_frame=pf))
    torch.cuda.synchronize()
    assert (pf != -7.0).all()
