"""egp_contact_f64 (csrc/egp_contact.hip) against float64 forward kinematics of the oracle (oracle/dynamics.py: fk, R and p) and the
definitions written out point by point (contact_fixture.py) -- never against the product's host path, never against the kernel."""
import functools

import numpy as np
import pytest
import torch

import contact_fixture as CF
import tree_fixture as F
from conftest import load_golden

pytestmark = pytest.mark.gpu

# Bounds on the absolute error against the yardstick, in metres: 10 x the largest error seen on the first run on an MI355X (FMA
# contraction and reduction order), per output, over n = 1, 63, 130 on the humanoid with `row` given and absent, K = 1, 16, 32 and the
# six trees; anything above 1e-8 would be wrong rather than loose. The two counts are compared exactly (the fixture keeps every point
# more than 1e-9 m from contact_height). MEASURED holds what was seen; every test prints its figures before it asserts.
#   largest, where: pen 3.643e-16 (tree full64), gap 6.731e-16 (tree humanoid-topology), skate and skate_max 1.818e-15 (n = 63, item 20:
#   an unrelated following row, metres away), points 2.665e-15 (n = 63 and K = 32; roots up to ~10 m from the origin, 2 ulp there).
#   On the humanoid pen and gap stayed below 2.8e-16. backend='hip' against 'host' on the two takes and their windows: at most
#   1.2e-16 m in any figure, contact_ratio equal.
MEASURED = dict(pen=3.643e-16, gap=6.731e-16, skate=1.818e-15, skate_max=1.818e-15, points=2.665e-15)
BOUND = {k: 10.0 * v for k, v in MEASURED.items()}
COLS = ("pen", "gap", "n_contact", "n_skate", "skate", "skate_max")
FIGS = ("pen_mean", "pen_max", "gap_mean", "contact_ratio", "skate_mean")


def dev(a):
    return torch.as_tensor(np.array(a, order="C"), device="cuda")          # (a copy: the shared cases are read-only)


@pytest.fixture(scope="module")
def ctx(skel):
    from egopose_amd.hip import EgpContext
    c = load_golden("config_subject_03.npz")
    cx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"])
    yield cx
    cx.close()


def _contacts(skel, K):
    """K = 16: the feet's boxes; otherwise K drawn points on drawn bodies."""
    from egopose_amd.plausibility import ContactSet
    if K == 16:
        return ContactSet.feet(skel)
    return ContactSet(*CF.random_contacts(skel, K, seed=300 + K), nbody=len(skel.body_names))


@functools.lru_cache(maxsize=None)
def _case(n, K=16, ground_z=0.0, contact_height=0.02):
    """Items on the humanoid with their oracle points, computed once per shape."""
    from egopose_amd.skeleton import load_skeleton
    sk = load_skeleton()
    cs = _contacts(sk, K)
    return cs, CF.case(sk, cs.body, cs.offset, n, seed=90 + n + K, ground_z=ground_z, contact_height=contact_height)


def _run(cx, cs, qpos, nxt, row, gz=0.0, h=0.02, canaries=3):
    """Launch with `points` (buffers with canary rows behind n) and without -> numpy outputs of the first launch."""
    cx.set_contact_points(cs)
    n, K = len(nxt), cs.K
    q, nx, rw = dev(qpos), dev(nxt), None if row is None else dev(row)
    buf = dict(per_frame=torch.full((n + canaries, 6), -7.0, dtype=torch.float64, device="cuda"),
               points=torch.full((n + canaries, K, 3), -7.0, dtype=torch.float64, device="cuda"))
    cx.contact(q, nx, row=rw, ground_z=gz, contact_height=h, out={k: v[:n] for k, v in buf.items()})
    torch.cuda.synchronize()
    for k, v in buf.items():
        assert (v[n:] == -7.0).all(), "%s: rows behind n were written" % k
    out = {k: v[:n].cpu().numpy() for k, v in buf.items()}
    lean_buf = torch.full((n + canaries, 6), -7.0, dtype=torch.float64, device="cuda")
    lean = cx.contact(q, nx, row=rw, ground_z=gz, contact_height=h, out=dict(per_frame=lean_buf[:n]))
    torch.cuda.synchronize()
    assert set(lean) == {"per_frame"} and (lean_buf[n:] == -7.0).all()
    np.testing.assert_array_equal(lean["per_frame"].cpu().numpy(), out["per_frame"])          # bit for bit
    return out


def _compare(tag, out, want, pts):
    seen = {c: float(np.abs(out["per_frame"][:, i] - want[:, i]).max()) for i, c in enumerate(COLS) if not c.startswith("n_")}
    seen["points"] = float(np.abs(out["points"] - pts).max())
    where = {c: int(np.abs(out["per_frame"][:, i] - want[:, i]).argmax()) for i, c in enumerate(COLS) if not c.startswith("n_")}
    print("CONTACT %s: " % tag + ", ".join("%s %.3e (item %d)" % (k, v, where.get(k, -1)) for k, v in seen.items()))
    assert np.isfinite(out["per_frame"]).all()
    np.testing.assert_array_equal(out["per_frame"][:, 2:4], want[:, 2:4])                     # n_contact, n_skate: exactly
    for k, v in seen.items():
        assert v <= BOUND[k], "%s %s: %.3e above the bound %.3e" % (tag, k, v, BOUND[k])


@pytest.mark.parametrize("with_row", [False, True], ids=["row-null", "row-given"])
@pytest.mark.parametrize("n", [1, 63, 130])
def test_kernel_against_the_yardstick(ctx, n, with_row):
    """One item; a ragged last workgroup (63 = 15 x 4 + 3 waves); more than one workgroup and the four kinds of following row many times
    over. Without `row` item i is row i of a longer array (the moved rows lie behind the items); with it the items come in reverse."""
    cs, c = _case(n)
    row = np.arange(n)[::-1].copy() if with_row else None
    nxt = c["nxt"][row] if with_row else c["nxt"]
    want, pts = CF.yardstick(c["points"], row, nxt)
    _compare("n=%d %s" % (n, "row" if with_row else "no row"), _run(ctx, cs, c["qpos"], nxt, row), want, pts)
    if n >= 8 and not with_row:                  # the regimes and kinds are what they claim
        assert (want[:, 0] > 0).any() and (want[:, 2] == 0).any() and ((want[:, 0] == 0) & (want[:, 2] > 0)).any()      # in, off, on the ground
        assert (want[c["kind"] == 2][:, 3:] == 0).all() and (want[c["kind"] == 3][:, 4:] == 0).all()
        assert (want[c["kind"] == 3][:, 3] == want[c["kind"] == 3][:, 2]).all()
        assert want[c["kind"] == 0][:, 4].max() > 1e-3 and want[c["kind"] == 1][:, 5].max() > 0.1


@pytest.mark.parametrize("K, gz, h", [(1, 0.0, 0.02), (32, 0.37, 0.035)])
def test_point_counts_and_the_parameters(ctx, K, gz, h):
    """One point (every reduction sees a single live lane) and 32 (half the wave), the ground and the contact height elsewhere."""
    cs, c = _case(63, K, gz, h)
    want, pts = CF.yardstick(c["points"], None, c["nxt"], gz, h)
    _compare("K=%d" % K, _run(ctx, cs, c["qpos"], c["nxt"], None, gz, h), want, pts)
    assert (want[:, 2] > 0).any() and (want[:, 2] == 0).any() and (want[:, 3] > 0).any()


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
    """Contact points on the leaf bodies of every tree: star4 has 5 bodies and full64 has 64 dofs, the ends of the LDS budget."""
    from egopose_amd.plausibility import ContactSet
    sk, cx = F.skeleton(name), contexts(name)
    cs = ContactSet(*CF.random_contacts(sk, 12, seed=F.SEEDS[name] + 5, bodies=CF.leaves(sk)), nbody=len(sk.body_names))
    c = CF.case(sk, cs.body, cs.offset, 9, seed=F.SEEDS[name] + 6, gen=lambda s, n, rng: F.rand_state(s, rng, n)[0])
    want, pts = CF.yardstick(c["points"], None, c["nxt"])
    _compare("tree=%s" % name, _run(cx, cs, c["qpos"], c["nxt"], None), want, pts)


def test_compute_plausibility_on_the_kernel_matches_the_host_loop(ctx, skel):
    from egopose_amd import plausibility as P
    res = CF.two_takes(skel)
    a = P.compute_plausibility(res, skel, backend="hip", ctx=ctx, contact_height=0.03)
    b = P.compute_plausibility(res, skel, backend="host", contact_height=0.03)
    win = lambda d: {"a": np.stack([d["a"][s:s + 9] for s in (0, 2, 5)]), "b": d["b"][None]}
    wins = {"traj_pred": win(res["traj_pred"]), "traj_orig": win(res["traj_orig"])}
    c = P.compute_forecast_plausibility(wins, skel, 3, 5, backend="hip", ctx=ctx, contact_height=0.03)
    d = P.compute_forecast_plausibility(wins, skel, 3, 5, backend="host", contact_height=0.03)
    bound = dict(pen_mean=BOUND["pen"], pen_max=BOUND["pen"], gap_mean=BOUND["gap"], contact_ratio=0.0, skate_mean=BOUND["skate"])
    for tag, x, y in (("takes", a, b), ("windows", c, d)):
        assert x["contact_height"] == 0.03 and x["ground_z"] == 0.0
        for key in ("traj_pred", "traj_orig"):
            seen = {k: abs(x[key][k] - y[key][k]) for k in FIGS}
            print("CONTACT plausibility %s %s: " % (tag, key) + ", ".join("%s %.3e" % kv for kv in seen.items()))
            assert 0.0 < x[key]["contact_ratio"] <= 1.0 and x[key]["skate_mean"] > 1e-4 and set(x[key]["per_take"]) == {"a", "b"}
            for k, v in seen.items():
                assert v <= bound[k]
            for g in (0, 1):
                assert np.abs(x[key]["per_group"][g] - y[key]["per_group"][g]).max() <= max(bound.values())


def test_command_line_on_the_kernel(skel, tmp_path, monkeypatch, capsys):
    """`--mode stats --physical` without --host makes its own context from the config and agrees with --host."""
    import yaml
    from egopose_amd import evaluate, metrics, plausibility as P
    monkeypatch.chdir(tmp_path)
    (tmp_path / "datasets" / "meta").mkdir(parents=True)
    with open("datasets/meta/meta_subject_03.yml", "w") as f:
        yaml.safe_dump({"train": ["x"], "test": ["a", "b"]}, f)
    em, sr = CF.two_takes(skel, seed=11), CF.two_takes(skel, seed=12)
    metrics.save_results("results/egomimic/subject_03/results/iter_0003_test.p", em, {"algo": "ego_mimic", "num_reset": 0})
    metrics.save_results("results/statereg/subject_03/results/iter_0100_test.p", sr, {"algo": "state_reg"})
    argv = ["--cfg", "subject_03", "--iter", "3", "--statereg-cfg", "subject_03", "--mode", "stats", "--physical", "--joint-pos"]
    hip = evaluate.main(argv)
    text = capsys.readouterr().out
    host = evaluate.main(argv + ["--host"])
    bound = dict(pen_mean=BOUND["pen"], pen_max=BOUND["pen"], gap_mean=BOUND["gap"], contact_ratio=0.0, skate_mean=BOUND["skate"])
    for algo in ("ego mimic", "state reg"):
        a, b = hip[algo]["physical"], host[algo]["physical"]
        assert P.format_line([a["traj_pred"][k] for k in FIGS], algo) in text and a["traj_pred"]["contact_ratio"] > 0
        for k in FIGS:
            assert abs(a["traj_pred"][k] - b["traj_pred"][k]) <= bound[k]
        assert hip[algo]["joint_pos"]["mpjpe"] > 1e-3            # the two kernels share the context
    assert text.count("mocap - pen:") == 1


def test_argument_errors_launch_nothing(ctx, skel):
    from egopose_amd import _lib as L
    from egopose_amd.hip import EgpContext
    from egopose_amd.plausibility import ContactSet
    nb = len(skel.body_names)
    cs, c = _case(1)
    q = dev(np.repeat(c["qpos"][:1], 3, 0))
    nxt = dev(np.array([1, -1], np.int64))
    ctx.set_contact_points(cs)
    assert torch.isfinite(ctx.contact(q, nxt)["per_frame"]).all()          # (tree and contact set are there: the refusals below are about the arguments)
    pf = torch.full((2, 6), -7.0, dtype=torch.float64, device="cuda")
    bad_nxt = [dev(np.array([3, -1], np.int64)), dev(np.array([0, -2], np.int64)), nxt.int(), nxt.cpu(), nxt[:1]]
    for nx in bad_nxt:
        with pytest.raises(ValueError):
            ctx.contact(q, nx, out=dict(per_frame=pf))
    for kw in (dict(row=dev(np.array([0, 3], np.int64))), dict(row=dev(np.array([-1, 0], np.int64))), dict(row=nxt[:1]), dict(row=nxt.int()),
               dict(contact_height=float("nan")), dict(ground_z=float("inf")), dict(out=dict(per_frame=pf[:1])), dict(out=dict(per_frame=pf.float())),
               dict(out=dict(per_frame=pf, points=torch.zeros(2, cs.K + 1, 3, dtype=torch.float64, device="cuda"))), dict(out=dict(per_frame=pf, p=pf))):
        kw.setdefault("out", dict(per_frame=pf))
        with pytest.raises(ValueError):
            ctx.contact(q, nxt, **kw)
    with pytest.raises(ValueError):
        ctx.contact(q[:1], nxt, out=dict(per_frame=pf))                    # two items, one row, no `row`
    with pytest.raises(ValueError):
        ctx.contact(q[:, :-1].contiguous(), nxt, out=dict(per_frame=pf))
    for body, off in (([nb], np.zeros((1, 3))), ([0] * 33, np.zeros((33, 3))), ([0], np.full((1, 3), np.nan))):
        with pytest.raises(ValueError):
            ctx.set_contact_points(type("CS", (), dict(body=np.array(body, np.int32), offset=off))())
    # the C entries refuse the same on their own (EGP_E_INVALID = -1, EGP_E_STATE = -3), and n = 0 is fine
    p = lambda t: L.C.c_void_p(t.data_ptr())
    null = L.C.c_void_p(0)
    ip, dp = lambda a: a.ctypes.data_as(L.c_int_p), lambda a: a.ctypes.data_as(L.c_dbl_p)
    body33, off33 = np.zeros(33, np.int32), np.zeros((33, 3))
    setp = lambda b, o, K: ctx.lib.egp_set_contact_points(ctx.handle, ip(b), dp(o), K)
    assert setp(body33, off33, 0) == -1 and setp(body33, off33, 33) == -1 and setp(np.array([nb], np.int32), off33, 1) == -1
    assert setp(np.array([-1], np.int32), off33, 1) == -1 and setp(body33, np.full((1, 3), np.inf), 1) == -1
    call = lambda q_=p(q), nx=p(nxt), o=p(pf), n=2, h=0.02: ctx.lib.egp_contact_f64(ctx.handle, q_, nx, null, 0.0, h, o, null, n, L.current_stream())
    assert call(q_=null) == -1 and call(nx=null) == -1 and call(o=null) == -1 and call(n=-1) == -1 and call(h=float("nan")) == -1
    assert call(n=0) == 0
    g = load_golden("config_subject_03.npz")
    fresh = EgpContext(skel, g["jkp"], g["jkd"], g["a_ref"], g["a_scale"], g["torque_lim"], g["b_diffw"])
    try:
        fcall = lambda: fresh.lib.egp_contact_f64(fresh.handle, p(q), p(nxt), null, 0.0, 0.02, p(pf), null, 2, L.current_stream())
        assert fcall() == -3                                               # no dynamics model
        with pytest.raises(RuntimeError):
            fresh.contact(q, nxt, out=dict(per_frame=pf))
        fresh.set_dynamics_model()
        assert fcall() == -3                                               # a model, no contact set
    finally:
        fresh.close()
    torch.cuda.synchronize()
    assert (pf == -7.0).all()
    ctx.contact(q, nxt, out=dict(per_frame=pf))                            # the refused calls left the context's contact set alone
    torch.cuda.synchronize()
    want, _ = CF.yardstick(c["points"][[0, 0, 0]], None, np.array([1, -1]))
    assert (pf != -7.0).all() and np.abs(pf.cpu().numpy() - want).max() <= max(BOUND.values())
