"""The tree-generic kernels -- K8 dynamics (csrc/egp_dynamics_dev.hpp), the stable-PD variants of K1, body quaternions and
observations -- on the synthetic trees of tree_fixture.py against float64 (oracle/dynamics.py, oracle/humanoid.py): general
hinge axes, full inertia tensors, 0- and 2-dof bodies, a 33-dof chain (six pointer-jumping rounds), nv == 64, tilted gravity,
the 6-env workgroup form with a ragged tail, PD variant 2 off the humanoid tree and variant 1 at nv != 58.
test_dynamics_trees.py pins the oracle on the same trees and shows that a model wrong in one table entry misses the bounds
used here (1e-12 max|M|, 1e-9 max(1, max|C|): test_dynamics.py's, written relative) by a factor of 1000 or more.

Every comparison prints `RATIO <tree> <what> <worst error / bound>` before it asserts (pytest -s shows them). Measured on an
MI355X when the file was written, worst over all tests of a tree (no bound had to move; qM's worst, 5.3e-15 max|M|, is
24 eps against the 8 eps by which the oracle's own two float64 formulations differ):

    tree                 xpos      qM        bias      torque (rtol = atol = 1e-8)
    star4                2.2e-4    5.3e-3    8.5e-7    3.3e-5   variant 1
    welded               4.4e-4    4.1e-3    1.0e-6    1.5e-5   variant 1
    chain33              1.0e-3    2.7e-3    8.0e-7    5.2e-4   variant 1
    full64               8.8e-4    3.5e-3    9.7e-7    9.8e-4   variant 1
    other58              1.1e-3    2.0e-3    4.0e-7    1.0e-3   variants 2 and 1
    humanoid-topology    9.1e-4    3.6e-3    1.5e-6    1.0e-3   variant 0
    shipped, tilted g    5.2e-4    7.6e-4    3.9e-7"""
import numpy as np
import pytest
import torch

import tree_fixture as F
from oracle import dynamics as D
from oracle import humanoid as H

pytestmark = pytest.mark.gpu

TREE_NAMES = list(F.TREES)
G = F.TILTED_GRAVITY


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


@pytest.fixture(scope="module")
def contexts():
    """name -> the tree's one context of this module (limits asserted before it exists; gains of the tree's K8 -> K1 case)."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = F.context_for(F.skeleton(name), F.SEEDS[name], gains=F.pd_case(name)["gains"])
        return made[name]

    yield get
    for cx in made.values():
        cx.close()


def _report(tree, what, ratio):
    print("RATIO %s %s %.4g" % (tree, what, ratio))
    return ratio


def _compare(tree, sk, out, q, v, idx, gravity=D.GRAVITY, tag=""):
    """qM, bias and xpos rows `idx` of a K8 result against the oracle; prints the worst error / bound of each, then asserts."""
    qM, bias, xpos = (out[k].cpu().numpy() for k in ("qM", "bias", "xpos"))
    n = q.shape[0]
    assert qM.shape == (n, sk.nM) and bias.shape == (n, sk.nv) and xpos.shape == (n, len(sk.body_names), 3)
    worst = dict(xpos=0.0, qM=0.0, bias=0.0)
    for i in idx:
        Ms, Cs, kin = D.crba_rne_spatial(sk, q[i], v[i], gravity=gravity)
        worst["xpos"] = max(worst["xpos"], float((np.abs(xpos[i] - kin["p"]) / (F.XPOS_TOL * np.maximum(1.0, np.abs(kin["p"])))).max()))
        worst["qM"] = max(worst["qM"], float(np.abs(sk.full_from_sparse(qM[i]) - Ms).max() / F.qM_bound(Ms)))
        worst["bias"] = max(worst["bias"], float(np.abs(bias[i] - Cs).max() / F.bias_bound(Cs)))
    for k, r in worst.items():
        _report(tree, k + tag, r)
    for k, r in worst.items():
        assert np.isfinite(r) and r <= 1.0, "%s %s%s: %.4g x the bound" % (tree, k, tag, r)


# ---------------------------------------------------------------------------------------------- a. every tree, every env
@pytest.mark.parametrize("name", TREE_NAMES)
def test_every_tree_every_env(contexts, name):
    """n = 7: workgroups of 4 + 3 envs; all of them against crba_rne_spatial / fk."""
    sk, cx = F.skeleton(name), contexts(name)
    q, v = F.rand_state(sk, np.random.RandomState(F.SEEDS[name] + 1), 7)
    _compare(name, sk, cx.dynamics(dev(q), dev(v), want_xpos=True), q, v, range(7))


# ---------------------------------------------------------------------------------------------- b. state edges
@pytest.mark.parametrize("name", ["humanoid-topology", "welded"])
def test_state_edges(contexts, name):
    sk, cx = F.skeleton(name), contexts(name)
    rng = np.random.RandomState(F.SEEDS[name] + 2)
    q, v = F.rand_state(sk, rng, 3, quat_norm=(0.3, 3.0))
    assert np.abs(np.linalg.norm(q[:, 3:7], axis=1) - 1.0).min() > 1e-3
    _compare(name, sk, cx.dynamics(dev(q), dev(v), want_xpos=True), q, v, range(3), tag="/unnormalised-quat")
    q, v = F.rand_state(sk, rng, 4, hinge_2pi=True)
    assert np.all(np.abs(q[0, 7:]) == 2 * np.pi)
    _compare(name, sk, cx.dynamics(dev(q), dev(v), want_xpos=True), q, v, range(4), tag="/hinges-2pi")
    q, v = F.rand_state(sk, rng, 2, zero_vel=True)
    out = cx.dynamics(dev(q), dev(v), want_xpos=True)
    _compare(name, sk, out, q, v, range(2), tag="/at-rest")
    weight = -D.GRAVITY * sk.body_mass.sum()               # at rest the root force carries the weight, against g
    np.testing.assert_allclose(out["bias"].cpu().numpy()[:, :3], np.tile(weight, (2, 1)), rtol=0, atol=F.BIAS_TOL * np.abs(weight).max())
    q, v = F.rand_state(sk, rng, 3)
    try:
        cx.set_dynamics_model(gravity=G)
        out = cx.dynamics(dev(q), dev(v), want_xpos=True)
        at_rest = cx.dynamics(dev(q), dev(0 * v))["bias"].cpu().numpy()
    finally:
        cx.set_dynamics_model()
    _compare(name, sk, out, q, v, range(3), gravity=G, tag="/tilted-gravity")
    weight = -np.array(G) * sk.body_mass.sum()
    np.testing.assert_allclose(at_rest[:, :3], np.tile(weight, (3, 1)), rtol=0, atol=F.BIAS_TOL * np.abs(weight).max())
    _compare(name, sk, cx.dynamics(dev(q), dev(v), want_xpos=True), q, v, range(3), tag="/gravity-restored")


def test_shipped_skeleton_under_tilted_gravity(skel):
    from conftest import load_golden
    from egopose_amd.hip import EgpContext
    c = load_golden("config_subject_03.npz")
    F.check_limits(skel)
    cx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"])
    try:
        q, v = F.rand_state(skel, np.random.RandomState(41), 3)
        cx.set_dynamics_model(gravity=G)
        _compare("shipped", skel, cx.dynamics(dev(q), dev(v), want_xpos=True), q, v, range(3), gravity=G, tag="/tilted-gravity")
    finally:
        cx.close()


# ---------------------------------------------------------------------------------------------- c. the 6-env workgroup form
def test_wide_form_on_full64(contexts):
    """n = 4101 = 683 * 6 + 3 launches the 6-envs-per-workgroup kernel at the largest per-env LDS block (nv == 64): the first
    workgroup, the last two (the ragged one has 3 envs) and 9 envs in between against the oracle, and every row bit-identical
    to the 4-env form's."""
    name = "full64"
    sk, cx = F.skeleton(name), contexts(name)
    n = 4101
    assert n >= 4096 and n % 6 == 3 and F.check_limits(sk)["env_doubles"] * 8 * 6 <= 100 * 1024
    q, v = F.rand_state(sk, np.random.RandomState(F.SEEDS[name] + 3), n)
    qd, vd = dev(q), dev(v)
    big = cx.dynamics(qd, vd, want_xpos=True)
    idx = list(range(6)) + [int(i) for i in np.linspace(6, n - 10, 9)] + list(range(n - 9, n))
    assert len(set(idx)) == 24
    _compare(name, sk, big, q, v, idx, tag="/wide")
    parts = [cx.dynamics(qd[a:b], vd[a:b], want_xpos=True) for a, b in ((0, 2050), (2050, n))]
    for key in ("qM", "bias", "xpos"):
        assert torch.equal(big[key], torch.cat([p[key] for p in parts])), key


# ---------------------------------------------------------------------------------------------- d. outputs
def test_outputs_on_chain33(contexts):
    name = "chain33"
    sk, cx = F.skeleton(name), contexts(name)
    n = 5
    q, v = F.rand_state(sk, np.random.RandomState(F.SEEDS[name] + 4), n)
    qd, vd = dev(q), dev(v)
    full = cx.dynamics(qd, vd, want_xpos=True)
    _compare(name, sk, full, q, v, range(n), tag="/outputs")
    rows = torch.full((n, sk.nM + 10), float("nan"), dtype=torch.float64, device="cuda")
    only = cx.dynamics(qd, vd, want_bias=False, want_xpos=True, qM_out=rows)
    assert "bias" not in only and only["qM"] is rows
    assert torch.equal(rows[:, :sk.nM], full["qM"]) and bool(torch.isnan(rows[:, sk.nM:]).all())
    assert torch.equal(only["xpos"], full["xpos"])
    no_qM = cx.dynamics(qd, vd, want_qM=False, want_xpos=True)
    assert "qM" not in no_qM and torch.equal(no_qM["bias"], full["bias"]) and torch.equal(no_qM["xpos"], full["xpos"])
    no_bias = cx.dynamics(qd, vd, want_bias=False)
    assert set(no_bias) == {"qM"} and torch.equal(no_bias["qM"], full["qM"])
    empty = cx.dynamics(qd[:0], vd[:0], want_xpos=True)
    assert empty["qM"].shape == (0, sk.nM) and empty["bias"].shape == (0, sk.nv) and empty["xpos"].shape == (0, len(sk.body_names), 3)


# ---------------------------------------------------------------------------------------------- e. K8 -> K1
PD_VARIANT = {"humanoid-topology": 0, "other58": 2}        # every other tree: the generic kernel, 1


def _pd_against_oracle(name, cx, tag):
    """Torques from the device's (qM, bias) against the oracle's stable PD on the oracle's M, C: rtol 1e-8, atol 1e-8 (the
    tolerance of test_dynamics_feeds_stable_pd), clipped and unclipped -- the unclipped ones because gains this high clip a lot."""
    sk, c = F.skeleton(name), F.pd_case(name)
    g = c["gains"]
    assert c["cond"] <= c["cond_limit"]
    qd, vd = dev(c["q"]), dev(c["v"])
    dyn = cx.dynamics(qd, vd)
    tq, raw = (t.cpu().numpy() for t in cx.pd_torque(qd, vd, dev(c["a"]), dyn["qM"], dyn["bias"], want_raw=True))
    worst = 0.0
    for i in range(F.PD_N):
        tau, ref = H.pd_torque(c["q"][i], c["v"][i], c["a"][i], c["M"][i], c["C"][i], g["jkp"], g["jkd"], g["a_ref"], g["a_scale"],
                               g["torque_lim"], sk.timestep)
        for got, want in ((tq[i], ref[0]), (raw[i], tau[0])):
            worst = max(worst, float((np.abs(got - want) / (1e-8 + 1e-8 * np.abs(want))).max()))
    _report(name, "torque" + tag, worst)
    free = float(np.mean(np.abs(raw) < g["torque_lim"]))
    print("INFO %s gain scale %g, cond %.0f (humanoid %.0f), %.0f %% of the torques unclipped" % (name, c["scale"], c["cond"], c["cond_limit"], 100 * free))
    assert np.isfinite(worst) and worst <= 1.0, "%s torque%s: %.4g x the tolerance" % (name, tag, worst)


@pytest.mark.parametrize("name", TREE_NAMES)
def test_dynamics_feeds_stable_pd_on_tree(contexts, name):
    sk, cx = F.skeleton(name), contexts(name)
    want = PD_VARIANT.get(name, 1)
    assert cx.pd_variant == want, "%s: stable-PD variant %d, expected %d" % (name, cx.pd_variant, want)
    _pd_against_oracle(name, cx, "/variant%d" % want)
    if name == "other58":
        for bad in (0, 3):
            with pytest.raises(ValueError, match="humanoid_1205_v1 dof tree"):
                cx.set_pd_variant(bad)
        try:
            cx.set_pd_variant(1)
            assert cx.pd_variant == 1
            _pd_against_oracle(name, cx, "/variant1")
        finally:
            cx.set_pd_variant(2)
    elif name != "humanoid-topology":
        assert sk.nv != 58
        with pytest.raises(ValueError, match="nv == 58"):
            cx.set_pd_variant(2)
    assert cx.pd_variant == want


# ---------------------------------------------------------------------------------------------- f. body quaternions, observations
@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("name", ["welded", "other58"])
def test_body_quat_and_obs(contexts, name, n):
    sk, cx = F.skeleton(name), contexts(name)
    assert {0, 1, 2, 3} >= set(sk.body_ndof[1:].tolist()) >= {2, 3}
    q, v = F.rand_state(sk, np.random.RandomState(F.SEEDS[name] + 5 + n), n)
    bq = cx.body_quat(dev(q)).cpu().numpy()
    np.testing.assert_allclose(bq, H.body_quat(q, sk.body_qpos_start, sk.body_ndof), rtol=0, atol=1e-12)
    welded = np.where(sk.body_ndof == 0)[0]
    assert np.all(bq.reshape(n, -1, 4)[:, welded] == [1.0, 0.0, 0.0, 0.0])
    np.testing.assert_allclose(cx.obs(dev(q), dev(v)).cpu().numpy(), H.full_obs(q, v), rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------- trees the library refuses
def _raw_context(sk):
    from egopose_amd.hip import EgpContext
    g = F.gains_for(sk, 0)
    return EgpContext(sk, g["jkp"], g["jkd"], g["a_ref"], g["a_scale"], g["torque_lim"], g["b_diffw"])


@pytest.mark.parametrize("why,parent,ndof", [
    (r"nbody must be in \[2, 21\]", [-1] + list(range(21)), [6] + [1] * 21),
    (r"nM must be in \(0, 960\]", [-1] + list(range(20)), [6] + [3] * 19 + [1]),
    (r"nv must be in \(6, 64\]", F.tree_of("full64")[0], [6] + [3] * 19 + [2]),
], ids=["22-bodies", "nM-2080", "nv-65"])
def test_create_refuses_trees_outside_the_limits(why, parent, ndof):
    sk = F.synthetic_skeleton(parent, ndof, 0)
    with pytest.raises(AssertionError):
        F.check_limits(sk)
    with pytest.raises(ValueError, match=why):
        _raw_context(sk)


@pytest.mark.parametrize("why,parent,ndof", [
    ("more than 4 children", [-1, 0, 0, 0, 0, 0], [6, 1, 1, 1, 1, 1]),
    ("depth-first order", [-1, 0, 0, 1, 2], [6, 1, 1, 1, 1]),
], ids=["five-children", "not-depth-first"])
def test_dynamics_model_refuses_trees_outside_the_limits(why, parent, ndof):
    sk = F.synthetic_skeleton(parent, ndof, 0)
    with pytest.raises(AssertionError):
        F.check_limits(sk)
    cx = _raw_context(sk)                                  # the model itself is within egp_create's limits
    try:
        with pytest.raises(ValueError, match=why):
            cx.set_dynamics_model()
        q, v = F.rand_state(sk, np.random.RandomState(0), 2)
        with pytest.raises(ValueError, match=why):
            cx.dynamics(dev(q), dev(v))                    # ... and no launch follows the refusal
    finally:
        cx.close()
