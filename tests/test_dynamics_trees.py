"""The oracle of the tree kernels (oracle/dynamics.py) on the synthetic trees of tree_fixture.py, on the CPU: pinned to first
principles where the shipped skeleton cannot expose a mistake (general hinge axes, full inertias, welded bodies, tilted
gravity, unnormalised root quaternions), and shown to tell a slightly wrong model from the right one by a wide margin over the
bounds test_dynamics_reference_gpu.py holds the HIP kernels to."""
import numpy as np
import pytest

import tree_fixture as F
from oracle import dynamics as D

TREE_NAMES = list(F.TREES)
G = np.array(F.TILTED_GRAVITY)


def _states(name, n=2):
    """The first rows of the GPU comparison's own states (test_every_tree_every_env draws them the same way)."""
    sk = F.skeleton(name)
    q, v = F.rand_state(sk, np.random.RandomState(F.SEEDS[name] + 1), 7)
    return sk, q[:n], v[:n]


@pytest.mark.parametrize("name", TREE_NAMES)
def test_tree_sizes_and_limits(name):
    sk = F.skeleton(name)                                  # asserts nb / nv / nM / longest chain against the table
    s = F.check_limits(sk)
    assert s["env_doubles"] == {"full64": 1464}.get(name, s["env_doubles"])
    assert list(sk.body_names[:5]) == list(F.EE_NAMES) and sk.armature == 0.02 and sk.timestep == 1.0 / 450.0
    # qpos addresses count welded bodies correctly: a body's hinges sit at 7 + the hinges of all bodies before it
    before = np.r_[0, np.cumsum(sk.body_ndof[1:])[:-1]]
    assert np.array_equal(sk.body_qpos_start[1:], 7 + before) and sk.body_qpos_start[0] == 0
    assert np.array_equal(sk.joint_body, np.repeat(np.arange(1, s["nb"]), sk.body_ndof[1:]))
    np.testing.assert_allclose(np.linalg.norm(sk.joint_axis, axis=1), 1.0, atol=1e-15)
    assert np.abs(sk.body_inertia[:, [0, 0, 1], [1, 2, 2]]).min() > 1e-6, "full inertia tensors"
    assert np.abs(sk.joint_axis).min() > 1e-4, "general hinge axes"
    assert np.linalg.eigvalsh(sk.body_inertia).min() > 0


def test_the_table_reaches_what_it_claims():
    nd = {n: set(int(x) for x in F.skeleton(n).body_ndof[1:]) for n in TREE_NAMES}
    assert nd["welded"] == {0, 1, 2, 3} and 2 in nd["other58"] and 2 in nd["full64"] and 0 in nd["chain33"]
    w = F.skeleton("welded")
    assert w.body_ndof[1] == 0 and w.body_parent[1] == 0            # 0-dof first child of the root
    assert w.body_ndof[3] == 0 and w.body_ndof[6] == 0              # mid-chain (sibling subtree follows) and leaf
    assert max(np.bincount(F.skeleton("star4").body_parent[1:])) == 4
    assert len(F.skeleton("star4").joint_names) < len(F.skeleton("star4").body_names)
    assert F.skeleton("full64").nv == 64 and F.skeleton("other58").nv == 58
    assert F.check_limits(F.skeleton("chain33"))["scan_rounds"] == 6
    from egopose_amd.skeleton import load_skeleton
    assert not np.array_equal(F.skeleton("other58").dof_parentid, load_skeleton().dof_parentid)
    assert np.array_equal(F.skeleton("humanoid-topology").dof_parentid, load_skeleton().dof_parentid)


def test_limits_refuse_out_of_range_trees():
    """What the library must refuse fails here as a Python assertion, before any launch."""
    bad = {
        "nbody must be": ([-1] + list(range(21)), [6] + [1] * 21),
        "4 children": ([-1, 0, 0, 0, 0, 0], [6, 1, 1, 1, 1, 1]),
        "nM must be": ([-1] + list(range(20)), [6] + [3] * 19 + [1]),
        "nv must be": (F.tree_of("full64")[0], [6] + [3] * 19 + [2]),
        "depth first": ([-1, 0, 0, 1, 2], [6, 1, 1, 1, 1]),
    }
    for why, (parent, ndof) in bad.items():
        sk = F.synthetic_skeleton(parent, ndof, 0)
        with pytest.raises(AssertionError, match=why):
            F.check_limits(sk)


@pytest.mark.parametrize("name", TREE_NAMES)
def test_oracle_first_principles_on_tree(name):
    """Tolerances of test_dynamics.py::test_oracle_dynamics_first_principles, on every tree, under a tilted gravity."""
    sk = F.skeleton(name)
    rng = np.random.RandomState(F.SEEDS[name] + 7)
    q, v = F.rand_state(sk, rng, 2, quat_norm=(0.3, 3.0))
    rows, cols = sk.sparse_index()
    mask = np.zeros((sk.nv, sk.nv), bool)
    mask[rows, cols] = mask[cols, rows] = True
    for i in range(2):
        np.testing.assert_allclose(D.fk(sk, q[i])[1], sk.body_xpos(q[i]), atol=1e-12)
        M = D.inertia_matrix(sk, q[i])
        assert np.linalg.eigvalsh(M).min() > 0 and np.abs(M - M.T).max() == 0
        ke = 0.5 * v[i] @ M @ v[i] - 0.5 * sk.armature * (v[i, 6:] @ v[i, 6:])
        assert ke == pytest.approx(D.kinetic_energy_fd(sk, q[i], v[i]), rel=1e-7)
        assert mask.all() or np.abs(M[~mask]).max() < 1e-12
        Ms, Cs, _ = D.crba_rne_spatial(sk, q[i], v[i], gravity=G)
        np.testing.assert_allclose(Ms, M, atol=1e-11)
        C = D.bias_force(sk, q[i], v[i], gravity=G)
        np.testing.assert_allclose(Cs, C, rtol=0, atol=2e-5 * max(1.0, np.abs(C).max()))
        assert np.abs(Cs - D.crba_rne_spatial(sk, q[i], v[i])[1]).max() > 1e-3        # the argument is not ignored
    # at rest the bias is pure gravity: the root force carries the weight, against g
    weight = -G * sk.body_mass.sum()
    np.testing.assert_allclose(D.bias_force(sk, q[0], np.zeros(sk.nv), gravity=G)[:3], weight, atol=1e-5)
    np.testing.assert_allclose(D.crba_rne_spatial(sk, q[0], np.zeros(sk.nv), gravity=G)[1][:3], weight, rtol=0, atol=1e-9 * np.abs(weight).max())


def _mutants(name, sk):
    last = len(sk.body_names) - 1
    I = sk.body_inertia.copy()
    I[last, 0, 2], I[last, 1, 2] = sk.body_inertia[last, 1, 2], sk.body_inertia[last, 0, 2]
    I[last, 2, 0], I[last, 2, 1] = I[last, 0, 2], I[last, 1, 2]
    anc = sk.joint_anchor.copy()
    anc[-1, 0] += 1e-3
    com = sk.body_com.copy()
    com[last, 1] += 1e-4
    return {
        "xz / yz inertia swapped on the last body": (F.mutate(sk, body_inertia=I), G, "MC"),
        "armature 0": (F.mutate(sk, armature=0.0), G, "M"),
        "last hinge anchor + 1e-3": (F.mutate(sk, joint_anchor=anc), G, "MC"),
        "last body's centre of mass + 1e-4": (F.mutate(sk, body_com=com), G, "MC"),
        "axis-aligned hinges, diagonal inertias": (F.skeleton(name, general=False), G, "MC"),
        "gravity left at -z": (sk, D.GRAVITY, "C"),
    }


@pytest.mark.parametrize("name", TREE_NAMES)
def test_bounds_tell_wrong_models_apart(name):
    """Every mutant of the model moves M or C, on the GPU comparison's own states, by at least 1000 x the bound the kernels are
    held to (1e-12 max|M|, 1e-9 max(1, max|C|)): a kernel that reads one table entry wrongly cannot pass."""
    sk, q, v = _states(name)
    for i in range(len(q)):
        M, C, _ = D.crba_rne_spatial(sk, q[i], v[i], gravity=G)
        for why, (mut, g, looks_at) in _mutants(name, sk).items():
            Mm, Cm, _ = D.crba_rne_spatial(mut, q[i], v[i], gravity=g)
            rM = np.abs(Mm - M).max() / F.qM_bound(M)
            rC = np.abs(Cm - C).max() / F.bias_bound(C)
            margin = max(rM if "M" in looks_at else 0.0, rC if "C" in looks_at else 0.0)
            assert margin >= 1000.0, "%s, env %d, %s: only %.3g x the bound (M %.3g, C %.3g)" % (name, i, why, margin, rM, rC)


@pytest.mark.parametrize("name", TREE_NAMES)
def test_pd_case_is_conditioned_like_the_humanoid(name):
    c = F.pd_case(name)
    assert c["cond"] <= c["cond_limit"] and c["scale"] in (1.0, 2.0, 4.0, 8.0, 16.0)
    kd = np.r_[np.zeros(6), c["gains"]["jkd"]]
    assert max(np.linalg.cond(M + np.diag(kd) / 450.0) for M in c["M"]) == pytest.approx(c["cond"])
