"""Shared by the tree-kernel tests (test_dynamics_trees.py on the CPU, test_dynamics_reference_gpu.py on the GPU): free-root
hinge trees that are generated, not shipped -- general hinge axes, full inertia tensors, arbitrary anchors and centres of
mass, 0-, 1-, 2- and 3-dof bodies -- with their contexts, states, and a restatement of the library's host-side limits.
reward_fixture.py builds the reward and pose-feature cases of test_reward_reference_*.py on the same trees."""
import dataclasses
import functools

import numpy as np

from egopose_amd.skeleton import EE_NAMES, Skeleton, load_skeleton

TILTED_GRAVITY = (1.3, -2.1, -9.4)

_CHAINS4 = [-1] + [p for c in range(4) for p in [0] + list(range(5 * c + 1, 5 * c + 5))]      # root + 4 chains of 5 bodies

# name -> (parents, hinges per body; the root's 6 dofs are implied); None: the shipped skeleton's tree
TREES = {
    "star4": ([-1, 0, 0, 0, 0], [6, 1, 1, 1, 1]),
    "welded": ([-1, 0, 1, 2, 2, 1, 5, 0, 7], [6, 0, 3, 0, 2, 1, 0, 2, 3]),
    "chain33": ([-1] + list(range(9)) + [0, 10, 0, 0], [6] + [3] * 9 + [2, 0, 1, 2]),
    "full64": (_CHAINS4, [6] + [3] * 18 + [2, 2]),
    "other58": (_CHAINS4, [6] + [3] * 12 + [2] * 8),
    "humanoid-topology": None,
}
# name -> (nb, nv, nM, longest dof chain), as Skeleton.finalize() gives them: a change of the generator cannot drop a case unseen
SIZES = {"star4": (5, 10, 49, 7), "welded": (9, 17, 118, 11), "chain33": (14, 38, 598, 33), "full64": (21, 64, 820, 21),
         "other58": (21, 58, 706, None), "humanoid-topology": (21, 58, 910, 28)}
SEEDS = {name: 100 + i for i, name in enumerate(TREES)}


def longest_chain(skel):
    best = 0
    for i in range(skel.nv):
        n, k = 0, i
        while k >= 0:
            n, k = n + 1, int(skel.dof_parentid[k])
        best = max(best, n)
    return best


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def synthetic_skeleton(parent, ndof, seed, general=True):
    """A finalized Skeleton over the tree (parent, ndof) with random inertial parameters. general=False: the same draws, but
    hinge axes snapped to the nearest coordinate axis and the inertias left diagonal (what the shipped skeleton looks like)."""
    parent, ndof = np.asarray(parent, np.int32), np.asarray(ndof, np.int32)
    nb = len(parent)
    assert nb >= len(EE_NAMES) and parent[0] == -1 and ndof[0] == 6
    rng = np.random.RandomState(seed)
    names = list(EE_NAMES) + ["B%d" % i for i in range(nb - len(EE_NAMES))]
    pos, com, mass, inertia = np.zeros((nb, 3)), np.zeros((nb, 3)), np.zeros(nb), np.zeros((nb, 3, 3))
    qstart = np.zeros(nb, np.int32)
    jn, jb, jax, janc = [], [], [], []
    qadr = 7
    for b in range(nb):
        if b > 0:
            assert 0 <= parent[b] < b
            pos[b] = pos[parent[b]] + rng.uniform(-0.3, 0.3, 3)
            qstart[b] = qadr                       # a welded body owns no qpos: its start is where the next hinge goes
            qadr += int(ndof[b])
        com[b] = pos[b] + rng.uniform(-0.1, 0.1, 3)
        mass[b] = rng.uniform(0.5, 8.0)
        R, d = _rotation(rng), rng.uniform(0.002, 0.05, 3)
        inertia[b] = R @ np.diag(d) @ R.T if general else np.diag(d)
        inertia[b] = 0.5 * (inertia[b] + inertia[b].T)
        for k in range(int(ndof[b]) if b > 0 else 0):
            a = rng.normal(size=3)
            a /= np.linalg.norm(a)
            if not general:
                i = int(np.argmax(np.abs(a)))
                a = np.sign(a[i]) * np.eye(3)[i]
            jn.append("J%d_%d" % (b, k))
            jb.append(b)
            jax.append(a)
            janc.append(pos[b] + rng.uniform(-0.05, 0.05, 3))
    nj = len(jn)
    sk = Skeleton(body_names=names, body_parent=parent, body_pos=pos, body_qpos_start=qstart, body_ndof=ndof, joint_names=jn,
                  joint_body=np.array(jb, np.int32), joint_axis=np.array(jax).reshape(nj, 3), joint_anchor=np.array(janc).reshape(nj, 3),
                  joint_range=np.tile([-np.pi, np.pi], (nj, 1)), actuator_names=list(jn), timestep=1.0 / 450.0, armature=0.02,
                  body_mass=mass, body_com=com, body_inertia=inertia).finalize()
    assert qadr == sk.nq
    return sk


def tree_of(name):
    if TREES[name] is None:
        sk = load_skeleton()
        return sk.body_parent.tolist(), sk.body_ndof.tolist()
    return TREES[name]


@functools.lru_cache(maxsize=None)
def skeleton(name, general=True):
    parent, ndof = tree_of(name)
    sk = synthetic_skeleton(parent, ndof, SEEDS[name], general)
    nb, nv, nM, chain = SIZES[name]
    assert (len(sk.body_names), sk.nv, sk.nM) == (nb, nv, nM), (name, len(sk.body_names), sk.nv, sk.nM)
    assert chain is None or longest_chain(sk) == chain, (name, longest_chain(sk))
    return sk


def mutate(sk, **fields):
    """A finalized copy of `sk` with some arrays replaced."""
    return dataclasses.replace(sk, **fields).finalize()


# ---------------------------------------------------------------------------------------------- host-side limits, restated
# include/egopose_hip.h and csrc/egp_dynamics_dev.hpp: what egp_create / egp_set_dynamics_model / the K8 launch accept.
MAX_NV, MAX_NBODY, MAX_NJOINT, MAX_NM, MAX_CHILDREN, MAX_SCAN_ROUNDS = 64, 21, 58, 960, 4, 6
DY_LW, DY_LJ, DY_LS, DY_LI = 13, 7, 7, 11
DYN_TABLE_BYTES = 10 * 1024            # the tree tables K8 stages next to the per-env blocks (9.9 kB), rounded up


def dy_env_doubles(nb, nj, nv):
    r1 = max(nb * DY_LW + nj * DY_LJ, nb * (DY_LI + DY_LS), nv * DY_LS)
    return r1 + nb * DY_LW + nv * DY_LS + nv


def check_limits(sk):
    """AssertionError for a tree the library must refuse, so that it can never become an out-of-range launch; -> sizes."""
    nb, nj, nv = len(sk.body_names), len(sk.joint_names), sk.nv
    assert 6 < nv <= MAX_NV and sk.nq == nv + 1 and sk.nu == nv - 6, "nv must be in (6, 64], one free root + hinges"
    assert 2 <= nb <= MAX_NBODY, "nbody must be in [2, 21]"
    assert nj <= MAX_NJOINT and nj == int(np.sum(sk.body_ndof[1:])), "at most 58 hinges"
    assert 0 < sk.nM <= MAX_NM, "nM must be in (0, 960]"
    par = np.asarray(sk.body_parent)
    assert par[0] == -1 and all(0 <= par[b] < b for b in range(1, nb)), "parents first, body 0 the root"
    assert max(np.bincount(par[1:], minlength=nb)) <= MAX_CHILDREN, "at most 4 children per body"
    for b in range(nb):                            # depth first: a subtree is a contiguous range of bodies
        under = [c for c in range(b + 1, nb) if b in _ancestors(par, c)]
        assert under == list(range(b + 1, b + 1 + len(under))), "bodies must be listed depth first"
    assert all(0 <= int(n) <= 3 for n in sk.body_ndof[1:]), "0 to 3 hinges per body (the body quaternion is one Euler triple)"
    rounds = int(np.ceil(np.log2(max(longest_chain(sk), 1))))
    assert rounds <= MAX_SCAN_ROUNDS, "the ancestor jump table holds 6 rounds"
    ed = dy_env_doubles(nb, nj, nv)
    assert 4 * ed * 8 <= 64 * 1024 and 4 * ed * 8 + DYN_TABLE_BYTES <= 64 * 1024, "K8 LDS, 4 envs per workgroup"
    assert 6 * ed * 8 <= 100 * 1024 and 6 * ed * 8 + DYN_TABLE_BYTES <= 160 * 1024, "K8 LDS, 6 envs per workgroup"
    return dict(nb=nb, nj=nj, nv=nv, nM=sk.nM, env_doubles=ed, scan_rounds=rounds)


def _ancestors(par, c):
    out, a = [], int(par[c])
    while a >= 0:
        out.append(a)
        a = int(par[a])
    return out


# ---------------------------------------------------------------------------------------------- gains, contexts, states
def gains_for(sk, seed, scale=1.0):
    """Gains shaped like the shipped configs'; `scale` multiplies jkp and jkd."""
    rng = np.random.RandomState(seed)
    jkp = rng.uniform(50.0, 500.0, sk.nu)
    return dict(jkp=jkp * scale, jkd=jkp * scale / 10.0, a_ref=rng.normal(size=sk.nu) * 0.1, a_scale=rng.uniform(0.2, 1.0, sk.nu),
                torque_lim=rng.uniform(50.0, 200.0, sk.nu), b_diffw=np.ones(len(sk.body_names) - 1))


def context_for(sk, seed, gains=None, obs_options=None, **kw):
    """An EgpContext over `sk` (limits checked first); the gains it was made with are kept as `.gains`. `obs_options`: as
    EgpContext's (None: the shipped configs' defaults); further keywords (episode_len, ...) go to EgpContext as they are."""
    from egopose_amd.hip import EgpContext
    check_limits(sk)
    g = gains if gains is not None else gains_for(sk, seed)
    cx = EgpContext(sk, g["jkp"], g["jkd"], g["a_ref"], g["a_scale"], g["torque_lim"], g["b_diffw"], obs_options=obs_options, **kw)
    cx.gains = g
    return cx


def rand_state(sk, rng, n, joint_scale=1.5, vel_scale=1.0, quat_norm=None, hinge_2pi=False, zero_vel=False):
    """(qpos [n][nq], qvel [n][nv]). quat_norm=(lo, hi): root quaternions of that norm instead of 1; hinge_2pi: even rows have
    every hinge at +-2 pi exactly, odd rows uniform in [-2 pi, 2 pi]; zero_vel: the system at rest."""
    q = np.zeros((n, sk.nq))
    q[:, :3] = rng.normal(size=(n, 3))
    quat = rng.normal(size=(n, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    if quat_norm is not None:
        quat *= rng.uniform(quat_norm[0], quat_norm[1], size=(n, 1))
    q[:, 3:7] = quat
    q[:, 7:] = rng.normal(size=(n, sk.nq - 7)) * joint_scale
    if hinge_2pi:
        exact = 2 * np.pi * rng.choice([-1.0, 1.0], size=(n, sk.nq - 7))
        q[:, 7:] = np.where(np.arange(n)[:, None] % 2 == 0, exact, rng.uniform(-2 * np.pi, 2 * np.pi, size=(n, sk.nq - 7)))
    v = rng.normal(size=(n, sk.nv)) * vel_scale
    if zero_vel:
        v[:] = 0.0
    return q, v


# ---------------------------------------------------------------------------------------------- bounds of the GPU comparison
XPOS_TOL, QM_TOL, BIAS_TOL = 1e-12, 1e-12, 1e-9


def qM_bound(M):
    return QM_TOL * np.abs(M).max()


def bias_bound(C):
    return BIAS_TOL * max(1.0, np.abs(C).max())


# ---------------------------------------------------------------------------------------------- the K8 -> K1 case of a tree
PD_N = 9


def _pd_states(sk, seed):
    rng = np.random.RandomState(seed)
    q, v = rand_state(sk, rng, PD_N, joint_scale=0.3, vel_scale=0.5)
    return q, v, rng.normal(size=(PD_N, sk.nu)) * 0.2


def _worst_cond(Ms, jkd, dt):
    kd = np.r_[np.zeros(6), jkd]
    return max(np.linalg.cond(M + np.diag(kd) * dt) for M in Ms)


@functools.lru_cache(maxsize=None)
def humanoid_pd_cond():
    """Worst cond(M + Kd dt) of the shipped skeleton with the shipped gains on the states of test_dynamics_feeds_stable_pd:
    the conditioning at which that test's tolerance (rtol 1e-8, atol 1e-8) was set."""
    from conftest import load_golden
    from oracle import dynamics as D
    sk, c = load_skeleton(), load_golden("config_subject_03.npz")
    q, v = rand_state(sk, np.random.RandomState(8), PD_N, joint_scale=0.3, vel_scale=0.5)      # that test's draws, in its order
    return _worst_cond([D.crba_rne_spatial(sk, q[i], v[i])[0] for i in range(PD_N)], c["jkd"], sk.timestep)


@functools.lru_cache(maxsize=None)
def pd_case(name):
    """States, the oracle's (M, C) and gains for the K8 -> K1 comparison on a tree, conditioned no worse than the humanoid's
    system (the existing tolerance was set there). Kd dt sits on the hinge diagonal and lifts the small eigenvalues (light
    distal links, armature 0.02), while the largest (the root block, ~ total mass) does not move: measured, cond(M + Kd dt) FALLS
    as the gains grow -- chain33: 4373 at Kd = 0, 2391 at half gains, 1720 at the drawn gains, 1154 at twice; the humanoid with
    its shipped gains: 1529. So a tree that starts above the humanoid's figure has its gains doubled until it is not."""
    from oracle import dynamics as D
    sk = skeleton(name)
    q, v, a = _pd_states(sk, SEEDS[name] + 1000)
    MC = [D.crba_rne_spatial(sk, q[i], v[i])[:2] for i in range(PD_N)]
    Ms = [m for m, _ in MC]
    limit, scale = humanoid_pd_cond(), 1.0
    while _worst_cond(Ms, gains_for(sk, SEEDS[name], scale)["jkd"], sk.timestep) > limit:
        scale *= 2.0
        assert scale <= 16.0, "%s: cond(M + Kd dt) stays above the humanoid's (%g)" % (name, limit)
    g = gains_for(sk, SEEDS[name], scale)
    return dict(q=q, v=v, a=a, M=np.stack(Ms), C=np.stack([c for _, c in MC]), gains=g, scale=scale,
                cond=_worst_cond(Ms, g["jkd"], sk.timestep), cond_limit=limit)
