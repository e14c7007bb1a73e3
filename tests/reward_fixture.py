"""Shared by test_reward_reference_cpu.py and test_reward_reference_gpu.py: seeded float64 cases for the imitation reward K2
(k_reward_quat_v3) and the pose features K7 (k_pose_features) on the trees of tree_fixture.py -- three expert takes per tree,
per-env rows built as expert frame + a perturbation, special rows at fixed indices, a non-uniform b_diffw -- with the oracle's
results (oracle/reward.py, oracle/humanoid.py, oracle/quat.py), a restatement of K2's tile layout and the bounds of the GPU
comparison. Nothing here touches a device."""
import functools
import math

import numpy as np

import tree_fixture as F
from oracle import humanoid as H
from oracle import quat as Q
from oracle import reward as R

TAKE_LENS = (7, 23, 40)
TAKE_OFF = (0, 7, 30, 70)
N_FRAMES = TAKE_OFF[-1]
BOUNDARY_FRAMES = (0, 6, 7, 29, 30, 69)                      # first and last row of every take
NEG_FRAME = TAKE_OFF[1] + 5                                  # the frame whose expert quaternion of `neg_body` is negated
END_REWARD, EPISODE_LEN, FRAME_SKIP = 0.3, 200, 15           # (episode_len, frame_skip: EgpContext's defaults)
WEIGHT_SETS = {"default": {}, "v1": {"v_ord": 1}, "v1.5-decay": {"v_ord": 1.5, "decay": True},
               "v3": {"v_ord": 3, "k_v": 0.05, "w_v": 0.3}}
ROOT_TREES = ("welded", "humanoid-topology")                 # the trees that also run under obs_coord 'root'
FIVE_PASS_N = 16384 + 77
FIVE_PASS_TREES = ("welded", "chain33", "humanoid-topology")
K7_SIZES = (1, 8, 9, 65)                                     # a K7 workgroup holds eight envs
K7_KEYS = dict(qvel="vel", rlinv_local="vel", rangv="vel", rq_rmh="quat", ee_pos="quat", bquat="quat", bangvel="vel")

ORDINARY, STILL_BODY, STILL_ENV, ROOT_NEG, EXPERT_NEG, HINGE_2PI, INACTIVE = range(7)
KIND_NAMES = ("ordinary", "still-body", "still-env", "root-negated", "expert-negated", "hinge-2pi", "inactive")
SPECIAL_AT = {2: STILL_BODY, 3: STILL_ENV, 4: INACTIVE, 5: ROOT_NEG, 7: EXPERT_NEG, 9: HINGE_2PI, 11: INACTIVE}
ROW_SCALES = (0.0, 0.5, 1.0, 2.0)
ZERO_ROW = 6                 # rows 6, 14, 22, ... are the expert's frame pair exactly (every scale 0)
TERM_TARGET = 0.5            # -log of a term at row scale 1 (so 0.5 / 1 / 2 give terms of 0.88 / 0.61 / 0.14)
STILL_ULP, MOVING_MIN = 4, 1e-6


# ---------------------------------------------------------------------------------------------- K2's tile layout, restated
# csrc/egp_reward.hip: reward_envs_per_wave, reward_tile_envs and launch_reward's threshold between the two instantiations
FIVE_PASS_FROM = 16384


def envs_per_wave(nbody):
    return max(64 // (nbody - 1), 1) if nbody > 1 else 1


def tile_envs(nbody, passes):
    return min(4 * envs_per_wave(nbody) * passes, 16 if passes == 1 else 64)


def k2_sizes(nbody):
    t = tile_envs(nbody, 1)
    return (1, t - 1, t, t + 1, 3 * t + 5)


# ---------------------------------------------------------------------------------------------- model side
def dt_of(sk):
    return sk.timestep * FRAME_SKIP


@functools.lru_cache(maxsize=None)
def gains(tree):
    """tree_fixture's gains with a non-uniform b_diffw: distinct values in [0.3, 2], the smallest on a body that has hinges
    (that body's expert quaternion is the negated one: its half-angle near pi then leaves the pose term off saturation)."""
    sk = F.skeleton(tree)
    g = dict(F.gains_for(sk, F.SEEDS[tree]))
    nb = len(sk.body_names)
    bw = np.random.RandomState(F.SEEDS[tree] + 3000).permutation(np.linspace(0.3, 2.0, nb - 1))
    j = int(np.argmin(bw))
    if sk.body_ndof[j + 1] == 0:
        k = next(b for b in range(1, nb) if sk.body_ndof[b] > 0) - 1
        bw[j], bw[k] = bw[k], bw[j]
    assert len(set(bw.tolist())) == nb - 1 and bw.min() == 0.3 and bw.max() == 2.0
    g["b_diffw"] = bw
    return g


def neg_body(tree):
    return int(np.argmin(gains(tree)["b_diffw"])) + 1


def _hinged(sk):
    return [b for b in range(1, len(sk.body_names)) if sk.body_ndof[b] > 0]


def features(sk, cur, prev, ee_w, expert_convention, obs_coord="heading"):
    """What K7 writes for the frame pair (prev, cur). Expert convention (gen_expert.py): heading frame of the CURRENT root
    quaternion whatever obs_coord says; learner convention (reward_function.py:19-23): obs_coord's frame of the PREVIOUS one."""
    dt = dt_of(sk)
    qvel = H.qvel_fd(prev, cur, dt)
    if expert_convention:
        rl, ee = Q.transform_vec(qvel[:, :3], cur[:, 3:7], "heading"), H.ee_pos(cur, ee_w, "heading")
    else:
        rl, ee = Q.transform_vec(qvel[:, :3], prev[:, 3:7], obs_coord), H.ee_pos(cur, ee_w, obs_coord)
    bq = H.body_quat(cur, sk.body_qpos_start, sk.body_ndof)
    bav = H.angvel_fd(H.body_quat(prev, sk.body_qpos_start, sk.body_ndof), bq, dt)
    return dict(qvel=qvel, rlinv_local=rl, rangv=qvel[:, 3:6].copy(), rq_rmh=Q.de_heading(cur[:, 3:7]), ee_pos=ee, bquat=bq, bangvel=bav)


def _unit(q):
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _walk(sk, rng, length):
    """A random walk of `length` poses: every hinge steps by 0.01 to 0.03 rad and the root turns by 0.03 rad per frame (no
    frame-to-frame rotation comes near the reference's identity threshold), the heading stays well defined."""
    q = np.zeros((length, sk.nq))
    q[0, :3] = rng.normal(size=3) * 0.5 + [0.0, 0.0, 0.9]
    while True:
        q0 = _unit(rng.normal(size=4))
        if q0[0] ** 2 + q0[3] ** 2 >= 0.3:
            break
    q[0, 3:7] = q0
    q[0, 7:] = rng.normal(size=sk.nq - 7) * 0.5
    for f in range(1, length):
        q[f, :3] = q[f - 1, :3] + rng.uniform(-0.03, 0.03, 3)
        q[f, 3:7] = _unit(Q.qmul(Q.quat_from_expmap(_unit(rng.normal(size=3)) * 0.03), q[f - 1, 3:7]))
        q[f, 7:] = q[f - 1, 7:] + rng.choice([-1.0, 1.0], sk.nq - 7) * rng.uniform(0.01, 0.03, sk.nq - 7)
    return q


@functools.lru_cache(maxsize=None)
def takes(tree):
    """The tree's three expert takes, as `upload_experts` wants them (plus the world end-effector positions they were made
    from): the pose features of every frame pair in the expert convention; a take's first frame is paired with itself."""
    sk = F.skeleton(tree)
    rng = np.random.RandomState(F.SEEDS[tree] + 2000)
    out = []
    for length in TAKE_LENS:
        q = _walk(sk, rng, length)
        ee_w = q[:, None, :3] + rng.uniform(-0.6, 0.6, (length, 5, 3))
        take = features(sk, q, np.concatenate([q[:1], q[:-1]]), ee_w, True)
        take.update(qpos=q, ee_wpos=ee_w.reshape(length, 15), head_height_lb=1.2)
        out.append(take)
    b = neg_body(tree)
    out[1]["bquat"][NEG_FRAME - TAKE_OFF[1], 4 * b:4 * b + 4] *= -1.0
    return out


TABLE_KEYS = ("qpos", "qvel", "rlinv_local", "rangv", "rq_rmh", "ee_pos", "bquat", "bangvel")


@functools.lru_cache(maxsize=None)
def table(tree):
    """The three takes as one table [N_FRAMES][...] (frame = take offset + index)."""
    return {k: np.concatenate([t[k] for t in takes(tree)], axis=0) for k in TABLE_KEYS}


def one_take(tree):
    """The same rows as a single take of N_FRAMES frames."""
    t = dict(table(tree))
    t["head_height_lb"] = 1.2
    return t


# ---------------------------------------------------------------------------------------------- cases
def _abs_moment(p):
    """E|z|^p of a standard normal z."""
    return 2.0 ** (p / 2.0) * math.gamma((p + 1.0) / 2.0) / math.sqrt(math.pi)


def noise_scales(sk, bw, ws):
    """Standard deviations of the perturbations at row scale 1, from the weights: each of the five terms then has -log(term) of
    about TERM_TARGET (small-angle estimates: a body's half-angle is half the norm of its hinge offsets). The joint offsets
    scale as 1 / sqrt(sum of b_diffw^2 over the hinges), the velocity offsets with v_ord, k_v and the number of hinges."""
    nd = np.asarray(sk.body_ndof[1:], float)
    p, x = float(ws["v_ord"]), TERM_TARGET
    return dict(joint=math.sqrt(4.0 * x / (ws["k_p"] * float(np.sum(bw ** 2 * nd)))),
                jvel=math.sqrt(x / ws["k_v"]) / (float(nd.sum()) * _abs_moment(p)) ** (1.0 / p),
                ee=math.sqrt(x / (15.0 * ws["k_e"])), z=math.sqrt(x / (2.0 * ws["k_rh"])), rquat=math.sqrt(x / ws["k_rq"]),
                rlin=math.sqrt(x / (6.0 * ws["k_rl"])), rang=math.sqrt(x / (6.0 * ws["k_ra"])))


def _frame_matrix(q, obs_coord):
    return Q.qmat(q if obs_coord == "root" else Q.heading_q(q))


def one_minus_w(sk, cur, prev):
    """1 - w of every frame-to-frame rotation of the rows: [n][nbody], column 0 the root."""
    d = Q.multi_quat_diff(H.body_quat(cur, sk.body_qpos_start, sk.body_ndof), H.body_quat(prev, sk.body_qpos_start, sk.body_ndof))
    return 1.0 - d[:, ::4]


def in_the_gap(g):
    """Rotations that are neither still (1 - w == 0 up to STILL_ULP ulp) nor clear of the reference's 1 - w < 1e-8 branch."""
    return (np.abs(g) > STILL_ULP * np.finfo(float).eps) & ~(g >= MOVING_MIN)


def case(tree, n, seed, weights=None, obs_coord="heading"):
    return _case(tree, int(n), int(seed), tuple(sorted((weights or {}).items())), obs_coord)


@functools.lru_cache(maxsize=None)
def _case(tree, n, seed, weights, obs_coord):
    sk, tb = F.skeleton(tree), table(tree)
    ws, bw, dt = R.resolve_weights(dict(weights)), gains(tree)["b_diffw"], dt_of(sk)
    rng = np.random.RandomState(seed)
    nj, sd = sk.nq - 7, noise_scales(sk, bw, ws)
    kind = np.zeros(n, np.int64)
    for i, k in SPECIAL_AT.items():
        if i < n:
            kind[i] = k
    if n > 32:
        kind[n - 3], kind[n - 2] = INACTIVE, ROOT_NEG            # the last, ragged tile gets an inactive and a wrapped row too
    # frames: the takes' first and last rows first, on ordinary rows, then anything but the frame with the negated quaternion
    free = np.array([f for f in range(N_FRAMES) if f != NEG_FRAME])
    frame = free[rng.randint(0, len(free), n)]
    ordinary = np.where(kind == ORDINARY)[0]
    edge = np.roll(BOUNDARY_FRAMES, seed % len(BOUNDARY_FRAMES))
    frame[ordinary[:len(edge)]] = edge[:len(ordinary)]
    frame[kind == EXPERT_NEG] = NEG_FRAME
    first = np.isin(frame, TAKE_OFF[:-1])
    fprev = np.where(first, frame, frame - 1)
    # per-row, per-term scales (pose, velocity, end effectors, root pose, root velocity); some rows are the expert's exactly
    sc = rng.choice(ROW_SCALES, size=(n, 5))
    sc[ZERO_ROW::8] = 0.0
    sc[kind == EXPERT_NEG] = 0.5             # (so that the pose term of that row stays off saturation next to the half-angle near pi)
    # joints
    a = sc[:, :1] * sd["joint"] * rng.normal(size=(n, nj))
    b = sc[:, 1:2] * sd["jvel"] * dt * rng.normal(size=(n, nj))
    cur, prev = np.zeros((n, sk.nq)), np.zeros((n, sk.nq))
    cur[:, 7:] = tb["qpos"][frame, 7:] + a
    prev[:, 7:] = tb["qpos"][fprev, 7:] + a + b
    # root pose
    cur[:, :3] = tb["qpos"][frame, :3] + np.c_[rng.normal(size=(n, 2)) * 0.1, sc[:, 3] * sd["z"] * rng.normal(size=n)]
    cur[:, 3:7] = _unit(Q.qmul(tb["qpos"][frame, 3:7], Q.quat_from_expmap(sc[:, 3:4] * sd["rquat"] * rng.normal(size=(n, 3)))))
    # root velocity: the previous root pose is the one from which the learner's local velocities are the expert's + noise
    w_loc = tb["rangv"][frame] + sc[:, 4:5] * sd["rang"] * rng.normal(size=(n, 3))
    slow = np.linalg.norm(w_loc, axis=1) * dt < 4e-3           # (the turn is |w_loc| dt: keep it clear of the identity branch)
    w_loc[slow] += [0.3, 0.0, 0.0]
    qrel = Q.quat_from_expmap(Q.quat_mul_vec(cur[:, 3:7], w_loc) * dt)
    prev[:, 3:7] = _unit(Q.qmul(Q.qinv(qrel), cur[:, 3:7]))
    v_loc = tb["rlinv_local"][frame] + sc[:, 4:5] * sd["rlin"] * rng.normal(size=(n, 3))
    prev[:, :3] = cur[:, :3] - np.einsum("nij,nj->ni", _frame_matrix(prev[:, 3:7], obs_coord), v_loc) * dt
    # end effectors: free world positions whose local offsets are the expert's + noise
    loc = tb["ee_pos"][frame].reshape(n, 5, 3) + sc[:, 2, None, None] * sd["ee"] * rng.normal(size=(n, 5, 3))
    ee_w = (cur[:, None, :3] + np.einsum("nij,nkj->nki", _frame_matrix(cur[:, 3:7], obs_coord), loc)).reshape(n, 15)
    # special rows
    hinged = _hinged(sk)
    still_b, jump_b = hinged[-1], hinged[0]
    s0, n0 = int(sk.body_qpos_start[still_b]), int(sk.body_ndof[still_b])
    prev[kind == STILL_BODY, s0:s0 + n0] = cur[kind == STILL_BODY, s0:s0 + n0]
    prev[kind == STILL_ENV] = cur[kind == STILL_ENV]
    j0 = int(sk.body_qpos_start[jump_b])
    prev[kind == HINGE_2PI, j0] = cur[kind == HINGE_2PI, j0] - (2.0 * np.pi - 0.05)
    # no frame-to-frame rotation in the gap between still and clear of the identity branch: move the body's first hinge on
    for _ in range(8):
        gap = in_the_gap(one_minus_w(sk, cur, prev))
        assert not gap[:, 0].any()
        if not gap.any():
            break
        for i, l in zip(*np.where(gap)):
            prev[i, int(sk.body_qpos_start[l])] += 0.01
    assert not in_the_gap(one_minus_w(sk, cur, prev)).any(), "%s n=%d seed=%d: a rotation stayed in the gap" % (tree, n, seed)
    cur[kind == ROOT_NEG, 3:7] *= -1.0
    active = (kind != INACTIVE).astype(np.int32)
    cur_finite = cur.copy()
    cur[active == 0] = np.nan
    other = free[rng.randint(0, len(free), n)]
    frame = np.where(active == 0, np.where(other == frame, free[(np.searchsorted(free, other) + 1) % len(free)], other), frame)
    c = dict(tree=tree, n=n, seed=seed, weights=dict(weights), obs_coord=obs_coord, kind=kind, scale=sc, cur_qpos=cur,
             cur_finite=cur_finite, prev_qpos=prev, ee_wpos=ee_w, t=rng.randint(1, EPISODE_LEN, n).astype(np.int32),
             frame=frame.astype(np.int32), end=(rng.rand(n) < 0.25).astype(np.int32), active=active, b_diffw=bw)
    c["reward"], c["c_info"] = oracle_reward(c)
    c["features"] = {conv: features(sk, cur_finite, prev, ee_w, conv, obs_coord) for conv in (False, True)}
    for v in list(c.values()) + list(c["features"][False].values()) + list(c["features"][True].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ---------------------------------------------------------------------------------------------- the oracle on a case
def r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def oracle_reward(c, rounded=False, **over):
    """(reward [n], c_info [n][5]) of R.quat_v3 on the case's active rows, zeros elsewhere. rounded: inputs and expert rows
    rounded to float32 first (what the float32 kernels are given). `over` replaces items of the case or names the expert
    `table` (the mutants of test_reward_reference_cpu.py)."""
    d = dict(c)
    tb = over.pop("table", None) or table(c["tree"])
    d.update(over)
    sk = F.skeleton(c["tree"])
    rd = r32 if rounded else (lambda x: x)
    on = np.where(d["active"] != 0)[0]
    cur, prev, ee_w = rd(d["cur_qpos"][on]), rd(d["prev_qpos"][on]), rd(d["ee_wpos"][on])
    row = {k: rd(tb[k][d["frame"][on]]) for k in TABLE_KEYS}
    r, ci = R.quat_v3(cur, prev, H.body_quat(prev, sk.body_qpos_start, sk.body_ndof), ee_w, d["t"][on], row, d["weights"], d["b_diffw"],
                      dt_of(sk), EPISODE_LEN, d["end"][on] != 0, END_REWARD, sk.body_qpos_start, sk.body_ndof, d["obs_coord"])
    reward, c_info = np.zeros(c["n"]), np.zeros((c["n"], 5))
    reward[on], c_info[on] = r, ci
    return reward, c_info


def oracle_features(c, expert_convention, rounded=False):
    sk = F.skeleton(c["tree"])
    rd = r32 if rounded else (lambda x: x)
    return features(sk, rd(c["cur_finite"]), rd(c["prev_qpos"]), rd(c["ee_wpos"]), expert_convention, c["obs_coord"])


# ---------------------------------------------------------------------------------------------- bounds of the GPU comparison
# float64: the project's parity gate (as test_hip_parity.py applies it). float32: the same gate at float32's
# figures, or 8 x the shift of the float64 oracle's own output when its inputs are rounded to float32, whichever is larger
# (8: the kernel rounds at every intermediate step -- quaternion, difference, division by dt, square -- where that shift holds
# one rounding). All absolute, but the reward's, which is atol + rtol |reward|.
GATES = {"f64": dict(c_info=5e-10, reward_atol=5e-10, reward_rtol=1e-10, quat=1e-10, vel=5e-9),
         "f32": dict(c_info=5e-5, reward_atol=5e-5, reward_rtol=1e-5, quat=1e-5, vel=5e-4)}
ROUNDING_FACTOR = 8.0


def reward_bounds(c, dt):
    """dt 'f64' / 'f32' -> (want_reward, want_c_info, bound_reward [n], bound_c_info [5])."""
    g = GATES[dt]
    if dt == "f64":
        return c["reward"], c["c_info"], g["reward_atol"] + g["reward_rtol"] * np.abs(c["reward"]), np.full(5, g["c_info"])
    r, ci = oracle_reward(c, rounded=True)
    s_r, s_c = np.abs(r - c["reward"]).max(), np.abs(ci - c["c_info"]).max(axis=0)
    return r, ci, np.maximum(g["reward_atol"] + g["reward_rtol"] * np.abs(r), ROUNDING_FACTOR * s_r), np.maximum(g["c_info"], ROUNDING_FACTOR * s_c)


def feature_bounds(c, expert_convention, dt):
    """-> {key: (want, bound)} for the seven outputs of K7."""
    g, exact = GATES[dt], c["features"][expert_convention]
    if dt == "f64":
        return {k: (exact[k], g[K7_KEYS[k]]) for k in K7_KEYS}
    want = oracle_features(c, expert_convention, rounded=True)
    return {k: (want[k], max(g[K7_KEYS[k]], ROUNDING_FACTOR * float(np.abs(want[k] - exact[k]).max()))) for k in K7_KEYS}


# ---------------------------------------------------------------------------------------------- the GPU module's cases
TREE_COORDS = [(t, "heading") for t in F.TREES] + [(t, "root") for t in ROOT_TREES]
FIVE_PASS_WEIGHTS = ("default", "v1.5-decay")                # v_ord 2 and 1.5


def _seed(tree, k):
    return F.SEEDS[tree] * 1000 + k


def k2_cases(tree, obs_coord):
    """[(weight set's name, case)] of the one-pass comparison: every weight set at every size around the tree's tile."""
    sizes = k2_sizes(len(F.skeleton(tree).body_names))
    return [(wn, case(tree, n, _seed(tree, 10 * wi + si), ws, obs_coord))
            for wi, (wn, ws) in enumerate(WEIGHT_SETS.items()) for si, n in enumerate(sizes)]


def five_pass_cases(tree):
    return [(wn, case(tree, FIVE_PASS_N, _seed(tree, 100 + i), WEIGHT_SETS[wn], "heading")) for i, wn in enumerate(FIVE_PASS_WEIGHTS)]


POSE_DIST_TREE = "welded"                                    # nq = 18


def pose_dist_case():
    return case(POSE_DIST_TREE, 37, _seed(POSE_DIST_TREE, 300), {}, "heading")


def k7_cases(tree, obs_coord):
    return [case(tree, n, _seed(tree, 200 + i), {}, obs_coord) for i, n in enumerate(K7_SIZES)]
