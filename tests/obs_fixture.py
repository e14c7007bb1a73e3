"""Shared by the observation tests on the synthetic trees (test_obs_reference_cpu.py on the CPU, test_obs_reference_gpu.py on the
GPU): the cases, references and bounds for K3 (k_obs, k_obs_rows), K4 (k_body_quat) and K3 fused into K6 (ZfSrc with x == nullptr:
k_zf_partial<T, true>, the rows form of k_zf_apply, the filter prologue of the policy step), and numpy models of the ways those
kernels could go wrong, which the CPU file holds against the bounds.

Trees: tree_fixture.TREES. Observation widths (obs_width): star4 9..21, welded 16..35, chain33 37..77, full64 63..129, other58 and
humanoid-topology 57..117. References: oracle/humanoid.py (full_obs, body_quat) on the inputs as the entry point sees them,
oracle/zfilter.py for the running statistics. Bounds: the project's own -- raw observations and body quaternions rtol = atol =
1e-12 (float64) and 3e-6 (float32), from test_observation_variants_on_device; the filter's state and output scan_fixture.ZF_TOL.

The noise column. With root_deheading, column h + 4 is the de-headed root quaternion's z component: zero up to rounding (the
oracle's own max |z| on unit roots is 1.1e-16), with a standard deviation of ~1e-17, so (x - mean) / (std + 1e-8) magnifies
rounding by 1e8. That one column is left out of the relative bounds on S and y and held absolutely instead (NOISE_*); zf_case
asserts that the oracle's |z| stays below 1e-15 and that every other column's standard deviation exceeds 0.1, so a change of the
inputs cannot widen the hole unseen.

Worst excess measured on the MI355X, as multiples of the bound (test_obs_reference_gpu.py prints them per case); no case failed and
no kernel changed:
  body quaternions      float64 0.00025, float32 0.033
  raw observations      k_obs: float64 0.0008, float32 0.12; 32 805 rows (k_obs_rows, and k_obs at 129 columns): 0.0011 / 0.19
  fused state and y     float64 0.0048 (the noise column 0.17 of its absolute bounds: a mean of 1.7e-16), float32 0.0024
  policy prologue       0.00032 (noise column 0.11): filtered rows and state against the oracle; all else there is bit-equality
numpy float32 on the same formula reaches 0.12 of the float32 raw bound (test_obs_reference_cpu.py), so 3e-6 stays as it is.
"""
import collections
import functools

import numpy as np

import scan_fixture as S
import tree_fixture as TF
from oracle import humanoid as H, quat as Q, zfilter as Z

EPISODE_LEN = 120               # cur_t is uniform in [0, 300): the phase column min(cur_t / 120, 1) saturates on 60 % of the rows
T_MAX = 300
RAW_TOL = {"f64": 1e-12, "f32": 3e-6}              # rtol = atol; test_observation_variants_on_device's
NOISE_RAW, NOISE_MEAN, NOISE_S_PER_ROW, NOISE_Y = 1e-15, 1e-15, 1e-30, 1e-7
MIN_SPREAD = 0.1
ZF_CLIP = S.ZF_CLIP

Opt = collections.namedtuple("Opt", "heading keep root vel phase", defaults=(False, False, False, "full", False))
DEFAULT = Opt()


def opt_id(o):
    parts = [k for k in ("heading", "keep", "root") if getattr(o, k)] + (["vel=" + o.vel] if o.vel != "full" else []) + (["phase"] if o.phase else [])
    return "+".join(parts) or "default"


def obs_options(o):
    """`o` as EgpContext's obs_options."""
    return dict(obs_heading=o.heading, root_deheading=not o.keep, obs_coord="root" if o.root else "heading", obs_vel=o.vel, obs_phase=o.phase)


def obs_width(sk, o):
    """egp_filter_dev.hpp's obs_width."""
    return (1 if o.heading else 0) + (sk.nq - 2) + {"full": sk.nv, "root": 6}.get(o.vel, 0) + (1 if o.phase else 0)


def noise_col(o):
    """The de-headed quaternion's z component, or None (`keep`: the root quaternion goes through as it is)."""
    return None if o.keep else (1 if o.heading else 0) + 4


def vel_cols(sk, o):
    """The three columns of the rotated root velocity ([] without a velocity block)."""
    a = (1 if o.heading else 0) + sk.nq - 2
    return [] if o.vel == "no" else [a, a + 1, a + 2]


# the 24 switch combinations of test_observation_variants_on_device, each with and without the phase column
OPT_ALL = [Opt(bool(h), bool(k), bool(r), v, bool(p)) for p in (0, 1) for h in (0, 1) for k in (0, 1) for r in (0, 1) for v in ("full", "root", "no")]
OPT_FEW = [DEFAULT, Opt(heading=True), Opt(heading=True, keep=True, root=True, vel="root"), Opt(vel="no", phase=True)]
OPTS = {"star4": OPT_ALL, "full64": OPT_ALL, "welded": OPT_FEW, "chain33": OPT_FEW, "other58": OPT_FEW, "humanoid-topology": OPT_FEW}
TREE_NAMES = list(TF.TREES)

BQ_ROWS = (1, 63, 130)
OBS_ROWS = (1, 5, 257)
N_ROWS_KERNEL = 32768 + 37           # k_obs_rows from 32 768 rows on: 512 whole workgroups and one of 37 rows
NONUNIT_TAIL = 4096                  # ... the last of them with root quaternions of norm 0.3 .. 3
CHUNK_ROWS = 9000                    # the same rows again through calls that stay with k_obs
H_ONLY, H_PHASE = Opt(heading=True), Opt(heading=True, phase=True)
# (tree, options) -> width: k_obs_rows with its 128-thread row and spec_col table at 9, 11, 19, 75, 127, 128; at 129 the launch
# must stay with k_obs (a row truncated to 128 threads would show in column 128)
ROWS_CASES = [("star4", DEFAULT, 19), ("star4", Opt(vel="no"), 9), ("star4", Opt(heading=True, vel="no", phase=True), 11),
              ("chain33", DEFAULT, 75), ("full64", DEFAULT, 127), ("full64", H_ONLY, 128), ("full64", H_PHASE, 129)]

# K3 + K6. rows -> route (scan_fixture.ZF_ROWS and): 5: the 4-row chunk of ZfSrc::load_rows clamps past n - 1
ZF_ROWS = (1, 5, 64, 1024, 1025, 4100)
ZF_TREES = [("star4", DEFAULT, 19), ("star4", Opt(vel="no"), 9), ("welded", DEFAULT, 33), ("chain33", Opt(heading=True, vel="root", phase=True), 45),
            ("full64", DEFAULT, 127), ("full64", H_ONLY, 128), ("full64", H_PHASE, 129), ("other58", DEFAULT, 115)]
ZF_TWO_LEVEL = (16385, [("full64", H_ONLY, 128), ("full64", H_PHASE, 129)])
ZF_CASES = [(nm, o, n) for nm, o, _ in ZF_TREES for n in ZF_ROWS] + [(nm, o, ZF_TWO_LEVEL[0]) for nm, o, _ in ZF_TWO_LEVEL[1]]
ZF_FROZEN = [("full64", H_PHASE, n) for n in (64, 1025)]
SPLIT_CASES = [(nm, o, n) for nm, o in [("star4", DEFAULT), ("full64", DEFAULT), ("full64", H_ONLY), ("full64", H_PHASE)] for n in (5, 64, 1024)]
ZF32_CASES = [(nm, o, n) for nm, o in [("star4", DEFAULT), ("chain33", DEFAULT), ("full64", H_ONLY), ("full64", H_PHASE)] for n in (64, 4100)]
# (tree, options, context width H, state width): the route of the policy step's filter prologue
POLICY_CASES = [("star4", DEFAULT, 128, 19), ("full64", H_ONLY, 128, 128), ("full64", H_PHASE, 128, 129), ("full64", H_PHASE, 40, 129)]
POLICY_ROWS = (37, 512)


def case_id(c):
    return "-".join(opt_id(x) if isinstance(x, Opt) else str(x) for x in c)


def context(name, o):
    """An EgpContext over the tree with the options `o` (GPU only). The caller closes it."""
    return TF.context_for(TF.skeleton(name), TF.SEEDS[name], obs_options=obs_options(o), episode_len=EPISODE_LEN)


# ---------------------------------------------------------------------------------------------- states
def _rng(name, purpose, n):
    return np.random.RandomState(TF.SEEDS[name] + 2000 + 100000 * purpose + n)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def bq_states(name, n, hinge_2pi=False):
    """qpos [n][nq] for k_body_quat; hinge_2pi: even rows with every hinge at +-2 pi exactly, odd rows uniform in [-2 pi, 2 pi]."""
    q, _ = TF.rand_state(TF.skeleton(name), _rng(name, 1 + hinge_2pi, n), n, hinge_2pi=hinge_2pi)
    return _frozen(q)[0]


@functools.lru_cache(maxsize=8)
def obs_states(name, n, nonunit=0):
    """(qpos, qvel, cur_t int32) for the raw observations: unit root quaternions, the last `nonunit` rows of norm 0.3 .. 3."""
    sk, rng = TF.skeleton(name), _rng(name, 3 + (nonunit > 0), n)
    q, v = TF.rand_state(sk, rng, n - nonunit)
    if nonunit:
        q2, v2 = TF.rand_state(sk, rng, nonunit, quat_norm=(0.3, 3.0))
        q, v = np.concatenate([q, q2]), np.concatenate([v, v2])
    return _frozen(q, v, rng.randint(0, T_MAX, size=n).astype(np.int32))


def as_dtype(arrays, dtype):
    return S.as_dtype(arrays, dtype)


def ref_obs(o, qpos, qvel, cur_t):
    return H.full_obs(qpos, qvel, obs_heading=o.heading, root_deheading=not o.keep, obs_coord="root" if o.root else "heading", obs_vel=o.vel,
                      phase=(cur_t, EPISODE_LEN) if o.phase else None)


def ref_body_quat(name, qpos):
    sk = TF.skeleton(name)
    return H.body_quat(qpos, sk.body_qpos_start, sk.body_ndof)


def raw_excess(got, ref, dtype):
    """By how many times `got` misses rtol = atol = RAW_TOL[dtype] (nan: infinitely)."""
    tol = RAW_TOL[dtype]
    q = np.abs(np.asarray(got, np.float64) - ref) / (tol + tol * np.abs(ref))
    return float(np.where(np.isnan(q), np.inf, q).max()) if q.size else 0.0


# ---------------------------------------------------------------------------------------------- K3 + K6
def zf_state(rs):
    return S.zf_state(rs)


def zf_from_rows(X0, X, act, clip=ZF_CLIP):
    """-> (state after 300 earlier rows X0, state after merging X[act == 1] into it, y) by the oracle."""
    rs = Z.RunningStatOracle(X.shape[1])
    rs.merge_block(X0)
    s0 = zf_state(rs)
    rs.merge_block(X[act == 1])
    return s0, zf_state(rs), Z.zfilter_apply(X, rs.mean, rs.std, clip), rs.std.copy()


@functools.lru_cache(maxsize=6)
def zf_case(name, o, n, dtype="f64", frozen=False, clip=ZF_CLIP):
    """One fused K3 + K6 call: n states with unit root quaternions, cur_t, an 80 % active mask with row 0 active (frozen: nothing
    active -- the statistics stay as they are), and the running state the call starts from, that of 300 earlier rows.
    -> dict(qpos, qvel, t, act, X0, X: the oracle's observations, s0, s1, y, noise: the column held absolutely)."""
    sk = TF.skeleton(name)
    rng = _rng(name, 5, n)
    q0, v0 = TF.rand_state(sk, rng, 300)
    t0 = rng.randint(0, T_MAX, size=300).astype(np.int32)
    q, v = TF.rand_state(sk, rng, n)
    v[5::101] *= 6.0              # a few rows far out: the clip must have something to do (as scan_fixture.zf_inputs)
    t = rng.randint(0, T_MAX, size=n).astype(np.int32)
    act = (rng.uniform(size=n) < 0.8).astype(np.int32)
    act[0] = 1
    if frozen:
        act[:] = 0
    q, v = as_dtype((q, v), dtype)
    X0, X = ref_obs(o, q0, v0, t0), ref_obs(o, q, v, t)
    s0, s1, y, std = zf_from_rows(X0, X, act, clip)
    nz = noise_col(o)
    rest = np.array([c for c in range(X.shape[1]) if c != nz])
    # the two conditions the bounds rest on (module docstring)
    if nz is not None and dtype == "f64":
        assert max(np.abs(X0[:, nz]).max(), np.abs(X[:, nz]).max()) < NOISE_RAW, (name, o, n)
    assert std[rest].min() > MIN_SPREAD, (name, o, n, std[rest].min())
    out = dict(qpos=q, qvel=v, t=t, act=act, X0=X0, X=X, s0=s0, s1=s1, y=y, noise=nz, rest=rest, std=std, clip=clip)
    _frozen(*[a for a in out.values() if isinstance(a, np.ndarray)])
    return out


def zf_obs_parts(state, y, case, ytol=S.ZF_TOL["y"], dtype="f64", s1=None, y_ref=None):
    """-> (by how many times count, mean, S and y miss scan_fixture.ZF_TOL on every column but the noise column, by how many times
    the noise column misses its absolute bounds -- float64; float32: 0 for finite values, else infinite). `s1`, `y_ref`: another
    reference than the case's."""
    s1 = case["s1"] if s1 is None else s1
    y_ref = case["y"] if y_ref is None else y_ref
    dim, rest, nz = y_ref.shape[1], case["rest"], case["noise"]
    sub = lambda st: np.r_[st[0], st[1:1 + dim][rest], st[1 + dim:][rest]]
    y = np.asarray(y, np.float64)
    main = S.zf_excess(sub(state), y[:, rest], sub(s1), y_ref[:, rest], ytol=ytol)
    noise = 0.0
    if nz is not None:
        m, SS = state[1 + nz], state[1 + dim + nz]
        if dtype == "f64":
            noise = max(abs(m) / NOISE_MEAN, SS / (NOISE_S_PER_ROW * max(state[0], 1.0)), 0.0 if SS >= 0 else np.inf, np.abs(y[:, nz]).max() / NOISE_Y)
        else:
            noise = 0.0 if np.isfinite(y[:, nz]).all() and np.isfinite(m) and np.isfinite(SS) else np.inf
        noise = np.inf if np.isnan(noise) else float(noise)
    return main, noise


def zf_obs_excess(*a, **kw):
    """The worse of zf_obs_parts' two."""
    return max(zf_obs_parts(*a, **kw))


def stats_of(Xm, case, rows=None):
    """(state, y) the oracle makes of the observations Xm in place of the case's own (`rows`: of these rows only)."""
    act = case["act"].copy()
    if rows is not None:
        keep = np.zeros_like(act)
        keep[rows] = 1
        act = act * keep
    _, s1, y, _ = zf_from_rows(case["X0"], Xm, act, case["clip"])
    return s1, y


# ---------------------------------------------------------------------------------------------- wrong kernels, in numpy
CHUNK = 4                        # rows of one ZfSrc::load_rows / finish_rows


def mut_vel_with_next_rows_quat(name, o, case):
    """finish_rows reads the rotated velocity of row r from lane R + r + 1: the next row's, inside a 4-row chunk."""
    sk, X = TF.skeleton(name), case["X"].copy()
    n = len(X)
    r = np.arange(n)
    other = np.where((r % CHUNK != CHUNK - 1) & (r + 1 < n), r + 1, r)
    X[:, vel_cols(sk, o)] = Q.transform_vec(case["qvel"][:, :3], case["qpos"][other, 3:7], "root" if o.root else "heading")
    return X


def mut_deheaded_to_wrong_row(name, o, case):
    """The de-headed quaternion of lane r handed to row r ^ 1 of the chunk."""
    X = case["X"].copy()
    n, h = len(X), 1 if o.heading else 0
    other = np.minimum(np.arange(n) ^ 1, n - 1)
    X[:, h + 1:h + 5] = case["X"][other, h + 1:h + 5]
    return X


def mut_column_left_out(case, c=128):
    """Column c never reaches the statistics: its mean and S stay at the starting state's."""
    dim = case["X"].shape[1]
    st = case["s1"].copy()
    st[1 + c], st[1 + dim + c] = case["s0"][1 + c], case["s0"][1 + dim + c]
    cnt, mean, SS = st[0], st[1:1 + dim], st[1 + dim:]
    return st, Z.zfilter_apply(case["X"], mean, np.sqrt(SS / (cnt - 1)), case["clip"])


def mut_strides_of_the_humanoid(name, o, qpos, qvel, cur_t):
    """Rows addressed with strides 59 / 58 in place of nq / nv (reads past the end wrap round: the model needs values, not faults)."""
    n = len(qpos)
    fq, fv = qpos.ravel(), qvel.ravel()
    iq = (np.arange(n)[:, None] * 59 + np.arange(qpos.shape[1])) % fq.size
    iv = (np.arange(n)[:, None] * 58 + np.arange(qvel.shape[1])) % fv.size
    return ref_obs(o, fq[iq], fv[iv], cur_t)


def mut_phase_of_the_chunks_first_row(X):
    X = X.copy()
    X[:, -1] = X[CHUNK * (np.arange(len(X)) // CHUNK), -1]
    return X


def mut_body_quat(name, qpos, how):
    """how = "slot2": a 2-dof body's second angle in Euler slot 2 | "welded": a 0-dof body takes the preceding body's angles (after
    the root: the root quaternion's x, y, z)."""
    sk = TF.skeleton(name)
    qpos = np.asarray(qpos, float)
    nb = len(sk.body_ndof)
    e = np.zeros((len(qpos), nb, 3))
    for b in range(1, nb):
        s, k = int(sk.body_qpos_start[b]), int(sk.body_ndof[b])
        e[:, b, :k] = qpos[:, s:s + k]
        if how == "slot2" and k == 2:
            e[:, b, 1], e[:, b, 2] = 0.0, qpos[:, s + 1]
        if how == "welded" and k == 0:
            e[:, b] = e[:, b - 1] if b > 1 else qpos[:, 4:7]
    out = np.empty((len(qpos), nb, 4))
    out[:, 0] = qpos[:, 3:7]
    out[:, 1:] = Q.q_from_euler_sxyz(e[:, 1:, 0], e[:, 1:, 1], e[:, 1:, 2])
    return out.reshape(len(qpos), nb * 4)


# ---------------------------------------------------------------------------------------------- float32, the formula itself
def obs_in_float32(o, qpos, qvel, cur_t):
    """get_full_obs evaluated in numpy float32, operation by operation as oracle/quat.py writes it (heading: 2 atan2(z, w), as
    the float32 kernel's: acos loses its digits near w = 1 in float32): what float32 arithmetic makes of the formula."""
    f = np.float32
    q, v = np.asarray(qpos, f), np.asarray(qvel, f)
    w, x, y, z = (q[:, 3 + i] for i in range(4))
    hn = np.sqrt(w * w + z * z)
    hw, hz = w / hn, z / hn

    def rotate_T(qw, qx, qy, qz, u):
        n = qw * qw + qx * qx + qy * qy + qz * qz
        s = f(2) / n
        xx, yy, zz, xy, xz, yz = s * qx * qx, s * qy * qy, s * qz * qz, s * qx * qy, s * qx * qz, s * qy * qz
        wx, wy, wz = s * qw * qx, s * qw * qy, s * qw * qz
        return np.stack([(f(1) - yy - zz) * u[:, 0] + (xy + wz) * u[:, 1] + (xz - wy) * u[:, 2],
                         (xy - wz) * u[:, 0] + (f(1) - xx - zz) * u[:, 1] + (yz + wx) * u[:, 2],
                         (xz + wy) * u[:, 0] + (yz - wx) * u[:, 1] + (f(1) - xx - yy) * u[:, 2]], axis=1)

    zero = np.zeros_like(w)
    lin = rotate_T(w, x, y, z, v[:, :3]) if o.root else rotate_T(hw, zero, zero, hz, v[:, :3])
    parts = []
    if o.heading:
        sg = np.where(z < 0, f(-1), f(1))
        parts.append((f(2) * np.arctan2(sg * z, sg * w))[:, None])
    qq = q[:, 2:].copy()
    if not o.keep:
        nn = hw * hw + hz * hz
        iw, iz = hw / nn, -hz / nn
        qq[:, 1:5] = np.stack([iw * w - iz * z, iw * x - iz * y, iw * y + iz * x, iw * z + iz * w], axis=1)
    parts.append(qq)
    if o.vel in ("full", "root"):
        vv = v.copy() if o.vel == "full" else v[:, :6].copy()
        vv[:, :3] = lin
        parts.append(vv)
    if o.phase:
        parts.append(np.minimum(np.asarray(cur_t, f) / f(EPISODE_LEN), f(1))[:, None])
    out = np.concatenate(parts, axis=1)
    assert out.dtype == f
    return out
