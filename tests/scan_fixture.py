"""Shared by the scan/reduction tests (test_scan_reference_cpu.py on the CPU, test_scan_reference_gpu.py on the GPU): the inputs,
references and bounds for K5 (GAE: egp_gae_*) and K6 (the running filter: egp_zfilter_*), and numpy models of the kernels' tile
structure that the CPU file turns into wrong kernels.

K5's one-pass kernel gives a workgroup a tile of TILE = 2 048 samples; the carry entering a tile is the composition of the affine
maps of the tiles to its right, 64 per round, until the product of their slopes is below 2^-200 or the batch ends. Which of those
steps a case reaches depends on gamma * tau and on where the episodes end, so the cases below are chosen by tile arithmetic, not
by size: nothing here needs more than 131 tiles.
"""
import functools
import zlib

import numpy as np

from oracle import zfilter as Z

L = np.longdouble
TILE = 2048                     # samples per workgroup of k_gae_onepass (256 threads x GAE_CHUNK = 4)
ROUND = 64                      # tiles per round of the look to the right
P_STOP = 2.0 ** -200            # the look to the right ends once |P| is below this

# name -> (gamma, tau). gamma * tau = 1: P stays 1, the look runs to the batch's end. 0.9999: 0.9999^2048 = 0.81 per tile, never below
# 2^-200 within 131 tiles. 0.9405: 0.9405^2048 = 2^-181, the stop comes after two tiles. 0.9025: 2^-303, one tile (every shipped config).
GAMMA_TAU = {"1x1": (1.0, 1.0), "0.9999x1": (0.9999, 1.0), "0.99x0.95": (0.99, 0.95), "0.95x0.95": (0.95, 0.95)}

SMALL_SIZES = (4, 5, TILE, TILE + 1, 2 * TILE)
N_ONE_ROUND, N_SECOND_ROUND, N_INTO_SECOND, N_THIRD_ROUND = ROUND * TILE, ROUND * TILE + 1, 66 * TILE + 3, 130 * TILE + 1021
BIG_SIZES = (N_ONE_ROUND, N_SECOND_ROUND, N_INTO_SECOND, N_THIRD_ROUND)
# a single episode end at: a chunk edge, the last sample of a wave's share of the tile and the first of the next wave's, the last
# sample of a tile and the first of the next, the first sample of tile 64 (where the second round of the look starts for tile 0 - 1)
END_POSITIONS = (3, 4, 255, 256, TILE - 1, TILE, ROUND * TILE)


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def gae_masks(n):
    """The mask kinds that exist at size n."""
    return ["open1", "open0"] + ["end@%d" % p for p in END_POSITIONS if p < n] + ["zeros", "episodes"]


# what the GPU file runs beyond the small sizes (each with every gamma * tau and both dtypes): the open batch at every size, m[-1] in
# both states at one whole round and in the third; the single ends that sit at tile edges 66 tiles + 3 samples in (those at chunk
# and wave edges act inside a tile: the two-tile size of SMALL_CASES has them, with a carry coming in); no carry at all; the
# rollout's episodes
BIG_CASES = ([(n, "open1") for n in BIG_SIZES] + [(N_ONE_ROUND, "open0"), (N_THIRD_ROUND, "open0")] +
             [(N_INTO_SECOND, "end@%d" % p) for p in (TILE - 1, TILE, ROUND * TILE)] + [(N_SECOND_ROUND, "zeros")] +
             [(N_INTO_SECOND, "episodes"), (N_THIRD_ROUND, "episodes")])
SMALL_CASES = [(n, mk) for n in SMALL_SIZES for mk in gae_masks(n)]


@functools.lru_cache(maxsize=16)
def gae_inputs(n, mask, salt=0):
    """(rewards, masks, values), float64, read-only: rewards in [0, 1.2], values N(5, 2^2), as the rollout's."""
    rng = np.random.RandomState(_seed("gae", n, mask, salt))
    r = rng.uniform(0.0, 1.2, size=n)
    v = rng.normal(size=n) * 2 + 5
    m = np.ones(n)
    if mask == "open0":
        m[-1] = 0.0
    elif mask.startswith("end@"):
        m[int(mask[4:])] = 0.0
    elif mask == "zeros":
        m[:] = 0.0
    elif mask == "episodes":                      # 30-200-step episodes, the last one cut at the batch's end
        ends = np.cumsum(rng.randint(30, 201, size=n // 30 + 1))
        m[ends[ends < n] - 1] = 0.0
        m[-1] = 0.0
    else:
        assert mask == "open1", mask
    for a in (r, m, v):
        a.setflags(write=False)
    return r, m, v


def as_dtype(arrays, dtype):
    """The inputs as the entry point of `dtype` ("f64" / "f32") sees them, widened back to float64."""
    return tuple(np.asarray(a, np.float32 if dtype == "f32" else np.float64).astype(np.float64) for a in arrays)


def moments(x):
    """{n, mean, M2} of x in long double, two passes."""
    x = np.asarray(x).astype(L)
    mean = x.sum() / L(x.size)
    return np.array([L(x.size), mean, ((x - mean) ** 2).sum()], dtype=L)


def gae_sweep(r, m, v, gamma, tau, dtype=np.longdouble):
    """estimate_advantages as one plain reverse sweep in `dtype`: a_i = delta_i + gamma tau m_i a_{i+1},
    delta_i = r_i + gamma m_i v_{i+1} - v_i, v_N = a_N = 0. gamma and tau are float64 parameters and their product is formed in
    float64, as the reference's own expression does. -> raw advantages, returns (both `dtype`)."""
    T = dtype
    r, m, v = (np.asarray(a, np.float64).astype(T) for a in (r, m, v))
    vn = np.concatenate([v[1:], np.zeros(1, T)])
    d = (r + T(gamma) * vn * m - v).tolist()
    c = (T(float(gamma) * float(tau)) * m).tolist()
    out = [None] * len(d)
    a = T(0)
    for i in range(len(d) - 1, -1, -1):
        a = d[i] + c[i] * a
        out[i] = a
    adv = np.array(out, dtype=T)
    return adv, v + adv


@functools.lru_cache(maxsize=8)               # (a 131-tile reference is 20 MB: the tests of one case share it, no more)
def gae_reference(n, mask, gt, dtype, salt=0):
    """The long-double sweep over case (n, mask) as the entry point of `dtype` sees it: on the float32-rounded inputs for "f32", and
    the statistics those of the advantages as stored (rounded to float32). -> dict(adv, ret, stats, std: the standardised
    advantages), long double."""
    gamma, tau = GAMMA_TAU[gt]
    adv, ret = gae_sweep(*as_dtype(gae_inputs(n, mask, salt), dtype), gamma, tau)
    stored = adv.astype(np.float32).astype(L) if dtype == "f32" else adv
    st = moments(stored)
    out = dict(adv=adv, ret=ret, stats=st, stored=stored, std=(stored - st[1]) / np.sqrt(st[2] / (st[0] - 1)))
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- bounds. float64: the project's 1e-11, per element and on the batch's scale (gamma tau = 1 takes advantages to 1.6e5).
# Measured, plain float64 sweep against the long-double one at the largest case of each kind x GAMMA_TAU: at most 0.0014 of this bound
# (test_scan_reference_cpu.py::test_float64_sweep_sits_far_inside_the_bound asserts 1/16), so the constant stays as it is.
F64_TOL = 1e-11
STATS_RTOL = 1e-9
U32 = 2.0 ** -24


def gae_bound(ref, dtype):
    """Per-element bound on adv (or ret) against `ref`. float32: the kernel works in float64 on the float32 inputs and rounds once on
    store, so |fl32(x) - ref| <= |x - ref| + 2^-24 |x| <= (1 + 2^-24) B64 + 2^-24 |ref|."""
    ref = np.abs(np.asarray(ref).astype(L))
    b = L(F64_TOL) * ref + L(F64_TOL) * max(L(1), ref.max())
    return b if dtype == "f64" else (1 + L(U32)) * b + L(U32) * ref


def standardized_bound(ref, dtype):
    """Bound on z = (a - mean) / sd given the bounds above: |dz| <= (|da| + |dmean|) / sd + |z| |dsd| / sd + one rounding of z, with
    |dmean| <= 1e-9 |mean|, |dsd| / sd <= 0.5e-9 (M2 within 1e-9) and |da| the advantage's bound -- for float32 against the STORED
    reference advantage, from which the kernel's stored one is at most the float64 bound plus one float32 ulp (2^-23 |a|) away."""
    st = ref["stats"]
    sd = np.sqrt(st[2] / (st[0] - 1))
    a = np.abs(ref["stored"])
    da = L(F64_TOL) * a + L(F64_TOL) * max(L(1), a.max()) + (2 * L(U32) * a if dtype == "f32" else 0)
    u = L(U32) if dtype == "f32" else L(2.0 ** -53)
    return (da + L(STATS_RTOL) * abs(st[1])) / sd + (L(0.5 * STATS_RTOL) + u) * np.abs(ref["std"])


def worst(got, ref, bound):
    """max |got - ref| / bound, in long double (nan counts as infinite)."""
    q = np.abs(np.asarray(got).astype(L) - ref) / bound
    return float(np.where(np.isnan(q), np.inf, q).max())


# ---- K5 as tiles in float64 numpy: the maps, the look to the right, the replay -- and the ways to get them wrong
GAE_MUTANTS = ("no_carry", "one_tile", "one_round", "swapped", "v_edge", "stale")


def gae_tiled(r, m, v, gamma, tau, mutant=None, stale=None):
    """The one-pass kernel's arithmetic on tiles of TILE samples (vectorised over the tiles). `mutant`:
    no_carry: the carry into every tile dropped | one_tile: the look to the right stopped after one tile | one_round: after 64 |
    swapped: the first two maps to the right composed in the wrong order | v_edge: v_{i+1} taken as 0 at tile edges |
    stale: the maps looked at are those of `stale` = (r, m, v) of an earlier call (slots that were not armed again)."""
    assert mutant is None or mutant in GAE_MUTANTS
    n = len(r)
    nt = (n + TILE - 1) // TILE

    def coeffs(r, m, v):
        vn = np.r_[v[1:], 0.0]
        if mutant == "v_edge":
            vn[TILE - 1::TILE] = 0.0
        D, C = np.zeros(nt * TILE), np.ones(nt * TILE)           # past the end: the identity map
        D[:n], C[:n] = r + gamma * vn * m - v, (gamma * tau) * m
        return D.reshape(nt, TILE), C.reshape(nt, TILE)

    def maps(D, C):
        P, A = np.ones(nt), np.zeros(nt)
        for k in range(TILE - 1, -1, -1):
            A = D[:, k] + C[:, k] * A
            P = C[:, k] * P
        return P, A

    D, C = coeffs(r, m, v)
    P, A = maps(*coeffs(*stale)) if mutant == "stale" else maps(D, C)
    carry = np.zeros(nt)
    for t in range(nt):
        order = list(range(t + 1, nt))
        if mutant == "no_carry":
            order = []
        elif mutant == "one_tile":
            order = order[:1]
        elif mutant == "one_round":
            order = order[:ROUND]
        elif mutant == "swapped" and len(order) >= 2:
            order[0], order[1] = order[1], order[0]
        Pacc, Aacc = 1.0, 0.0
        for j in order:
            Aacc = Aacc + Pacc * A[j]
            Pacc = Pacc * P[j]
            if abs(Pacc) < P_STOP:
                break
        carry[t] = Aacc
    a, out = carry, np.empty((nt, TILE))
    for k in range(TILE - 1, -1, -1):
        a = D[:, k] + C[:, k] * a
        out[:, k] = a
    adv = out.ravel()[:n]
    return adv, v + adv


# ================================================================================================ K6
ZF_DIMS = (1, 63, 64, 127, 128, 129, 300)
# rows -> route of the batch's tile statistics into the state (64-row tiles): <= 16 tiles: k_zf_apply merges them itself;
# 17 .. 256: one block of k_zf_merge; more: 16 blocks of k_zf_merge, then k_zf_apply
ZF_ROWS = (1, 64, 1024, 1025, 4100)
ZF_TWO_LEVEL = (16385, (129, 300))
ZF_CASES = [(n, d) for d in ZF_DIMS for n in ZF_ROWS] + [(ZF_TWO_LEVEL[0], d) for d in ZF_TWO_LEVEL[1]]
ZF_TOL = dict(mean=1e-12, S=1e-10, y=1e-10, y32=2e-5)          # the parity tests' own; the count is exact
ZF_CLIP = 5.0


@functools.lru_cache(maxsize=8)
def zf_inputs(n, dim):
    """(X0: the rows behind the running state the call starts from, X, active): columns of different scale and offset, a few rows far
    out (the clip must have something to do), 80 % of the rows active (the first one always: n = 1 must count)."""
    rng = np.random.RandomState(_seed("zf", n, dim))
    X0 = rng.normal(size=(300, dim)) * 2 - 0.5
    X = rng.normal(size=(n, dim)) * np.linspace(0.5, 4.0, dim) + np.linspace(-2, 2, dim)
    X[5::101] *= 6.0
    act = (rng.uniform(size=n) < 0.8).astype(np.int32)
    act[0] = 1
    for a in (X0, X, act):
        a.setflags(write=False)
    return X0, X, act


def zf_state(rs):
    return np.r_[float(rs.n), rs.mean, rs.S]


def zf_reference(n, dim, dtype="f64", update=True, clip=ZF_CLIP):
    """-> (state the call starts from, state after it, y) by the oracle, on the inputs as the entry point of `dtype` sees them."""
    X0, X, act = zf_inputs(n, dim)
    X, = as_dtype((X,), dtype)
    rs = Z.RunningStatOracle(dim)
    rs.merge_block(X0)
    s0 = zf_state(rs)
    if update:
        rs.merge_block(X[act == 1])
    return s0, zf_state(rs), Z.zfilter_apply(X, rs.mean, rs.std, clip)


def zf_excess(state, y, ref_state, ref_y, ytol=ZF_TOL["y"]):
    """By how many times (count, mean, S, y) miss the tolerances, the worst of the four (a wrong count: infinitely)."""
    dim = (len(state) - 1) // 2
    over = lambda got, ref, rtol, atol: float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())
    return max(0.0 if state[0] == ref_state[0] else np.inf,
               over(state[1:1 + dim], ref_state[1:1 + dim], ZF_TOL["mean"], ZF_TOL["mean"]),
               over(state[1 + dim:], ref_state[1 + dim:], ZF_TOL["S"], 0.0),
               over(y, ref_y, ytol, ytol))


ZF_MUTANTS = ("wrong_group_count", "skip_last_partial_tile")


def zf_tiled(X, act, state0, clip=ZF_CLIP, mutant=None):
    """K6 as tiles in float64 numpy, for batches of 64-row tiles (n <= 32 768): eight row groups of 8 rows per tile, each with
    (count, mean, M2) per column, merged in group order, the tiles then merged in order into the running state. `mutant`:
    wrong_group_count: columns 128 and up take the NEXT group's count in the merge of the groups (the count is kept once per
    group, by column block 0) | skip_last_partial_tile: a last tile of fewer than 64 rows never reaches the state."""
    assert mutant is None or mutant in ZF_MUTANTS
    n, dim = X.shape
    assert n <= 64 * 512
    cnt, mean, S = state0[0], state0[1:1 + dim].copy(), state0[1 + dim:].copy()

    def merge(c, mu, s, nb, mb, sb):              # Chan: (c, mu, s) <- (c, mu, s) + (nb, mb, sb); nb may differ by column
        tot = c + nb
        w = np.where(tot > 0, nb / np.where(tot > 0, tot, 1.0), 0.0)
        d = mb - mu
        return tot, mu + d * w, s + sb + d * d * (c * w)

    for r0 in range(0, n, 64):
        r1 = min(n, r0 + 64)
        if mutant == "skip_last_partial_tile" and r1 - r0 < 64:
            continue
        groups = []
        for g in range(8):
            rows = np.arange(r0 + 8 * g, min(r1, r0 + 8 * g + 8))
            rows = rows[act[rows] == 1] if len(rows) else rows
            k = len(rows)
            mb = X[rows].mean(axis=0) if k else np.zeros(dim)
            groups.append((float(k), mb, ((X[rows] - mb) ** 2).sum(axis=0) if k else np.zeros(dim)))
        tc, tm, ts = np.zeros(dim), np.zeros(dim), np.zeros(dim)
        for g in range(8):
            k = np.full(dim, groups[g][0])
            if mutant == "wrong_group_count":
                k[128:] = groups[(g + 1) % 8][0]
            tc, tm, ts = merge(tc, tm, ts, k, groups[g][1], groups[g][2])
        cnt_new, mean, S = merge(np.full(dim, cnt), mean, S, tc, tm, ts)
        cnt = cnt_new[0]                           # (the state's count is column 0's)
    var = S / (cnt - 1) if cnt > 1 else mean * mean
    return np.r_[cnt, mean, S], Z.zfilter_apply(X, mean, np.sqrt(var), clip)
