"""Shared by test_update_tail_reference_cpu.py and test_update_tail_reference_gpu.py: cases, float64 references and error bounds
for the kernels of csrc/egp_update.hip -- the fused PPO losses (k_ppo_loss, k_ppo_loss_mb), and clip + Adam (k_sqnorm, k_adam).
numpy / torch on the CPU only; nothing here calls egopose_amd.optim or a kernel.

References restate the reference project's expressions: the diagonal Gaussian log-density (core/distributions.py:6-25 over
utils/math.py:14-17), the clipped surrogate (agents/agent_ppo.py:58-65), the critic's MSE (agents/agent_pg.py:19-26) with float64
torch autograd for their gradients, and clip_grad_norm_ + torch.optim.Adam (agents/agent_ppo.py:24-30,53-56) from the formula in
include/egopose_hip.h over flat float64 arrays.

Bounds come from operation counts, with u = 2^-24 for float32 outputs and 2^-53 for float64 ones:

  logp           delta_i = (A / 16 + 12) u sum_j |term_ij|: a lane adds at most A / 16 terms in sequence, the 16 lanes combine in four
                 butterfly levels, every term is ~6 operations on its operands and an expf. The |term|s are the summands the kernel
                 adds: z^2 / 2, log(2 pi) / 2 and |log_std_j| of every column, NOT the |.| of a column's finished log-density --
                 with log_std near -1 (these draws) a column's three summands cancel to ~0 around |z| = 0.4, its rounding
                 errors do not, and a row of one or three columns then has an error of several times (A / 16 + 12) u |density|
                 (the float32 emulation reached 2.4 x that at A = 1 within 67 rows)
  near rows      the float32 log-ratio decides on which side of the clip range a row falls. A row is `near` when its float64
                 log-ratio is within delta_i + u |logp_i| + 4 u of log lo or log hi (4 u: expf, and lo / hi rounded to float32) --
                 such rows are re-drawn when a case is made, so NO row is ever left out of a comparison
  fixed_logp     delta_i                                        d_pred   4 u |ref|
  d_mean         (delta_i + 16 u) |ref_ij| when the ratio is read (its relative error is the log-ratio's absolute one),
                 16 u |ref_ij| in the write pass, where the ratio is exactly 1
  both losses    (delta_max + 8 u) sum |terms| / n: float64 sums of float32 terms
  d_log_std      (P + 8) u sum_i |g_i| (z_ij^2 + 1) + the d_mean-type relative error of every row's term; P = rows one lane adds
                 up in float32: ceil(n_pol / (16 pol_blocks)) for the full-batch kernel, ceil(n / 32) for the window kernel.
                 Again the summands before they cancel: g z^2 and -g. (|g (z^2 - 1)| vanishes at |z| = 1 while the rounding
                 error of z^2 does not; with a single policy row the emulation exceeded that form 8-fold)
  squared norm   N 2^-53 relative
  Adam           first-order propagation through one step, g' = the clipped, decayed gradient:
                     e_g = 4 u (|coef g| + wd |p|)
                     e_m = 8 u (|m| + |g'|) + (1 - beta1) e_g
                     e_v = 8 u (beta2 |v| + (1 - beta2) g'^2) + 2 (1 - beta2) |g'| e_g
                     e_den = e_v / (2 sqrt(v') sqrt(bias2)) + 6 u denom
                     e_p = 2 u |p'| + step_size (e_m / denom + |m'| e_den / denom^2) + 6 u |step|
                 A chain of k steps carries the errors along by the same first-order rules: beta1 E_m and beta2 E_v enter the next
                 step's e_m and e_v, E_p its e_g (through the weight decay) and its e_p. For m and v that is never more than the
                 sum of the k single-step bounds (k times the single-step bound for steps that are alike). For p it can be more:
                 the carried E_m and E_v also enter the step through step_size (E_m / denom + |m'| e_den / denom^2), on top of the
                 carried E_p -- a step with a small gradient after one with a large one inherits the large one's error in m, which
                 "k times the last step's bound" would not cover.
"""
import functools
import math
import zlib

import numpy as np
import torch

U32, U64 = 2.0 ** -24, 2.0 ** -53
CLIP = 0.2
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
LOSS_GROUP = 16                 # lanes per policy row
LOSS_GPB = 16                   # row groups per workgroup of k_ppo_loss
LOSS_MAX_BLOCKS = 1024
LOSS_MAX_ACT = 256
MB_GROUPS = 32                  # row groups of k_ppo_loss_mb's one workgroup
MB_MAX_ROWS = 16384
ADAM_MAX_SEGMENTS = 8

f32 = np.float32


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def _ro(a):
    a.setflags(write=False)
    return a


def pol_blocks(n_pol):
    """Workgroups k_ppo_loss gives the policy rows: ~4 passes of 16 rows each, at most 1 024."""
    return min(max(-(-n_pol // (4 * LOSS_GPB)), 1 if n_pol > 0 else 0), LOSS_MAX_BLOCKS)


def rows_per_lane(n_pol, window=False):
    if window:
        return -(-n_pol // MB_GROUPS)
    return -(-n_pol // (LOSS_GPB * pol_blocks(n_pol))) if n_pol else 0


# ------------------------------------------------------------------------------------------------ the losses
def loss_reference(c, mean, fixed, n_val, n_exp, clip=CLIP, mask=None):
    """float64 autograd over the plain expressions. `c`: a case (below); `mean` (n_pol, A); `fixed` (n_pol,) or None = the write
    pass (the ratio is exactly 1); `mask` (n_pol,) bool or None = the rows that enter the surrogate (the window kernel's exps)."""
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))
    rows = c["rows"]
    pred, mean_t, ls = (t(a).requires_grad_(True) for a in (c["pred"], mean, c["log_std"]))
    returns = t(c["returns"])
    act = t(c["actions"] if rows is None else c["actions"][rows])
    adv = t(c["adv"] if rows is None else c["adv"][rows])
    var = torch.exp(ls).pow(2)
    terms = -(act - mean_t).pow(2) / (2.0 * var) - HALF_LOG_2PI - ls
    logp = terms.sum(1)
    logp.retain_grad()
    fx = logp.detach() if fixed is None else t(fixed)
    ratio = torch.exp(logp - fx)
    surr = torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv)
    if mask is not None:
        surr = surr[torch.from_numpy(np.asarray(mask, dtype=bool))]
    s_loss = -surr.sum() / n_exp
    v_terms = (pred - returns).pow(2)
    v_loss = v_terms.sum() / n_val
    (v_loss + s_loss).backward()
    g = logp.grad if logp.grad is not None else torch.zeros_like(logp)
    z = ((act - mean_t) / torch.exp(ls)).detach()
    dls_terms = g.abs().reshape(-1, 1) * (z * z + 1.0)                      # |g z^2| + |g|: the summands before they cancel
    abs_terms = (0.5 * z * z + HALF_LOG_2PI + ls.detach().abs()).sum(1)    # likewise: z^2 / 2, log(2 pi) / 2 and |log_std| of every column
    zero = lambda x: torch.zeros_like(x)
    n = lambda x: x.detach().numpy()
    return {"v_loss": v_loss.item(), "s_loss": s_loss.item(), "v_abs": v_loss.item(), "s_abs": surr.detach().abs().sum().item() / n_exp,
            "d_pred": n(pred.grad if pred.grad is not None else zero(pred)), "d_mean": n(mean_t.grad if mean_t.grad is not None else zero(mean_t)),
            "d_log_std": n(ls.grad if ls.grad is not None else zero(ls)), "logp": n(logp), "abs_terms": n(abs_terms),
            "log_ratio": n(logp - fx), "g_logp": n(g), "dls_terms": n(dls_terms), "dls_abs": n(dls_terms.sum(0))}


def logp_delta(ref, A, u=U32):
    return (A / 16.0 + 12.0) * u * ref["abs_terms"]


def near_rows(ref, A, clip=CLIP, u=U32):
    d = logp_delta(ref, A, u) + u * np.abs(ref["logp"]) + 4.0 * u
    lr = ref["log_ratio"]
    return (np.abs(lr - math.log(1.0 - clip)) <= d) | (np.abs(lr - math.log(1.0 + clip)) <= d)


def regimes(ref, clip=CLIP):
    """shares of the rows with ratio < lo, inside, > hi"""
    lr = ref["log_ratio"]
    n = max(lr.size, 1)
    below, above = (lr < math.log(1.0 - clip)).sum() / n, (lr > math.log(1.0 + clip)).sum() / n
    return below, 1.0 - below - above, above


def loss_bounds(ref, A, P, write_pass, u=U32):
    delta = logp_delta(ref, A, u)
    dmax = float(delta.max()) if delta.size else 0.0
    rel = np.full(delta.shape, 16.0 * u) if write_pass else delta + 16.0 * u
    return {"logp": delta, "d_pred": 4.0 * u * np.abs(ref["d_pred"]), "d_mean": rel.reshape(-1, 1) * np.abs(ref["d_mean"]),
            "v_loss": (dmax + 8.0 * u) * ref["v_abs"], "s_loss": (dmax + 8.0 * u) * ref["s_abs"],
            "d_log_std": (P + 8.0) * u * ref["dls_abs"] + (rel.reshape(-1, 1) * ref["dls_terms"]).sum(0)}


def worst(got, ref, bound):
    """largest |got - ref| / bound over the elements (0 / 0 counts as 0, anything over a zero bound as inf)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)).reshape(-1)
    b = np.broadcast_to(np.asarray(bound, dtype=np.float64), np.shape(ref)).reshape(-1)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / b)
    r = np.where(np.isnan(r), np.inf, r)            # (a NaN result is a miss, not a pass)
    return float(r.max())


@functools.lru_cache(maxsize=None)
def policy_case(n, n_pol, A, with_rows, clip=CLIP, salt=0):
    """One batch, read-only float32 arrays: log_std (A,), actions (n, A), pred / returns / adv (n,), rows (n_pol,) int64 -- an
    UNSORTED random subset -- or None (then n_pol == n), mean0 (the write pass), fixed = float32 of the float64 log-density
    under mean0, mean = mean0 moved by N(0, (0.3 / sqrt(A) std_j)^2): the log-ratio is ~N(-0.045, 0.3^2) for every width, which
    puts ~28 % of the rows below lo, ~22 % above hi. Rows near the clip boundary are drawn again until none is left.
    `ref_write` / `ref_read`: the float64 references of the two passes with the "global" counts n_val = n + 3, n_exp = n_pol + 5."""
    assert with_rows or n_pol == n
    rng = np.random.RandomState(_seed("policy", n, n_pol, A, with_rows, clip, salt))
    c = {"n": n, "n_pol": n_pol, "A": A, "clip": clip, "n_val": n + 3.0, "n_exp": n_pol + 5.0}
    c["log_std"] = (rng.normal(size=A) * 0.2 - 1.0).astype(f32)
    c["actions"] = (rng.normal(size=(n, A)) * 0.3).astype(f32)
    c["pred"], c["returns"], c["adv"] = (rng.normal(size=n).astype(f32) for _ in range(3))
    c["rows"] = rng.permutation(n)[:n_pol].astype(np.int64) if with_rows else None
    act = c["actions"] if c["rows"] is None else c["actions"][c["rows"]]
    std = np.exp(c["log_std"].astype(np.float64))
    c["mean0"] = (act + rng.normal(size=(n_pol, A)) * std).astype(f32)
    c["ref_write"] = loss_reference(c, c["mean0"], None, c["n_val"], c["n_exp"], clip)
    c["fixed"] = c["ref_write"]["logp"].astype(f32)
    move = 0.3 / math.sqrt(A) * std
    mean = (c["mean0"] + rng.normal(size=(n_pol, A)) * move).astype(f32)
    redrawn = 0
    for _ in range(50):
        ref = loss_reference(c, mean, c["fixed"], c["n_val"], c["n_exp"], clip)
        near = near_rows(ref, A, clip)
        if not near.any():
            break
        redrawn += int(near.sum())
        mean[near] = (c["mean0"][near] + rng.normal(size=(int(near.sum()), A)) * move).astype(f32)
    c["mean"], c["ref_read"], c["redrawn"], c["near"] = mean, ref, redrawn, int(near_rows(ref, A, clip).sum())
    for v in c.values():
        if isinstance(v, np.ndarray):
            _ro(v)
    return c


# (n, n_pol, A, with_rows) of the full-batch kernel
WIDTH_CASES = [(101, 67, A, True) for A in (1, 15, 16, 17, 52, 255, 256)] + [(101, 101, 17, False)]
ROW_CASES = [(n_pol + 9, n_pol, 17, True) for n_pol in (1, 16, 17, 63, 64, 65)]
POL_CAP_CASE = (70001, 65555, 3, True)                 # 1 024 workgroups, a fifth pass: whole in block 0, ragged in block 1
VAL_CAP_CASE = (1048576 + 261, 19, 3, True)            # more value elements than 1 024 workgroups x 256 threads x 4
EMPTY_POL_CASE = (300, 0, 17, True)
STRIDE_CASE = (101, 67, 17, True)
FULL_CASES = WIDTH_CASES + ROW_CASES + [POL_CAP_CASE, VAL_CAP_CASE, EMPTY_POL_CASE]

WINDOW_SHAPES = [(1, 1), (31, 16), (32, 17), (33, 17), (511, 5), (512, 52), (513, 256), (16384, 3)]
WINDOW_FORMS = ("ones", "last", "mixed")


def window_exps(n, form):
    if form == "ones":
        return _ro(np.ones(n, dtype=f32))
    if form == "last":
        e = np.zeros(n, dtype=f32)
        e[-1] = 1.0
        return _ro(e)
    e = (np.random.RandomState(_seed("exps", n)).rand(n) < 0.6).astype(f32)
    e[0] = 1.0                                           # (never an empty window: its surrogate loss is NaN by definition)
    return _ro(e)


@functools.lru_cache(maxsize=None)
def window_case(n, A, form):
    """(case, exps, float64 reference) of one window: the full-batch case of n rows without `rows`, the window's own counts."""
    c = policy_case(n, n, A, False)
    e = window_exps(n, form)
    return c, e, loss_reference(c, c["mean"], c["fixed"], float(n), float((e != 0).sum()), c["clip"], mask=e != 0)


def loss_emulation(c, mean, fixed, n_val, n_exp, clip=CLIP, mask=None, window=False, mutant=None):
    """The kernels' arithmetic in numpy float32, in their summation order: lane l adds the terms of columns l, l + 16, ..., the 16
    lanes combine in a butterfly; a lane's d_log_std sums run over its rows in float32, everything across lanes in float64.
    `mutant`: None, "drop" (one row missing from every sum), "tie" (a tie of min sends the whole gradient down BOTH branches
    instead of half each way), "ends" (clamp's sub-gradient 0 at lo and hi)."""
    rows = c["rows"]
    act = c["actions"] if rows is None else c["actions"][rows]
    adv = (c["adv"] if rows is None else c["adv"][rows]).astype(f32)
    mean = np.asarray(mean, dtype=f32)
    n_pol, A = mean.shape
    ok = np.ones(n_pol, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    ls = c["log_std"]
    istd = np.exp(-ls).astype(f32)
    z = ((act - mean) * istd).astype(f32)
    terms = (f32(-0.5) * z * z - f32(HALF_LOG_2PI) - ls).astype(f32)
    maxd = LOSS_MAX_ACT // LOSS_GROUP
    pad = np.zeros((n_pol, maxd * LOSS_GROUP), dtype=f32)
    pad[:, :A] = terms
    pad = pad.reshape(n_pol, maxd, LOSS_GROUP)
    acc = np.zeros((n_pol, LOSS_GROUP), dtype=f32)
    for k in range(maxd):
        acc = acc + pad[:, k, :]
    lane = np.arange(LOSS_GROUP)
    for off in (8, 4, 2, 1):
        acc = acc + acc[:, lane ^ off]
    logp = acc[:, 0]
    fx = logp if fixed is None else np.asarray(fixed, dtype=f32)
    lo, hi = f32(1.0 - clip), f32(1.0 + clip)
    ratio = np.exp((logp - fx).astype(f32)).astype(f32)
    clamped = np.minimum(np.maximum(ratio, lo), hi)
    s1, s2 = ratio * adv, clamped * adv
    surr = np.minimum(s1, s2)
    inside = ((ratio > lo) & (ratio < hi) if mutant == "ends" else (ratio >= lo) & (ratio <= hi)).astype(f32)
    w = f32(1.0) if mutant == "tie" else f32(0.5)
    g_ratio = np.where(s1 < s2, adv, np.where(s1 > s2, adv * inside, w * adv + w * adv * inside)).astype(f32)
    g_logp = np.where(ok, f32(-1.0 / n_exp) * g_ratio * ratio, f32(0.0)).astype(f32)
    d_mean = (g_logp.reshape(-1, 1) * z * istd).astype(f32)
    dterm = (g_logp.reshape(-1, 1) * (z * z - f32(1.0))).astype(f32)
    live = ok.copy()
    if mutant == "drop" and live.any():
        live[np.nonzero(live)[0][-1]] = False
    groups = MB_GROUPS if window else LOSS_GPB * max(pol_blocks(n_pol), 1)
    lanes = np.zeros((groups, A), dtype=f32)
    for p0 in range(0, n_pol, groups):
        k = min(groups, n_pol - p0)
        lanes[:k] = lanes[:k] + np.where(live[p0:p0 + k, None], dterm[p0:p0 + k], f32(0.0))
    d = (c["pred"] - c["returns"]).astype(f32)
    dd = d.astype(np.float64) ** 2
    if mutant == "drop":
        dd = dd[:-1]
    return {"v_loss": float(dd.sum() / n_val), "s_loss": float(-surr[live].astype(np.float64).sum() / n_exp),
            "d_pred": (f32(2.0 / n_val) * d).astype(f32), "d_mean": d_mean, "d_log_std": lanes.astype(np.float64).sum(0).astype(f32),
            "logp": logp}


# ------------------------------------------------------------------------------------------------ clip + Adam
def _seg(begin, end, group=0, max_norm=0.0, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, wd=0.0):
    return {"begin": begin, "end": end, "clip_group": group, "max_norm": max_norm, "lr": lr, "beta1": betas[0], "beta2": betas[1],
            "eps": eps, "wd": wd}


# L1: a leading gap, gaps between segments, one empty segment, groups {0, 1, 3} with 2 unused, two segments in group 1
L1_TOTAL = 3000
L1 = [_seg(7, 300), _seg(313, 900, 1, 40.0, lr=5e-5), _seg(900, 900), _seg(905, 1411, 1, 40.0, lr=2e-4, wd=1e-3),
      _seg(1411, 1800, 3, 5.0, lr=1e-3, betas=(0.85, 0.99)), _seg(1850, 2100, lr=1e-4), _seg(2100, 2613, lr=3e-4, eps=1e-6),
      _seg(2700, 2950, 3, 5.0, lr=7e-4)]
# L2: one clipped segment longer than k_adam's grid of 2 048 x 256 threads
L2_TOTAL = 524288 + 257 + 64
L2 = [_seg(0, 524288 + 257, 1, 40.0)]


def with_step(segs, t):
    """the segments with the bias corrections of step t (>= 1)"""
    return [dict(s, bias1=1.0 - s["beta1"] ** t, bias2=1.0 - s["beta2"] ** t) for s in segs]


def covered(segs, total):
    m = np.zeros(total, dtype=bool)
    for s in segs:
        m[s["begin"]:s["end"]] = True
    return m


def adam_gradient(segs, total, seed, norm_over_max):
    """float64 gradient over the flat buffer, magnitudes log-uniform in [1e-5, 1] (so that sqrt(v) meets eps), every clip group
    scaled to norm = norm_over_max[group] x its max_norm (0: an all-zero gradient). The gaps hold gradient values too."""
    rng = np.random.RandomState(_seed("grad", total, seed))
    g = rng.choice([-1.0, 1.0], size=total) * 10.0 ** rng.uniform(-5.0, 0.0, size=total)
    for grp, k in norm_over_max.items():
        mine = [s for s in segs if s["clip_group"] == grp and s["end"] > s["begin"]]
        sq = sum(float((g[s["begin"]:s["end"]] ** 2).sum()) for s in mine)
        for s in mine:
            g[s["begin"]:s["end"]] *= k * s["max_norm"] / math.sqrt(sq)
    return g


def adam_state(total, seed, warm):
    """(p, m, v) float64: p ~ N(0, 0.1^2); zero moments, or a warm state"""
    rng = np.random.RandomState(_seed("state", total, seed))
    p = rng.normal(size=total) * 0.1
    if not warm:
        return p, np.zeros(total), np.zeros(total)
    return p, rng.normal(size=total) * 1e-2, (rng.normal(size=total) * 3e-2) ** 2 + 1e-10


def adam_reference(segs, grad, p, m, v, ptype, err_in=None, weights="torch"):
    """One clip + Adam step over flat float64 arrays, header formula. `ptype`: the kernel's parameter type -- `1 - beta` is formed
    in double and rounded to it, as torch does; u follows it. weights="kernel": the two weights as k_adam forms them today,
    (ptype)1 - (ptype)beta -- the same number in float64, 0.00099998713 for beta2 = 0.999 in float32. -> dict: p, m, v (elements outside every segment untouched),
    norms[9] (NaN where no group), coef{group}, and the bounds e_p, e_m, e_v given the incoming errors `err_in` = (E_p, E_m, E_v)."""
    u = U32 if ptype == np.float32 else U64
    p2, m2, v2 = p.copy(), m.copy(), v.copy()
    Ep, Em, Ev = (np.zeros_like(p) for _ in range(3)) if err_in is None else (e.copy() for e in err_in)
    norms, coef = np.full(ADAM_MAX_SEGMENTS + 1, np.nan), {0: 1.0}
    for grp in sorted({s["clip_group"] for s in segs} - {0}):
        sq = sum(((grad[s["begin"]:s["end"]].astype(np.longdouble)) ** 2).sum() for s in segs if s["clip_group"] == grp)
        norms[grp] = float(np.sqrt(np.longdouble(sq)))
        max_norm = [s["max_norm"] for s in segs if s["clip_group"] == grp][-1]
        coef[grp] = min(1.0, max_norm / (norms[grp] + 1e-6))
    for s in segs:
        sl = slice(s["begin"], s["end"])
        if s["end"] <= s["begin"]:
            continue
        if weights == "kernel":
            w1, w2 = float(ptype(1.0) - ptype(s["beta1"])), float(ptype(1.0) - ptype(s["beta2"]))
        else:
            w1, w2 = float(ptype(1.0 - s["beta1"])), float(ptype(1.0 - s["beta2"]))
        c, wd, b1, b2 = coef[s["clip_group"]], s["wd"], s["beta1"], s["beta2"]
        g, p0, m0, v0 = grad[sl], p[sl], m[sl], v[sl]
        gq = c * g + wd * p0                                   # weight decay after the clip
        mm = m0 + w1 * (gq - m0)
        vv = b2 * v0 + w2 * gq * gq
        sb2 = math.sqrt(s["bias2"])
        denom = np.sqrt(vv) / sb2 + s["eps"]
        step_size = s["lr"] / s["bias1"]
        step = step_size * mm / denom
        pn = p0 - step
        e_g = 4.0 * u * (np.abs(c * g) + wd * np.abs(p0)) + wd * Ep[sl]
        e_m = 8.0 * u * (np.abs(m0) + np.abs(gq)) + (1.0 - b1) * e_g + b1 * Em[sl]
        e_v = 8.0 * u * (b2 * np.abs(v0) + (1.0 - b2) * gq * gq) + 2.0 * (1.0 - b2) * np.abs(gq) * e_g + b2 * Ev[sl]
        with np.errstate(divide="ignore", invalid="ignore"):
            e_den = np.where(vv > 0.0, e_v / (2.0 * np.sqrt(vv) * sb2), 0.0) + 6.0 * u * denom
        e_p = Ep[sl] + 2.0 * u * np.abs(pn) + step_size * (e_m / denom + np.abs(mm) * e_den / denom ** 2) + 6.0 * u * np.abs(step)
        p2[sl], m2[sl], v2[sl] = pn, mm, vv
        Ep[sl], Em[sl], Ev[sl] = e_p, e_m, e_v
    return {"p": p2, "m": m2, "v": v2, "norms": norms, "coef": coef, "e_p": Ep, "e_m": Em, "e_v": Ev}


def adam_emulation_f32(segs, grad, p, m, v, mutant=None):
    """k_adam<float, float>'s arithmetic in numpy float32 (the norm in float64, as k_sqnorm). `mutant`: None, "eps" (eps inside the
    square root), "wd" (weight decay before the clip), "beta" (`1.f - (float)beta2` in place of (float)(1.0 - beta2)), "kernel" (both
    weights as 1.f - (float)beta: k_adam<float> as it is today)."""
    grad, p, m, v = (np.asarray(a, dtype=f32) for a in (grad, p, m, v))
    p2, m2, v2 = p.copy(), m.copy(), v.copy()
    coef = {0: 1.0}
    for grp in {s["clip_group"] for s in segs} - {0}:
        sq = sum(float((grad[s["begin"]:s["end"]].astype(np.float64) ** 2).sum()) for s in segs if s["clip_group"] == grp)
        coef[grp] = min(1.0, [s["max_norm"] for s in segs if s["clip_group"] == grp][-1] / (math.sqrt(sq) + 1e-6))
    for s in segs:
        sl = slice(s["begin"], s["end"])
        if s["end"] <= s["begin"]:
            continue
        c, wd, b2 = f32(coef[s["clip_group"]]), f32(s["wd"]), f32(s["beta2"])
        w1 = f32(1.0) - f32(s["beta1"]) if mutant == "kernel" else f32(1.0 - s["beta1"])
        w2 = f32(1.0) - b2 if mutant in ("beta", "kernel") else f32(1.0 - s["beta2"])
        g = (grad[sl] + wd * p[sl]) * c if mutant == "wd" else grad[sl] * c + wd * p[sl]
        mm = m[sl] + (g - m[sl]) * w1
        vv = b2 * v[sl] + w2 * g * g
        sb2 = f32(math.sqrt(s["bias2"]))
        if mutant == "eps":
            denom = np.sqrt(vv.astype(np.float64) / s["bias2"] + s["eps"]).astype(f32)
        else:
            denom = np.sqrt(vv.astype(np.float64)).astype(f32) / sb2 + f32(s["eps"])
        p2[sl], m2[sl], v2[sl] = p[sl] - f32(s["lr"] / s["bias1"]) * (mm / denom), mm, vv
    return {"p": p2, "m": m2, "v": v2}


# what the step tests run: name -> (first step number t, warm start, [per step: {group: norm / max_norm}], {step index: lr factor})
ADAM_RUNS = {
    "t1": (1, False, [{1: 2.5, 3: 0.8}], {}),                                   # from zero moments; group 1 clipped, group 3 not
    "t1000": (1000, True, [{1: 0.8, 3: 2.5}], {}),                              # warm state
    "zero": (1, False, [{1: 0.0, 3: 0.8}], {}),                                 # group 1's gradient is all zeros: norm 0, coefficient 1
    "chain4": (1, False, [{1: 2.5, 3: 0.8}, {1: 0.8, 3: 2.5}, {1: 2.5, 3: 0.8}, {1: 0.8, 3: 2.5}], {2: 0.4}),   # lr x 0.4 after step 2
}


def adam_run(layout, total, run, ptype, f32_grad, weights="torch"):
    """-> (p0, m0, v0, [(segments, gradient, reference)] per step), float64, the inputs already rounded to what the entry point
    stores (`ptype` for p / m / v, float32 for the gradient when `f32_grad`); the bounds chain through the steps."""
    t0, warm, norms, lr_at = ADAM_RUNS[run]
    p, m, v = (a.astype(ptype).astype(np.float64) for a in adam_state(total, run, warm))
    state, err, segs, steps = (p, m, v), None, [dict(s) for s in layout], []
    for k, nm in enumerate(norms):
        if k in lr_at:
            segs = [dict(s, lr=s["lr"] * lr_at[k]) for s in segs]
        g = adam_gradient(segs, total, (run, k), nm)
        g = g.astype(f32).astype(np.float64) if f32_grad else g
        sg = with_step(segs, t0 + k)
        ref = adam_reference(sg, g, state[0], state[1], state[2], ptype, err, weights)
        steps.append((sg, g, ref))
        state, err = (ref["p"], ref["m"], ref["v"]), (ref["e_p"], ref["e_m"], ref["e_v"])
    return p, m, v, steps
