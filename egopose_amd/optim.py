"""The element-wise tail of a PPO epoch on the HIP kernels of csrc/egp_update.hip.

  ppo_losses(...)   critic MSE (agents/agent_pg.py:19-26) + clipped surrogate (agents/agent_ppo.py:58-65 over
                    core/distributions.py:6-25) and their gradients w.r.t. `values_pred` / `action_mean` in ONE launch; the caller
                    back-propagates from those two tensors (no scalar-loss graph)
  ppo_stats(...) / ppo_stats_torch(...) / stats_summary(...)   the update monitor: one record of float64 raw sums about the tensors
                    an epoch hands to ppo_losses (KL estimators, clipped rows, ratio range, moments for the critic's explained
                    variance, non-finite rows, entropy) from a launch of its own, the same definitions in torch ops for any device
                    and dtype, and the host-side combination of the ranks' records into the figures
  minibatch_plan(...)  one launch per mini-batch epoch (agents/agent_ppo.py:25-31): the update's six columns gathered through the
                    epoch's permutation into the caller's buffers + the number of exploration rows of every window, on the device
  ppo_losses_mb(...)   ppo_losses for ONE window of those buffers with shapes that do not depend on the data: the rows with
                    exps == 0 are masked (d_mean = 0), the surrogate's mean divides by the window's device-side count
  gail_rows(...) / GailRows, bce_logits(...)   the GAIL discriminator step (ego_pose/core/agent_vgail.py:54-73, csrc/egp_gail.hip): the
                    [generated; expert] input block from one set of video-context rows with its adjoint, and nn.BCELoss on the
                    logits of that block with d loss / d logits and the per-row score -log D
  FlatUpdater / TorchUpdater   the update step after backward, one protocol in two forms:
                        zero_grad()  ...forward, backward...  collect_grads(which); all_reduce(which); step(which)
                    (`which` = indices of the optimizers to step, None = all; `rebind()` after a caller moved its modules;
                    `grad_norm(group)` = the last step's pre-clip norm). FlatUpdater is clip_policy_grad (agent_ppo.py:53-56) +
                    optimizer_value.step() + optimizer_policy.step() (agent_ppo.py:24-30) as two launches over flat buffers. The
                    caller's torch.optim.Adam objects stay the source of every hyper-parameter (`set_optimizer_lr` keeps working)
                    and see the moments as their own state; the parameters of the caller's modules become views of one flat
                    buffer, the gradient buffer doubles as the all-reduce buffer (no copies in or out), and with float64 master
                    modules (the unmodified driver) the float32 compute copies are refreshed by the same launch. TorchUpdater is
                    the same sequence with the caller's optimizers stepping themselves (any device, dtype and optimizer class).

The kernels have no CPU form: on a CPU device (the oracle-side parity tests) the agent runs the plain torch formulation.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L
from . import dist as D

_WS = {}            # (key, device, stream handle) -> zeroed scratch; least recently used entries dropped beyond _WS_MAX
_WS_MAX = 8


def _zeroed_workspace(key, nbytes, device):
    """Partial-sum scratch of the loss kernels, one per (device, stream): two updates issued on different streams of one device
    must not share it between k_ppo_loss and k_ppo_loss_final. INVARIANT: the buffer is all zeros between calls --
    the kernels' arrival counter lives in it, starts at zero and is reset by the last workgroup to arrive; a fresh buffer is
    zero-filled here. The cache is bounded (code that creates short-lived streams must not grow it for ever): an evicted entry's
    stream handle may be recycled by the runtime for a new stream, which then simply gets a fresh zeroed buffer."""
    k = (key, str(device), int(torch.cuda.current_stream(device).cuda_stream))
    buf = _WS.pop(k, None)
    if buf is None or buf.numel() < nbytes:
        buf = torch.zeros(int(nbytes), dtype=torch.uint8, device=device)
    _WS[k] = buf                       # (re-inserted: dict order = recency)
    while len(_WS) > _WS_MAX:
        _WS.pop(next(iter(_WS)))
    return buf


def losses_available(pred, mean, log_std):
    return (pred.is_cuda and pred.dtype == torch.float32 and mean.dtype == torch.float32 and mean.dim() == 2 and mean.stride(1) == 1
            and log_std.dtype == torch.float32 and log_std.numel() == mean.shape[1] and mean.shape[1] <= 256)


def ppo_losses(pred, returns, mean, actions, log_std, adv, fixed_logp, write_fixed, clip_eps, n_val, n_exp, rows=None,
               d_pred=None, d_mean=None, want_d_log_std=False, losses_out=None):
    """-> (losses float64[2] on the device = value loss, surrogate loss; d_pred (n, 1); d_mean (n_pol, A); d_log_std (1, A) or None).
    `fixed_logp` (n_pol,) float32 is written when `write_fixed`, read otherwise. `rows`: int64 sample index of every policy row."""
    lib = L.load()
    n, n_pol, A = pred.shape[0], mean.shape[0], mean.shape[1]
    dev = pred.device
    pred1 = pred.reshape(-1)
    ret1 = returns.reshape(-1)
    adv1 = adv.reshape(-1)
    for name, t, want in (("pred", pred1, n), ("returns", ret1, n), ("adv", adv1, n), ("fixed_logp", fixed_logp, n_pol)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == want):
            raise ValueError("%s must be a contiguous float32 HIP tensor of %d elements" % (name, want))
    if not (actions.dtype == torch.float32 and actions.dim() == 2 and actions.stride(1) == 1 and actions.shape == (n, A)):
        raise ValueError("actions must be (n, act_dim) float32 with unit column stride")
    ls = log_std.reshape(-1).contiguous()
    if rows is not None and not (rows.dtype == torch.int64 and rows.is_contiguous() and rows.numel() == n_pol):
        raise ValueError("rows must be a contiguous int64 tensor with one entry per policy row")
    if d_pred is None:
        d_pred = torch.empty(n, 1, dtype=torch.float32, device=dev)
    if d_mean is None:
        d_mean = torch.empty(n_pol, A, dtype=torch.float32, device=dev)
    d_ls = torch.empty(1, A, dtype=torch.float32, device=dev) if want_d_log_std else None
    losses = losses_out if losses_out is not None else torch.empty(2, dtype=torch.float64, device=dev)
    ws = _zeroed_workspace("ppo_loss", lib.egp_ppo_loss_workspace_bytes(n, n_pol, A), dev)
    d = L.PpoLossDesc()
    d.n, d.n_pol, d.act_dim = n, n_pol, A
    d.rows = rows.data_ptr() if rows is not None else None
    d.pred, d.returns = pred1.data_ptr(), ret1.data_ptr()
    d.mean, d.ld_mean = mean.data_ptr(), mean.stride(0) if n_pol > 1 else A
    d.actions, d.ld_act = actions.data_ptr(), actions.stride(0) if n > 1 else A
    d.log_std, d.adv = ls.data_ptr(), adv1.data_ptr()
    d.fixed_logp, d.write_fixed = fixed_logp.data_ptr(), 1 if write_fixed else 0
    d.clip_eps, d.inv_n_val, d.inv_n_exp = float(clip_eps), 1.0 / max(float(n_val), 1.0), 1.0 / max(float(n_exp), 1.0)
    d.d_pred = d_pred.data_ptr()
    d.d_mean, d.ld_dmean = d_mean.data_ptr(), d_mean.stride(0) if n_pol > 1 else A
    d.d_log_std = d_ls.data_ptr() if d_ls is not None else None
    d.losses, d.workspace = losses.data_ptr(), ws.data_ptr()
    L.check(lib.egp_ppo_loss_f32(C.byref(d), L.current_stream()), "egp_ppo_loss_f32")
    return losses, d_pred, d_mean, d_ls


def ppo_stats(pred, returns, mean, actions, log_std, adv, fixed_logp, clip_eps, rows=None, out=None, logp_out=None):
    """-> the update monitor's record: float64[len(L.PPO_STATS_FIELDS)] on the device (`out`, or a new tensor), RAW sums over
    this rank's rows from one `egp_ppo_stats_f32` call on the tensors an epoch hands to `ppo_losses` (same shapes and `rows`;
    the layout is the header's, index by L.PPO_STATS[name]). `logp_out` (n_pol,) float32 receives the log-probabilities. Nothing
    is read back; `stats_summary` turns the record of one rank, or those of several, into the figures."""
    lib = L.load()
    n, n_pol, A = pred.shape[0], mean.shape[0], mean.shape[1]
    dev = pred.device
    pred1, ret1, adv1 = pred.reshape(-1), returns.reshape(-1), adv.reshape(-1)
    for name, t, want in (("pred", pred1, n), ("returns", ret1, n), ("adv", adv1, n), ("fixed_logp", fixed_logp, n_pol)):
        _f32_vector(name, t, want)
    if not (mean.is_cuda and mean.dtype == torch.float32 and mean.dim() == 2 and mean.stride(1) == 1 and (n_pol <= 1 or mean.stride(0) >= A)):
        raise ValueError("mean must be (n_pol, act_dim) float32 on the HIP device with unit column stride")
    if not (actions.is_cuda and actions.dtype == torch.float32 and actions.dim() == 2 and actions.stride(1) == 1 and actions.shape == (n, A)
            and (n <= 1 or actions.stride(0) >= A)):
        raise ValueError("actions must be (n, act_dim) float32 with unit column stride")
    if not (log_std.is_cuda and log_std.dtype == torch.float32 and log_std.numel() == A):
        raise ValueError("log_std must hold act_dim float32 values on the HIP device")
    ls = log_std.reshape(-1).contiguous()
    if rows is None and n_pol != n:
        raise ValueError("without rows every sample is a policy row: mean must have one row per sample")
    if rows is not None and not (rows.is_cuda and rows.dtype == torch.int64 and rows.is_contiguous() and rows.numel() == n_pol):
        raise ValueError("rows must be a contiguous int64 tensor with one entry per policy row")
    if logp_out is not None:
        _f32_vector("logp_out", logp_out, n_pol)
    F = len(L.PPO_STATS_FIELDS)
    rec = out if out is not None else torch.empty(F, dtype=torch.float64, device=dev)
    if not (rec.is_cuda and rec.dtype == torch.float64 and rec.is_contiguous() and rec.numel() == F):
        raise ValueError("out must be a contiguous float64 HIP tensor of %d elements" % F)
    ws = _zeroed_workspace("ppo_stats", lib.egp_ppo_stats_workspace_bytes(n, n_pol, A), dev)     # (per stream; every partial is written before it is read)
    d = L.PpoStatsDesc()
    d.n, d.n_pol, d.act_dim = n, n_pol, A
    d.rows = rows.data_ptr() if rows is not None else None
    d.pred, d.returns = pred1.data_ptr(), ret1.data_ptr()
    d.mean, d.ld_mean = mean.data_ptr(), mean.stride(0) if n_pol > 1 else A
    d.actions, d.ld_act = actions.data_ptr(), actions.stride(0) if n > 1 else A
    d.log_std, d.adv, d.fixed_logp = ls.data_ptr(), adv1.data_ptr(), fixed_logp.data_ptr()
    d.clip_eps = float(clip_eps)
    d.logp_out = logp_out.data_ptr() if logp_out is not None else None
    d.record, d.workspace = rec.data_ptr(), ws.data_ptr()
    L.check(lib.egp_ppo_stats_f32(C.byref(d), L.current_stream()), "egp_ppo_stats_f32")
    return rec


def ppo_stats_torch(pred, returns, mean, actions, log_std, adv, fixed_logp, clip_eps, rows=None, out=None, logp_out=None, logp=None):
    """`ppo_stats` in plain torch ops on any device and dtype: the record's definitions, and what the non-fused update path
    evaluates. The log-probabilities come from `mean`, `actions[rows]` and `log_std` with the reference's formula
    (core/distributions.py:6-25 over utils/math.py:14-17) in the inputs' dtype -- or are `logp` (n_pol,) / (n_pol, 1) when the
    caller has them (then `mean` / `actions` may be None); the log-ratio is formed in that dtype, everything after it in float64.
    -> float64[len(L.PPO_STATS_FIELDS)] on the inputs' device."""
    with torch.no_grad():
        pred1, ret1, adv1 = pred.reshape(-1), returns.reshape(-1), adv.reshape(-1)
        ls = log_std.reshape(-1) if log_std is not None else None       # (None: a policy without a Gaussian head -- entropy NaN)
        if logp is None:
            act = actions if rows is None else actions[rows]
            var = torch.exp(ls * 2.0)
            logp = (-(act - mean).pow(2) / (2.0 * var) - 0.5 * math.log(2.0 * math.pi) - ls).sum(1)
        logp = logp.reshape(-1)
        if logp_out is not None:
            logp_out.copy_(logp)
        n, n_pol = pred1.shape[0], logp.shape[0]
        lr = (logp - fixed_logp.reshape(-1)).double()
        r = torch.exp(lr)
        y, d = ret1.double(), ret1.double() - pred1.double()
        bad = ~(torch.isfinite(pred1) & torch.isfinite(ret1))
        pol_bad = ~(torch.isfinite(adv1 if rows is None else adv1[rows]) & torch.isfinite(logp))
        if rows is None:
            bad = bad | pol_bad
        else:
            bad = bad.index_put((rows,), pol_bad, accumulate=False) | bad
        seen = r[~torch.isnan(r)]                       # (the kernel's fmin / fmax skip NaN ratios)
        inf = torch.tensor(float("inf"), dtype=torch.float64, device=pred.device)
        rec = torch.stack([
            torch.tensor(float(n_pol), dtype=torch.float64, device=pred.device),
            (-lr).sum(), (torch.expm1(lr) - lr).sum(), ((r - 1.0).abs() > float(clip_eps)).sum().double(),
            seen.min() if seen.numel() else inf, seen.max() if seen.numel() else -inf,
            torch.tensor(float(n), dtype=torch.float64, device=pred.device),
            y.sum(), (y * y).sum(), d.sum(), (d * d).sum(), bad.sum().double(),
            ls.double().sum() + 0.5 * ls.shape[0] * (1.0 + math.log(2.0 * math.pi)) if ls is not None else -inf * 0.0])
        if out is not None:
            out.copy_(rec)
            return out
        return rec


def stats_summary(records):
    """Host side of the update monitor: one record (13 numbers: a list, an array or a tensor) or the records of several ranks
    (a sequence of them, or a 2-d tensor) -> dict of the derived figures. Ranks combine by adding the sums and counts and taking
    the min / max of the ratio range (the entropy is every rank's own copy of the same number: the first is taken).
      approx_kl (k3 mean), approx_kl_k1, clip_frac, ratio_min, ratio_max   over the policy rows
      explained_var = 1 - Var(d) / Var(y), population variances of y = returns and d = returns - pred
      entropy, nonfinite_rows
    Means over zero rows are NaN."""
    if torch.is_tensor(records):
        records = records.detach().cpu().tolist()
    rows = [list(map(float, records))] if len(records) and not hasattr(records[0], "__len__") else [list(map(float, r)) for r in records]
    I = L.PPO_STATS
    tot = lambda k: sum(r[I[k]] for r in rows)             # (rank order: every rank that combines the same records gets the same bits)
    nan = float("nan")
    n_pol, n = tot("n_pol"), tot("n")
    mean_pol = lambda k: tot(k) / n_pol if n_pol > 0 else nan
    if n > 0:
        my, md = tot("sum_y") / n, tot("sum_d") / n
        var_y, var_d = tot("sum_yy") / n - my * my, tot("sum_dd") / n - md * md
        ev = 1.0 - var_d / var_y if var_y != 0 else nan
    else:
        ev = nan
    return {"approx_kl": mean_pol("k3"), "approx_kl_k1": mean_pol("k1"), "clip_frac": mean_pol("clipped"),
            "ratio_min": min(r[I["ratio_min"]] for r in rows), "ratio_max": max(r[I["ratio_max"]] for r in rows),
            "explained_var": ev, "entropy": rows[0][I["entropy"]], "nonfinite_rows": int(tot("nonfinite"))}


STATS_KEYS = ("approx_kl", "approx_kl_k1", "clip_frac", "ratio_min", "ratio_max", "explained_var", "entropy", "nonfinite_rows")


def _f32_vector(name, t, want):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == want):
        raise ValueError("%s must be a contiguous float32 HIP tensor of %d elements" % (name, want))
    return t


def _f32_rows(name, t, n, width=None):
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] == n and (width is None or t.shape[1] == width)
            and t.shape[1] >= 1 and t.stride(1) == 1 and (n <= 1 or t.stride(0) >= t.shape[1])):
        raise ValueError("%s must be (%d, %s) float32 on the HIP device with unit column stride" % (name, n, "width" if width is None else width))
    return t


def minibatch_plan(states, actions, returns, adv, fixed_logp, exps, perm, batch, out=None, mb_n_exp=None):
    """-> (out, mb_n_exp). `out` = the six columns with row r taken from source row perm[r] (dense float32 buffers of the sources'
    shapes, allocated here unless given); mb_n_exp int32[ceil(N / batch)] = rows with exps != 0 in every window of `batch` rows.
    `perm`: int64 permutation of 0 .. N-1 on the device. One launch; nothing is read back."""
    lib = L.load()
    N = states.shape[0]
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be >= 1")
    _f32_rows("states", states, N)
    _f32_rows("actions", actions, N)
    cols = [states, actions] + [_f32_vector(k, t.reshape(-1), N) for k, t in (("returns", returns), ("adv", adv), ("fixed_logp", fixed_logp), ("exps", exps))]
    if not (perm.is_cuda and perm.dtype == torch.int64 and perm.is_contiguous() and perm.numel() == N):
        raise ValueError("perm must be a contiguous int64 HIP tensor with one entry per row")
    dev = states.device
    n_win = (N + batch - 1) // batch
    if out is None:
        out = [torch.empty(c.shape, dtype=torch.float32, device=dev) for c in (states, actions, returns, adv, fixed_logp, exps)]
    if len(out) != 6:
        raise ValueError("out must hold six destination buffers")
    for c, o in zip(cols, out):
        if not (o.is_cuda and o.dtype == torch.float32 and o.is_contiguous() and o.numel() == c.numel()) or o.data_ptr() == c.data_ptr() and N > 0:
            raise ValueError("every destination must be a contiguous float32 HIP buffer of its source's size, distinct from it")
    if mb_n_exp is None:
        mb_n_exp = torch.empty(n_win, dtype=torch.int32, device=dev)
    if not (mb_n_exp.is_cuda and mb_n_exp.dtype == torch.int32 and mb_n_exp.is_contiguous() and mb_n_exp.numel() == n_win):
        raise ValueError("mb_n_exp must be a contiguous int32 HIP tensor of %d elements" % n_win)
    d = L.MinibatchPlanDesc()
    d.n, d.state_dim, d.act_dim, d.batch = N, states.shape[1], actions.shape[1], batch
    d.perm = perm.data_ptr()
    d.states, d.ld_states = states.data_ptr(), states.stride(0) if N > 1 else states.shape[1]
    d.actions, d.ld_act = actions.data_ptr(), actions.stride(0) if N > 1 else actions.shape[1]
    d.returns, d.adv, d.fixed_logp, d.exps = (c.data_ptr() for c in cols[2:])
    d.out_states, d.out_actions, d.out_returns, d.out_adv, d.out_fixed_logp, d.out_exps = (o.data_ptr() for o in out)
    d.mb_n_exp = mb_n_exp.data_ptr()
    L.check(lib.egp_minibatch_plan_f32(C.byref(d), L.current_stream()), "egp_minibatch_plan_f32")
    return out, mb_n_exp


def ppo_losses_mb(pred, returns, mean, actions, log_std, adv, fixed_logp, exps, n_exp, clip_eps, d_pred=None, d_mean=None,
                  want_d_log_std=False, losses_out=None):
    """-> (losses float64[2] on the device, d_pred (n, 1), d_mean (n, A), d_log_std (1, A) or None) of one window of n rows.
    `mean` covers EVERY row of the window; `exps` (n,) marks the exploration rows, `n_exp` is the int32 device tensor of one
    element that holds their number (the window's entry of minibatch_plan's mb_n_exp). No host read, no data-dependent shape."""
    lib = L.load()
    n, A = mean.shape[0], mean.shape[1]
    if not 1 <= n <= L.PPO_LOSS_MB_MAX_ROWS:
        raise ValueError("a window has 1 .. %d rows, got %d" % (L.PPO_LOSS_MB_MAX_ROWS, n))
    dev = pred.device
    pred1, ret1, adv1, fix1, exp1 = (_f32_vector(k, t.reshape(-1), n) for k, t in
                                     (("pred", pred), ("returns", returns), ("adv", adv), ("fixed_logp", fixed_logp), ("exps", exps)))
    _f32_rows("mean", mean, n)
    _f32_rows("actions", actions, n, A)
    if not (log_std.is_cuda and log_std.dtype == torch.float32 and log_std.numel() == A and A <= 256):
        raise ValueError("log_std must hold act_dim <= 256 float32 values on the HIP device")
    if not (n_exp.is_cuda and n_exp.dtype == torch.int32 and n_exp.numel() == 1):
        raise ValueError("n_exp must be an int32 HIP tensor of one element")
    ls = log_std.reshape(-1).contiguous()
    if d_pred is None:
        d_pred = torch.empty(n, 1, dtype=torch.float32, device=dev)
    if d_mean is None:
        d_mean = torch.empty(n, A, dtype=torch.float32, device=dev)
    _f32_vector("d_pred", d_pred.reshape(-1), n)
    _f32_rows("d_mean", d_mean, n, A)
    d_ls = torch.empty(1, A, dtype=torch.float32, device=dev) if want_d_log_std else None
    losses = losses_out if losses_out is not None else torch.empty(2, dtype=torch.float64, device=dev)
    if not (losses.is_cuda and losses.dtype == torch.float64 and losses.is_contiguous() and losses.numel() == 2):
        raise ValueError("losses_out must be a contiguous float64 HIP tensor of 2 elements")
    d = L.PpoLossMbDesc()
    d.n, d.act_dim = n, A
    d.pred, d.returns = pred1.data_ptr(), ret1.data_ptr()
    d.mean, d.ld_mean = mean.data_ptr(), mean.stride(0) if n > 1 else A
    d.actions, d.ld_act = actions.data_ptr(), actions.stride(0) if n > 1 else A
    d.log_std = ls.data_ptr()
    d.adv, d.fixed_logp, d.exps = adv1.data_ptr(), fix1.data_ptr(), exp1.data_ptr()
    d.n_exp = n_exp.data_ptr()
    d.clip_eps = float(clip_eps)
    d.d_pred = d_pred.data_ptr()
    d.d_mean, d.ld_dmean = d_mean.data_ptr(), d_mean.stride(0) if n > 1 else A
    d.d_log_std = d_ls.data_ptr() if d_ls is not None else None
    d.losses = losses.data_ptr()
    L.check(lib.egp_ppo_loss_mb_f32(C.byref(d), L.current_stream()), "egp_ppo_loss_mb_f32")
    return losses, d_pred, d_mean, d_ls


def _gail_rows_desc(n, H, idx, ctx_rows, ld_ctx, ldo):
    if not (idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous() and idx.numel() == n):
        raise ValueError("idx must be a contiguous int64 HIP tensor with one entry per sample")
    d = L.GailRowsDesc()
    d.n, d.H, d.idx, d.ctx_rows, d.ld_ctx, d.ldo = n, H, idx.data_ptr(), ctx_rows, ld_ctx, ldo
    return d


def gail_rows(ctx2d, idx, x, tab, src, mean=None, inv_std=None, out=None, src_host=None):
    """-> X (2n, H + S) float32: rows [0, n) = [ctx2d[idx[i]] | x[i]], rows [n, 2n) = [ctx2d[idx[i]] | (tab[src[i]] - mean) * inv_std]
    (`egp_gail_rows_f32`; mean = inv_std = None: the table rows as they are). `src_host`: the values of `src` on the host (a
    NumPy int64 array), when the caller has them -- an entry that is no row of `tab` then raises ValueError before the launch."""
    n, H, S = idx.shape[0], ctx2d.shape[1], x.shape[1]
    _f32_rows("ctx2d", ctx2d, ctx2d.shape[0])
    _f32_rows("x", x, n)
    _f32_rows("tab", tab, tab.shape[0], S)
    if (mean is None) != (inv_std is None):
        raise ValueError("mean and inv_std go together")
    for k, t in (("mean", mean), ("inv_std", inv_std)):
        if t is not None:
            _f32_vector(k, t, S)
    if not (src.is_cuda and src.dtype == torch.int64 and src.is_contiguous() and src.numel() == n):
        raise ValueError("src must be a contiguous int64 HIP tensor with one entry per sample")
    if out is None:
        out = torch.empty(2 * n, H + S, dtype=torch.float32, device=x.device)
    _f32_rows("out", out, 2 * n, H + S)
    d = _gail_rows_desc(n, H, idx, ctx2d.shape[0], ctx2d.stride(0) if ctx2d.shape[0] > 1 else H, out.stride(0) if n > 0 else H + S)
    d.S = S
    d.ctx = ctx2d.data_ptr()
    d.x, d.ldx = x.data_ptr(), x.stride(0) if n > 1 else S
    d.tab, d.ld_tab, d.tab_rows = tab.data_ptr(), tab.stride(0) if tab.shape[0] > 1 else S, tab.shape[0]
    d.src = src.data_ptr()
    if src_host is not None:
        import numpy as np
        src_host = np.ascontiguousarray(src_host, dtype=np.int64)
        if src_host.shape != (n,):
            raise ValueError("src_host must hold one entry per sample")
        d.src_host = src_host.ctypes.data
    if mean is not None:
        d.mean, d.inv_std = mean.data_ptr(), inv_std.data_ptr()
    d.out = out.data_ptr()
    L.check(L.load().egp_gail_rows_f32(C.byref(d), L.current_stream()), "egp_gail_rows_f32")
    return out


def gail_rows_bwd(dout, idx, ctx_shape):
    """-> dctx (ctx_shape) float32: zero, except dctx[idx[i]] = dout[i, :H] + dout[n + i, :H] (`egp_gail_rows_bwd_f32`; idx distinct)."""
    n = idx.shape[0]
    R, H = ctx_shape
    _f32_rows("dout", dout, 2 * n)
    if dout.shape[1] < H:
        raise ValueError("dout has fewer columns than the context")
    dctx = torch.zeros(R, H, dtype=torch.float32, device=dout.device)
    d = _gail_rows_desc(n, H, idx, R, H, dout.stride(0) if n > 0 else dout.shape[1])
    d.dout, d.dctx = dout.data_ptr(), dctx.data_ptr()
    L.check(L.load().egp_gail_rows_bwd_f32(C.byref(d), L.current_stream()), "egp_gail_rows_bwd_f32")
    return dctx


class GailRows(torch.autograd.Function):
    """gail_rows as an autograd node: gradient to the context only (the states and the expert table need none)."""

    @staticmethod
    def forward(ctx, ctx2d, idx, x, tab, src, mean, inv_std):
        ctx.save_for_backward(idx)
        ctx.shape = tuple(ctx2d.shape)
        return gail_rows(ctx2d, idx, x, tab, src, mean, inv_std)

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        dout = dout if dout.stride(1) == 1 else dout.contiguous()
        return (gail_rows_bwd(dout, idx, ctx.shape),) + (None,) * 6


def bce_logits(z, n_g, n_e, dz=None, want_dz=True, want_score=False, losses_out=None, expert_rows=None):
    """-> (losses float64[2] on the device = generated, expert; dz (2n, 1) or None; score (n,) or None) for the logits z (2n, 1) of
    a [generated; expert] block (`egp_bce_logits_f32`). n_g / n_e: the GLOBAL row counts the two means divide by."""
    lib = L.load()
    if expert_rows is None and z.numel() % 2:
        raise ValueError("z holds the logits of n generated rows followed by n expert rows")
    rows_e = z.numel() // 2 if expert_rows is None else int(expert_rows)
    n = z.numel() - rows_e
    z1 = _f32_vector("z", z.reshape(-1), n + rows_e)
    dev = z.device
    if want_dz:
        dz = torch.empty(n + rows_e, 1, dtype=torch.float32, device=dev) if dz is None else dz
        _f32_vector("dz", dz.reshape(-1), n + rows_e)
    else:
        dz = None
    score = torch.empty(n, dtype=torch.float32, device=dev) if want_score else None
    losses = losses_out if losses_out is not None else torch.empty(2, dtype=torch.float64, device=dev)
    if not (losses.is_cuda and losses.dtype == torch.float64 and losses.is_contiguous() and losses.numel() == 2):
        raise ValueError("losses_out must be a contiguous float64 HIP tensor of 2 elements")
    ws = _zeroed_workspace("bce_logits", lib.egp_bce_logits_workspace_bytes(n), dev)
    d = L.BceLogitsDesc()
    d.n, d.n_e, d.z = n, rows_e, z1.data_ptr()
    d.inv_n_g, d.inv_n_e = 1.0 / max(float(n_g), 1.0), 1.0 / max(float(n_e), 1.0)
    d.dz = dz.data_ptr() if dz is not None else None
    d.score_out = score.data_ptr() if score is not None else None
    d.losses, d.workspace = losses.data_ptr(), ws.data_ptr()
    L.check(lib.egp_bce_logits_f32(C.byref(d), L.current_stream()), "egp_bce_logits_f32")
    return losses, dz, score


def bce_scores(z):
    """-> softplus(-z) = -log sigmoid(z) per row, (n,) float32: a score-only call of `egp_bce_logits_f32` (no expert rows, no dz)."""
    return bce_logits(z, z.numel(), 1, want_dz=False, want_score=True, expert_rows=0)[2]


class FlatUpdater:
    """Flat storage + fused clip / Adam step for the parameter groups of `optimizers` (stepped in that order, all at once).

    `clip`: AgentPPO.policy_grad_clip -- [(params, max_norm), ...]. `compute_of`: {master parameter: float32 compute copy} when
    the optimizers own float64 master modules (agent.ShadowNets), else None (the optimizers' parameters compute themselves)."""

    @staticmethod
    def build(optimizers, clip, compute_of=None):
        """A FlatUpdater, or None when this set-up is not the one the kernels implement (the caller then keeps torch's path)."""
        try:
            return FlatUpdater(optimizers, clip, compute_of)
        except _NotEligible:
            return None

    def __init__(self, optimizers, clip, compute_of=None):
        self.optimizers = list(optimizers)
        self.lib = L.load()
        clip = list(clip or [])
        self.n_clip = len(clip)
        clip_of = {}
        for gi, (params, max_norm) in enumerate(clip, start=1):
            for p in params:
                if id(p) in clip_of:
                    raise _NotEligible("a parameter sits in two clip lists")
                clip_of[id(p)] = (gi, float(max_norm))
        self.entries = []            # (optimizer index, group index, master param, clip group, max_norm)
        for oi, opt in enumerate(self.optimizers):
            if type(opt) is not torch.optim.Adam:
                raise _NotEligible("not torch.optim.Adam")
            for gi, g in enumerate(opt.param_groups):
                if g.get("amsgrad") or g.get("maximize") or g.get("differentiable") or g.get("capturable"):
                    raise _NotEligible("Adam variant")
                for p in g["params"]:
                    if p.requires_grad:
                        cg, mn = clip_of.get(id(p), (0, 0.0))
                        self.entries.append((oi, gi, p, cg, mn))
        if not self.entries:
            raise _NotEligible("nothing to train")
        masters = [e[2] for e in self.entries]
        dev, mdt = masters[0].device, masters[0].dtype
        if dev.type != "cuda" or mdt not in (torch.float32, torch.float64) or any(p.device != dev or p.dtype != mdt for p in masters):
            raise _NotEligible("parameters must be float32 / float64 on one HIP device")
        if len({id(p) for p in masters}) != len(masters):
            raise _NotEligible("a parameter is owned by two groups")
        self.compute = [compute_of[p] if compute_of is not None else p for p in masters]
        cdt = self.compute[0].dtype
        if any(c.dtype != cdt or c.device != dev or c.shape != p.shape for c, p in zip(self.compute, masters)):
            raise _NotEligible("compute copies do not match their masters")
        if (mdt, cdt) not in ((torch.float32, torch.float32), (torch.float64, torch.float32), (torch.float64, torch.float64)):
            raise _NotEligible("unsupported dtype pair")
        if compute_of is None and cdt != mdt:
            raise _NotEligible("dtype pair without compute copies")
        self.device, self.mdt, self.cdt = dev, mdt, cdt
        self.shadowed = compute_of is not None
        # segments: maximal runs of consecutive parameters with the same (optimizer, group, clip group)
        self.offsets, pos = [], 0
        self.segments = []           # [begin, end, optimizer index, group index, clip group, max_norm]
        for oi, gi, p, cg, mn in self.entries:
            self.offsets.append(pos)
            if self.segments and self.segments[-1][2:5] == [oi, gi, cg]:
                self.segments[-1][1] = pos + p.numel()
            else:
                self.segments.append([pos, pos + p.numel(), oi, gi, cg, mn])
            pos += p.numel()
        self.numel = pos
        if len(self.segments) > L.ADAM_MAX_SEGMENTS:
            raise _NotEligible("more parameter segments than the kernel takes")
        mk = lambda dt: torch.zeros(self.numel, dtype=dt, device=dev)
        self.P, self.M, self.V = mk(mdt), mk(mdt), mk(mdt)
        self.G = mk(cdt)                                         # gradients of the compute parameters = the all-reduce buffer
        self.S = mk(torch.float32) if self.shadowed else None    # float32 compute copies of float64 masters
        self.steps = [0] * len(self.optimizers)
        self.time_collectives, self.collective_events = False, []
        # what the optimizers' state shows as `step`: a tensor of its OWN per parameter (torch's optimizer.step() increments every
        # state["step"] it finds -- one shared tensor per optimizer would be incremented once per parameter)
        self.step_tensors = [torch.tensor(0.0) for _ in self.entries]
        self._views = lambda flat: [flat[o:o + p.numel()].view_as(p) for o, p in zip(self.offsets, masters)]
        self.p_views, self.m_views, self.v_views, self.g_views = (self._views(f) for f in (self.P, self.M, self.V, self.G))
        self.s_views = self._views(self.S) if self.shadowed else None
        self.ws = torch.empty(int(self.lib.egp_adam_workspace_bytes()), dtype=torch.uint8, device=dev)
        self.norms = torch.zeros(L.ADAM_MAX_SEGMENTS + 1, dtype=torch.float64, device=dev)
        # moments the optimizers may already hold (a resumed run) move into the flat buffers; from now on the optimizers' state
        # entries ARE views of them
        with torch.no_grad():
            for k, (oi, gi, p, _, _) in enumerate(self.entries):
                st = self.optimizers[oi].state.get(p)
                if st and "exp_avg" in st:
                    self.m_views[k].copy_(st["exp_avg"])
                    self.v_views[k].copy_(st["exp_avg_sq"])
                    self.steps[oi] = max(self.steps[oi], int(float(st["step"])))
        self.rebind()
        self._publish_state()

    # ---------------------------------------------------------------------------------------------- storage
    def _aliases(self, p, view):
        return p.data_ptr() == view.data_ptr() and p.device == view.device and p.dtype == view.dtype and p.is_contiguous()

    @torch.no_grad()
    def rebind(self):
        """Make every parameter a view of its flat buffer again. Cheap when nothing happened; needed after a caller replaced
        the storage of its modules (`module.to(...)`, the driver's `with to_cpu(...)` around a checkpoint)."""
        for k, (_, _, p, _, _) in enumerate(self.entries):
            if not self._aliases(p, self.p_views[k]):
                self.p_views[k].copy_(p.data)
                p.data = self.p_views[k]
            if self.shadowed:
                c = self.compute[k]
                if not self._aliases(c, self.s_views[k]):
                    self.s_views[k].copy_(p.data)
                    c.data = self.s_views[k]

    def _publish_state(self):
        for k, (oi, gi, p, _, _) in enumerate(self.entries):
            self.step_tensors[k].fill_(float(self.steps[oi]))
            self.optimizers[oi].state[p] = {"step": self.step_tensors[k], "exp_avg": self.m_views[k], "exp_avg_sq": self.v_views[k]}

    # ---------------------------------------------------------------------------------------------- one epoch
    def zero_grad(self):
        for c in self.compute:
            c.grad = None
        if self.shadowed:
            for _, _, p, _, _ in self.entries:
                p.grad = None

    @torch.no_grad()
    def collect_grads(self, which=None):
        """compute parameters' .grad -> the flat gradient buffer (one multi-tensor copy)."""
        dst, src = [], []
        for k, (oi, _, _, _, _) in enumerate(self.entries):
            if which is not None and oi not in which:
                continue
            g = self.compute[k].grad
            if g is None:
                raise RuntimeError("parameter %d of optimizer %d received no gradient: the fused step updates every parameter of the "
                                   "optimizers it serves" % (k, oi))
            dst.append(self.g_views[k])
            src.append(g)
        if dst:
            torch._foreach_copy_(dst, src)

    def all_reduce(self, which=None):
        """SUM over ranks of the flat gradient (the span of the optimizers in `which`): each rank already divided its losses by
        the GLOBAL counts. The buffer autograd's results were gathered into IS the collective's buffer."""
        if not D.is_on():
            return
        spans = [(b, e) for b, e, oi, _, _, _ in self.segments if which is None or oi in which]
        if not spans:
            return
        G = self.G[min(b for b, _ in spans):max(e for _, e in spans)]
        dev = D._comm_device(self.device)
        ev = None
        if self.time_collectives:           # HIP events around the collective (bench.py --gpus N: allreduce_ms_per_epoch)
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        D._note()
        if dev == G.device:
            torch.distributed.all_reduce(G)
        else:
            tmp = G.to(dev)
            torch.distributed.all_reduce(tmp)
            G.copy_(tmp)
        if ev is not None:
            ev[1].record()
            self.collective_events.append(ev)

    def collective_ms(self):
        """[ms] of every timed gradient all-reduce since the last call (synchronises)."""
        if not self.collective_events:
            return []
        torch.cuda.synchronize(self.device)
        out = [a.elapsed_time(b) for a, b in self.collective_events]
        self.collective_events = []
        return out

    def step(self, which=None):
        """Clip + Adam for the optimizers in `which` (indices; None = all), hyper-parameters read from their param_groups now."""
        which = set(range(len(self.optimizers))) if which is None else set(which)
        for oi in which:
            self.steps[oi] += 1
        segs = (L.AdamSegment * L.ADAM_MAX_SEGMENTS)()
        n = 0
        for b, e, oi, gi, cg, mn in self.segments:
            if oi not in which:
                continue
            g = self.optimizers[oi].param_groups[gi]
            t = self.steps[oi]
            b1, b2 = g["betas"]
            s = segs[n]
            s.begin, s.end = b, e
            s.lr, s.beta1, s.beta2, s.eps, s.weight_decay = float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"])
            s.bias1, s.bias2 = 1.0 - float(b1) ** t, 1.0 - float(b2) ** t
            s.max_norm, s.clip_group = float(mn), int(cg)
            n += 1
        st = L.current_stream(self.device.index)
        ptr = lambda t: t.data_ptr() if t is not None else None
        if self.mdt == torch.float32:
            rc = self.lib.egp_adam_step_f32(n, segs, ptr(self.G), ptr(self.P), ptr(self.M), ptr(self.V), ptr(self.ws), ptr(self.norms), st)
        elif self.cdt == torch.float32:
            rc = self.lib.egp_adam_step_f64(n, segs, ptr(self.G), ptr(self.P), ptr(self.M), ptr(self.V), ptr(self.S), ptr(self.ws), ptr(self.norms), st)
        else:
            rc = self.lib.egp_adam_step_f64g(n, segs, ptr(self.G), ptr(self.P), ptr(self.M), ptr(self.V), ptr(self.ws), ptr(self.norms), st)
        L.check(rc, "egp_adam_step")
        for k, (oi, _, _, _, _) in enumerate(self.entries):
            if oi in which:
                self.step_tensors[k].fill_(float(self.steps[oi]))

    def grad_norm(self, group):
        """Gradient norm of clip group `group` (1 = the first entry of `clip`) at the last step, before the clip: a 0-d device
        tensor (no host read), or None when there is no such group."""
        return self.norms[group] if 1 <= group <= self.n_clip else None


class _NotEligible(Exception):
    pass


class TorchUpdater:
    """FlatUpdater's calls over the caller's own optimizers, which step themselves (any device, dtype and optimizer class).

    `shadow`: agent.ShadowNets when the optimizers own float64 masters of float32 compute copies, else None. `pre_step`:
    {optimizer index: callable run immediately before that optimizer's step()} -- the gradient clip; what it returned last is
    `grad_norm(k)` for the k-th entry (from 1, as FlatUpdater numbers its clip groups). With more than one rank the gradients of
    all the optimizers' parameters live in one dist.FlatGradSync buffer, built by the first zero_grad() (so before the first
    step), which from then on attaches that buffer instead of clearing the gradients."""

    def __init__(self, optimizers, shadow=None, pre_step=None):
        self.optimizers, self.shadow, self.pre_step = list(optimizers), shadow, dict(pre_step or {})
        self.sync = None
        self.returned = {}

    def _get_sync(self):
        if self.sync is None and D.world_size() > 1:
            self.sync = D.FlatGradSync([p for opt in self.optimizers for g in opt.param_groups for p in g["params"]])
        return self.sync

    def zero_grad(self):
        sync = self._get_sync()
        if sync is not None:
            sync.attach()            # gradients accumulate inside the all-reduce buffer (p.grad = its views)
        else:
            for opt in self.optimizers:
                opt.zero_grad()
        if self.shadow is not None:
            self.shadow.zero_grad()

    def collect_grads(self, which=None):
        """The compute copies' gradients -> the .grad of the parameters the optimizers own."""
        if self.shadow is not None:
            self.shadow.push_grads()

    def all_reduce(self, which=None):
        """SUM over ranks of the whole buffer, whatever `which` says (each rank divided its losses by the GLOBAL counts)."""
        sync = self._get_sync()
        if sync is not None:
            sync.all_reduce()

    def step(self, which=None):
        for oi, opt in enumerate(self.optimizers):
            if which is None or oi in which:
                if oi in self.pre_step:
                    self.returned[oi] = self.pre_step[oi]()
                opt.step()
        if self.shadow is not None:
            self.shadow.pull()

    def rebind(self):
        return

    def grad_norm(self, group):
        keys = list(self.pre_step)
        return self.returned.get(keys[group - 1]) if 1 <= group <= len(keys) else None
