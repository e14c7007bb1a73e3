"""Joint-position metrics: how far the estimated BODY is from the MoCap body, in metres.

`metrics.compute_metrics` scores `qpos` rows (joint angles, velocities, accelerations); 0.1 rad at the hip and 0.1 rad at the wrist
are the same to it and very different to the body. Here a predicted row `P` and a MoCap row `G` (both `[nq]`) become body positions
`X = body_xpos(P)`, `Y = body_xpos(G)` (`[nbody][3]`, metres), and over the bodies `B` of a body mask (an int; bit b = body b counts;
default all bodies; at least 3, else ValueError) a frame gets

    g_mpjpe   mean over B of |X_b - Y_b|                        global, nothing aligned
    mpjpe     mean over B of |(X_b - X_0) - (Y_b - Y_0)|        root-relative; body 0 is the root whether or not its bit is set
    pa_mpjpe  mean over B of |s R (X_b - mx) + my - Y_b|        mx, my the centroids over B; (s, R) the least-squares similarity of
                                                                X onto Y over B with R a PROPER rotation -- a reflection is never
                                                                allowed: a mirrored pose must not score ~0
    root_err  |X_0 - Y_0|
    err[b]    |(X_b - X_0) - (Y_b - Y_0)| per body, 0 where the mask bit is clear (the per-joint table)

and a trajectory (`dt` between its frames) gets

    accel_err mean over frames 1..T-2 and B of |(X[t-1] - 2 X[t] + X[t+1]) - (Y[t-1] - 2 Y[t] + Y[t+1])| / dt^2, in m/s^2;
              nan for fewer than 3 frames, and such a trajectory is left out of the mean over takes (windows)

(MPJPE, root-relative MPJPE and Procrustes-aligned PA-MPJPE of the pose-estimation literature, and its acceleration error.)
`accel_err` is always host numpy on the positions: it needs neighbouring frames, the kernel's wavefront owns one frame, and both
backends share the function. Aggregation mirrors `metrics`: per take the mean over frames, then the mean over takes; for forecast
results the frames [m, m + horizon) of every window, the mean over a take's windows, then over takes. Values are metres; the
printed line is millimetres.

`score_xpos` is the numpy path from body POSITIONS (SVD with determinant correction for the similarity), `score_host` feeds it from
the skeleton's host forward kinematics (`Skeleton.body_xpos`), `score` hands all frames to ONE launch of `egp_pose3d_f64`
(csrc/egp_pose3d.hip: both forward kinematics, the sums and Horn's quaternion form of the similarity per frame, a wavefront each).
All three return the same dict of arrays. `backend='hip' | 'host'` is the caller's choice; nothing falls back.
"""
from __future__ import annotations

import numpy as np

HANDS = ("LeftHand", "RightHand")
FIGURES = ("g_mpjpe", "mpjpe", "pa_mpjpe", "root_err", "accel_err")


def body_mask(skel, exclude=()):
    """The mask of all bodies of `skel` but the named ones (e.g. `HANDS`) -> int."""
    names = list(skel.body_names)
    unknown = [n for n in exclude if n not in names]
    if unknown:
        raise ValueError("no such body: %s" % ", ".join(unknown))
    return sum(1 << b for b, n in enumerate(names) if n not in exclude)


def mask_bits(mask, nbody):
    """`mask` (None: all bodies) -> bool [nbody]; ValueError for bits at or above nbody or fewer than 3 bodies."""
    mask = (1 << nbody) - 1 if mask is None else int(mask)
    if mask < 0 or mask >> nbody:
        raise ValueError("body mask has bits at or above nbody = %d" % nbody)
    sel = np.array([(mask >> b) & 1 for b in range(nbody)], bool)
    if sel.sum() < 3:
        raise ValueError("body mask must select at least 3 bodies (a similarity needs them), got %d" % sel.sum())
    return sel


def similarity(xc, yc):
    """Least-squares (s, R), R proper, of the centred set xc [k][3] onto yc [k][3]: SVD of the cross-covariance with the
    determinant correction (Umeyama 1991). A set that equals its target needs no fit: s = 1, R = I exactly."""
    if np.array_equal(xc, yc):
        return 1.0, np.eye(3)
    U, sv, Vt = np.linalg.svd(xc.T @ yc)
    d = 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0
    D = np.array([1.0, 1.0, d])
    return float((sv * D).sum() / (xc * xc).sum()), (Vt.T * D) @ U.T


def score_xpos(xpos_pred, xpos_gt, mask=None):
    """Body positions [n][nbody][3] of both sides -> dict(g_mpjpe, mpjpe, pa_mpjpe, root_err [n], err [n][nbody], xpos_pred, xpos_gt)."""
    X, Y = np.asarray(xpos_pred, float), np.asarray(xpos_gt, float)
    if X.shape != Y.shape or X.ndim != 3 or X.shape[2] != 3:
        raise ValueError("positions must be two [n][nbody][3] arrays of one shape, got %s and %s" % (X.shape, Y.shape))
    n, nbody = X.shape[:2]
    sel = mask_bits(mask, nbody)
    rel = np.linalg.norm((X - X[:, :1]) - (Y - Y[:, :1]), axis=2)
    out = dict(g_mpjpe=np.linalg.norm(X - Y, axis=2)[:, sel].mean(1) if n else np.zeros(0), mpjpe=rel[:, sel].mean(1) if n else np.zeros(0),
               pa_mpjpe=np.zeros(n), root_err=np.linalg.norm(X[:, 0] - Y[:, 0], axis=1), err=np.where(sel[None, :], rel, 0.0),
               xpos_pred=X, xpos_gt=Y)
    for i in range(n):
        x, y = X[i, sel], Y[i, sel]
        xc, yc = x - x.mean(0), y - y.mean(0)
        s, R = similarity(xc, yc)
        out["pa_mpjpe"][i] = np.linalg.norm(s * xc @ R.T - yc, axis=1).mean()
    return out


def _rows(skel, qpos_pred, qpos_gt):
    qp, qg = np.asarray(qpos_pred, float), np.asarray(qpos_gt, float)
    if qp.shape != qg.shape or qp.ndim != 2 or qp.shape[1] != skel.nq:
        raise ValueError("qpos_pred and qpos_gt must both be [n][%d], got %s and %s" % (skel.nq, qp.shape, qg.shape))
    return qp, qg


def score_host(skel, qpos_pred, qpos_gt, mask=None):
    """The numpy path: host forward kinematics of every row, then `score_xpos`."""
    qp, qg = _rows(skel, qpos_pred, qpos_gt)
    nbody = len(skel.body_names)
    mask_bits(mask, nbody)
    fk = lambda q: np.stack([skel.body_xpos(r) for r in q]) if len(q) else np.zeros((0, nbody, 3))
    return score_xpos(fk(qp), fk(qg), mask)


def score(ctx, qpos_pred, qpos_gt, mask=None):
    """All frames in one launch of egp_pose3d_f64 on `ctx`'s device -> the dict of `score_xpos`, numpy."""
    import torch
    qp, qg = _rows(ctx.skel, qpos_pred, qpos_gt)
    nbody = len(ctx.skel.body_names)
    mask_bits(mask, nbody)
    n = len(qp)
    if n == 0:
        return score_xpos(np.zeros((0, nbody, 3)), np.zeros((0, nbody, 3)), mask)
    dev = torch.device("cuda", ctx.device)
    with torch.cuda.device(dev):
        d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
        r = ctx.pose3d(d(qp), d(qg), body_mask=mask, want_err=True, want_xpos=True)
        pf = r["per_frame"].cpu().numpy()
        return dict(g_mpjpe=pf[:, 0].copy(), mpjpe=pf[:, 1].copy(), pa_mpjpe=pf[:, 2].copy(), root_err=pf[:, 3].copy(), err=r["err"].cpu().numpy(),
                    xpos_pred=r["xpos_pred"].cpu().numpy(), xpos_gt=r["xpos_gt"].cpu().numpy())


def accel_err(xpos_pred, xpos_gt, dt, mask=None):
    """Mean acceleration error of one trajectory from its positions [T][nbody][3], m/s^2; nan for T < 3."""
    X, Y = np.asarray(xpos_pred, float), np.asarray(xpos_gt, float)
    if X.shape != Y.shape or X.ndim != 3:
        raise ValueError("positions must be two [T][nbody][3] arrays of one shape, got %s and %s" % (X.shape, Y.shape))
    sel = mask_bits(mask, X.shape[1])
    if X.shape[0] < 3:
        return float("nan")
    acc = lambda P: P[:-2] - 2.0 * P[1:-1] + P[2:]
    return float(np.linalg.norm(acc(X) - acc(Y), axis=2)[:, sel].mean() / (dt * dt))


def _score_all(skel, qpos_pred, qpos_gt, mask, backend, ctx, cfg, device_index):
    if backend not in ("hip", "host"):
        raise ValueError("backend must be 'hip' or 'host'")
    if backend == "host":
        return score_host(skel, qpos_pred, qpos_gt, mask)
    own = ctx is None
    if own:
        if cfg is None:
            raise ValueError("backend='hip' needs `ctx` (an EgpContext) or `cfg` to make one from")
        from .pose2d import context_of
        ctx = context_of(cfg, skel, device_index)
    try:
        return score(ctx, qpos_pred, qpos_gt, mask)
    finally:
        if own:
            ctx.close()


def _span_row(r, lo, hi, dt, mask):
    """Frames [lo, hi) of a scored batch as one trajectory -> (the five figures, err mean [nbody])."""
    row = [float(r[k][lo:hi].mean()) for k in FIGURES[:4]] + [accel_err(r["xpos_pred"][lo:hi], r["xpos_gt"][lo:hi], dt, mask)]
    return np.array(row), r["err"][lo:hi].mean(0)


def _mean_rows(rows):
    """Mean of rows of five figures; a nan accel_err is left out of its mean (all nan: nan)."""
    rows = np.asarray(rows, float).reshape(-1, 5)
    acc = rows[:, 4][~np.isnan(rows[:, 4])]
    return np.append(rows[:, :4].mean(0), acc.mean() if acc.size else np.nan)


def format_line(row, what="all"):
    return "%s - g-mpjpe: %.2f mm, mpjpe: %.2f mm, pa-mpjpe: %.2f mm, root: %.2f mm, accel err: %.3f m/s^2" % (
        (what,) + tuple(1e3 * v for v in row[:4]) + (row[4],))


def format_body_table(skel, per_body, mask=None):
    sel = mask_bits(mask, len(skel.body_names))
    lines = ["%-16s %10s" % ("body", "mpjpe (mm)")]
    lines += ["%-16s %10.2f" % (n, 1e3 * per_body[b]) if sel[b] else "%-16s %10s" % (n, "-") for b, n in enumerate(skel.body_names)]
    return "\n".join(lines)


def _finish(out_rows, out_bodies, skel, mask, algo, verbose):
    acc = _mean_rows(list(out_rows.values()))
    per_body = np.mean(list(out_bodies.values()), axis=0)
    out = {k: float(acc[i]) for i, k in enumerate(FIGURES)}
    out.update(per_take=out_rows, per_body=per_body)
    if verbose:
        print("=" * 10 + " %s: joint positions " % (algo or "") + "=" * 10)
        print(format_line(acc))
        print(format_body_table(skel, per_body, mask))
    return out


def compute_joint_metrics(results, skel, dt=1.0 / 30.0, mask=None, backend="hip", ctx=None, verbose=False, algo=None, cfg=None, device_index=0):
    """`results` = {'traj_pred': {take: [T][nq]}, 'traj_orig': {take: [T][nq]}} -> dict(g_mpjpe, mpjpe, pa_mpjpe, root_err, accel_err:
    the mean over takes; per_take {take: the five figures}; per_body [nbody]: the root-relative error per body, 0 outside the mask).
    All frames of all takes go through one launch (`backend='hip'`, on `ctx` or on a context made from `cfg`)."""
    mask_bits(mask, len(skel.body_names))
    spans, pred, orig = {}, [], []
    lo = 0
    for take, traj in results["traj_pred"].items():
        traj, gt = np.asarray(traj, float), np.asarray(results["traj_orig"][take], float)
        if traj.shape != gt.shape:
            raise ValueError("take %s: predicted and MoCap trajectories differ in shape (%s, %s)" % (take, traj.shape, gt.shape))
        if traj.shape[0] == 0:
            raise ValueError("take %s has no frames" % take)
        pred.append(traj)
        orig.append(gt)
        spans[take] = (lo, lo + traj.shape[0])
        lo += traj.shape[0]
    if not spans:
        raise ValueError("no takes to score")
    r = _score_all(skel, np.concatenate(pred), np.concatenate(orig), mask, backend, ctx, cfg, device_index)
    rows, bodies = {}, {}
    for take, (a, b) in spans.items():
        rows[take], bodies[take] = _span_row(r, a, b, dt, mask)
    return _finish(rows, bodies, skel, mask, algo, verbose)


def compute_forecast_joint_metrics(results, skel, fr_margin, horizon, dt=1.0 / 30.0, mask=None, backend="hip", ctx=None, verbose=False,
                                   algo="ego forecast", cfg=None, device_index=0):
    """The same for forecast results {'traj_pred': {take: [n_win][m + T][nq]}, 'traj_orig': ...}: frames [m, m + horizon) of every
    window (one launch for all of them), the mean over a take's windows, then over takes."""
    mask_bits(mask, len(skel.body_names))
    m = int(fr_margin)
    spans, pred, orig = {}, [], []
    lo = 0
    for take, wins in results["traj_pred"].items():
        wins, gts = np.asarray(wins, float), np.asarray(results["traj_orig"][take], float)
        if wins.shape != gts.shape or wins.ndim != 3:
            raise ValueError("take %s: predicted and MoCap windows differ in shape (%s, %s)" % (take, wins.shape, gts.shape))
        a, b = wins[:, m:m + horizon], gts[:, m:m + horizon]
        if a.shape[0] == 0 or a.shape[1] == 0:
            raise ValueError("take %s has no frames in [%d, %d)" % (take, m, m + horizon))
        pred.append(a.reshape(-1, a.shape[2]))
        orig.append(b.reshape(-1, b.shape[2]))
        spans[take] = (lo, a.shape[0], a.shape[1])
        lo += a.shape[0] * a.shape[1]
    if not spans:
        raise ValueError("no takes to score")
    r = _score_all(skel, np.concatenate(pred), np.concatenate(orig), mask, backend, ctx, cfg, device_index)
    rows, bodies = {}, {}
    for take, (a, n_win, T) in spans.items():
        per_win = [_span_row(r, a + i * T, a + (i + 1) * T, dt, mask) for i in range(n_win)]
        rows[take] = _mean_rows([w[0] for w in per_win])
        bodies[take] = np.mean([w[1] for w in per_win], axis=0)
    return _finish(rows, bodies, skel, mask, "%s, horizon %d" % (algo, horizon), verbose)
