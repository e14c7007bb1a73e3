"""Physical plausibility of an estimated motion against the ground: foot sliding, ground penetration and floating.

`metrics`, `pose2d` and `pose3d` score how far an estimate is from MoCap (or from 2D keypoints). None of them says whether the motion
could happen: a kinematic regressor may skate over the floor or sink into it, a simulated humanoid cannot. The figures here need no
ground truth, so they are also the only 3D figures of takes without MoCap.

A `ContactSet` is K (1..32) points, each fixed to a body: `offset[k]` in the zero pose's global axes relative to `body_pos[body[k]]`
(the convention of the centres of mass), world point `P_k = p_b + R_b @ offset[k]`; `group[k]` names the foot a point belongs to and
is used by the per-foot report only. The default, `ContactSet.feet`, is the 8 corners of each foot's equivalent inertia box, built
from the asset's masses and inertias alone.

Two parameters belong to the DEFINITION, not to a measurement, and are carried in every result dict and printed line: `ground_z`
(default 0) and `contact_height` (default 0.02 m). For a row t with points P_k, a following row nxt[t] (-1: none) with points P'_k,
and z measured from ground_z, a frame gets

    pen        max_k max(0, -z_k)                                   ground penetration, metres
    gap        max(0, min_k z_k)                                    floating, metres
    n_contact  number of k with z_k <= contact_height
    n_skate    number of k with z_k <= contact_height and z'_k <= contact_height; 0 without a following row
    skate      mean over those k of |(P'_k - P_k)_xy|               metres per frame step; 0 when n_skate = 0
    skate_max  max over the same k                                  0 when n_skate = 0

and a trajectory gets, on the host in float64 for both backends,

    pen_mean       mean of pen over frames          pen_max   max of pen over frames          gap_mean  mean of gap over frames
    contact_ratio  share of frames with n_contact > 0
    skate_mean     mean of skate over frames with n_skate > 0; nan when there are none, and such a trajectory is left out of the
                   mean over takes (windows), as pose3d's accel_err is

Aggregation is pose3d's: per take over its frames, then the mean over takes; for forecast results the frames [m, m + horizon) of
every window with the following row inside the window, the mean over a take's windows, then over takes. Dicts hold metres; the
printed line is millimetres.

`score_points` is numpy from world points, `score_host` feeds it from `Skeleton.body_frames`, `score` hands all frames to ONE launch
of `egp_contact_f64` (csrc/egp_contact.hip: two forward kinematics per wavefront and shuffle reductions over the points). All three
return the same dict of arrays. `backend='hip' | 'host'` is the caller's choice; nothing falls back.
"""
from __future__ import annotations

import itertools
import json

import numpy as np

MAX_POINTS = 32
COLS = ("pen", "gap", "n_contact", "n_skate", "skate", "skate_max")
FIGURES = ("pen_mean", "pen_max", "gap_mean", "contact_ratio", "skate_mean")
FEET = ("LeftFoot", "RightFoot")


class ContactSet:
    """body int32 [K], offset float64 [K][3], group int32 [K] (default: all 0), 1 <= K <= 32. `nbody` (or `check`) bounds the bodies."""

    def __init__(self, body, offset, group=None, nbody=None):
        body_in = np.asarray(body)
        if body_in.ndim != 1 or not np.issubdtype(body_in.dtype, np.integer):
            raise ValueError("body must be a list of K integers")
        self.body = np.ascontiguousarray(body_in, np.int32)
        K = self.body.shape[0]
        if not 1 <= K <= MAX_POINTS:
            raise ValueError("a contact set has 1 to %d points, got %d" % (MAX_POINTS, K))
        self.offset = np.ascontiguousarray(np.asarray(offset, np.float64))
        if self.offset.shape != (K, 3):
            raise ValueError("offset must be [%d][3], got %s" % (K, self.offset.shape))
        if not np.isfinite(self.offset).all():
            raise ValueError("contact offsets must be finite")
        self.group = np.zeros(K, np.int32) if group is None else np.ascontiguousarray(np.asarray(group), np.int32)
        if self.group.shape != (K,):
            raise ValueError("group must have %d entries" % K)
        if self.body.min() < 0:
            raise ValueError("contact body out of range")
        if nbody is not None:
            self.check(nbody)

    @property
    def K(self):
        return int(self.body.shape[0])

    def check(self, skel_or_nbody):
        """ValueError unless every body index is one of the skeleton's -> self."""
        nbody = skel_or_nbody if isinstance(skel_or_nbody, (int, np.integer)) else len(skel_or_nbody.body_names)
        if self.body.max() >= nbody:
            raise ValueError("contact body %d out of range [0, %d)" % (self.body.max(), nbody))
        return self

    @classmethod
    def feet(cls, skel, bodies=FEET):
        """The 8 corners of each named body's equivalent inertia box: with (lam, V) = eigh(body_inertia[b]) and m = body_mass[b] the
        solid box of mass m with the same inertia has half sizes h_i = sqrt(3 / (2 m) * (tr I - 2 lam_i)) along the columns of V, centred
        on the COM. Point 8 g + c belongs to bodies[g] (group g); corner c has the signs of itertools.product((-1, 1), repeat=3)."""
        names = list(skel.body_names)
        body, offset, group = [], [], []
        for g, name in enumerate(bodies):
            if name not in names:
                raise ValueError("no such body: %s" % name)
            b = names.index(name)
            I, m = np.asarray(skel.body_inertia[b], float), float(skel.body_mass[b])
            lam, V = np.linalg.eigh(0.5 * (I + I.T))
            h2 = 1.5 / m * (lam.sum() - 2.0 * lam) if m > 0 else np.full(3, -1.0)
            if not (np.isfinite(h2).all() and (h2 > 0).all()):
                raise ValueError("body %s: no solid box has this inertia (half sizes squared %s)" % (name, h2))
            h = np.sqrt(h2)
            centre = np.asarray(skel.body_com[b], float) - np.asarray(skel.body_pos[b], float)
            for s in itertools.product((-1.0, 1.0), repeat=3):
                body.append(b)
                offset.append(centre + V @ (np.array(s) * h))
                group.append(g)
        return cls(body, offset, group, nbody=len(names))

    def to_file(self, path):
        with open(path, "w") as f:
            json.dump(dict(body=self.body.tolist(), offset=self.offset.tolist(), group=self.group.tolist()), f)

    @classmethod
    def from_file(cls, path):
        with open(path) as f:
            d = json.load(f)
        if not isinstance(d, dict) or set(d) != {"body", "offset", "group"}:
            raise ValueError("%s: a contact file holds the three arrays body, offset, group" % path)
        return cls(d["body"], d["offset"], d["group"])

    def world_points(self, R, p):
        """Body frames (R [nb][3][3], p [nb][3]) -> the K world points [K][3]."""
        return p[self.body] + np.einsum("kij,kj->ki", R[self.body], self.offset)


def _nxt_of(nxt, n):
    nxt = np.asarray(nxt)
    if nxt.shape != (n,) or not np.issubdtype(nxt.dtype, np.integer):
        raise ValueError("nxt must be %d integers (the following row of every row, -1: none)" % n)
    nxt = nxt.astype(np.int64)
    if n and (nxt.min() < -1 or nxt.max() >= n):
        raise ValueError("nxt must lie in [-1, %d)" % n)
    return nxt


def _params(ground_z, contact_height):
    ground_z, contact_height = float(ground_z), float(contact_height)
    if not (np.isfinite(ground_z) and np.isfinite(contact_height)):
        raise ValueError("ground_z and contact_height must be finite")
    return ground_z, contact_height


def score_points(points, nxt, ground_z=0.0, contact_height=0.02):
    """World points [n][K][3] of every row and nxt [n] -> dict(pen, gap, n_contact, n_skate, skate, skate_max [n], points)."""
    P = np.asarray(points, float)
    if P.ndim != 3 or P.shape[2] != 3 or not 1 <= P.shape[1] <= MAX_POINTS:
        raise ValueError("points must be [n][K][3] with 1 <= K <= %d, got %s" % (MAX_POINTS, P.shape))
    n = P.shape[0]
    nxt = _nxt_of(nxt, n)
    ground_z, contact_height = _params(ground_z, contact_height)
    z = P[:, :, 2] - ground_z
    has = nxt >= 0
    Q = P[np.where(has, nxt, np.arange(n))]
    down = z <= contact_height
    both = down & (Q[:, :, 2] - ground_z <= contact_height) & has[:, None]
    slide = np.where(both, np.hypot(Q[:, :, 0] - P[:, :, 0], Q[:, :, 1] - P[:, :, 1]), 0.0)
    n_skate = both.sum(1)
    zmin = z.min(1) if n else np.zeros(0)
    return dict(pen=np.maximum(0.0, -zmin) + 0.0, gap=np.maximum(0.0, zmin), n_contact=down.sum(1).astype(np.int64), n_skate=n_skate.astype(np.int64),
                skate=slide.sum(1) / np.maximum(n_skate, 1), skate_max=slide.max(1) if n else np.zeros(0), points=P)


def _rows(skel, qpos):
    q = np.asarray(qpos, float)
    if q.ndim != 2 or q.shape[1] != skel.nq:
        raise ValueError("qpos must be [n][%d], got %s" % (skel.nq, q.shape))
    return q


def score_host(skel, cs, qpos, nxt, ground_z=0.0, contact_height=0.02):
    """The numpy path: host forward kinematics with rotations of every row (`Skeleton.body_frames`), then `score_points`."""
    q = _rows(skel, qpos)
    cs.check(skel)
    pts = np.stack([cs.world_points(*skel.body_frames(r)) for r in q]) if len(q) else np.zeros((0, cs.K, 3))
    return score_points(pts, nxt, ground_z, contact_height)


def score(ctx, cs, qpos, nxt, ground_z=0.0, contact_height=0.02):
    """All rows in one launch of egp_contact_f64 on `ctx`'s device (its contact set becomes `cs`) -> the dict of `score_points`, numpy."""
    import torch
    q = _rows(ctx.skel, qpos)
    cs.check(ctx.skel)
    n = len(q)
    nxt = _nxt_of(nxt, n)
    ground_z, contact_height = _params(ground_z, contact_height)
    if n == 0:
        return score_points(np.zeros((0, cs.K, 3)), nxt, ground_z, contact_height)
    dev = torch.device("cuda", ctx.device)
    with torch.cuda.device(dev):
        ctx.set_contact_points(cs)
        d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
        r = ctx.contact(d(q), d(nxt), ground_z=ground_z, contact_height=contact_height, want_points=True, validate=False)     # (checked above)
        pf = r["per_frame"].cpu().numpy()
        out = {k: pf[:, i].copy() for i, k in enumerate(COLS)}
        out["n_contact"], out["n_skate"] = out["n_contact"].astype(np.int64), out["n_skate"].astype(np.int64)
        out["points"] = r["points"].cpu().numpy()
        return out


def trajectory_figures(r, lo=0, hi=None):
    """Frames [lo, hi) of a scored batch as one trajectory -> the five figures (FIGURES)."""
    hi = len(r["pen"]) if hi is None else hi
    if hi <= lo:
        raise ValueError("a trajectory needs at least one frame")
    pen, gap, skated = r["pen"][lo:hi], r["gap"][lo:hi], r["n_skate"][lo:hi] > 0
    return np.array([pen.mean(), pen.max(), gap.mean(), float((r["n_contact"][lo:hi] > 0).mean()),
                     r["skate"][lo:hi][skated].mean() if skated.any() else np.nan])


def _mean_rows(rows):
    """Mean of rows of five figures; a nan skate_mean is left out of its mean (all nan: nan)."""
    rows = np.asarray(rows, float).reshape(-1, 5)
    sk = rows[:, 4][~np.isnan(rows[:, 4])]
    return np.append(rows[:, :4].mean(0), sk.mean() if sk.size else np.nan)


def format_line(row, what="all", ground_z=0.0, contact_height=0.02):
    return ("%s - pen: %.2f mm (max %.2f mm), float: %.2f mm, contact: %.1f %%, skate: %.2f mm/frame [ground z: %.1f mm, contact height: %.1f mm]"
            % (what, 1e3 * row[0], 1e3 * row[1], 1e3 * row[2], 1e2 * row[3], 1e3 * row[4], 1e3 * ground_z, 1e3 * contact_height))


def _chain(length):
    """Following rows of one trajectory of `length` frames, relative to its first: 1, 2, ..., length - 1, none."""
    nxt = np.arange(1, length + 1, dtype=np.int64)
    nxt[-1] = -1
    return nxt


def _collect(results, which, windows, m, horizon):
    """-> {key: (rows [N][nq], nxt [N], spans {take: [(lo, hi) of every trajectory]})} for the keys of `which` that `results` has."""
    if "traj_pred" in which and "traj_pred" not in results:
        raise ValueError("results have no traj_pred")
    out = {}
    for key in which:
        if key not in results:                   # (wild results carry no traj_orig: the prediction is scored alone)
            continue
        rows, nxt, spans, lo = [], [], {}, 0
        for take, traj in results[key].items():
            traj = np.asarray(traj, float)
            if windows:
                if traj.ndim != 3:
                    raise ValueError("take %s: forecast results are [n_win][m + T][nq], got %s" % (take, traj.shape))
                traj = traj[:, m:m + horizon]
            else:
                if traj.ndim != 2:
                    raise ValueError("take %s: a trajectory is [T][nq], got %s" % (take, traj.shape))
                traj = traj[None]
            if traj.shape[0] == 0 or traj.shape[1] == 0:
                raise ValueError("take %s has no frames" % take)
            T = traj.shape[1]
            spans[take] = []
            for w in range(traj.shape[0]):
                rows.append(traj[w])
                nxt.append(np.where(_chain(T) >= 0, _chain(T) + lo, -1))
                spans[take].append((lo, lo + T))
                lo += T
        if not spans:
            raise ValueError("no takes to score")
        out[key] = (np.concatenate(rows), np.concatenate(nxt), spans)
    return out


def _compute(results, skel, contacts, which, windows, m, horizon, ground_z, contact_height, backend, ctx, cfg, verbose, algo, device_index):
    cs = (contacts if contacts is not None else ContactSet.feet(skel)).check(skel)
    ground_z, contact_height = _params(ground_z, contact_height)
    if backend not in ("hip", "host"):
        raise ValueError("backend must be 'hip' or 'host'")
    jobs = _collect(results, which, windows, m, horizon)
    own = backend == "hip" and ctx is None
    if own:
        if cfg is None:
            raise ValueError("backend='hip' needs `ctx` (an EgpContext) or `cfg` to make one from")
        from .pose2d import context_of
        ctx = context_of(cfg, skel, device_index)
    out = dict(ground_z=ground_z, contact_height=contact_height)
    try:
        for key, (rows, nxt, spans) in jobs.items():
            r = (score_host(skel, cs, rows, nxt, ground_z, contact_height) if backend == "host" else
                 score(ctx, cs, rows, nxt, ground_z, contact_height))
            per_take = {take: _mean_rows([trajectory_figures(r, a, b) for a, b in sp]) for take, sp in spans.items()}
            acc = _mean_rows(list(per_take.values()))
            per_group = {}
            for g in np.unique(cs.group):        # the per-foot report: the same figures over one foot's points
                rg = score_points(r["points"][:, cs.group == g], nxt, ground_z, contact_height)
                per_group[int(g)] = _mean_rows([_mean_rows([trajectory_figures(rg, a, b) for a, b in sp]) for sp in spans.values()])
            out[key] = {k: float(acc[i]) for i, k in enumerate(FIGURES)}
            out[key].update(per_take=per_take, per_group=per_group)
            if verbose:
                print("=" * 10 + " %s: physical plausibility, %s " % (algo or "", key) + "=" * 10)
                print(format_line(acc, "all", ground_z, contact_height))
                for g, row in per_group.items():
                    print(format_line(row, "group %d" % g, ground_z, contact_height))
    finally:
        if own:
            ctx.close()
    return out


def compute_plausibility(results, skel, contacts=None, which=("traj_pred", "traj_orig"), backend="hip", ctx=None, cfg=None, ground_z=0.0,
                         contact_height=0.02, verbose=False, algo=None, device_index=0):
    """`results` = {'traj_pred': {take: [T][nq]}[, 'traj_orig': ...]} -> dict(ground_z, contact_height, and per key of `which` that the
    results have: pen_mean, pen_max, gap_mean, contact_ratio, skate_mean -- the mean over takes; per_take {take: the five figures};
    per_group {group: the five figures over that group's points}). `contacts`: a ContactSet (None: `ContactSet.feet(skel)`). All frames
    of all takes of a key go through one launch (`backend='hip'`, on `ctx` or on a context made from `cfg`)."""
    return _compute(results, skel, contacts, which, False, 0, 0, ground_z, contact_height, backend, ctx, cfg, verbose, algo, device_index)


def compute_forecast_plausibility(results, skel, fr_margin, horizon, contacts=None, which=("traj_pred", "traj_orig"), backend="hip", ctx=None,
                                  cfg=None, ground_z=0.0, contact_height=0.02, verbose=False, algo="ego forecast", device_index=0):
    """The same for forecast results {'traj_pred': {take: [n_win][m + T][nq]}, ...}: frames [m, m + horizon) of every window with the
    following row inside the window (one launch for all of them), the mean over a take's windows, then over takes."""
    return _compute(results, skel, contacts, which, True, int(fr_margin), int(horizon), ground_z, contact_height, backend, ctx, cfg, verbose,
                    "%s, horizon %d" % (algo, horizon), device_index)


def add_arguments(ap):
    """The `--physical` flags of both evaluation command lines."""
    ap.add_argument("--physical", action="store_true", help="also foot skate, ground penetration and floating (egopose_amd.plausibility)")
    ap.add_argument("--contacts", default=None, help="--physical: a contact-set JSON file (default: the corners of the feet's inertia boxes)")
    ap.add_argument("--contact-height", type=float, default=0.02, help="--physical: a point at or below this height is in contact, metres")
    ap.add_argument("--ground-z", type=float, default=0.0, help="--physical: height of the ground plane, metres")


def from_args(results, cfg, args, algo, which=("traj_pred",), forecast=None, ctx=None, what="all"):
    """The `--physical` line(s) of `results` for the parsed flags of `add_arguments` (+ --host, --gpu-index): one printed line per key
    of `which`, named `what` (traj_pred) and 'mocap' (traj_orig). `forecast` = (fr_margin, horizon) for forecast results."""
    from .skeleton import load_skeleton
    skel = load_skeleton()
    cs = ContactSet.from_file(args.contacts).check(skel) if args.contacts else None
    kw = dict(contacts=cs, which=which, backend="host" if args.host else "hip", ctx=ctx, cfg=cfg, ground_z=args.ground_z,
              contact_height=args.contact_height, algo=algo, device_index=args.gpu_index)
    out = compute_plausibility(results, skel, **kw) if forecast is None else compute_forecast_plausibility(results, skel, *forecast, **kw)
    for key in which:
        if key in out:
            print(format_line([out[key][k] for k in FIGURES], what if key == "traj_pred" else "mocap", out["ground_z"], out["contact_height"]))
    return out
