"""The 2D keypoint metric of in-the-wild takes: the only score a take without MoCap can be given.

`Pose2DContext` restates the numeric parts of ego_pose/utils/pose2d.py (the 12-body set, `joints_map` from OpenPose
BODY_25 indices to bodies, `load_gt_pose`, `check_gt`, `project_qpos`, `align_qpos` with scale=None, `get_pose_dist`); drawing is
out of scope. The host numpy path takes BODY POSITIONS as input (`project_xpos`, `align_xpos`): the reference's
`env.data.body_xpos[1:]` rows of the 12 bodies. `*_qpos` get them from the skeleton's host forward kinematics
(`Skeleton.body_xpos`). On the GPU nothing of this runs: `Pose2DContext.score` hands all frames to one launch of
`egp_pose2d_f64` (csrc/egp_pose2d.hip: forward kinematics, camera, alignment and distance per frame, a wavefront each).

`eval_pose_wild_stats` / `eval_forecast_wild_stats` are the `--mode stats` loops of ego_pose/eval_pose_wild.py:50-98 and
ego_pose/eval_forecast_wild.py:50-116: per take (per window) the mean keypoint distance over the valid frames and the mean absolute
joint acceleration (`metrics`), `traj_ub` / `tpv_offset` / `tpv_flip` of the take's meta honoured, frames whose keypoints fail
`check_gt` skipped. `backend='hip'` scores every frame of every take (every horizon frame of every window) in ONE kernel launch;
`backend='host'` is the per-frame numpy loop, for machines without a GPU -- the choice is the caller's, nothing falls back.
"""
from __future__ import annotations

import json

import numpy as np

from . import metrics

BODY_SET = ("LeftForeArm", "RightForeArm", "LeftHand", "RightHand", "LeftArm", "RightArm",
            "LeftUpLeg", "RightUpLeg", "LeftLeg", "RightLeg", "LeftFoot", "RightFoot")
# OpenPose BODY_25 index -> body (pose2d.py:35-46)
OPENPOSE_JOINTS = ((2, "RightArm"), (3, "RightForeArm"), (4, "RightHand"), (5, "LeftArm"), (6, "LeftForeArm"), (7, "LeftHand"),
                   (9, "RightUpLeg"), (10, "RightLeg"), (11, "RightFoot"), (12, "LeftUpLeg"), (13, "LeftLeg"), (14, "LeftFoot"))
ROLES = ("LeftUpLeg", "RightUpLeg", "LeftLeg", "RightLeg", "LeftArm", "RightArm")     # egp_set_pose2d_bodies' `roles` order


class Pose2DContext:

    def __init__(self, skel=None):
        from .skeleton import load_skeleton
        self.skel = skel if skel is not None else load_skeleton()
        names = list(self.skel.body_names)
        self.body_set = set(BODY_SET)
        self.nbody = len(self.body_set)
        self.body_filter = np.array([n in self.body_set for n in names])          # over data.body_xpos[1:] = the skeleton's bodies
        self.body_names = [n for n in names if n in self.body_set]                # model order, as the reference's filter leaves them
        self.body2id = {body: i for i, body in enumerate(self.body_names)}
        self.body_index = np.array([names.index(n) for n in self.body_names], np.int32)
        self.joints_map = [(i1, self.body2id[b]) for i1, b in OPENPOSE_JOINTS]

    def kernel_tables(self):
        """(kp_body [12], roles [6]) for EgpContext.set_pose2d_bodies."""
        return self.body_index.copy(), np.array([self.body2id[r] for r in ROLES], np.int32)

    # ------------------------------------------------------------------ pose2d.py:67-76
    def gt_from_keypoints(self, keypoints):
        """One OpenPose `pose_keypoints_2d` row (75 floats: x, y, confidence of BODY_25) -> [12][3] in body order."""
        keypoints = np.asarray(keypoints, float)
        p = np.zeros((self.nbody, 3))
        for i1, i2 in self.joints_map:
            p[i2, :] = keypoints[3 * i1: 3 * i1 + 3]
        return p

    def load_gt_pose(self, filename):
        with open(filename) as f:
            data = json.load(f)
        return self.gt_from_keypoints(data["people"][0]["pose_keypoints_2d"])

    def check_gt(self, gt_pose):
        return bool(gt_pose[self.body2id["LeftUpLeg"], 2] > 0.1 or gt_pose[self.body2id["RightUpLeg"], 2] > 0.1)

    # ------------------------------------------------------------------ pose2d.py:78-95
    def get_pose_dist(self, p, gt_p):
        body2id = self.body2id
        if gt_p[body2id["LeftArm"], 2] > 0.1 and gt_p[body2id["LeftUpLeg"], 2] > 0.1:
            kp1, kp2 = "LeftArm", "LeftUpLeg"
        else:
            kp1, kp2 = "RightArm", "RightUpLeg"
        scale = 0.5 / abs(gt_p[body2id[kp1], 1] - gt_p[body2id[kp2], 1])
        dist, num = 0, 0
        for i in range(gt_p.shape[0]):
            if gt_p[i, 2] > 0.1:
                dist += np.linalg.norm(gt_p[i, :2] - p[i, :]) * scale
                num += 1
        return dist / num

    # ------------------------------------------------------------------ pose2d.py:97-123, from the 12 body positions
    def body_positions(self, qpos):
        """[12][3] world positions of the keypoint bodies (the reference's sim.forward + body_xpos[1:][body_filter]), host FK."""
        return self.skel.body_xpos(np.asarray(qpos, float))[self.body_index]

    def project_xpos(self, pose_3d, flip):
        pose_3d = np.asarray(pose_3d, float)
        body2id = self.body2id
        vp = (pose_3d[body2id["LeftUpLeg"], :] + pose_3d[body2id["RightUpLeg"], :]) * 0.5
        v = pose_3d[body2id["RightUpLeg"], :] - pose_3d[body2id["LeftUpLeg"], :]
        if flip:
            v *= -1
        v[2] = 0
        v /= np.linalg.norm(v)
        x = v
        z = np.array([0, 0, 1])
        y = np.cross(z, x)
        R = np.hstack((-y[:, None], z[:, None], x[:, None]))        # camera -> world
        t = (vp - 10 * x)[:, None]
        E = np.hstack((R.T, -R.T.dot(t)))
        p = np.hstack((pose_3d, np.ones((pose_3d.shape[0], 1)))).dot(E.T)
        p = p[:, :2] / p[:, [2]]
        p[:, 1] *= -1
        return p

    def project_qpos(self, qpos, flip):
        return self.project_xpos(self.body_positions(qpos), flip)

    # ------------------------------------------------------------------ pose2d.py:125-148
    def align_xpos(self, pose_3d, gt_p, scale=None, flip=False):
        body2id = self.body2id
        p = self.project_xpos(pose_3d, flip)
        base = np.zeros((1, 2))
        n = 0
        if gt_p[body2id["LeftUpLeg"], 2] > 0.1:
            base += gt_p[[body2id["LeftUpLeg"]], :2]
            n += 1
        if gt_p[body2id["RightUpLeg"], 2] > 0.1:
            base += gt_p[[body2id["RightUpLeg"]], :2]
            n += 1
        base /= n
        if scale is None:
            if gt_p[body2id["LeftLeg"], 2] > 0.1 and gt_p[body2id["LeftUpLeg"], 2] > 0.1:
                kp1, kp2 = "LeftLeg", "LeftUpLeg"
            else:
                kp1, kp2 = "RightLeg", "RightUpLeg"
            # the reference's numerator runs over the whole keypoint row: x, y and the confidence
            scale = np.linalg.norm(gt_p[body2id[kp1]] - gt_p[body2id[kp2]]) / np.linalg.norm(p[body2id[kp1]] - p[body2id[kp2]])
        return p * scale + base

    def align_qpos(self, qpos, gt_p, scale=None, flip=False):
        return self.align_xpos(self.body_positions(qpos), gt_p, scale, flip)

    # ------------------------------------------------------------------ many frames at once
    def score_host(self, qpos, gt, flip):
        """Per-frame numpy loop -> (dist [n], valid [n] bool); dist = 0 on invalid frames, as the kernel leaves it."""
        n = len(qpos)
        dist, valid = np.zeros(n), np.zeros(n, bool)
        for i in range(n):
            valid[i] = self.check_gt(gt[i])
            if valid[i]:
                dist[i] = self.get_pose_dist(self.align_qpos(qpos[i], gt[i], flip=bool(flip[i])), gt[i])
        return dist, valid

    def score(self, ctx, qpos, gt, flip, want_p=False):
        """All frames in one launch of egp_pose2d_f64 on `ctx`'s device -> (dist [n], valid [n] bool[, p [n][12][2]]) numpy."""
        import torch
        want = self.kernel_tables()
        if getattr(ctx, "_pose2d_tables", None) != (tuple(want[0].tolist()), tuple(want[1].tolist())):
            ctx.set_pose2d_bodies(*want)
        dev = torch.device("cuda", ctx.device)
        n = len(qpos)
        if n == 0:
            out = (np.zeros(0), np.zeros(0, bool))
            return out + (np.zeros((0, 12, 2)),) if want_p else out
        with torch.cuda.device(dev):
            d = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)
            r = ctx.pose2d(d(qpos, np.float64), d(gt, np.float64), d(flip, np.int32), want_p=want_p)
            out = (r["dist"].cpu().numpy(), r["valid"].cpu().numpy().astype(bool))
            return out + (r["p"].cpu().numpy(),) if want_p else out


def file_keypoint_loader(data_dir, pose_ctx):
    """`keypoint_loader(take, gt_fr)` over <data_dir>/tpv/poses/<take>/%05d_keypoints.json (OpenPose output of the side camera)."""
    return lambda take, gt_fr: pose_ctx.load_gt_pose("%s/tpv/poses/%s/%05d_keypoints.json" % (data_dir, take, gt_fr))


def wild_stats_front(cfg, test_feat):
    """What `--mode wild-stats` of both evaluation CLIs starts from -> (the takes' meta of <data_dir>/meta/meta_<test_feat>.yml,
    a Pose2DContext, the keypoint loader over it)."""
    import yaml
    with open("%s/meta/meta_%s.yml" % (cfg.data_dir, test_feat)) as f:
        meta = yaml.safe_load(f)
    pose_ctx = Pose2DContext()
    return meta, pose_ctx, file_keypoint_loader(cfg.data_dir, pose_ctx)


def context_of(cfg, skel=None, device_index=0):
    """An EgpContext for scoring alone (the model constants of `cfg`, no engine, no experts)."""
    from .hip import EgpContext, obs_options_of
    from .skeleton import load_skeleton
    sk = skel if skel is not None else load_skeleton()
    return EgpContext(sk, cfg.jkp, cfg.jkd, cfg.a_ref, cfg.a_scale, cfg.torque_lim, cfg.b_diffw, reward_weights=getattr(cfg, "reward_weights", None),
                      episode_len=cfg.env_episode_len, device=device_index, obs_options=obs_options_of(cfg))


def _score_jobs(jobs, pose_ctx, keypoint_loader, backend, cfg, ctx, device_index):
    """jobs: [(take, qpos row, gt frame, flip)] -> (dist, valid) per job, one launch for all of them on the GPU."""
    if backend not in ("hip", "host"):
        raise ValueError("backend must be 'hip' or 'host'")
    gt = np.zeros((len(jobs), pose_ctx.nbody, 3))
    for k, (take, _, gt_fr, _) in enumerate(jobs):
        g = np.asarray(keypoint_loader(take, gt_fr), float)
        gt[k] = pose_ctx.gt_from_keypoints(g) if g.ndim == 1 else g
    qpos = np.stack([j[1] for j in jobs]) if jobs else np.zeros((0, pose_ctx.skel.nq))
    flip = np.array([1 if j[3] else 0 for j in jobs], np.int32)
    if backend == "host":
        return pose_ctx.score_host(qpos, gt, flip)
    own = ctx is None
    if own:
        ctx = context_of(cfg, pose_ctx.skel, device_index)
    try:
        return pose_ctx.score(ctx, qpos, gt, flip)
    finally:
        if own:
            ctx.close()


def _mean_valid(dist, valid, lo, hi, what):
    pose_dist, valid_num = 0, 0
    for k in range(lo, hi):                      # the reference's running sum, in frame order
        if valid[k]:
            pose_dist += dist[k]
            valid_num += 1
    if valid_num == 0:                           # (the reference divides by zero here)
        raise ValueError("%s: no frame with valid keypoints to score (all cut by traj_ub / tpv_offset, or no hip seen)" % what)
    return pose_dist / valid_num


def _meta_dicts(meta):
    """The take meta's `traj_ub`, `tpv_offset`, `tpv_flip` dicts; a missing or empty key means no take has an entry."""
    return tuple(meta.get(key) or {} for key in ("traj_ub", "tpv_offset", "tpv_flip"))


def eval_pose_wild_stats(results, meta, keypoint_loader, cfg, backend="hip", ctx=None, pose_ctx=None, dt=1.0 / 30.0, algo="ego mimic",
                         verbose=False, device_index=0):
    """eval_pose_wild.py:50-98 -> dict(takes={take: (pose_dist, accels)}, pose_dist, accels). `results` = {'traj_pred': {take: [T][nq]}};
    `meta` = the take meta with `traj_ub`, `tpv_offset`, `tpv_flip` dicts; `keypoint_loader(take, gt_fr)` -> [12][3] (or the 75 floats)."""
    pose_ctx = pose_ctx if pose_ctx is not None else Pose2DContext()
    trajs, jobs, spans = {}, [], {}
    m_ub, m_off, m_flip = _meta_dicts(meta)
    for take in results["traj_pred"].keys():
        traj_pred = np.asarray(results["traj_pred"][take], float)
        traj_pred = traj_pred[:m_ub.get(take, traj_pred.shape[0])]
        tpv_offset = m_off.get(take, cfg.fr_margin)
        flip = m_flip.get(take, False)
        lo = len(jobs)
        for fr in range(max(0, -tpv_offset), traj_pred.shape[0]):
            jobs.append((take, traj_pred[fr], fr + tpv_offset, flip))
        trajs[take], spans[take] = traj_pred, (lo, len(jobs))
    dist, valid = _score_jobs(jobs, pose_ctx, keypoint_loader, backend, cfg, ctx, device_index)
    out, g_pose_dist, g_smoothness = {}, 0, 0
    if verbose:
        print("=" * 10 + " %s " % algo + "=" * 10)
    for take, traj_pred in trajs.items():
        pose_dist = _mean_valid(dist, valid, *spans[take], "take %s" % take)
        smoothness = metrics.get_mean_abs(metrics.get_joint_accels(metrics.get_joint_vels(traj_pred, dt), dt))
        out[take] = (pose_dist, smoothness)
        g_pose_dist += pose_dist
        g_smoothness += smoothness
        if verbose:
            print("%s - pose dist: %.4f, accels: %.4f" % (take, pose_dist, smoothness))
    g_pose_dist /= len(trajs)
    g_smoothness /= len(trajs)
    if verbose:
        print("-" * 60 + "\nall - pose dist: %.4f, accels: %.4f\n" % (g_pose_dist, g_smoothness) + "-" * 60 + "\n")
    return dict(takes=out, pose_dist=g_pose_dist, accels=g_smoothness)


def eval_forecast_wild_stats(results, meta, keypoint_loader, cfg, horizon=30, backend="hip", ctx=None, pose_ctx=None, dt=1.0 / 30.0,
                             algo="ego forecast", verbose=False, device_index=0):
    """eval_forecast_wild.py:50-116 -> dict(takes={take: (pose_dist, accels)}, pose_dist, accels). `results` = {'traj_pred': {take:
    [n_win][m + T][nq]}}; window i covers the take rows from (i + 1) * cfg.fr_margin (the numbering of the wild ego_mimic result). The
    wrist joints are zeroed first (remove_noisy_hands), on a copy."""
    pose_ctx = pose_ctx if pose_ctx is not None else Pose2DContext()
    m = cfg.fr_margin
    res = {"traj_pred": {take: np.array(tr, float, copy=True) for take, tr in results["traj_pred"].items()}}
    metrics.remove_noisy_hands(res)
    jobs, spans = [], {}
    m_ub, m_off, m_flip = _meta_dicts(meta)
    for take, windows in res["traj_pred"].items():
        traj_ub = m_ub.get(take, None)
        tpv_offset = m_off.get(take, m)
        flip = m_flip.get(take, False)
        for i in range(windows.shape[0]):
            traj, start_fr = windows[i, m:m + horizon], (i + 1) * m
            lo = len(jobs)
            for fr in range(traj.shape[0]):
                if traj_ub is not None and start_fr + fr >= traj_ub:
                    break
                jobs.append((take, traj[fr], start_fr + fr + tpv_offset, flip))
            spans[take, i] = (lo, len(jobs))
    dist, valid = _score_jobs(jobs, pose_ctx, keypoint_loader, backend, cfg, ctx, device_index)
    out, g_pose_dist, g_smoothness = {}, 0, 0
    if verbose:
        print("=" * 10 + " %s " % algo + "=" * 10)
    for take, windows in res["traj_pred"].items():
        t_pose_dist, t_smoothness = 0, 0
        for i in range(windows.shape[0]):
            traj = windows[i, m:m + horizon]
            t_pose_dist += _mean_valid(dist, valid, *spans[take, i], "take %s, window %d" % (take, i))
            t_smoothness += metrics.get_mean_abs(metrics.get_joint_accels(metrics.get_joint_vels(traj, dt), dt))
        t_pose_dist /= windows.shape[0]
        t_smoothness /= windows.shape[0]
        out[take] = (t_pose_dist, t_smoothness)
        g_pose_dist += t_pose_dist
        g_smoothness += t_smoothness
        if verbose:
            print("%s - pose dist: %.4f, accels: %.4f" % (take, t_pose_dist, t_smoothness))
    g_pose_dist /= len(res["traj_pred"])
    g_smoothness /= len(res["traj_pred"])
    if verbose:
        print("-" * 60 + "\nall - pose dist: %.4f, accels: %.4f\n" % (g_pose_dist, g_smoothness) + "-" * 60 + "\n")
    return dict(takes=out, pose_dist=g_pose_dist, accels=g_smoothness)
