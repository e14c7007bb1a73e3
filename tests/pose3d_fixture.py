"""Shared by the joint-position tests (test_pose3d_cpu.py on the CPU, test_pose3d_gpu.py on the GPU): poses of the 2D keypoint test's
generator, pairs of five kinds, and the yardstick -- float64 forward kinematics of oracle/dynamics.py plus the numpy SVD with the
determinant correction, written out here so that it is neither the product's host path nor the kernel."""
import numpy as np

KINDS = ("small noise", "unrelated", "identical", "root translated", "root rotated about z")


def poses(skel, n, rng):
    """Joint angles over the full range, root headings over +-pi (the generator of test_pose2d_gpu.py)."""
    qpos = np.zeros((n, skel.nq))
    qpos[:, :2] = rng.normal(size=(n, 2)) * 3.0
    qpos[:, 2] = rng.uniform(0.7, 1.1, size=n)
    yaw = rng.uniform(-np.pi, np.pi, size=n)
    qpos[:, 3], qpos[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
    qpos[:, 3:7] += rng.normal(size=(n, 4)) * 0.05
    qpos[:, 3:7] /= np.linalg.norm(qpos[:, 3:7], axis=1, keepdims=True)
    qpos[:, 7:] = rng.uniform(skel.joint_range[:, 0], skel.joint_range[:, 1], size=(n, skel.nq - 7))
    return qpos


def _qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def pairs(skel, n, seed, gen=poses):
    """(predicted, MoCap) rows; pair i is of kind i % 5 (KINDS)."""
    rng = np.random.RandomState(seed)
    gt = gen(skel, n, rng)
    other = gen(skel, n, rng)
    pred = gt.copy()
    for i in range(n):
        kind = i % 5
        if kind == 0:
            pred[i, :3] += rng.normal(size=3) * 0.03
            pred[i, 3:7] += rng.normal(size=4) * 0.02
            pred[i, 3:7] /= np.linalg.norm(pred[i, 3:7])
            pred[i, 7:] += rng.normal(size=skel.nq - 7) * 0.05
        elif kind == 1:
            pred[i] = other[i]
        elif kind == 3:
            pred[i, :3] += rng.normal(size=3) * 0.5
        elif kind == 4:
            a = rng.uniform(0.3, 2.5) * rng.choice([-1.0, 1.0])
            pred[i, 3:7] = _qmul(np.array([np.cos(a / 2), 0.0, 0.0, np.sin(a / 2)]), gt[i, 3:7])
    return pred, gt


def procrustes(x, y, correct=True):
    """Mean residual of the least-squares similarity of x [k][3] onto y [k][3]; correct=False: the plain SVD, reflections allowed."""
    xc, yc = x - x.mean(0), y - y.mean(0)
    U, s, Vt = np.linalg.svd(xc.T @ yc)
    D = np.eye(3)
    if correct and np.linalg.det(Vt.T @ U.T) < 0:
        D[2, 2] = -1.0
    R = Vt.T @ D @ U.T
    scale = np.trace(np.diag(s) @ D) / (xc ** 2).sum()
    return float(np.linalg.norm(scale * xc @ R.T - yc, axis=1).mean())


def figures_of_positions(X, Y, sel):
    """One frame's (g_mpjpe, mpjpe, pa_mpjpe, root_err), err [nbody] from positions [nbody][3] and a bool body selection."""
    rel = np.linalg.norm((X - X[0]) - (Y - Y[0]), axis=1)
    row = np.array([np.linalg.norm(X - Y, axis=1)[sel].mean(), rel[sel].mean(), procrustes(X[sel], Y[sel]), np.linalg.norm(X[0] - Y[0])])
    return row, np.where(sel, rel, 0.0)


def yardstick(skel, qpos_pred, qpos_gt, mask=None):
    """-> dict(per_frame [n][4], err [n][nbody], xpos_pred, xpos_gt [n][nbody][3]) from oracle.dynamics.fk."""
    from oracle import dynamics as D
    n, nb = len(qpos_pred), len(skel.body_names)
    sel = np.array([True] * nb if mask is None else [(mask >> b) & 1 == 1 for b in range(nb)])
    out = dict(per_frame=np.zeros((n, 4)), err=np.zeros((n, nb)), xpos_pred=np.zeros((n, nb, 3)), xpos_gt=np.zeros((n, nb, 3)))
    for i in range(n):
        X, Y = D.fk(skel, qpos_pred[i])[1], D.fk(skel, qpos_gt[i])[1]
        out["per_frame"][i], out["err"][i] = figures_of_positions(X, Y, sel)
        out["xpos_pred"][i], out["xpos_gt"][i] = X, Y
    return out


def two_takes(skel, seed=7):
    """Two smooth takes of 14 and 9 frames with a noisy prediction each -> results dict."""
    rng = np.random.RandomState(seed)

    def traj(n):
        q = np.zeros((n, skel.nq))
        q[:, :2] = np.cumsum(rng.normal(size=(n, 2)) * 0.02, 0)
        q[:, 2] = 0.9
        yaw = np.cumsum(rng.normal(size=n) * 0.05) + rng.uniform(-3, 3)
        q[:, 3], q[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
        q[:, 7:] = np.cumsum(rng.normal(size=(n, skel.nq - 7)) * 0.02, 0)
        return q

    def noisy(q):
        p = q.copy()
        p[:, :3] += rng.normal(size=(len(q), 3)) * 0.02
        p[:, 3:7] += rng.normal(size=(len(q), 4)) * 0.03
        p[:, 3:7] /= np.linalg.norm(p[:, 3:7], axis=1, keepdims=True)
        p[:, 7:] += rng.normal(size=(len(q), skel.nq - 7)) * 0.08
        return p
    orig = {"a": traj(14), "b": traj(9)}
    return {"traj_pred": {k: noisy(v) for k, v in orig.items()}, "traj_orig": orig}
