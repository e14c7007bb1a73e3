"""egp_pose2d_f64 (csrc/egp_pose2d.hip) against the numpy restatement of the reference's 2D keypoint metric (egopose_amd/pose2d.py, itself
held against the reference's numbers by tests/test_wild_cpu.py) fed with the oracle's float64 body positions."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

# The issue asks for 10 x the largest error measured against the numpy restatement on the first GPU run, and calls anything above
# 1e-8 wrong rather than loose. Measured on an MI355X over n = 1, 63, 130: largest relative error of p (against max(1, |p|))
# 8.329e-14 (at n = 63), largest absolute error of dist 5.274e-15 (at n = 130). The bounds are 10 x those; the test prints its figures.
P_RTOL = 8.4e-13
DIST_ATOL = 5.3e-14


@pytest.fixture(scope="module")
def ctx(skel):
    from egopose_amd.hip import EgpContext
    c = load_golden("config_subject_03.npz")
    cx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"])
    yield cx
    cx.close()


@pytest.fixture(scope="module")
def pctx(skel):
    from egopose_amd.pose2d import Pose2DContext
    return Pose2DContext(skel)


def _frames(skel, pctx, n, seed, all_invalid=False):
    """Random poses (joint angles over the full range, root headings over +-pi) and keypoints near their projection with the
    fixture's mix of confidences: all seen, left knee / left shoulder / one hip unseen, both hips unseen, random."""
    rng = np.random.RandomState(seed)
    qpos = np.zeros((n, skel.nq))
    qpos[:, :2] = rng.normal(size=(n, 2)) * 3.0
    qpos[:, 2] = rng.uniform(0.7, 1.1, size=n)
    yaw = rng.uniform(-np.pi, np.pi, size=n)
    qpos[:, 3], qpos[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
    qpos[:, 3:7] += rng.normal(size=(n, 4)) * 0.05
    qpos[:, 3:7] /= np.linalg.norm(qpos[:, 3:7], axis=1, keepdims=True)
    qpos[:, 7:] = rng.uniform(skel.joint_range[:, 0], skel.joint_range[:, 1], size=(n, skel.nq - 7))
    flip = (rng.uniform(size=n) < 0.5).astype(np.int32)
    b2 = pctx.body2id
    gt = np.zeros((n, 12, 3))
    for i in range(n):
        pr = pctx.project_qpos(qpos[i], bool(flip[i]))
        gt[i, :, :2] = pr * rng.uniform(3000.0, 4000.0) + np.array([960.0, 540.0]) + rng.normal(size=pr.shape) * 6.0
        gt[i, :, 2] = rng.uniform(0.3, 0.95, size=12)
        kind = i % 7
        low = lambda: rng.uniform(0.0, 0.09)
        if kind == 1:
            gt[i, b2["LeftLeg"], 2] = low()
        elif kind == 2:
            gt[i, b2["LeftArm"], 2] = low()
        elif kind == 3:
            gt[i, b2["LeftUpLeg"], 2] = low()
        elif kind == 4:
            gt[i, b2["RightUpLeg"], 2] = low()
        elif kind == 5:
            gt[i, b2["LeftUpLeg"], 2], gt[i, b2["RightUpLeg"], 2] = low(), low()
        elif kind == 6:
            gt[i, :, 2] = rng.uniform(0.0, 1.0, size=12)
            gt[i, b2["RightUpLeg"], 2] = 0.7
        if all_invalid:
            gt[i, b2["LeftUpLeg"], 2], gt[i, b2["RightUpLeg"], 2] = low(), 0.1          # exactly 0.1 is not > 0.1
    return qpos, gt, flip


def _reference(skel, pctx, qpos, gt, flip):
    from oracle import dynamics as D
    n = len(qpos)
    p, dist, valid = np.zeros((n, 12, 2)), np.zeros(n), np.zeros(n, bool)
    for i in range(n):
        x = D.fk(skel, qpos[i])[1][pctx.body_index]
        valid[i] = pctx.check_gt(gt[i])
        if valid[i]:
            p[i] = pctx.align_xpos(x, gt[i], flip=bool(flip[i]))
            dist[i] = pctx.get_pose_dist(p[i], gt[i])
        else:
            p[i] = pctx.project_xpos(x, bool(flip[i]))
    return p, dist, valid


@pytest.mark.parametrize("n", [1, 63, 130])
def test_pose2d_kernel_against_the_restatement(ctx, skel, pctx, n):
    """One frame; a ragged last workgroup (63 = 15 x 4 + 3 waves); more than one workgroup and the branch mix several times over.
    Output buffers hold 3 canary rows behind the n the kernel is given."""
    qpos, gt, flip = _frames(skel, pctx, n, seed=40 + n)
    p_ref, d_ref, v_ref = _reference(skel, pctx, qpos, gt, flip)
    if n > 1:
        assert v_ref.any() and (~v_ref).any()
    ctx.set_pose2d_bodies(*pctx.kernel_tables())
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device="cuda")
    p = torch.full((n + 3, 12, 2), -7.0, dtype=torch.float64, device="cuda")
    dist = torch.full((n + 3,), -7.0, dtype=torch.float64, device="cuda")
    valid = torch.full((n + 3,), -7, dtype=torch.int32, device="cuda")
    ctx.pose2d(dev(qpos, np.float64), dev(gt, np.float64), dev(flip, np.int32), out=dict(p=p[:n], dist=dist[:n], valid=valid[:n]))
    torch.cuda.synchronize()
    assert (p[n:] == -7.0).all() and (dist[n:] == -7.0).all() and (valid[n:] == -7).all()
    p, dist, valid = p[:n].cpu().numpy(), dist[:n].cpu().numpy(), valid[:n].cpu().numpy()
    np.testing.assert_array_equal(valid, v_ref.astype(np.int32))
    assert (dist[~v_ref] == 0.0).all()
    err_p = float((np.abs(p - p_ref) / np.maximum(1.0, np.abs(p_ref))).max())
    err_d = float(np.abs(dist - d_ref).max())
    print("pose2d n=%d: max relative error of p %.3e, max absolute error of dist %.3e" % (n, err_p, err_d))
    assert err_p <= P_RTOL and err_d <= DIST_ATOL
    # p_out = NULL: the same dist / valid
    r = ctx.pose2d(dev(qpos, np.float64), dev(gt, np.float64), dev(flip, np.int32), want_p=False)
    assert "p" not in r
    np.testing.assert_array_equal(r["dist"].cpu().numpy(), dist)
    np.testing.assert_array_equal(r["valid"].cpu().numpy(), valid)


def test_pose2d_all_invalid_and_the_context_path(ctx, skel, pctx):
    qpos, gt, flip = _frames(skel, pctx, 9, seed=3, all_invalid=True)
    dist, valid, p = pctx.score(ctx, qpos, gt, flip, want_p=True)
    assert not valid.any() and (dist == 0.0).all()
    p_ref, _, _ = _reference(skel, pctx, qpos, gt, flip)           # the unaligned projection
    assert float((np.abs(p - p_ref) / np.maximum(1.0, np.abs(p_ref))).max()) <= P_RTOL
    d0, v0 = pctx.score(ctx, qpos[:0], gt[:0], flip[:0])
    assert d0.shape == (0,) and v0.shape == (0,)
    with pytest.raises(ValueError):
        ctx.pose2d(torch.zeros(2, 58, dtype=torch.float64, device="cuda"), torch.zeros(2, 12, 3, dtype=torch.float64, device="cuda"),
                   torch.zeros(2, dtype=torch.int32, device="cuda"))


def test_pose2d_golden_frames_through_the_host_path(pctx):
    """The kernel cannot be fed body positions, so the reference's frames are checked through the host path."""
    g = load_golden("pose2d.npz")
    for i in np.nonzero(g["valid"])[0][:8]:
        p = pctx.align_xpos(g["xpos"][i][pctx.body_index], g["gt"][i], flip=bool(g["flip"][i]))
        np.testing.assert_allclose(pctx.get_pose_dist(p, g["gt"][i]), g["dist"][i], rtol=1e-12, atol=1e-12)


def _stats_case(pctx, skel, seed=7):
    """Two smooth takes + synthetic keypoints: traj_ub cuts take 'a', take 'b' has a negative tpv_offset and is flipped; every 5th
    keypoint frame has both hips unseen."""
    rng = np.random.RandomState(seed)

    def traj(n):
        q = np.zeros((n, skel.nq))
        q[:, :2] = np.cumsum(rng.normal(size=(n, 2)) * 0.02, 0)
        q[:, 2] = 0.9
        yaw = np.cumsum(rng.normal(size=n) * 0.05) + rng.uniform(-3, 3)
        q[:, 3], q[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
        q[:, 7:] = np.cumsum(rng.normal(size=(n, skel.nq - 7)) * 0.02, 0)
        return q

    b2 = pctx.body2id

    def loader(take, gt_fr):
        r = np.random.RandomState(1000 * (take == "b") + gt_fr)
        gt = np.zeros((12, 3))
        gt[:, 0], gt[:, 1], gt[:, 2] = r.uniform(400, 1500, 12), np.sort(r.uniform(100, 1000, 12)), r.uniform(0.0, 1.0, 12)
        gt[b2["RightUpLeg"], 2] = 0.8
        if gt_fr % 5 == 0:
            gt[b2["RightUpLeg"], 2] = gt[b2["LeftUpLeg"], 2] = 0.05
        return gt
    return {"a": traj(14), "b": traj(9)}, {"traj_ub": {"a": 11}, "tpv_offset": {"b": -3}, "tpv_flip": {"b": True}}, loader


def test_stats_loops_on_the_kernel_match_the_host_loop(ctx, skel, pctx):
    import types
    from egopose_amd.pose2d import eval_forecast_wild_stats, eval_pose_wild_stats
    trajs, meta, loader = _stats_case(pctx, skel)
    cfg = types.SimpleNamespace(fr_margin=3)
    a = eval_pose_wild_stats({"traj_pred": trajs}, meta, loader, cfg, backend="hip", ctx=ctx, pose_ctx=pctx)
    b = eval_pose_wild_stats({"traj_pred": trajs}, meta, loader, cfg, backend="host", pose_ctx=pctx)
    wins = {"a": np.stack([trajs["a"][s:s + 9] for s in (0, 2, 5)]), "b": trajs["b"][None]}
    c = eval_forecast_wild_stats({"traj_pred": wins}, meta, loader, cfg, horizon=5, backend="hip", ctx=ctx, pose_ctx=pctx)
    d = eval_forecast_wild_stats({"traj_pred": wins}, meta, loader, cfg, horizon=5, backend="host", pose_ctx=pctx)
    for x, y in ((a, b), (c, d)):
        assert np.isfinite(x["pose_dist"]) and x["pose_dist"] > 0
        np.testing.assert_allclose(x["pose_dist"], y["pose_dist"], rtol=1e-12)      # (the restatement's own tolerance against the reference)
        assert x["accels"] == y["accels"]
