"""GPU parity: the HIP kernels (through the C-ABI) against the golden vectors generated from the
reference and against the oracle on seeded inputs.

Tolerances (BASELINE.md "parity gates"): float64 variants <= 1e-10 (abs, on O(1) quantities; torques are
O(100) so they get rtol 1e-10), float32 variants <= 1e-5 relative to the quantity's scale.
"""
import numpy as np
import pytest
import torch
import yaml

from conftest import load_golden
from oracle import humanoid as H, reward as R, gae as G, zfilter as Z

pytestmark = pytest.mark.gpu


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


@pytest.fixture(scope="module")
def ctx(skel):
    from egopose_amd.hip import EgpContext
    c = load_golden("config_subject_03.npz")
    ws = dict(zip([str(k) for k in c["reward_keys"]], [float(v) for v in c["reward_vals"]]))
    cx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"],
                    reward_weights=ws, episode_len=int(c["env_episode_len"]))
    yield cx
    cx.close()


# ------------------------------------------------------------------------------------------------ K4 / K3
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 2e-6)])
def test_body_quat_and_obs_golden(ctx, dtype, tol):
    g = load_golden("body_quat_obs.npz")
    bq = ctx.body_quat(dev(g["qpos"], dtype)).cpu().numpy()
    np.testing.assert_allclose(bq, g["bquat"], rtol=0, atol=tol)
    obs = ctx.obs(dev(g["qpos"], dtype), dev(g["qvel"], dtype)).cpu().numpy()
    np.testing.assert_allclose(obs, g["obs"], rtol=tol, atol=tol * 10)


def test_body_quat_angle_range(ctx, skel):
    """The kernels' own float64 sincos (two-FMA Cody-Waite reduction, egp_quat.hpp) against the oracle's libm over the whole
    range it serves -- many turns, the reduction's quadrant boundaries -- and beyond 2^18 rad, where it hands over to the
    library routine."""
    rng = np.random.RandomState(3)
    n = 4096
    qpos = np.zeros((n, 59))
    qpos[:, 3] = 1.0
    ang = np.concatenate([rng.uniform(-1e3, 1e3, (n // 4, 52)), rng.uniform(-2.5e5, 2.5e5, (n // 4, 52)),
                          (rng.randint(-4000, 4000, (n // 4, 52)) + rng.choice([0.0, 1e-9, -1e-9, 0.5], (n // 4, 52))) * (np.pi / 2),
                          rng.uniform(-3e6, 3e6, (n // 4, 52))])
    qpos[:, 7:] = ang
    want = H.body_quat(qpos, skel.body_qpos_start, skel.body_ndof)
    got = ctx.body_quat(dev(qpos, torch.float64)).cpu().numpy()
    # half-angles up to 1.5e6 rad: one ulp of the ARGUMENT is 2e-10 there, the small ranges must hold 1e-12
    np.testing.assert_allclose(got[: n // 4], want[: n // 4], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got[n // 4: 3 * n // 4], want[n // 4: 3 * n // 4], rtol=0, atol=1e-10)
    np.testing.assert_allclose(got[3 * n // 4:], want[3 * n // 4:], rtol=0, atol=2e-9)
    np.testing.assert_allclose(np.linalg.norm(got.reshape(n, 21, 4), axis=2), 1.0, rtol=0, atol=1e-12)


def test_obs_and_body_quat_edge_sizes(ctx):
    g = load_golden("body_quat_obs.npz")
    assert ctx.body_quat(dev(g["qpos"][:0])).shape == (0, 84)          # empty batch is a no-op
    assert ctx.obs(dev(g["qpos"][:0]), dev(g["qvel"][:0])).shape == (0, 115)
    one = ctx.obs(dev(g["qpos"][:1]), dev(g["qvel"][:1])).cpu().numpy()
    np.testing.assert_allclose(one, g["obs"][:1], rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError):
        ctx.obs(dev(g["qpos"][:4]), dev(g["qvel"][:3]))


# ------------------------------------------------------------------------------------------------ K1
@pytest.mark.parametrize("variant", [0, 1, 2, 3])     # tree-ordered on the lane grid / generic LDS / dense in-register / tree-ordered, lane per row
def test_pd_torque_golden_f64(ctx, variant):
    g = load_golden("pd_torque.npz")
    ctx.set_pd_variant(variant)
    try:
        tq, raw = ctx.pd_torque(dev(g["qpos"]), dev(g["qvel"]), dev(g["action"]), dev(g["qM"]), dev(g["C"]), want_raw=True)
    finally:
        ctx.set_pd_variant(0)
    np.testing.assert_allclose(raw.cpu().numpy(), g["torque"], rtol=1e-10, atol=1e-9)
    np.testing.assert_allclose(tq.cpu().numpy(), g["torque_clipped"], rtol=1e-10, atol=1e-9)


def test_pd_torque_golden_f32_io(ctx):
    g = load_golden("pd_torque.npz")
    f = torch.float32
    tq, raw = ctx.pd_torque(dev(g["qpos"], f), dev(g["qvel"], f), dev(g["action"], f), dev(g["qM"], f), dev(g["C"], f), want_raw=True)
    scale = np.abs(g["torque"]).max()
    assert np.abs(raw.cpu().numpy() - g["torque"]).max() / scale < 1e-5


def test_pd_torque_ragged_and_large_vs_oracle(ctx, skel):
    c = load_golden("config_subject_03.npz")
    rng = np.random.RandomState(5)
    M0 = skel.zero_pose_inertia()
    for n in (1, 3, 5, 130):          # not multiples of the 4-envs-per-block tiling
        d = 1.0 + 0.2 * rng.uniform(-1, 1, size=(n, 58))
        qM = np.stack([skel.sparse_from_full(M0 * di[:, None] * di[None, :]) for di in d])
        qpos = rng.normal(size=(n, 59)) * 0.3
        qvel = rng.normal(size=(n, 58)) * 3
        act = rng.normal(size=(n, 52)) * 0.5
        C = rng.normal(size=(n, 58)) * 20
        tq, raw = ctx.pd_torque(dev(qpos), dev(qvel), dev(act), dev(qM), dev(C), want_raw=True)
        M = H.full_from_sparse(qM, skel.dof_parentid, skel.dof_Madr)
        t_ref, tc_ref = H.pd_torque(qpos, qvel, act, M, C, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], skel.timestep)
        np.testing.assert_allclose(raw.cpu().numpy(), t_ref, rtol=1e-10, atol=1e-9)
        np.testing.assert_allclose(tq.cpu().numpy(), tc_ref, rtol=1e-10, atol=1e-9)
    # full size (BASELINE config 2): linearity-free property -- the solve satisfies its own equation
    n = 1024
    qM = np.tile(skel.sparse_from_full(M0), (n, 1))
    qpos, qvel = rng.normal(size=(n, 59)) * 0.3, rng.normal(size=(n, 58))
    act, C = rng.normal(size=(n, 52)) * 0.3, rng.normal(size=(n, 58)) * 5
    _, raw = ctx.pd_torque(dev(qpos), dev(qvel), dev(act), dev(qM), dev(C), want_raw=True)
    raw = raw.cpu().numpy()
    kp, kd, dt = np.r_[np.zeros(6), c["jkp"]], np.r_[np.zeros(6), c["jkd"]], skel.timestep
    e_q = np.c_[np.zeros((n, 6)), qpos[:, 7:] - (c["a_ref"] + act * c["a_scale"])]
    # recover qacc from tau: tau = -kp e - kd (v + a dt)  =>  a = (-(tau + kp e)/kd - v)/dt   (actuated dofs)
    acc_act = (-(raw + c["jkp"] * e_q[:, 6:]) / c["jkd"] - qvel[:, 6:]) / dt
    A = M0 + np.diag(kd) * dt
    rhs = -C - kp * e_q - kd * qvel
    # residual of the actuated block after eliminating the 6 root rows
    Arr, Ara, Aar, Aaa = A[:6, :6], A[:6, 6:], A[6:, :6], A[6:, 6:]
    S = Aaa - Aar @ np.linalg.solve(Arr, Ara)
    rs = rhs[:, 6:] - (Aar @ np.linalg.solve(Arr, rhs[:, :6].T)).T
    resid = acc_act @ S.T - rs
    assert np.abs(resid).max() / np.abs(rs).max() < 1e-8


# ------------------------------------------------------------------------------------------------ K2
def _upload_golden_expert(ctx, g):
    take = {k: g["expert_" + k] for k in ["qpos", "qvel", "rlinv_local", "rangv", "rq_rmh", "ee_pos", "bquat", "bangvel"]}
    take["head_height_lb"] = 1.2
    ctx.upload_experts([take])


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-10), (torch.float32, 1e-5)])
def test_reward_golden(ctx, dtype, tol):
    g = load_golden("reward.npz")
    _upload_golden_expert(ctx, g)
    wsets = [yaml.safe_load(str(s)) for s in g["wset_json"]]
    i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32, device="cuda")
    try:
        for wi, ws in enumerate(wsets):
            ctx.set_reward_weights(ws)
            sel = np.where(g["wset"] == wi)[0]
            # end_reward is a per-call scalar: group by value (each golden case has its own)
            for j in sel:
                r, ci = ctx.reward(dev(g["cur_qpos"][[j]], dtype), dev(g["prev_qpos"][[j]], dtype), dev(g["ee_wpos"][[j]], dtype),
                                   i32(g["t"][[j]]), i32(g["start_ind"][[j]] + g["t"][[j]]), i32(g["end"][[j]]),
                                   float(g["end_reward"][j]))
                np.testing.assert_allclose(ci.cpu().numpy()[0], g["c_info"][j], rtol=0, atol=tol * 5)
                np.testing.assert_allclose(r.cpu().numpy()[0], g["reward"][j], rtol=tol, atol=tol * 5)
            # batched call, end_reward 0 -> compare with golden minus the per-case bonus
            r, ci = ctx.reward(dev(g["cur_qpos"][sel], dtype), dev(g["prev_qpos"][sel], dtype), dev(g["ee_wpos"][sel], dtype),
                               i32(g["t"][sel]), i32(g["start_ind"][sel] + g["t"][sel]), i32(g["end"][sel]), 0.0)
            want = g["reward"][sel] - np.where(g["end"][sel], g["end_reward"][sel], 0.0)
            np.testing.assert_allclose(r.cpu().numpy(), want, rtol=tol, atol=tol * 5)
            np.testing.assert_allclose(ci.cpu().numpy(), g["c_info"][sel], rtol=0, atol=tol * 5)
    finally:
        ctx.set_reward_weights(wsets[0])


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-10), (torch.float32, 1e-5)])
def test_reward_and_pose_features_in_the_root_frame(skel, dtype, tol):
    """cfg.obs_coord = 'root' reaches the reward (reward_function.py:19,23): K2 and the learner convention of K7 against the
    reference's own numbers (tests/golden/reward_root.npz); the same cases under 'heading' differ and are matched too."""
    from egopose_amd.hip import EgpContext
    g = load_golden("reward_root.npz")
    c = load_golden("config_subject_03.npz")
    wsets = [yaml.safe_load(str(s)) for s in g["wset_json"]]
    i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32, device="cuda")
    for coord, rk, ck in (("root", "reward", "c_info"), ("heading", "reward_heading", "c_info_heading")):
        cx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"], episode_len=int(g["episode_len"]),
                        obs_options=dict(obs_coord=coord))
        _upload_golden_expert(cx, g)
        for wi, ws in enumerate(wsets):
            cx.set_reward_weights(ws)
            sel = np.where(g["wset"] == wi)[0]
            r, ci = cx.reward(dev(g["cur_qpos"][sel], dtype), dev(g["prev_qpos"][sel], dtype), dev(g["ee_wpos"][sel], dtype),
                              i32(g["t"][sel]), i32(g["start_ind"][sel] + g["t"][sel]), i32(g["end"][sel]), 0.0)
            want = g[rk][sel] - np.where(g["end"][sel], g["end_reward"][sel], 0.0)
            np.testing.assert_allclose(ci.cpu().numpy(), g[ck][sel], rtol=0, atol=tol * 5, err_msg=coord)
            np.testing.assert_allclose(r.cpu().numpy(), want, rtol=tol, atol=tol * 5, err_msg=coord)
        f = cx.pose_features(dev(g["cur_qpos"], dtype), dev(g["prev_qpos"], dtype), dev(g["ee_wpos"], dtype))
        if coord == "root":
            vtol = tol * 50          # velocities are O(10) finite differences over dt = 1/30
            np.testing.assert_allclose(f["rlinv_local"].cpu().numpy(), g["learner_qvel_root"][:, :3], rtol=vtol, atol=vtol)
            np.testing.assert_allclose(f["rangv"].cpu().numpy(), g["learner_qvel_root"][:, 3:6], rtol=vtol, atol=vtol)
            np.testing.assert_allclose(f["ee_pos"].cpu().numpy(), g["learner_ee_root"], rtol=0, atol=tol * 5)
        # the expert convention (gen_expert.py) stays in the heading frame whatever cfg.obs_coord says
        fe = cx.pose_features(dev(g["cur_qpos"], dtype), dev(g["prev_qpos"], dtype), dev(g["ee_wpos"], dtype), expert_convention=True)
        np.testing.assert_allclose(fe["ee_pos"].cpu().numpy(), H.ee_pos(g["cur_qpos"], g["ee_wpos"], "heading"), rtol=0, atol=tol * 5)
        cx.close()


def test_action_type_torque_and_position_controls(skel):
    """do_simulation's control law (humanoid_v1.py:167-172) through the K1 entry point under both action types, against the
    controls the reference wrote into data.ctrl (tests/golden/do_simulation.npz); float32 i/o; unknown types refused."""
    from egopose_amd.hip import EgpContext
    g = load_golden("do_simulation.npz")
    c = load_golden("config_subject_03.npz")
    for mode in ("position", "torque"):
        cx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"], obs_options=dict(action_type=mode))
        for variant in ((0, 1, 2, 3) if mode == "position" else (0, 1)):
            cx.set_pd_variant(variant)
            for s in range(g["qpos"].shape[1]):
                tq = cx.pd_torque(dev(g["qpos"][:, s]), dev(g["qvel"][:, s]), dev(g["action"]), dev(g["qM"]), dev(g["C"]))
                np.testing.assert_allclose(tq.cpu().numpy(), g["ctrl_" + mode][:, s], rtol=1e-10, atol=1e-9, err_msg="%s v%d" % (mode, variant))
        cx.set_pd_variant(0)
        f32 = torch.float32
        tq = cx.pd_torque(dev(g["qpos"][:, 0], f32), dev(g["qvel"][:, 0], f32), dev(g["action"], f32), dev(g["qM"], f32), dev(g["C"], f32))
        # (float32 i/o on PD targets of up to 1 000 rad: the rounding of the inputs alone moves the unclipped torques by 1e-2)
        np.testing.assert_allclose(tq.cpu().numpy(), g["ctrl_" + mode][:, 0], rtol=1e-4, atol=5e-2 if mode == "position" else 1e-4)
        cx.close()
    with pytest.raises(ValueError, match="action_type"):
        EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"], obs_options=dict(action_type="velocity"))


def test_reward_active_mask_and_state_errors(ctx, skel):
    from egopose_amd.hip import EgpContext
    g = load_golden("reward.npz")
    _upload_golden_expert(ctx, g)
    i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32, device="cuda")
    sel = np.arange(8)
    act = np.array([1, 0, 1, 1, 0, 1, 1, 1])
    r, ci = ctx.reward(dev(g["cur_qpos"][sel]), dev(g["prev_qpos"][sel]), dev(g["ee_wpos"][sel]), i32(g["t"][sel]),
                       i32(g["start_ind"][sel] + g["t"][sel]), i32(g["end"][sel]), 0.0, active=i32(act))
    r = r.cpu().numpy()
    assert r[1] == 0.0 and r[4] == 0.0 and (ci.cpu().numpy()[[1, 4]] == 0).all() and (r[[0, 2, 3]] > 0).all()
    c = load_golden("config_subject_03.npz")
    fresh = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"])
    with pytest.raises(RuntimeError, match="egp_upload_experts"):      # reward before the expert table is resident
        fresh.reward(dev(g["cur_qpos"][sel]), dev(g["prev_qpos"][sel]), dev(g["ee_wpos"][sel]), i32(g["t"][sel]),
                     i32(g["t"][sel]), i32(g["end"][sel]), 0.0)
    fresh.close()


# ------------------------------------------------------------------------------------------------ K6
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-10), (torch.float32, 2e-5)])
def test_zfilter_blocks_match_sequential_reference(ctx, dtype, tol):
    g = load_golden("zfilter.npz")
    X = g["X"]
    st = torch.zeros(1 + 2 * 115, dtype=torch.float64, device="cuda")
    ys = []
    for lo, hi in [(0, 1), (1, 64), (64, 65), (65, 300)]:
        st2 = torch.empty_like(st)
        ys.append(ctx.zfilter(dev(X[lo:hi], dtype), st, st2, update=True, clip=5.0))
        st = st2
    s = st.cpu().numpy()
    assert s[0] == float(g["n"])
    np.testing.assert_allclose(s[1:116], g["mean"], rtol=1e-12, atol=1e-12 if dtype == torch.float64 else 1e-6)
    np.testing.assert_allclose(s[116:], g["S"], rtol=1e-10 if dtype == torch.float64 else 1e-5, atol=1e-9)
    # frozen filter == reference ZFilter.__call__(x, update=False) with the final statistics
    y = ctx.zfilter(dev(X[:16], dtype), st, update=False, clip=5.0).cpu().numpy()
    np.testing.assert_allclose(y, g["Yfrozen"], rtol=tol, atol=tol)
    # first block of one sample: n==1 branch (var = mean^2)
    np.testing.assert_allclose(ys[0].cpu().numpy()[0], g["y_first"], rtol=tol, atol=tol)
    # the last sample of a block is normalised with the same statistics as in the sequential reference
    np.testing.assert_allclose(ys[-1].cpu().numpy()[-1], g["Y"][-1], rtol=tol, atol=tol)


@pytest.mark.parametrize("n", [16385, 40000])
def test_zfilter_two_level_merge_continues_a_running_state(ctx, n):
    """More than 256 statistics tiles (> 16 384 rows): 16 workgroups reduce the tiles to 16 records and the apply kernel merges
    those into the running state itself. Against the oracle's sequential merge, starting from a non-empty state, with a mask."""
    rng = np.random.RandomState(n)
    dim = 115
    X0 = rng.normal(size=(3000, dim)) * 2 - 0.5
    X = rng.normal(size=(n, dim)) * np.linspace(0.5, 4.0, dim) + np.linspace(-2, 2, dim)
    act = (rng.uniform(size=n) < 0.8).astype(np.int32)
    st0 = torch.zeros(1 + 2 * dim, dtype=torch.float64, device="cuda")
    st1, st2 = torch.empty_like(st0), torch.empty_like(st0)
    ctx.zfilter(dev(X0), st0, st1, update=True, clip=5.0)
    y = ctx.zfilter(dev(X), st1, st2, update=True, clip=5.0, active=torch.as_tensor(act, device="cuda")).cpu().numpy()
    rs = Z.RunningStatOracle(dim)
    rs.merge_block(X0)
    rs.merge_block(X[act == 1])
    s = st2.cpu().numpy()
    assert s[0] == 3000 + act.sum()
    np.testing.assert_allclose(s[1:1 + dim], rs.mean, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(s[1 + dim:], rs.S, rtol=1e-10)
    np.testing.assert_allclose(y, Z.zfilter_apply(X, rs.mean, rs.std, 5.0), rtol=1e-10, atol=1e-10)


def test_zfilter_active_mask_and_large(ctx):
    rng = np.random.RandomState(0)
    n, dim = 5000, 115
    X = rng.normal(size=(n, dim)) * 3 + 1
    act = (rng.uniform(size=n) < 0.7).astype(np.int32)
    st0 = torch.zeros(1 + 2 * dim, dtype=torch.float64, device="cuda")
    st1 = torch.empty_like(st0)
    y = ctx.zfilter(dev(X), st0, st1, update=True, clip=5.0, active=torch.as_tensor(act, device="cuda")).cpu().numpy()
    rs = Z.RunningStatOracle(dim)
    rs.merge_block(X[act == 1])
    s = st1.cpu().numpy()
    assert s[0] == act.sum()
    np.testing.assert_allclose(s[1:1 + dim], rs.mean, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(s[1 + dim:], rs.S, rtol=1e-10)
    np.testing.assert_allclose(y, Z.zfilter_apply(X, rs.mean, rs.std, 5.0), rtol=1e-10, atol=1e-10)
    # no active rows: state passes through unchanged
    st2 = torch.empty_like(st0)
    ctx.zfilter(dev(X[:10]), st1, st2, update=True, clip=5.0, active=torch.zeros(10, dtype=torch.int32, device="cuda"))
    np.testing.assert_array_equal(st2.cpu().numpy(), s)


# ------------------------------------------------------------------------------------------------ K5
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-10), (torch.float32, 1e-4)])
def test_gae_golden(ctx, dtype, tol):
    g = load_golden("gae.npz")
    for mk, gm, tu, a_key, r_key in [("masks", "gamma", "tau", "adv", "ret"), ("masks2", "gamma2", "tau2", "adv2", "ret2")]:
        adv, ret, stats = ctx.gae(dev(g["rewards"], dtype), dev(g[mk], dtype), dev(g["values"].ravel(), dtype), float(g[gm]), float(g[tu]))
        np.testing.assert_allclose(ret.cpu().numpy(), g[r_key].ravel(), rtol=tol, atol=tol)   # north-star: returns within 1e-4 fp32
        ctx.gae_standardize(adv, stats)
        np.testing.assert_allclose(adv.cpu().numpy(), g[a_key].ravel(), rtol=tol, atol=tol)   # advantages within 1e-4 fp32


def test_gae_sizes_vs_oracle(ctx):
    rng = np.random.RandomState(3)
    # chunk edges (4 samples per thread), tile edges (2 048 per workgroup), the config-2 sweep size, and more than 1 024 tiles
    # (k_gae_stats then merges several tile partials per thread). gamma tau = 0.9025: every look to the right ends after one tile;
    # the longer looks are test_scan_reference_gpu.py's
    for n in (1, 2, 7, 8, 9, 31, 32, 33, 1000, 2047, 2048, 2049, 204800, 2048 * 1024 + 5):
        r = rng.uniform(0, 1.2, size=n)
        m = (rng.uniform(size=n) > 0.02).astype(float)
        v = rng.normal(size=n) * 2
        adv, ret, stats = ctx.gae(dev(r), dev(m), dev(v), 0.95, 0.95)
        if n <= 33000:
            a_ref, r_ref, raw_ref = G.estimate_advantages(r, m, v, 0.95, 0.95)
        else:   # size-independent check at full size: the recurrence holds element-wise
            a = adv.cpu().numpy()
            nxt_a = np.r_[a[1:], 0.0]
            nxt_v = np.r_[v[1:], 0.0]
            np.testing.assert_allclose(a, r + 0.95 * nxt_v * m - v + 0.95 * 0.95 * m * nxt_a, rtol=1e-11, atol=1e-11)
            np.testing.assert_allclose(ret.cpu().numpy(), v + a, rtol=1e-12, atol=1e-12)
            s = stats.cpu().numpy()
            np.testing.assert_allclose([s[0], s[1], s[2]], [n, a.mean(), ((a - a.mean()) ** 2).sum()], rtol=1e-9)
            continue
        np.testing.assert_allclose(adv.cpu().numpy(), raw_ref.ravel(), rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(ret.cpu().numpy(), r_ref.ravel(), rtol=1e-11, atol=1e-11)
        if n > 1:
            ctx.gae_standardize(adv, stats)
            np.testing.assert_allclose(adv.cpu().numpy(), a_ref.ravel(), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("n", [134656, 204800])
def test_gae_f32_at_update_batch_size_vs_oracle(ctx, n):
    """north_star: "returns/advantages within 1e-4 fp32 given identical trajectories" at the batch sizes the update really runs
    the float32 kernel on (k_gae_onepass<float>: ~134 k rows per iteration of config 2, 204 800 = the slot sweep's), against the
    oracle's reverse sweep (core/common.py:5-25) on episodes of the rollout's shape: rewards in [0, 1.2], 30-200-step episodes."""
    rng = np.random.RandomState(n)
    r = rng.uniform(0, 1.2, size=n)
    m = np.ones(n)
    ends = np.cumsum(rng.randint(30, 201, size=n // 30 + 1))
    m[ends[ends < n] - 1] = 0.0
    m[-1] = 0.0
    v = rng.normal(size=n) * 2 + 5
    a_ref, r_ref, raw_ref = G.estimate_advantages(r, m, v, 0.95, 0.95)
    f32 = torch.float32
    adv, ret, stats = ctx.gae(dev(r, f32), dev(m, f32), dev(v, f32), 0.95, 0.95)
    np.testing.assert_allclose(ret.cpu().numpy(), r_ref.ravel(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(adv.cpu().numpy(), raw_ref.ravel(), rtol=1e-4, atol=1e-4)
    ctx.gae_standardize(adv, stats)
    np.testing.assert_allclose(adv.cpu().numpy(), a_ref.ravel(), rtol=1e-4, atol=1e-4)
    s = stats.cpu().numpy()
    np.testing.assert_allclose([s[0], s[1]], [n, raw_ref.mean()], rtol=1e-4)


# ------------------------------------------------------------------------------------------------ engine
ENGINE_MODES = {                     # env switches read by egp_engine_create -> substeps per K1 launch
    "resident": ({}, 15),                                          # (go words in HBM, pushed by the host with fenced stores: the default)
    "resident-pinned-go": ({"EGP_BAR_GO": "0"}, 15),               # go words in pinned host memory, pulled by the waves
    "per-substep": ({"EGP_SERVER": "0"}, 1),                       # the fallback: one K1 launch per substep, completion flag polled
    # a resident wave serving 2 / 4 envs in turn (k_pd_server_tree58_multi: what the engine takes when the slots do not fit the chip
    # one env per wave -- more than 4 envs per CU, or fewer CUs to be had); forced here at sizes that would fit
    "resident-2-per-wave": ({"EGP_SERVER_KE": "2"}, 15),
    "resident-4-per-wave": ({"EGP_SERVER_KE": "4"}, 15),
}
ENGINE_KE = {"resident": 1, "resident-pinned-go": 1, "per-substep": 0, "resident-2-per-wave": 2, "resident-4-per-wave": 4}


@pytest.mark.parametrize("mode", list(ENGINE_MODES))
def test_engine_step_matches_host_loop(ctx, skel, mode, monkeypatch):
    """15 substeps of {K1 on GPU <-> surrogate physics on host threads} == the same loop done
    env by env with the oracle's stable-PD on the CPU (do_simulation, humanoid_v1.py:158-177),
    in every mode the engine can run the substep loop in."""
    from egopose_amd.physics import SurrogatePhysics, RolloutEngine
    for k, v in ENGINE_MODES[mode][0].items():
        monkeypatch.setenv(k, v)
    c = load_golden("config_subject_03.npz")
    g = load_golden("body_quat_obs.npz")
    n = 37
    rng = np.random.RandomState(9)
    qpos0, qvel0 = g["qpos"][:n], g["qvel"][:n] * 0.2
    action = rng.normal(size=(n, 52)) * 0.2
    for n_groups, n_threads in [(1, 3), (2, 4)]:
        ph = SurrogatePhysics(skel, n)
        eng = RolloutEngine(ctx, ph, n, n_threads=n_threads, n_groups=n_groups)
        assert eng.substeps_per_launch == ENGINE_MODES[mode][1] and eng.envs_per_wave == ENGINE_KE[mode]
        assert eng.envs_per_wave == 0 or eng.resident_capacity >= 1
        eng.reset(np.arange(n), qpos0, qvel0)
        act_d = dev(action)
        torch.cuda.synchronize()
        for gi in range(n_groups):
            eng.step_async(gi, act_d)
        for gi in range(n_groups):
            eng.wait(gi)
        torch.cuda.synchronize()
        got_q, got_v, got_ee = eng.qpos.cpu().numpy(), eng.qvel.cpu().numpy(), eng.ee_wpos.cpu().numpy()
        head_z = eng.head_z.copy()
        eng.close()
        ph.close()
        # host loop
        ref = SurrogatePhysics(skel, n)
        for e in range(n):
            ref.reset(e, qpos0[e], qvel0[e])
            for s in range(15):
                q, v, qM, bias, _ = ref.drain(e, want_xpos=False)
                M = H.full_from_sparse(qM, skel.dof_parentid, skel.dof_Madr)
                _, tc = H.pd_torque(q, v, action[e], M, bias, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], skel.timestep)
                ref.step(e, tc[0])
            q, v, _, _, xpos = ref.drain(e)
            np.testing.assert_allclose(got_q[e], q, rtol=1e-9, atol=1e-9)
            np.testing.assert_allclose(got_v[e], v, rtol=1e-8, atol=1e-8)
            np.testing.assert_allclose(got_ee[e], xpos[skel.ee_body].ravel(), rtol=1e-9, atol=1e-9)
            np.testing.assert_allclose(head_z[e], xpos[6, 2], rtol=1e-9, atol=1e-9)
        ref.close()


def test_engine_keeps_the_resident_form_when_cus_are_masked():
    """A process that gets 240 of the 256 CUs (ROC_GLOBAL_CU_MASK; a CU-masked partition, a co-tenant): the occupancy calculator
    still answers for the whole chip, the kernel's own residency probe counts what is really there, and the engine lets a wave serve
    two envs instead of waiting for workgroups that never become resident (or dropping to one launch per substep). Two env-steps of
    1 024 slots under the mask == without it (different K1 forms: 1e-9). The mask must be set before HIP starts: subprocesses."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(repo, "tools", "cu_mask_check.py"), "--envs", "1024", "--step"]

    def run(extra):
        out = subprocess.run(cmd, env=dict(os.environ, **extra), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads(out.stdout.strip().splitlines()[-1])
    full = run({})
    cus = full["cus_reported"]
    if cus < 64:
        pytest.skip("needs a chip with >= 64 CUs")
    keep = cus - 16
    masked = run({"ROC_GLOBAL_CU_MASK": "0x" + "f" * (keep // 4)})
    assert full["substeps_per_launch"] == 15 and masked["substeps_per_launch"] == 15
    assert full["envs_per_wave"] == 1 or full["resident_capacity"] < 256
    assert masked["resident_capacity"] <= keep, "the probe must not count more workgroups than CUs were left: %r" % (masked,)
    if 4 * masked["resident_capacity"] < 1024:
        assert masked["envs_per_wave"] >= 2
    assert masked["qpos_abs_sum"] == pytest.approx(full["qpos_abs_sum"], rel=1e-9)
    np.testing.assert_allclose(masked["qpos_probe"], full["qpos_probe"], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("mode", ["resident", "per-substep", "resident-2-per-wave"])
def test_engine_step_with_torque_actions(skel, mode, monkeypatch):
    """cfg.action_type = 'torque' through the engine: every substep applies clip(a_ref + a * a_scale) (humanoid_v1.py:167-172),
    no PD solve -- against the host loop with the oracle's control law, in every mode of the substep loop."""
    from egopose_amd.hip import EgpContext
    from egopose_amd.physics import SurrogatePhysics, RolloutEngine
    for k, v in ENGINE_MODES[mode][0].items():
        monkeypatch.setenv(k, v)
    c = load_golden("config_subject_03.npz")
    g = load_golden("body_quat_obs.npz")
    cx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"], obs_options=dict(action_type="torque"))
    n = 23
    rng = np.random.RandomState(19)
    qpos0, qvel0 = g["qpos"][:n], g["qvel"][:n] * 0.2
    action = rng.normal(size=(n, 52)) * 40.0                 # some beyond the limits (50 ... 200)
    ph = SurrogatePhysics(skel, n)
    eng = RolloutEngine(cx, ph, n, n_threads=3, n_groups=2)
    eng.reset(np.arange(n), qpos0, qvel0)
    act_d = dev(action)
    torch.cuda.synchronize()
    for gi in range(2):
        eng.step_async(gi, act_d)
    for gi in range(2):
        eng.wait(gi)
    torch.cuda.synchronize()
    got_q, got_v = eng.qpos.cpu().numpy(), eng.qvel.cpu().numpy()
    eng.close()
    ph.close()
    cx.close()
    ref = SurrogatePhysics(skel, n)
    _, tc = H.control_torque("torque", None, None, action, None, None, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], skel.timestep)
    assert (np.abs(tc) == c["torque_lim"]).any()
    for e in range(n):
        ref.reset(e, qpos0[e], qvel0[e])
        for s in range(15):
            ref.step(e, tc[e])
        q, v, _, _, _ = ref.drain(e)
        np.testing.assert_allclose(got_q[e], q, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(got_v[e], v, rtol=1e-12, atol=1e-12)
    ref.close()


@pytest.mark.parametrize("ke", ["1", "4"])
def test_resident_engine_dealt_slices_are_bit_identical(ctx, skel, monkeypatch, ke):
    """With an active mask the resident engine deals its slices out to the host threads per env-step once a substep of physics
    is expensive enough (2 us per env-substep; the free surrogate stays with fixed ownership): who steps an env changes, the
    env's numbers do not, and an inactive env is never touched."""
    from egopose_amd.physics import SurrogatePhysics, RolloutEngine
    monkeypatch.setenv("EGP_SERVER_KE", ke)
    g = load_golden("body_quat_obs.npz")
    n = 203
    rng = np.random.RandomState(11)
    pick = rng.randint(0, len(g["qpos"]), n)
    qpos0, qvel0 = g["qpos"][pick], g["qvel"][pick] * 0.2
    action = dev(rng.normal(size=(n, 52)) * 0.2)
    masks = [(rng.rand(n) < p).astype(np.int32) for p in (0.6, 0.5, 0.15, 0.03)]
    masks[3][:8] = 1                                   # a crowded first slice: the case dealing is for
    out = {}
    for bal in ("fixed", "by-cost", "by-cost-8us"):
        if bal != "fixed":              # a physics step slow enough (3 / 8 us) for the engine to start dealing
            monkeypatch.setenv("EGP_SURROGATE_SUBSTEP_US", "3" if bal == "by-cost" else "8")
        ph = SurrogatePhysics(skel, n)
        eng = RolloutEngine(ctx, ph, n, n_threads=6, n_groups=2)
        assert eng.substeps_per_launch == 15
        eng.reset(np.arange(n), qpos0, qvel0)
        torch.cuda.synchronize()
        for m in masks:
            for gi in range(2):
                eng.step_async(gi, action, active_host=m)
            for gi in range(2):
                eng.wait(gi)
            torch.cuda.synchronize()
        out[bal] = (eng.qpos.cpu().numpy().copy(), eng.qvel.cpu().numpy().copy(), eng.ee_wpos.cpu().numpy().copy())
        eng.close()
        ph.close()
    for other in ("by-cost", "by-cost-8us"):
        for a, b in zip(out["fixed"], out[other]):
            np.testing.assert_array_equal(a, b)
    never = (masks[0] | masks[1] | masks[2] | masks[3]) == 0
    assert never.any()
    np.testing.assert_array_equal(out["by-cost"][0][never], qpos0[never])
    assert np.abs(out["by-cost"][0][~never] - qpos0[~never]).max() > 0


def test_surrogate_always_dirty_changes_traffic_not_numbers(ctx, skel, monkeypatch):
    """EGP_SURROGATE_ALWAYS_DIRTY=1 (the inertia row crosses to the GPU on every substep, the traffic of a backend with a
    pose-dependent qM) must give bit-identical env-steps to the default (inertia sent once)."""
    from egopose_amd.physics import SurrogatePhysics, RolloutEngine
    g = load_golden("body_quat_obs.npz")
    n = 21
    rng = np.random.RandomState(4)
    qpos0, qvel0 = g["qpos"][:n], g["qvel"][:n] * 0.2
    actions = [rng.normal(size=(n, 52)) * 0.2 for _ in range(2)]
    outs = []
    for dirty in ("0", "1"):
        monkeypatch.setenv("EGP_SURROGATE_ALWAYS_DIRTY", dirty)
        ph = SurrogatePhysics(skel, n)
        eng = RolloutEngine(ctx, ph, n, n_threads=3, n_groups=1)
        assert eng.substeps_per_launch == 15
        eng.reset(np.arange(n), qpos0, qvel0)
        for a in actions:
            ad = dev(a)
            torch.cuda.synchronize()
            eng.step_async(0, ad)
            eng.wait(0)
        torch.cuda.synchronize()
        outs.append((eng.qpos.cpu().numpy().copy(), eng.qvel.cpu().numpy().copy(), eng.ee_wpos.cpu().numpy().copy()))
        eng.close()
        ph.close()
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


def _changing_inertia_env_steps(eng, be, qpos0, qvel0, seed=4):
    """reset all envs -> env-step -> re-seat envs 3, 4, 17 -> env-step on a VaryingInertiaBackend engine; returns the actions,
    the final qpos and every torque row the backend was handed, per env."""
    n = be.n_env
    rng = np.random.RandomState(seed)
    be.torques = [[] for _ in range(n)]
    eng.reset(np.arange(n), qpos0, qvel0)
    actions = []
    for step in range(2):
        a = rng.normal(size=(n, 52)) * 0.2
        actions.append(a)
        act_d = dev(a)
        torch.cuda.synchronize()
        eng.step_async(0, act_d)
        eng.wait(0)
        if step == 0:                                  # re-seat a few envs between the two env-steps (ordered by the engine, no sync)
            ids = np.array([3, 4, 17])
            eng.reset(ids, qpos0[ids], qvel0[ids])
    torch.cuda.synchronize()
    assert not be.physics.errors
    return actions, eng.qpos.cpu().numpy(), [np.array(t) for t in be.torques]


@pytest.mark.parametrize("mode", ["resident", "per-substep", "resident-2-per-wave"])
def test_engine_changing_inertia_repeats_bit_identically(ctx, skel, mode, monkeypatch):
    """Stress of the inertia path's orderings (K1 once read inertia rows a reset's scatter kernel was still
    writing -- found by one flaky run): the reset / env-step / partial reset / env-step sequence 50 times on one engine, no host
    synchronisation between a reset and the env-step behind it; every torque row and the final state bit-identical to the first run."""
    from conftest import VaryingInertiaBackend
    from egopose_amd.physics import RolloutEngine
    for k, v in ENGINE_MODES[mode][0].items():
        monkeypatch.setenv(k, v)
    g = load_golden("body_quat_obs.npz")
    n = 26
    qpos0, qvel0 = g["qpos"][:n], g["qvel"][:n] * 0.2
    be = VaryingInertiaBackend(skel, n)
    eng = RolloutEngine(ctx, be, n, n_threads=3, n_groups=1)
    assert eng.substeps_per_launch == ENGINE_MODES[mode][1]
    _, q0, t0 = _changing_inertia_env_steps(eng, be, qpos0, qvel0)
    for rep in range(49):
        _, q, t = _changing_inertia_env_steps(eng, be, qpos0, qvel0)
        np.testing.assert_array_equal(q, q0, err_msg="repeat %d" % rep)
        for e in range(n):
            np.testing.assert_array_equal(t[e], t0[e], err_msg="repeat %d env %d" % (rep, e))
    eng.close()
    be.close()


@pytest.mark.parametrize("mode", list(ENGINE_MODES))
def test_engine_follows_changing_inertia(ctx, skel, mode, monkeypatch):
    """A backend whose qM changes on every step (what a MuJoCo adapter looks like): every torque row the engine
    hands to step() must come from the inertia drained just before it, over two env-steps and a partial reset."""
    from conftest import VaryingInertiaBackend
    from egopose_amd.physics import RolloutEngine
    for k, v in ENGINE_MODES[mode][0].items():
        monkeypatch.setenv(k, v)
    c = load_golden("config_subject_03.npz")
    g = load_golden("body_quat_obs.npz")
    n = 26
    qpos0, qvel0 = g["qpos"][:n], g["qvel"][:n] * 0.2
    be = VaryingInertiaBackend(skel, n)
    eng = RolloutEngine(ctx, be, n, n_threads=3, n_groups=1)
    actions, got_q, logged = _changing_inertia_env_steps(eng, be, qpos0, qvel0)
    eng.close()
    # replay on the host with the oracle's stable PD and the same per-step inertia
    from egopose_amd.physics import SurrogatePhysics
    ref = SurrogatePhysics(skel, 1)
    for e in range(n):
        ref.reset(0, qpos0[e], qvel0[e])
        k = 0
        row = 0
        for step in range(2):
            if step == 1 and e in (3, 4, 17):
                ref.reset(0, qpos0[e], qvel0[e])
                k = 0
            for s in range(15):
                q, v, qM, bias, _ = ref.drain(0, want_xpos=False)
                M = H.full_from_sparse(qM * be.scale(e, k), skel.dof_parentid, skel.dof_Madr)
                _, tc = H.pd_torque(q, v, actions[step][e], M, bias, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], skel.timestep)
                np.testing.assert_allclose(logged[e][row], tc[0], rtol=1e-8, atol=1e-8, err_msg="env %d step %d substep %d" % (e, step, s))
                ref.step(0, tc[0])
                k += 1
                row += 1
        q, *_ = ref.drain(0, want_xpos=False)
        np.testing.assert_allclose(got_q[e], q, rtol=1e-8, atol=1e-8)
    ref.close()
    be.close()


# ------------------------------------------------------------------------------------------------ fused policy step
@pytest.mark.parametrize("act,hidden,n", [("relu", (300, 200), 517), ("tanh", (64,), 3), ("sigmoid", (130, 70, 33), 64),
                                          ("tanh", (330, 6), 5)])
def test_fused_policy_step_matches_torch(act, hidden, n):
    """egp_policy_step_f32 (plain) == cat(v_out[t], state) -> MLP -> action_mean -> mean + exp(log_std) * noise in torch
    (float32; tolerance 2e-5 relative to the output scale: different summation order only).
    (330, 6): a hidden layer of two column chunks (> 5 x 64) whose width is no multiple of 4 -- the zeroed pad columns of its
    last quad feed the next layer -- on two workgroups, the second ragged."""
    from egopose_amd.nets import MLP, PolicyGaussian
    from egopose_amd import policy_step
    torch.manual_seed(3)
    H, S, T, nu = 128, 115, 9, 52
    pol = PolicyGaussian(MLP(H + S, hidden, act), nu, log_std=-0.7).cuda()
    with torch.no_grad():
        pol.action_mean.weight.mul_(10.0)
        pol.action_mean.bias.normal_()
        pol.action_log_std.normal_(std=0.3)
    assert policy_step.supported(pol)
    fp = policy_step.FusedGaussianPolicy(pol, torch.device("cuda"))
    v_out = torch.randn(n, T, H, device="cuda")
    t_idx = torch.randint(0, T, (n,), device="cuda")
    state = torch.randn(n, S, dtype=torch.float64, device="cuda") * 2
    noise = torch.randn(n, nu, device="cuda")
    act_out = torch.empty(n, nu, dtype=torch.float64, device="cuda")
    mean_out = torch.empty(n, nu, device="cuda")
    fp(v_out, t_idx, state, act_out, noise=noise, mean_out=mean_out)
    with torch.no_grad():
        x = torch.cat((v_out[torch.arange(n, device="cuda"), t_idx], state.float()), 1)
        mean, std = pol.mean_std(x)
        ref = (mean + std * noise).double()
    scale = float(ref.abs().max())
    assert float((mean_out - mean).abs().max()) <= 2e-5 * max(1.0, float(mean.abs().max()))
    assert float((act_out - ref).abs().max()) <= 2e-5 * max(1.0, scale)
    # mean action (noise None) and a parameter refresh
    with torch.no_grad():
        pol.net.affine_layers[0].weight.add_(0.01)
    fp.refresh()
    fp(v_out, t_idx, state, act_out)
    with torch.no_grad():
        mean2, _ = pol.mean_std(x)
    assert float((act_out - mean2.double()).abs().max()) <= 2e-5 * max(1.0, float(mean2.abs().max()))
    assert float((mean2 - mean).abs().max()) > 1e-4


def test_fused_policy_step_matches_the_reference_policy_vectors():
    """policy_value.npz -- PolicyGaussian over MLP[10, 6] evaluated by the REFERENCE (core/policy_gaussian.py:19-24, models/mlp.py:22-25)
    -- straight through `egp_policy_step_f32` (plain): the golden input's first 5 columns play the video context, the other 8 the
    state. float32 kernel against the reference's float64 numbers: 1e-5 (one link, no torch module in between)."""
    from egopose_amd.nets import MLP, PolicyGaussian
    from egopose_amd import policy_step
    g = load_golden("policy_value.npz")
    pol = PolicyGaussian(MLP(13, [10, 6], "relu"), 4, log_std=-2.3, fix_std=True)
    pol.load_state_dict({k[4:]: torch.as_tensor(g[k], dtype=torch.float32) for k in g.files if k.startswith("pol_")}, strict=True)
    pol = pol.cuda()
    fp = policy_step.FusedGaussianPolicy(pol, torch.device("cuda"))
    x = g["x"]
    n, H = x.shape[0], 5
    v_out = torch.zeros(n, 3, H, device="cuda")
    t_idx = torch.tensor([i % 3 for i in range(n)], device="cuda")
    v_out[torch.arange(n, device="cuda"), t_idx] = torch.as_tensor(x[:, :H], dtype=torch.float32, device="cuda")
    state = torch.as_tensor(x[:, H:], device="cuda").contiguous()
    act, mean = torch.empty(n, 4, dtype=torch.float64, device="cuda"), torch.empty(n, 4, device="cuda")
    fp(v_out, t_idx, state, act, mean_out=mean)                                   # mean action
    np.testing.assert_allclose(mean.cpu().numpy(), g["mean"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(act.cpu().numpy(), g["mean"], rtol=1e-5, atol=1e-5)
    noise = torch.as_tensor((g["a"] - g["mean"]) / g["std"], dtype=torch.float32, device="cuda")      # the draw that gave the golden action
    fp(v_out, t_idx, state, act, noise=noise)
    np.testing.assert_allclose(act.cpu().numpy(), g["a"], rtol=1e-5, atol=1e-5)


def test_policy_desc_filled_by_hand_equals_the_wrapper():
    """The plain step through an `egp_policy_desc` written out field by field here, on 5 rows of the policy_value.npz net: the
    same bits as `FusedGaussianPolicy.__call__` -- the field mapping, held without the wrapper's helpers."""
    import ctypes
    from egopose_amd.nets import MLP, PolicyGaussian
    from egopose_amd import policy_step, _lib as L
    g = load_golden("policy_value.npz")
    pol = PolicyGaussian(MLP(13, [10, 6], "relu"), 4, log_std=-2.3, fix_std=True)
    pol.load_state_dict({k[4:]: torch.as_tensor(g[k], dtype=torch.float32) for k in g.files if k.startswith("pol_")}, strict=True)
    fp = policy_step.FusedGaussianPolicy(pol.cuda(), torch.device("cuda"))
    n, H, T = 5, 5, 3
    torch.manual_seed(5)
    v_out = torch.randn(n, T, H, device="cuda")
    t_idx = torch.tensor([i % T for i in range(n)], device="cuda")
    state = torch.as_tensor(g["x"][:n, H:], device="cuda").contiguous()
    noise = torch.randn(n, 4, device="cuda")
    want, want_mean = torch.empty(n, 4, dtype=torch.float64, device="cuda"), torch.empty(n, 4, device="cuda")
    fp(v_out, t_idx, state, want, noise=noise, mean_out=want_mean)
    got, got_mean = torch.full_like(want, -9.0), torch.full_like(want_mean, -9.0)
    d = L.PolicyDesc()
    d.n = n
    d.ctx_rows, d.ctx_row_stride, d.ctx_dim, d.t_idx = v_out.data_ptr(), T * H, H, t_idx.data_ptr()
    d.state, d.state_dim = state.data_ptr(), 13 - H
    d.layers, d.n_layers, d.activation = fp.desc, 3, 1
    d.log_std, d.noise = fp.log_std.data_ptr(), noise.data_ptr()
    d.action, d.mean_out = got.data_ptr(), got_mean.data_ptr()
    L.check(fp.lib.egp_policy_step_f32(ctypes.byref(d), L.current_stream()), "egp_policy_step_f32")
    assert torch.equal(got, want) and torch.equal(got_mean, want_mean)
    assert not torch.equal(want, want_mean.double())          # (the noise took part)


@pytest.mark.parametrize("mode", ["resident", "per-substep", "resident-2-per-wave"])
def test_engine_reports_backend_failure_instead_of_hanging(ctx, skel, mode, monkeypatch):
    """A physics callback that fails in the middle of an env-step: every engine mode must come back with an error
    (the resident K1 is drained through its go words, nothing is left spinning on the GPU), stay failed for further
    steps, and leave the device usable."""
    import time
    from conftest import VaryingInertiaBackend
    from egopose_amd.physics import RolloutEngine
    for k, v in ENGINE_MODES[mode][0].items():
        monkeypatch.setenv(k, v)
    g = load_golden("body_quat_obs.npz")
    n = 26
    be = VaryingInertiaBackend(skel, n, fail_at=(9, 3))
    eng = RolloutEngine(ctx, be, n, n_threads=3, n_groups=1)
    try:
        eng.reset(np.arange(n), g["qpos"][:n], g["qvel"][:n] * 0.2)
        act = dev(np.zeros((n, 52)))
        torch.cuda.synchronize()
        t0 = time.time()
        eng.step_async(0, act)
        with pytest.raises(RuntimeError, match="physics backend failed"):
            eng.wait(0)
        assert time.time() - t0 < 4.0, "a failure must not have to wait for a timeout"
        with pytest.raises(RuntimeError):
            eng.step_async(0, act)                 # the group stays failed
        torch.cuda.synchronize()                   # nothing is left running on the device
        assert float((dev(np.ones(4)) * 2).sum().item()) == 8.0
        assert any("injected" in str(e) for e in be.physics.errors)
    finally:
        eng.close()
        be.close()


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 2e-6)])
def test_quaternion_algebra_on_device_matches_reference_vectors(dtype, tol):
    """Row a7 directly: every function of csrc/egp_quat.hpp through `egp_quat_op_*` against the reference's own
    utils/transformation.py / utils/math.py outputs (tests/golden/quat.npz: 256 random cases + the doctest values)."""
    from egopose_amd.hip import quat_op
    g = load_golden("quat.npz")
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")
    chk = lambda got, ref, t=tol: np.testing.assert_allclose(got.double().cpu().numpy(), ref, rtol=t, atol=t)
    chk(quat_op("mul", d(g["q1"]), d(g["q0"])), g["mul"], tol * 10)
    chk(quat_op("mul", d([[4.0, 1, -2, 3]]), d([[8.0, -5, 6, 7]])), g["kat_mul"][None], tol * 100)   # transformation.py doctest
    chk(quat_op("inv", d(g["q0"])), g["inv"], tol * 10)
    chk(quat_op("from_euler_sxyz", d(g["eul"])), g["from_euler"])
    qn = g["qn"]
    chk(quat_op("heading_q", d(qn[4:])), g["heading_q"])
    chk(quat_op("de_heading", d(qn[4:])), g["de_heading"])
    chk(quat_op("transform_vec_root", d(g["v3"]), d(qn)), g["tv_root"], tol * 10)
    chk(quat_op("transform_vec_heading", d(g["v3"][4:]), d(qn[4:])), g["tv_heading"], tol * 10)
    rot = quat_op("rotation", d(qn)).double().cpu().numpy()
    assert (rot[:2, 3] == 0.0).all() and (rot[:2, :3] == [1.0, 0.0, 0.0]).all()          # the 1 - w < 1e-8 branch
    if dtype == torch.float64:
        np.testing.assert_allclose(rot[:, :3], g["rot_axis"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(rot[:, 3], g["rot_angle"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(rot[:, :3] * rot[:, 3:], g["rot_vec"], rtol=1e-9, atol=1e-9)
    else:       # float32 evaluates the angle through atan2(|xyz|, w) (documented deviation): compare the rotation vector
        np.testing.assert_allclose(rot[:, :3] * rot[:, 3:], g["rot_vec"], rtol=1e-5, atol=1e-5)
    half = quat_op("diff_half_angle", d(g["q1"]), d(qn))
    chk(half, g["multi_norm"], 1e-9 if dtype == torch.float64 else 1e-5)
    with pytest.raises(ValueError, match="unknown quaternion op"):
        from egopose_amd import _lib as L
        L.check(L.load().egp_quat_op_f64(99, None, None, 1, None, None), "egp_quat_op")


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 3e-6)])
def test_observation_variants_on_device(skel, dtype, tol):
    """K3 under every combination of the observation switches (24 of them, reference vectors of get_full_obs), also
    computed on the fly inside the fused K3+K6 call (raw observations: no filter state)."""
    from egopose_amd.hip import EgpContext
    c = load_golden("config_subject_03.npz")
    g = load_golden("obs_variants.npz")
    qpos = torch.as_tensor(g["qpos"], dtype=dtype, device="cuda")
    qvel = torch.as_tensor(g["qvel"], dtype=dtype, device="cuda")
    for k, (oh, deheading, root, vel) in enumerate(g["combos"]):
        opts = dict(obs_heading=bool(oh), root_deheading=bool(deheading), obs_coord="root" if root else "heading", obs_vel=["full", "root", "no"][vel])
        ctx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"], obs_options=opts)
        ref = g["obs_%d" % k]
        assert ctx.obs_dim == ref.shape[1]
        got = ctx.obs(qpos, qvel).double().cpu().numpy()
        np.testing.assert_allclose(got, ref, rtol=tol, atol=tol, err_msg=str(opts))
        if dtype == torch.float64:
            out = torch.empty(qpos.shape[0], ctx.obs_dim, dtype=dtype, device="cuda")
            ctx.obs_zfilter(qpos, qvel, None, None, 0.0, out)
            np.testing.assert_array_equal(out.cpu().numpy(), got)
        ctx.close()
    with pytest.raises(ValueError):
        EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"], obs_options=dict(obs_coord="bogus"))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_large_batch_observation_kernel_equals_the_element_kernel(skel, dtype):
    """K3 from 32 768 rows on streams whole rows through a workgroup (k_obs_rows: the columns that need quaternion arithmetic one
    wave per column, one lane per row); below that one thread per element (k_obs). Same obs_element on the same values: the
    large batch must equal its own chunks run through the small form bit for bit -- ragged size (a last workgroup of 37
    rows), every observation switch incl. the phase column."""
    from egopose_amd.hip import EgpContext
    c = load_golden("config_subject_03.npz")
    g = load_golden("obs_variants.npz")
    n = 32768 + 3 * 64 + 37
    gen = torch.Generator(device="cuda").manual_seed(11)
    qpos = torch.randn(n, 59, dtype=dtype, device="cuda", generator=gen) * 0.4
    qvel = torch.randn(n, 58, dtype=dtype, device="cuda", generator=gen)
    k = min(n, g["qpos"].shape[0])
    qpos[:k] = torch.as_tensor(g["qpos"][:k], dtype=dtype, device="cuda")              # the reference's rows lead the batch
    qvel[:k] = torch.as_tensor(g["qvel"][:k], dtype=dtype, device="cuda")
    t = torch.randint(0, 300, (n,), dtype=torch.int32, device="cuda", generator=gen)
    combos = [tuple(int(v) for v in cmb) + (0,) for cmb in g["combos"]] + [(0, 1, 0, 0, 1), (1, 0, 1, 1, 1), (1, 1, 0, 2, 1)]
    for oh, deheading, root, vel, phase in combos:
        opts = dict(obs_heading=bool(oh), root_deheading=bool(deheading), obs_coord="root" if root else "heading", obs_vel=["full", "root", "no"][vel],
                    obs_phase=bool(phase))
        ctx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"], episode_len=120, obs_options=opts)
        kw = (lambda a, b: dict(phase_t=t[a:b])) if phase else (lambda a, b: {})
        big = ctx.obs(qpos, qvel, **kw(0, n))
        parts = torch.cat([ctx.obs(qpos[a:a + 9000], qvel[a:a + 9000], **kw(a, a + 9000)) for a in range(0, n, 9000)], 0)
        assert big.shape == (n, ctx.obs_dim)
        np.testing.assert_array_equal(big.cpu().numpy(), parts.cpu().numpy(), err_msg=str(opts))
        ctx.close()


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 3e-6)])
def test_phase_observation_on_device(skel, dtype, tol):
    """cfg.obs_phase (humanoid_v1.py:92-94): K3's extra column from the rows' cur_t against the reference's get_full_obs
    (obs_phase.npz: cur_t below, at and beyond the episode length; default options and a non-default combination), also through
    the fused K3 + K6 call and the split statistics / apply pair; a model with obs_phase refuses a call without phase_t."""
    from egopose_amd.hip import EgpContext
    c = load_golden("config_subject_03.npz")
    g = load_golden("obs_phase.npz")
    qpos = torch.as_tensor(g["qpos"], dtype=dtype, device="cuda")
    qvel = torch.as_tensor(g["qvel"], dtype=dtype, device="cuda")
    t = torch.as_tensor(g["cur_t"], dtype=torch.int32, device="cuda")
    for key, opts in (("obs_default", {}), ("obs_variant", dict(obs_heading=True, root_deheading=False, obs_coord="root", obs_vel="root"))):
        ctx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"], episode_len=int(g["episode_len"]),
                         obs_options=dict(opts, obs_phase=True))
        ref = g[key]
        assert ctx.obs_dim == ref.shape[1]
        got = ctx.obs(qpos, qvel, phase_t=t).double().cpu().numpy()
        np.testing.assert_allclose(got, ref, rtol=tol, atol=tol, err_msg=key)
        if dtype == torch.float64:
            np.testing.assert_array_equal(got[:, -1], ref[:, -1])                # the division: bit for bit
            out = torch.empty(qpos.shape[0], ctx.obs_dim, dtype=dtype, device="cuda")
            ctx.obs_zfilter(qpos, qvel, None, None, 0.0, out, phase_t=t)
            np.testing.assert_array_equal(out.cpu().numpy(), got)
            # filtered: one fused call == statistics + apply, and the phase column's statistics are those of the column itself
            S = ctx.obs_dim
            st0 = torch.zeros(1 + 2 * S, dtype=torch.float64, device="cuda")
            st1, st2 = torch.empty_like(st0), torch.empty_like(st0)
            y1, y2 = torch.empty_like(out), torch.empty_like(out)
            ctx.obs_zfilter(qpos, qvel, st0, st1, 5.0, y1, phase_t=t)
            ws = torch.empty(int(ctx.lib.egp_zfilter_workspace_bytes(qpos.shape[0], S)) // 8, dtype=torch.float64, device="cuda")
            ctx.obs_zfilter_stats(qpos, qvel, ws, phase_t=t)
            ctx.obs_zfilter_apply(qpos, qvel, st0, st2, 5.0, y2, None, ws, phase_t=t)
            assert torch.equal(st1, st2) and torch.equal(y1, y2)
            np.testing.assert_allclose(float(st1[S]), ref[:, -1].mean(), rtol=1e-13)
        with pytest.raises(ValueError):
            ctx.obs(qpos, qvel)
        ctx.close()


def test_constant_and_pose_dist_rewards_on_device(skel):
    """The registry's two small rewards (reward_function.py:63-80) through `egp_reward_simple_f64` against the reference."""
    from egopose_amd.hip import EgpContext
    c = load_golden("config_subject_03.npz")
    g = load_golden("reward_simple.npz")
    ctx = EgpContext(skel, c["jkp"], c["jkd"], c["a_ref"], c["a_scale"], c["torque_lim"], c["b_diffw"])
    n = g["expert_qpos"].shape[0]
    z = lambda *s: np.zeros(s)
    bq = np.tile(np.array([1.0, 0, 0, 0]), (n, 21))
    ctx.upload_experts([dict(qpos=g["expert_qpos"], qvel=z(n, 58), rlinv_local=z(n, 3), rangv=z(n, 3), rq_rmh=bq[:, :4], ee_pos=z(n, 15),
                             bquat=bq, bangvel=z(n, 63), head_height_lb=1.0)])
    d = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")
    qpos, frame, end = d(g["qpos"]), d(g["frame"], torch.int32), d(g["end"], torch.int32)
    r, ci = ctx.reward_simple("pose_dist", qpos, frame, end, float(g["end_reward"]))
    np.testing.assert_allclose(r.cpu().numpy(), g["pose_dist_reward"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ci.cpu().numpy(), g["pose_dist_cinfo"], rtol=1e-12, atol=1e-12)
    r, ci = ctx.reward(qpos, qpos, torch.zeros(32, 15, dtype=torch.float64, device="cuda"), frame, frame, end, float(g["end_reward"]), kind="constant")
    assert (r.cpu().numpy() == g["constant_reward"]).all() and (ci.cpu().numpy() == g["constant_cinfo"]).all()
    active = torch.ones(32, dtype=torch.int32, device="cuda")
    active[::3] = 0
    keep = torch.full((32,), -7.0, dtype=torch.float64, device="cuda")
    ctx.reward_simple("pose_dist", qpos, frame, end, 0.0, active=active, reward_out=keep)
    assert (keep[::3] == -7.0).all() and (keep[1::3] != -7.0).all()
    ctx.close()


@pytest.mark.parametrize("n,H", [(512, 128), (37, 128), (1024, 128), (300, 192), (512, 40)])
def test_filter_apply_in_the_policy_step_is_bit_identical_to_the_two_launches(ctx, n, H):
    """egp_obs_zfilter_stats_f64 + egp_policy_step_f32 (filter block) against egp_obs_zfilter_f64 + egp_policy_step_f32 (plain) (what a
    rollout tick without resets runs, rollout.py defer_apply): filtered observations, running statistics and actions equal
    bit for bit; so does the split pair stats + apply. Context widths: 128 (shipped; one input column per thread, the thread
    that normalises a state column merges its statistics -- with the merge coefficients shared across the wave), 192 (more
    input columns than threads: the statistics go through LDS), 40 (state columns straddle a wave boundary)."""
    from egopose_amd.nets import MLP, PolicyGaussian
    from egopose_amd import policy_step
    torch.manual_seed(11)
    rng = np.random.RandomState(n)
    S, T, nu = 115, 7, 52
    pol = PolicyGaussian(MLP(H + S, (300, 200), "relu"), nu, log_std=-2.3).cuda()
    fp = policy_step.FusedGaussianPolicy(pol, torch.device("cuda"))
    qpos = rng.normal(size=(n, 59)) * 0.4
    qpos[:, 3:7] = rng.normal(size=(n, 4)); qpos[:, 3:7] /= np.linalg.norm(qpos[:, 3:7], axis=1, keepdims=True)
    qvel = rng.normal(size=(n, 58))
    qp, qv = dev(qpos), dev(qvel)
    act = torch.as_tensor((rng.uniform(size=n) < 0.8).astype(np.int32), device="cuda")
    st0 = torch.zeros(1 + 2 * S, dtype=torch.float64, device="cuda")
    st_a, st_b = torch.empty_like(st0), torch.empty_like(st0)
    ctx.obs_zfilter(dev(rng.normal(size=(300, 59)) * 0.3 + np.r_[0, 0, 1, 1, 0, 0, 0, np.zeros(52)]), dev(rng.normal(size=(300, 58))), st0, st_a, 5.0,
                    torch.empty(300, S, dtype=torch.float64, device="cuda"))          # a non-trivial running state to continue from
    v_out = torch.randn(n, T, H, device="cuda")
    t_idx = torch.randint(0, T, (n,), device="cuda")
    noise = torch.randn(n, nu, device="cuda")
    # reference: two filter launches, then the policy step on the filtered rows
    y_ref, y2_ref = torch.empty(n, S, dtype=torch.float64, device="cuda"), torch.empty(n, S, dtype=torch.float64, device="cuda")
    ctx.obs_zfilter(qp, qv, st_a, st_b, 5.0, y_ref, y2_ref, active=act)
    a_ref = torch.empty(n, nu, dtype=torch.float64, device="cuda")
    fp(v_out, t_idx, y2_ref, a_ref, noise=noise)
    ws = torch.empty(int(ctx.lib.egp_zfilter_workspace_bytes(n, S)) // 8, dtype=torch.float64, device="cuda")
    # split pair
    st_c = torch.empty_like(st0)
    y1, y2 = torch.empty_like(y_ref), torch.empty_like(y_ref)
    ctx.obs_zfilter_stats(qp, qv, ws, active=act)
    ctx.obs_zfilter_apply(qp, qv, st_a, st_c, 5.0, y1, y2, ws)
    assert torch.equal(st_c, st_b) and torch.equal(y1, y_ref) and torch.equal(y2, y2_ref)
    # apply pass inside the policy step
    st_d = torch.empty_like(st0)
    y1.zero_(); y2.zero_()
    a_f = torch.empty_like(a_ref)
    ctx.obs_zfilter_stats(qp, qv, ws, active=act)
    fp.with_filter(ctx, v_out, t_idx, qp, qv, st_a, st_d, 5.0, y1, y2, ws, a_f, noise=noise)
    assert torch.equal(st_d, st_b) and torch.equal(y1, y_ref) and torch.equal(y2, y2_ref)
    assert torch.equal(a_f, a_ref)


def test_large_batch_kernel_variants_equal_the_small_batch_ones(ctx, skel):
    """K2 switches to multi-pass 60-env tiles at >= 16 384 envs and K8 to 7-env workgroups at >= 4 096: the same arithmetic per
    env, so one large call must equal the same rows pushed through in small calls bit for bit (and the golden cases, tiled up
    to that size with varied frames / masks, keep their reference values: the small variants are pinned to them above)."""
    g = load_golden("reward.npz")
    _upload_golden_expert(ctx, g)
    wsets = [yaml.safe_load(str(s)) for s in g["wset_json"]]
    ctx.set_reward_weights(wsets[0])
    sel = np.where(g["wset"] == 0)[0]
    n = 16384 + 77
    rng = np.random.RandomState(5)
    pick = sel[rng.randint(0, len(sel), n)]
    i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32, device="cuda")
    cur, prev, ee = dev(g["cur_qpos"][pick]), dev(g["prev_qpos"][pick]), dev(g["ee_wpos"][pick])
    t, fr, en = i32(g["t"][pick]), i32(g["start_ind"][pick] + g["t"][pick]), i32(g["end"][pick])
    act = i32((rng.uniform(size=n) < 0.9).astype(np.int32))
    r_big, c_big = ctx.reward(cur, prev, ee, t, fr, en, 0.3, active=act)
    r_parts, c_parts = [], []
    for a in range(0, n, 5000):                      # 5 000-env calls: the one-pass variant
        b = min(n, a + 5000)
        r, c = ctx.reward(cur[a:b], prev[a:b], ee[a:b], t[a:b], fr[a:b], en[a:b], 0.3, active=act[a:b])
        r_parts.append(r); c_parts.append(c)
    assert torch.equal(r_big, torch.cat(r_parts)) and torch.equal(c_big, torch.cat(c_parts))
    on = act.cpu().numpy() == 1
    want = g["reward"][pick] - np.where(g["end"][pick], g["end_reward"][pick], 0.0) + np.where(g["end"][pick], 0.3, 0.0)
    np.testing.assert_allclose(r_big.cpu().numpy()[on], want[on], rtol=1e-10, atol=5e-10)
    assert float(r_big.cpu().numpy()[~on].max(initial=0.0)) == 0.0
    # K8
    m = 4096 + 13
    qpos = np.tile(g["cur_qpos"][sel][:64], (m // 64 + 1, 1))[:m] + rng.normal(size=(m, 59)) * 0.01
    qpos[:, 3:7] /= np.linalg.norm(qpos[:, 3:7], axis=1, keepdims=True)
    qvel = rng.normal(size=(m, 58)) * 0.5
    qp, qv = dev(qpos), dev(qvel)
    big = ctx.dynamics(qp, qv, want_xpos=True)
    parts = [ctx.dynamics(qp[a:a + 1500], qv[a:a + 1500], want_xpos=True) for a in range(0, m, 1500)]
    for key in ("qM", "bias", "xpos"):
        assert torch.equal(big[key], torch.cat([p[key] for p in parts])), key
