// K9: the 2D keypoint metric of in-the-wild evaluation on the GPU. Per frame: forward kinematics of the skeleton (the FK phases of
// K8, egp_dynamics_dev.hpp: fk_wave), the side camera of the reference's Pose2DContext.project_qpos, base / scale alignment to the
// visible third-person keypoints (align_qpos with scale=None) and the confidence-masked mean keypoint distance (get_pose_dist)
// (ego_pose/utils/pose2d.py:75-148). One launch scores all frames of all takes, or all horizon frames of all windows.
//
// Mapping: K8's -- one 64-lane wavefront per frame, 4 frames per 256-thread workgroup, the tree tables staged in LDS once per
// workgroup, the frame's body frames in wave-private LDS (odd row strides, DY_LW). The body positions never leave the LDS: after
// the FK the 12 keypoint bodies are 12 lanes (lane k reads the position of body kp.body[k] and row k of the frame's keypoints), the
// two hips are broadcast reads of the same LDS rows, and the pairs the alignment needs and the distance sum move by __shfl.
// No atomics; plain vector stores by lanes 0..11 (p_out) and lane 0 (dist, valid).
// As in the reference, nothing guards the divisions: a frame whose hip line is vertical (no horizontal direction for the camera), or
// whose chosen leg pair coincides in the projection or arm / up-leg pair is level in the keypoints, gives inf / NaN in p and dist.
#include <hip/hip_runtime.h>

#include <math.h>

#include "egp_internal.hpp"

#include "egp_dynamics_dev.hpp"

namespace {

using namespace egp_dyn;

constexpr int P2_WAVES = 4;          // frames per workgroup
constexpr int P2_NKP = EGP_POSE2D_NKP;

struct KpMap {                       // by value: body of every keypoint row, the rows with a role, and the two hips' bodies
    int body[P2_NKP];                // (read at compile-time indices only, so the struct stays in scalar registers)
    int l_upleg, r_upleg, l_leg, r_leg, l_arm, r_arm;
    int l_hip_body, r_hip_body;
};

__global__ __launch_bounds__(P2_WAVES * 64) void k_pose2d(const DynTables *__restrict__ tab_g, KpMap kp, const double *__restrict__ qpos, long ld_q,
                                                          const double *__restrict__ gt, const int *__restrict__ flip, double *__restrict__ p_out,
                                                          double *__restrict__ dist, int *__restrict__ valid_out, long n, int fk_doubles) {
    __shared__ DynTables tb;
    extern __shared__ double s_fk[];             // P2_WAVES x fk_doubles
    {
        const int words = sizeof(DynTables) / 4;
        const int *src = reinterpret_cast<const int *>(tab_g);
        int *dst = reinterpret_cast<int *>(&tb);
        for (int i = threadIdx.x; i < words; i += blockDim.x) dst[i] = src[i];
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long k = (long)blockIdx.x * P2_WAVES + wave;
    const bool live = k < n;
    const long fr = live ? k : 0;                // out-of-range waves shadow frame 0 and write nothing
    __syncthreads();
    const int nb = tb.nb, nj = tb.nj;
    double *sLoc = s_fk + wave * fk_doubles, *sJl = sLoc + nb * DY_LW, *sW = sJl + nj * DY_LJ, *sSC = sW + nb * DY_LW;
    fk_wave(tb, sLoc, sJl, sW, sSC, qpos + fr * ld_q, lane, false, nullptr);

    // ---- project_qpos: camera x along the hip line (z zeroed, normalised, negated by `flip`), world up as camera y, 10 m back
    const V3 hl = ld_v3(sW + kp.l_hip_body * DY_LW + 9), hr = ld_v3(sW + kp.r_hip_body * DY_LW + 9);
    const V3 vp = 0.5 * (hl + hr);
    V3 x = hr - hl;
    if (flip[fr] != 0) x = -1.0 * x;
    x.z = 0.0;
    x = (1.0 / sqrt(x.x * x.x + x.y * x.y)) * x;
    const V3 my = {x.y, -x.x, 0.0};              // -y, y = z x x
    const V3 t = vp - 10.0 * x;
    const bool is_kp = lane < P2_NKP;
    const int row = is_kp ? lane : 0;
    int body = kp.body[0];
#pragma unroll
    for (int i = 1; i < P2_NKP; ++i) body = row == i ? kp.body[i] : body;
    const V3 P = ld_v3(sW + body * DY_LW + 9);
    const double c0 = dot(my, P) - dot(my, t), c1 = P.z - t.z, c2 = dot(x, P) - dot(x, t);
    double px = c0 / c2, py = -(c1 / c2);

    // ---- the frame's keypoints: x, y, confidence of row `lane`
    const double *g = gt + (fr * P2_NKP + row) * 3;
    const double gx = g[0], gy = g[1], gc = g[2];
    const bool seen = is_kp && gc > 0.1;
    auto at = [&](double v, int r) { return __shfl(v, r, 64); };
    const double c_lu = at(gc, kp.l_upleg), c_ru = at(gc, kp.r_upleg);
    const bool ok = c_lu > 0.1 || c_ru > 0.1;     // check_gt

    // ---- align_qpos: base = mean of the visible hips, scale = |gt leg - gt up-leg| (x, y AND confidence: the reference's norm runs
    //      over the whole row) / |p leg - p up-leg| of the left pair if both are visible, else of the right pair
    double bx = 0.0, by = 0.0, nbase = 0.0;
    if (c_lu > 0.1) { bx += at(gx, kp.l_upleg); by += at(gy, kp.l_upleg); nbase += 1.0; }
    if (c_ru > 0.1) { bx += at(gx, kp.r_upleg); by += at(gy, kp.r_upleg); nbase += 1.0; }
    bx /= nbase; by /= nbase;
    const bool left_leg = at(gc, kp.l_leg) > 0.1 && c_lu > 0.1;
    const int s1 = left_leg ? kp.l_leg : kp.r_leg, s2 = left_leg ? kp.l_upleg : kp.r_upleg;
    const double dgx = at(gx, s1) - at(gx, s2), dgy = at(gy, s1) - at(gy, s2), dgc = at(gc, s1) - at(gc, s2);
    const double dpx = at(px, s1) - at(px, s2), dpy = at(py, s1) - at(py, s2);
    const double scale = sqrt(dgx * dgx + dgy * dgy + dgc * dgc) / sqrt(dpx * dpx + dpy * dpy);
    if (ok) { px = px * scale + bx; py = py * scale + by; }      // an invalid frame keeps the unaligned projection

    // ---- get_pose_dist: mean over the visible keypoints of |gt - p| x 0.5 / |dy(arm, up-leg)|, left pair if both visible, else right
    const bool left_arm = at(gc, kp.l_arm) > 0.1 && c_lu > 0.1;
    const int a1 = left_arm ? kp.l_arm : kp.r_arm, a2 = left_arm ? kp.l_upleg : kp.r_upleg;
    const double dscale = 0.5 / fabs(at(gy, a1) - at(gy, a2));
    const double ex = gx - px, ey = gy - py;
    double d = seen ? sqrt(ex * ex + ey * ey) * dscale : 0.0, cnt = seen ? 1.0 : 0.0;
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) {           // the 12 keypoints sit in lanes 0..15; lanes 12..63 hold zeros
        d += __shfl_xor(d, m, 64);
        cnt += __shfl_xor(cnt, m, 64);
    }
    if (!live) return;
    if (p_out && is_kp) {
        double *o = p_out + (fr * P2_NKP + lane) * 2;
        o[0] = px;
        o[1] = py;
    }
    if (lane == 0) {
        dist[fr] = ok ? d / cnt : 0.0;
        valid_out[fr] = ok ? 1 : 0;
    }
}

}  // namespace

extern "C" {

int egp_set_pose2d_bodies(egp_ctx *ctx, const int32_t *kp_body, const int32_t *roles) {
    EGP_REQUIRE(ctx && kp_body && roles, "NULL pointer");
    for (int i = 0; i < EGP_POSE2D_NKP; ++i) EGP_REQUIRE(kp_body[i] >= 0 && kp_body[i] < ctx->dm.nbody, "keypoint body out of range");
    for (int i = 0; i < 6; ++i) EGP_REQUIRE(roles[i] >= 0 && roles[i] < EGP_POSE2D_NKP, "role row out of range");
    for (int i = 0; i < EGP_POSE2D_NKP; ++i) ctx->pose2d_body[i] = kp_body[i];
    for (int i = 0; i < 6; ++i) ctx->pose2d_role[i] = roles[i];
    ctx->pose2d_set = true;
    return EGP_OK;
}

int egp_pose2d_f64(egp_ctx *ctx, const double *qpos, const double *gt, const int32_t *flip, double *p_out, double *dist, int32_t *valid,
                   int64_t n, void *stream) {
    EGP_REQUIRE(ctx, "ctx is NULL");
    if (!ctx->dyn_tables) { egp::set_error("egp_set_dynamics_model must be called before egp_pose2d"); return EGP_E_STATE; }
    if (!ctx->pose2d_set) { egp::set_error("egp_set_pose2d_bodies must be called before egp_pose2d"); return EGP_E_STATE; }
    EGP_REQUIRE(n >= 0 && n <= (int64_t)1 << 30, "n out of range");
    if (n == 0) return EGP_OK;
    EGP_REQUIRE(qpos && gt && flip && dist && valid, "NULL pointer");
    const int fk_doubles = dy_fk_doubles(ctx->dm.nbody, ctx->dm.nv - 6);
    const size_t lds = (size_t)P2_WAVES * fk_doubles * sizeof(double);
    if (lds + sizeof(DynTables) > 64 * 1024) { egp::set_error("k_pose2d: LDS budget (%zu bytes)", lds); return EGP_E_HIP; }
    KpMap kp;
    for (int i = 0; i < P2_NKP; ++i) kp.body[i] = ctx->pose2d_body[i];
    kp.l_upleg = ctx->pose2d_role[0]; kp.r_upleg = ctx->pose2d_role[1]; kp.l_leg = ctx->pose2d_role[2];
    kp.r_leg = ctx->pose2d_role[3]; kp.l_arm = ctx->pose2d_role[4]; kp.r_arm = ctx->pose2d_role[5];
    kp.l_hip_body = kp.body[kp.l_upleg]; kp.r_hip_body = kp.body[kp.r_upleg];
    k_pose2d<<<dim3((unsigned)((n + P2_WAVES - 1) / P2_WAVES)), dim3(P2_WAVES * 64), lds, (hipStream_t)stream>>>(
        (const DynTables *)ctx->dyn_tables, kp, qpos, (long)ctx->dm.nq, gt, flip, p_out, dist, valid, (long)n, fk_doubles);
    return after_launch("k_pose2d");
}

}  // extern "C"
