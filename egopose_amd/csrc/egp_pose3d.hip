// K10: joint-position metrics of a predicted pose against the MoCap pose on the GPU. Per frame pair (P, G): forward kinematics of both
// rows (the FK phases of K8, egp_dynamics_dev.hpp: fk_wave) -> body positions X, Y in metres, and over the bodies B of a 32-bit mask
//   g_mpjpe  = mean_B |X_b - Y_b|                        (nothing aligned)
//   mpjpe    = mean_B |(X_b - X_0) - (Y_b - Y_0)|        (root-relative; body 0 is the root whether or not its bit is set)
//   pa_mpjpe = mean_B |s R (X_b - mx) + my - Y_b|        (mx, my the centroids over B; (s, R) the least-squares similarity of X onto Y
//                                                         over B with R a PROPER rotation, egp_horn_dev.hpp)
//   root_err = |X_0 - Y_0|
// and, on request, the root-relative distance of every body (0 where the mask bit is clear) and both position sets.
// One launch scores all frames of all takes, or all horizon frames of all windows.
//
// Mapping: K8's and K9's -- one 64-lane wavefront per frame pair, 4 pairs per 256-thread workgroup, the tree tables staged in LDS
// once per workgroup, the FK scratch in wave-private LDS (dy_fk_doubles). The two FK passes run one after the other in the SAME
// scratch: lane b (< nbody) takes its body's position and the root's into registers after the first, so the kernel's LDS is K9's.
// Sums over bodies are __shfl_xor butterflies over the whole wave (lanes >= nbody and masked lanes hold zeros), which leave every
// sum in every lane: the centroids, then sum |X - mx|^2, the 3x3 cross-covariance and the two unaligned sums, then -- after the
// rotation, which every lane computes in registers from the same nine numbers -- the aligned sum. Centred sums, not raw moments:
// a take walks metres away from the origin. No atomics; plain vector stores by lanes 0..nbody-1 (err, xpos) and lane 0 (per_frame).
// Nothing guards the divisions: a mask whose bodies all coincide in X has no scale, and gives inf / NaN in pa_mpjpe.
#include <hip/hip_runtime.h>

#include <math.h>

#include "egp_internal.hpp"

#include "egp_dynamics_dev.hpp"
#include "egp_horn_dev.hpp"

namespace {

using namespace egp_dyn;

constexpr int P3_WAVES = 4;          // frame pairs per workgroup

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ double norm3(V3 a) { return sqrt(dot(a, a)); }

__global__ __launch_bounds__(P3_WAVES * 64) void k_pose3d(const DynTables *__restrict__ tab_g, const double *__restrict__ qpos_pred,
                                                          const double *__restrict__ qpos_gt, long ld_q, unsigned mask,
                                                          double *__restrict__ per_frame, double *__restrict__ err_out,
                                                          double *__restrict__ xpos_pred, double *__restrict__ xpos_gt, long n, int fk_doubles) {
    __shared__ DynTables tb;
    extern __shared__ double s_fk[];             // P3_WAVES x fk_doubles
    {
        const int words = sizeof(DynTables) / 4;
        const int *src = reinterpret_cast<const int *>(tab_g);
        int *dst = reinterpret_cast<int *>(&tb);
        for (int i = threadIdx.x; i < words; i += blockDim.x) dst[i] = src[i];
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long k = (long)blockIdx.x * P3_WAVES + wave;
    const bool live = k < n;
    const long fr = live ? k : 0;                // out-of-range waves shadow frame 0 and write nothing
    __syncthreads();
    const int nb = tb.nb, nj = tb.nj;
    double *sLoc = s_fk + wave * fk_doubles, *sJl = sLoc + nb * DY_LW, *sW = sJl + nj * DY_LJ, *sSC = sW + nb * DY_LW;
    const bool is_body = lane < nb;
    const int b = is_body ? lane : 0;

    fk_wave(tb, sLoc, sJl, sW, sSC, qpos_pred + fr * ld_q, lane, false, nullptr);
    const V3 X = ld_v3(sW + b * DY_LW + 9), X0 = ld_v3(sW + 9);
    wave_sync();                                 // every lane holds its rows before the second pass writes the scratch again
    fk_wave(tb, sLoc, sJl, sW, sSC, qpos_gt + fr * ld_q, lane, false, nullptr);
    const V3 Y = ld_v3(sW + b * DY_LW + 9), Y0 = ld_v3(sW + 9);

    const bool in = is_body && ((mask >> b) & 1u) != 0;
    const double w = in ? 1.0 : 0.0;

    // ---- centroids over B
    const double cnt = wave_sum(w), inv_cnt = 1.0 / cnt;
    const V3 mx = {wave_sum(w * X.x) * inv_cnt, wave_sum(w * X.y) * inv_cnt, wave_sum(w * X.z) * inv_cnt};
    const V3 my = {wave_sum(w * Y.x) * inv_cnt, wave_sum(w * Y.y) * inv_cnt, wave_sum(w * Y.z) * inv_cnt};
    const V3 xc = w * (X - mx), yc = w * (Y - my);                 // zeros outside B

    // ---- the unaligned distances, sum |X - mx|^2 and the cross-covariance S[3 a + c] = sum xc_a yc_c
    const double d_glob = norm3(X - Y), d_rel = norm3((X - X0) - (Y - Y0));
    const double g_sum = wave_sum(w * d_glob), r_sum = wave_sum(w * d_rel);
    const double sxx = wave_sum(dot(xc, xc));
    double S[9];
    S[0] = wave_sum(xc.x * yc.x); S[1] = wave_sum(xc.x * yc.y); S[2] = wave_sum(xc.x * yc.z);
    S[3] = wave_sum(xc.y * yc.x); S[4] = wave_sum(xc.y * yc.y); S[5] = wave_sum(xc.y * yc.z);
    S[6] = wave_sum(xc.z * yc.x); S[7] = wave_sum(xc.z * yc.y); S[8] = wave_sum(xc.z * yc.z);

    // ---- similarity: the same registers in every lane, so the rotation is wave-uniform without a broadcast
    M3 R;
    const double lam = egp_horn::best_rotation(S, R.m);
    const double scale = lam / sxx;
    const double pa_sum = wave_sum(norm3(scale * mul(R, xc) - yc));          // = |s R (X - mx) + my - Y| on B, 0 elsewhere

    if (!live) return;
    if (is_body) {
        if (err_out) err_out[fr * nb + lane] = in ? d_rel : 0.0;
        if (xpos_pred) st_v3(xpos_pred + (fr * nb + lane) * 3, X);
        if (xpos_gt) st_v3(xpos_gt + (fr * nb + lane) * 3, Y);
    }
    if (lane == 0) {
        double *o = per_frame + fr * 4;
        o[0] = g_sum * inv_cnt;
        o[1] = r_sum * inv_cnt;
        o[2] = pa_sum * inv_cnt;
        o[3] = norm3(X0 - Y0);
    }
}

}  // namespace

extern "C" {

int egp_pose3d_f64(egp_ctx *ctx, const double *qpos_pred, const double *qpos_gt, uint32_t body_mask, double *per_frame, double *err,
                   double *xpos_pred, double *xpos_gt, int64_t n, void *stream) {
    EGP_REQUIRE(ctx, "ctx is NULL");
    if (!ctx->dyn_tables) { egp::set_error("egp_set_dynamics_model must be called before egp_pose3d"); return EGP_E_STATE; }
    EGP_REQUIRE(n >= 0 && n <= (int64_t)1 << 30, "n out of range");
    if (n == 0) return EGP_OK;
    EGP_REQUIRE(qpos_pred && qpos_gt && per_frame, "NULL pointer");
    const int nbody = ctx->dm.nbody;
    EGP_REQUIRE(nbody <= DY_MAXB && (body_mask >> nbody) == 0, "body_mask has bits at or above nbody");
    EGP_REQUIRE(__builtin_popcount(body_mask) >= 3, "body_mask must select at least 3 bodies");
    const int fk_doubles = dy_fk_doubles(nbody, ctx->dm.nv - 6);
    const size_t lds = (size_t)P3_WAVES * fk_doubles * sizeof(double);
    if (lds + sizeof(DynTables) > 64 * 1024) { egp::set_error("k_pose3d: LDS budget (%zu bytes)", lds); return EGP_E_HIP; }
    k_pose3d<<<dim3((unsigned)((n + P3_WAVES - 1) / P3_WAVES)), dim3(P3_WAVES * 64), lds, (hipStream_t)stream>>>(
        (const DynTables *)ctx->dyn_tables, qpos_pred, qpos_gt, (long)ctx->dm.nq, (unsigned)body_mask, per_frame, err, xpos_pred, xpos_gt,
        (long)n, fk_doubles);
    return after_launch("k_pose3d");
}

}  // extern "C"
