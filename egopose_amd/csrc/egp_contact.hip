// K11: physical-plausibility figures of a pose against the ground on the GPU -- no ground truth needed. A contact set is K <= 32
// points, each fixed to a body: offset o_k in the zero pose's global axes relative to body_pos[body_k] (the convention of
// DynTables.com_l), world point P_k = p_b + R_b o_k. Item i scores pose row `row[i]` (P) against a following row `nxt[i]` (P'; -1:
// none); with z measured from ground_z and h = contact_height, per_frame[6] is
//   pen       = max_k max(0, -z_k)                                        ground penetration, metres
//   gap       = max(0, min_k z_k)                                         floating, metres
//   n_contact = #{k : z_k <= h}
//   n_skate   = #{k : z_k <= h and z'_k <= h}                             0 without a following row
//   skate     = mean over those k of |(P'_k - P_k)_xy|                    foot sliding, metres per frame step; 0 when n_skate = 0
//   skate_max = max over the same k                                       0 when n_skate = 0
// and, on request, the K world points of the row. One launch scores all frames of all takes, or all horizon frames of all windows.
//
// Mapping: K10's -- one 64-lane wavefront per item, 4 items per 256-thread workgroup, the tree tables and the contact table staged
// in static LDS once per workgroup, the FK scratch in wave-private LDS (dy_fk_doubles). fk_wave (egp_dynamics_dev.hpp) runs on the
// row; lane k (< K) forms P_k from its body's R, p in sW and keeps it in registers; after a wave_sync the second pass runs on the
// following row in the SAME scratch and gives P'_k, so the dynamic LDS is K9's and K10's. A wave without a following row runs the
// second pass on its own row (the wave stays convergent, no divergent LDS phases) and its three skate outputs are 0. Max, min and
// sum over points are __shfl_xor butterflies over the whole wave; lanes >= K hold the neutral element (0, +inf, 0). No atomics;
// plain vector stores by lane 0 (per_frame) and lanes 0..K-1 (points). Everything is float64.
// The kernel trusts `row` and `nxt`: the caller guarantees 0 <= row[i] < N and -1 <= nxt[i] < N (EgpContext.contact checks both).
#include <hip/hip_runtime.h>

#include <math.h>

#include "egp_internal.hpp"

#include "egp_dynamics_dev.hpp"

namespace {

using namespace egp_dyn;

constexpr int CT_WAVES = 4;          // items per workgroup
constexpr int CT_MAXK = EGP_CONTACT_MAXK;

struct ContactTab {                  // device copy of the contact set (egp_set_contact_points), staged in LDS beside DynTables
    int K, pad;
    int body[CT_MAXK];
    double off[CT_MAXK][3];
};
static_assert(sizeof(ContactTab) <= 1200 && sizeof(ContactTab) % 4 == 0, "the contact table is staged word by word");

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m, 64));
    return v;
}

__device__ __forceinline__ V3 world_point(const double *sW, int b, V3 o) {
    M3 R;
    ld_m3(sW + b * DY_LW, R);
    return ld_v3(sW + b * DY_LW + 9) + mul(R, o);
}

__global__ __launch_bounds__(CT_WAVES * 64) void k_contact(const DynTables *__restrict__ tab_g, const ContactTab *__restrict__ ct_g,
                                                           const double *__restrict__ qpos, long ld_q, const long long *__restrict__ nxt,
                                                           const long long *__restrict__ row, double ground_z, double contact_height,
                                                           double *__restrict__ per_frame, double *__restrict__ points, long n, int fk_doubles) {
    __shared__ DynTables tb;
    __shared__ ContactTab ct;
    extern __shared__ double s_fk[];             // CT_WAVES x fk_doubles
    {
        const int words = sizeof(DynTables) / 4;
        const int *src = reinterpret_cast<const int *>(tab_g);
        int *dst = reinterpret_cast<int *>(&tb);
        for (int i = threadIdx.x; i < words; i += blockDim.x) dst[i] = src[i];
        const int cwords = sizeof(ContactTab) / 4;
        const int *csrc = reinterpret_cast<const int *>(ct_g);
        int *cdst = reinterpret_cast<int *>(&ct);
        for (int i = threadIdx.x; i < cwords; i += blockDim.x) cdst[i] = csrc[i];
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * CT_WAVES + wave;
    const bool live = item < n;
    const long it = live ? item : 0;             // out-of-range waves shadow item 0 and write nothing
    const long r0 = row ? (long)row[it] : it;
    const long r1_in = (long)nxt[it];
    const bool has_next = r1_in >= 0;
    const long r1 = has_next ? r1_in : r0;       // no following row: the second pass runs on the wave's own row
    __syncthreads();
    const int nb = tb.nb, nj = tb.nj, K = ct.K;
    double *sLoc = s_fk + wave * fk_doubles, *sJl = sLoc + nb * DY_LW, *sW = sJl + nj * DY_LJ, *sSC = sW + nb * DY_LW;
    const bool is_pt = lane < K;
    const int k = is_pt ? lane : 0;
    const int b = ct.body[k];
    const V3 o = {ct.off[k][0], ct.off[k][1], ct.off[k][2]};

    fk_wave(tb, sLoc, sJl, sW, sSC, qpos + r0 * ld_q, lane, false, nullptr);
    const V3 P = world_point(sW, b, o);
    wave_sync();                                 // every lane holds its point before the second pass writes the scratch again
    fk_wave(tb, sLoc, sJl, sW, sSC, qpos + r1 * ld_q, lane, false, nullptr);
    const V3 Q = world_point(sW, b, o);

    const double z = P.z - ground_z, zn = Q.z - ground_z;
    const bool down = is_pt && z <= contact_height;
    const bool both = down && has_next && zn <= contact_height;
    const double dx = Q.x - P.x, dy = Q.y - P.y;
    const double slide = both ? sqrt(dx * dx + dy * dy) : 0.0;

    const double pen = wave_max(is_pt && z < 0.0 ? -z : 0.0);
    const double z_min = wave_min(is_pt ? z : INFINITY);
    const double n_contact = wave_sum(down ? 1.0 : 0.0), n_skate = wave_sum(both ? 1.0 : 0.0);
    const double s_sum = wave_sum(slide), s_max = wave_max(slide);

    if (!live) return;
    if (points && is_pt) st_v3(points + (it * K + lane) * 3, P);
    if (lane == 0) {
        double *out = per_frame + it * 6;
        out[0] = pen;
        out[1] = z_min > 0.0 ? z_min : 0.0;
        out[2] = n_contact;
        out[3] = n_skate;
        out[4] = n_skate > 0.0 ? s_sum / n_skate : 0.0;
        out[5] = s_max;
    }
}

}  // namespace

extern "C" {

int egp_set_contact_points(egp_ctx *ctx, const int32_t *body, const double *offset, int32_t K) {
    EGP_REQUIRE(ctx && body && offset, "NULL pointer");
    EGP_REQUIRE(K >= 1 && K <= CT_MAXK, "K must be in [1, 32]");
    ContactTab t{};
    t.K = K;
    for (int k = 0; k < K; ++k) {
        EGP_REQUIRE(body[k] >= 0 && body[k] < ctx->dm.nbody, "contact body out of range");
        t.body[k] = body[k];
        for (int c = 0; c < 3; ++c) {
            EGP_REQUIRE(isfinite(offset[3 * k + c]), "contact offset is not finite");
            t.off[k][c] = offset[3 * k + c];
        }
    }
    EGP_HIP_CHECK(hipSetDevice(ctx->device));
    if (!ctx->contact_tab) {
        void *p = nullptr;
        EGP_HIP_CHECK(hipMalloc(&p, sizeof(ContactTab)));
        ctx->allocs.push_back(p);
        ctx->contact_tab = p;
    }
    EGP_HIP_CHECK(hipMemcpy(ctx->contact_tab, &t, sizeof(ContactTab), hipMemcpyHostToDevice));
    ctx->contact_K = K;
    return EGP_OK;
}

int egp_contact_f64(egp_ctx *ctx, const double *qpos, const int64_t *nxt, const int64_t *row, double ground_z, double contact_height,
                    double *per_frame, double *points, int64_t n, void *stream) {
    EGP_REQUIRE(ctx, "ctx is NULL");
    if (!ctx->dyn_tables) { egp::set_error("egp_set_dynamics_model must be called before egp_contact"); return EGP_E_STATE; }
    if (!ctx->contact_tab || ctx->contact_K < 1) { egp::set_error("egp_set_contact_points must be called before egp_contact"); return EGP_E_STATE; }
    EGP_REQUIRE(n >= 0 && n <= (int64_t)1 << 30, "n out of range");
    if (n == 0) return EGP_OK;
    EGP_REQUIRE(qpos && nxt && per_frame, "NULL pointer");
    EGP_REQUIRE(isfinite(ground_z) && isfinite(contact_height), "ground_z and contact_height must be finite");
    const int nbody = ctx->dm.nbody;
    EGP_REQUIRE(nbody <= DY_MAXB, "nbody above the tree tables");
    const int fk_doubles = dy_fk_doubles(nbody, ctx->dm.nv - 6);
    const size_t lds = (size_t)CT_WAVES * fk_doubles * sizeof(double);
    if (lds + sizeof(DynTables) + sizeof(ContactTab) > 64 * 1024) { egp::set_error("k_contact: LDS budget (%zu bytes)", lds); return EGP_E_HIP; }
    k_contact<<<dim3((unsigned)((n + CT_WAVES - 1) / CT_WAVES)), dim3(CT_WAVES * 64), lds, (hipStream_t)stream>>>(
        (const DynTables *)ctx->dyn_tables, (const ContactTab *)ctx->contact_tab, qpos, (long)ctx->dm.nq, (const long long *)nxt,
        (const long long *)row, ground_z, contact_height, per_frame, points, (long)n, fk_doubles);
    return after_launch("k_contact");
}

}  // extern "C"
