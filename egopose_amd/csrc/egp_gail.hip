// egp_gail.hip -- the device pieces of the video-conditioned GAIL discriminator update (ego_pose/core/agent_vgail.py:54-88)
// that are neither a recurrent sweep nor a matrix product:
//
//   k_gail_rows      agent_vgail.py:60-61 + :86-87: the discriminator's input block [generated; expert] in one launch -- the
//                    video context rows gathered once and written to both halves, the batch's states beside the first, the
//                    expert's observations (normalised with the running filter, no clip) beside the second
//   k_gail_rows_bwd  its adjoint for the context: the two halves' context gradients added into the row they were gathered from
//   k_bce_logits     agent_vgail.py:66-68: nn.BCELoss on sigmoid(z) with targets one (generated) / zero (expert), written on the
//                    logits, with d loss / d z and the per-row score -log D
//
// All three are one pass over their operands. No atomics, no workgroup talks to another inside a launch: the loss sums are
// float64 per-workgroup partials in a fixed order, combined in index order by a one-workgroup launch (as k_ppo_loss does).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "egp_internal.hpp"

namespace {

constexpr int ROWS_BLOCK = 256;
constexpr int ROWS_MAX_BLOCKS = 2048;

struct RowsArgs {
    int n, H, S;
    const float *ctx; long ld_ctx, ctx_rows;
    const long long *idx;
    const float *x; long ldx;
    const float *tab; long ld_tab, tab_rows;
    const long long *src;
    const float *mean, *inv_std;
    float *out; long ldo;                     // forward: the (2n, H + S) block; backward: its gradient (read)
    float *dctx;                              // backward only
    int wide_ctx, wide_x, wide_tab;
};

template <typename V> __device__ __forceinline__ V vsub_mul(V t, V m, V s);
template <> __device__ __forceinline__ float vsub_mul<float>(float t, float m, float s) { return (t - m) * s; }
template <> __device__ __forceinline__ float4 vsub_mul<float4>(float4 t, float4 m, float4 s) {
    return make_float4((t.x - m.x) * s.x, (t.y - m.y) * s.y, (t.z - m.z) * s.z, (t.w - m.w) * s.w);
}
template <typename V> __device__ __forceinline__ V vadd(V a, V b);
template <> __device__ __forceinline__ float vadd<float>(float a, float b) { return a + b; }
template <> __device__ __forceinline__ float4 vadd<float4>(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// context columns: one read of ctx[idx[r]], two writes (rows r and n + r). The grid strides over (row, column group) elements.
template <typename V>
__device__ __forceinline__ void rows_ctx(const RowsArgs &a) {
    constexpr int W = (int)(sizeof(V) / sizeof(float));
    const int wv = a.H / W;
    const long total = (long)a.n * wv;
    for (long e = (long)blockIdx.x * ROWS_BLOCK + threadIdx.x; e < total; e += (long)gridDim.x * ROWS_BLOCK) {
        const long r = e / wv;
        const long c = (e - r * wv) * W;
        const long long sr = a.idx[r];
        if (sr < 0 || sr >= a.ctx_rows) continue;                 // (not a row of the context: both output rows keep their content)
        const V v = *reinterpret_cast<const V *>(a.ctx + sr * a.ld_ctx + c);
        *reinterpret_cast<V *>(a.out + r * a.ldo + c) = v;
        *reinterpret_cast<V *>(a.out + (r + a.n) * a.ldo + c) = v;
    }
}

// state columns of the generated half
template <typename V>
__device__ __forceinline__ void rows_state(const RowsArgs &a) {
    constexpr int W = (int)(sizeof(V) / sizeof(float));
    const int wv = a.S / W;
    const long total = (long)a.n * wv;
    for (long e = (long)blockIdx.x * ROWS_BLOCK + threadIdx.x; e < total; e += (long)gridDim.x * ROWS_BLOCK) {
        const long r = e / wv;
        const long c = (e - r * wv) * W;
        *reinterpret_cast<V *>(a.out + r * a.ldo + a.H + c) = *reinterpret_cast<const V *>(a.x + r * a.ldx + c);
    }
}

// expert columns of the second half: (tab[src[r]] - mean) * inv_std, or the table row as it is without a filter
template <typename V>
__device__ __forceinline__ void rows_expert(const RowsArgs &a) {
    constexpr int W = (int)(sizeof(V) / sizeof(float));
    const int wv = a.S / W;
    const long total = (long)a.n * wv;
    for (long e = (long)blockIdx.x * ROWS_BLOCK + threadIdx.x; e < total; e += (long)gridDim.x * ROWS_BLOCK) {
        const long r = e / wv;
        const long c = (e - r * wv) * W;
        const long long sr = a.src[r];
        if (sr < 0 || sr >= a.tab_rows) continue;                 // (the host check reports it when it can see `src`; nothing is read out of range)
        V v = *reinterpret_cast<const V *>(a.tab + sr * a.ld_tab + c);
        if (a.mean) v = vsub_mul<V>(v, *reinterpret_cast<const V *>(a.mean + c), *reinterpret_cast<const V *>(a.inv_std + c));
        *reinterpret_cast<V *>(a.out + (r + a.n) * a.ldo + a.H + c) = v;
    }
}

__global__ __launch_bounds__(ROWS_BLOCK) void k_gail_rows(RowsArgs a) {
    if (a.wide_ctx) rows_ctx<float4>(a); else rows_ctx<float>(a);
    if (a.wide_x) rows_state<float4>(a); else rows_state<float>(a);
    if (a.wide_tab) rows_expert<float4>(a); else rows_expert<float>(a);
}

template <typename V>
__device__ __forceinline__ void rows_bwd(const RowsArgs &a) {
    constexpr int W = (int)(sizeof(V) / sizeof(float));
    const int wv = a.H / W;
    const long total = (long)a.n * wv;
    for (long e = (long)blockIdx.x * ROWS_BLOCK + threadIdx.x; e < total; e += (long)gridDim.x * ROWS_BLOCK) {
        const long r = e / wv;
        const long c = (e - r * wv) * W;
        const long long sr = a.idx[r];
        if (sr < 0 || sr >= a.ctx_rows) continue;
        const V g = *reinterpret_cast<const V *>(a.out + r * a.ldo + c);
        const V x = *reinterpret_cast<const V *>(a.out + (r + a.n) * a.ldo + c);
        *reinterpret_cast<V *>(a.dctx + sr * a.ld_ctx + c) = vadd<V>(g, x);
    }
}

__global__ __launch_bounds__(ROWS_BLOCK) void k_gail_rows_bwd(RowsArgs a) {
    if (a.wide_ctx) rows_bwd<float4>(a); else rows_bwd<float>(a);
}

inline long rows_grid(long elements) {
    long b = (elements + ROWS_BLOCK - 1) / ROWS_BLOCK;
    return b < 1 ? 1 : (b > ROWS_MAX_BLOCKS ? ROWS_MAX_BLOCKS : b);
}

inline bool aligned16(const void *p) { return (uintptr_t)p % 16 == 0; }

// ------------------------------------------------------------------------------------------------ BCE on logits
constexpr int BCE_BLOCK = 256;
constexpr int BCE_MAX_BLOCKS = 1024;

struct BceArgs {
    long n, n_e;               // generated rows [0, n), expert rows [n, n + n_e)
    const float *z;
    double inv_n_g, inv_n_e;
    float *dz, *score;
    double *losses;
    double *part;              // [gridDim.x][2]: generated sum, expert sum
};

__device__ __forceinline__ double bce_block_sum(double v, double *s_red) {
    // fixed tree over the 256 threads: lane butterflies inside a wave, then the four wave sums in order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
    return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__global__ __launch_bounds__(BCE_BLOCK) void k_bce_logits(BceArgs a) {
    __shared__ double s_red[4];
    const float inv_g = (float)a.inv_n_g, inv_e = (float)a.inv_n_e;
    double g_sum = 0.0, e_sum = 0.0;
    for (long i = (long)blockIdx.x * BCE_BLOCK + threadIdx.x; i < a.n + a.n_e; i += (long)gridDim.x * BCE_BLOCK) {
        const float z = a.z[i];
        const float e = expf(-fabsf(z));                 // in (0, 1]: nothing overflows
        const float tail = log1pf(e);
        const float r = 1.f / (1.f + e);
        const float big = r, small = e * r;              // sigmoid(|z|), sigmoid(-|z|)
        if (i < a.n) {
            // label 1: -log sigmoid(z) = softplus(-z);  d / dz = sigmoid(z) - 1 = -sigmoid(-z)
            const float sp = fmaxf(-z, 0.f) + tail;
            g_sum += (double)sp;
            if (a.dz) a.dz[i] = -(z >= 0.f ? small : big) * inv_g;
            if (a.score) a.score[i] = sp;
        } else {
            // label 0: -log(1 - sigmoid(z)) = softplus(z);  d / dz = sigmoid(z)
            const float sp = fmaxf(z, 0.f) + tail;
            e_sum += (double)sp;
            if (a.dz) a.dz[i] = (z >= 0.f ? big : small) * inv_e;
        }
    }
    const double gs = bce_block_sum(g_sum, s_red);
    const double es = bce_block_sum(e_sum, s_red);
    if (threadIdx.x == 0) {
        a.part[2 * (long)blockIdx.x] = gs;
        a.part[2 * (long)blockIdx.x + 1] = es;
    }
}

__global__ __launch_bounds__(BCE_BLOCK) void k_bce_logits_final(BceArgs a, int nb) {
    __shared__ double s_red[4];
    double g = 0.0, e = 0.0;
    for (int b = threadIdx.x; b < nb; b += BCE_BLOCK) {       // 256 interleaved slices, combined by the fixed tree
        g += a.part[2 * (long)b];
        e += a.part[2 * (long)b + 1];
    }
    g = bce_block_sum(g, s_red);
    e = bce_block_sum(e, s_red);
    if (threadIdx.x == 0) {
        a.losses[0] = g * a.inv_n_g;
        a.losses[1] = e * a.inv_n_e;
    }
}

int fill_rows_args(const egp_gail_rows_desc *d, RowsArgs &a) {
    EGP_REQUIRE(d, "descriptor is NULL");
    EGP_REQUIRE(d->n >= 0 && d->H >= 0 && d->S >= 0, "negative size");
    EGP_REQUIRE(d->ctx_rows >= 0 && d->tab_rows >= 0, "negative row count");
    a.n = d->n; a.H = d->H; a.S = d->S;
    a.ctx = d->ctx; a.ld_ctx = d->ld_ctx; a.ctx_rows = d->ctx_rows;
    a.idx = (const long long *)d->idx;
    a.x = d->x; a.ldx = d->ldx;
    a.tab = d->tab; a.ld_tab = d->ld_tab; a.tab_rows = d->tab_rows;
    a.src = (const long long *)d->src;
    a.mean = d->mean; a.inv_std = d->inv_std;
    a.out = d->out; a.ldo = d->ldo;
    return EGP_OK;
}

}  // namespace

extern "C" {

int egp_gail_rows_f32(const egp_gail_rows_desc *d, void *stream) {
    RowsArgs a{};
    int rc = fill_rows_args(d, a);
    if (rc != EGP_OK) return rc;
    if (d->n == 0 || d->H + d->S == 0) return EGP_OK;
    EGP_REQUIRE(d->out && d->ldo >= (int64_t)d->H + d->S, "NULL out / row stride smaller than the row");
    EGP_REQUIRE(d->H == 0 || (d->ctx && d->idx && d->ld_ctx >= d->H), "NULL context operand / row stride smaller than the row");
    EGP_REQUIRE(d->S == 0 || (d->x && d->tab && d->src && d->ldx >= d->S && d->ld_tab >= d->S), "NULL state / expert operand / row stride smaller than the row");
    EGP_REQUIRE((d->mean == nullptr) == (d->inv_std == nullptr), "mean and inv_std go together");
    if (d->src_host && d->S > 0) {
        for (int32_t i = 0; i < d->n; ++i) {
            if (d->src_host[i] < 0 || d->src_host[i] >= d->tab_rows) {
                egp::set_error("invalid argument: src[%d] = %lld is no row of the expert table (%lld rows)", (int)i, (long long)d->src_host[i],
                               (long long)d->tab_rows);
                return EGP_E_INVALID;
            }
        }
    }
    // 16-byte moves when the width, every row stride and every base on both sides allow, single floats otherwise
    const bool out_ok = aligned16(d->out) && d->ldo % 4 == 0;
    a.wide_ctx = (d->H > 0 && d->H % 4 == 0 && out_ok && aligned16(d->ctx) && d->ld_ctx % 4 == 0) ? 1 : 0;
    const bool tail_ok = d->S > 0 && d->S % 4 == 0 && d->H % 4 == 0 && out_ok;
    a.wide_x = (tail_ok && aligned16(d->x) && d->ldx % 4 == 0) ? 1 : 0;
    a.wide_tab = (tail_ok && aligned16(d->tab) && d->ld_tab % 4 == 0 && (!d->mean || (aligned16(d->mean) && aligned16(d->inv_std)))) ? 1 : 0;
    const int widest = d->H > d->S ? d->H : d->S;
    const long blocks = rows_grid((long)d->n * ((a.wide_ctx && (a.wide_x || d->S == 0)) ? (widest + 3) / 4 : widest));
    k_gail_rows<<<dim3((unsigned)blocks), dim3(ROWS_BLOCK), 0, (hipStream_t)stream>>>(a);
    return after_launch("k_gail_rows");
}

int egp_gail_rows_bwd_f32(const egp_gail_rows_desc *d, void *stream) {
    RowsArgs a{};
    int rc = fill_rows_args(d, a);
    if (rc != EGP_OK) return rc;
    if (d->n == 0 || d->H == 0) return EGP_OK;
    EGP_REQUIRE(d->dout && d->idx && d->dctx, "NULL pointer");
    EGP_REQUIRE(d->ldo >= d->H && d->ld_ctx >= d->H, "row stride smaller than the row");
    a.out = const_cast<float *>(d->dout);
    a.dctx = d->dctx;
    a.wide_ctx = (d->H % 4 == 0 && aligned16(d->dout) && d->ldo % 4 == 0 && aligned16(d->dctx) && d->ld_ctx % 4 == 0) ? 1 : 0;
    const long blocks = rows_grid((long)d->n * (a.wide_ctx ? d->H / 4 : d->H));
    k_gail_rows_bwd<<<dim3((unsigned)blocks), dim3(ROWS_BLOCK), 0, (hipStream_t)stream>>>(a);
    return after_launch("k_gail_rows_bwd");
}

int64_t egp_bce_logits_workspace_bytes(int32_t n) {
    (void)n;
    return (int64_t)(2 * BCE_MAX_BLOCKS) * (int64_t)sizeof(double) + 64;
}

int egp_bce_logits_f32(const egp_bce_logits_desc *d, void *stream) {
    EGP_REQUIRE(d, "descriptor is NULL");
    EGP_REQUIRE(d->n >= 0 && d->n <= (1 << 30) && d->n_e >= 0 && d->n_e <= (1 << 30), "bad row count");
    EGP_REQUIRE(d->losses && d->workspace, "NULL losses / workspace");
    if (d->n + d->n_e == 0) {
        hipError_t e = hipMemsetAsync(d->losses, 0, 2 * sizeof(double), (hipStream_t)stream);
        if (e != hipSuccess) { egp::set_error("hipMemsetAsync failed: %s", hipGetErrorString(e)); return EGP_E_HIP; }
        return EGP_OK;
    }
    EGP_REQUIRE(d->z, "NULL logits");
    BceArgs a{};
    a.n = d->n; a.n_e = d->n_e; a.z = d->z;
    a.inv_n_g = d->inv_n_g; a.inv_n_e = d->inv_n_e;
    a.dz = d->dz; a.score = d->score_out;
    a.losses = d->losses;
    a.part = (double *)d->workspace;
    long nb = ((long)d->n + d->n_e + 4 * BCE_BLOCK - 1) / (4 * BCE_BLOCK);          // ~4 elements per thread
    nb = nb < 1 ? 1 : (nb > BCE_MAX_BLOCKS ? BCE_MAX_BLOCKS : nb);
    k_bce_logits<<<dim3((unsigned)nb), dim3(BCE_BLOCK), 0, (hipStream_t)stream>>>(a);
    int rc = after_launch("k_bce_logits");
    if (rc != EGP_OK) return rc;
    k_bce_logits_final<<<dim3(1), dim3(BCE_BLOCK), 0, (hipStream_t)stream>>>(a, (int)nb);
    return after_launch("k_bce_logits_final");
}

}  // extern "C"
