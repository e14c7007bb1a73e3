// Dilated temporal convolution of the TCN video net on time-major batches (egp_tcn_conv_f32, include/egopose_hip.h).
//
// In the (T*B, C) matrix of a (T, B, C) batch a tap of the convolution is the same matrix shifted by s*B whole rows, so a
// convolution is a sum of row-shifted matrix products
//     acc[r, :] = sum_j X[r + s_j*B, :] W_j^T        s_j = shift0 + j*dshift, rows whose time step leaves [0, T) are zero.
// The forward pass runs it with s_j = j*d - pad, the data gradient with the weights transposed and the shifts negated: one
// kernel, the epilogue (bias, ReLU, dropout mask, ReLU gate, the residual product, a second output) chosen by the descriptor.
//
// Products are exact float32 (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain). A workgroup of 4 waves owns 128 rows x 32*NT
// columns, a wave 32 rows x NT tiles of 32 columns; operands go through LDS 16 k-columns at a time, k-major, while the
// next chunk's global loads are in flight in registers. A row outside the buffer or the time range is never addressed.
#include "egp_internal.hpp"

namespace {

constexpr int BM = 128, KC = 16, NTHREADS = 256;
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int NT>
struct Tile {
    static constexpr int BN = 32 * NT;
    float a[KC][BM + 4];       // [k][row]: the MFMA's A operand reads 32 consecutive rows of one k
    float b[KC][BN + 4];       // [k][output column]
};

// acc += sum over `taps` row-shifted products of X (ldx, K columns) with W ([tap][n_out][K]) for this workgroup's tile.
template <int NT>
__device__ __forceinline__ void product(f32x16 (&acc)[NT], Tile<NT> &lds, const float *__restrict__ X, int64_t ldx,
                                        const float *__restrict__ W, int K, int taps, int shift0, int dshift, int T, int B, int M,
                                        int n_out, int r0, int c0) {
    constexpr int BN = Tile<NT>::BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kc = (tid & 3) * 4;                       // this thread's 4 k-columns of a chunk, for both operands
    const int xl[2] = {tid >> 2, (tid >> 2) + 64};      // its two rows of the X tile
    int xt[2];                                          // their time steps, -1 for rows behind the last one
    for (int i = 0; i < 2; i++) xt[i] = r0 + xl[i] < M ? (r0 + xl[i]) / B : -1;
    const int wl = tid >> 2;                            // its row (output column) of the W tile
    const bool w_ok = wl < BN && c0 + wl < n_out;
    // taps none of this workgroup's rows reach are skipped (uniform over the workgroup)
    const int t_lo = r0 / B, t_hi = (min(r0 + BM, M) - 1) / B;
    auto tap_live = [&](int j) { const int s = shift0 + j * dshift; return t_hi + s >= 0 && t_lo + s < T; };
    auto next_tap = [&](int j) { while (j < taps && !tap_live(j)) j++; return j; };

    float4 xr[2], wr;
    auto load = [&](int j, int k0) {
        const int s = shift0 + j * dshift;
        for (int i = 0; i < 2; i++) {
            xr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (xt[i] >= 0 && xt[i] + s >= 0 && xt[i] + s < T)          // the source row r + s*B then lies in [0, M)
                xr[i] = *reinterpret_cast<const float4 *>(X + (int64_t)(r0 + xl[i] + s * B) * ldx + k0 + kc);
        }
        wr = make_float4(0.f, 0.f, 0.f, 0.f);
        if (w_ok) wr = *reinterpret_cast<const float4 *>(W + ((int64_t)j * n_out + c0 + wl) * K + k0 + kc);
    };

    int j = next_tap(0), k0 = 0;
    if (j < taps) load(j, 0);
    while (j < taps) {
        __syncthreads();                                // the previous chunk's MFMAs have read the tile
        for (int i = 0; i < 2; i++) {
            lds.a[kc + 0][xl[i]] = xr[i].x; lds.a[kc + 1][xl[i]] = xr[i].y;
            lds.a[kc + 2][xl[i]] = xr[i].z; lds.a[kc + 3][xl[i]] = xr[i].w;
        }
        if (wl < BN) {
            lds.b[kc + 0][wl] = wr.x; lds.b[kc + 1][wl] = wr.y; lds.b[kc + 2][wl] = wr.z; lds.b[kc + 3][wl] = wr.w;
        }
        __syncthreads();
        int nj = j, nk = k0 + KC;
        if (nk >= K) { nk = 0; nj = next_tap(j + 1); }
        if (nj < taps) load(nj, nk);                    // in flight under the MFMAs below
        const int kh = lane >> 5, l31 = lane & 31;
#pragma unroll
        for (int kk = 0; kk < KC / 2; kk++) {
            const float a = lds.a[2 * kk + kh][wave * 32 + l31];
#pragma unroll
            for (int nt = 0; nt < NT; nt++)
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, lds.b[2 * kk + kh][nt * 32 + l31], acc[nt], 0, 0, 0);
        }
        j = nj; k0 = nk;
    }
}

// acc element = f(its value, row, column) for every element of this lane's accumulators that lies inside the (M, n_out) result
template <int NT, typename F>
__device__ __forceinline__ void for_each_element(f32x16 (&acc)[NT], int M, int n_out, int r0, int c0, F f) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
        const int col = c0 + nt * 32 + (lane & 31);
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int row = r0 + wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
            if (row < M && col < n_out) acc[nt][i] = f(acc[nt][i], row, col);
        }
    }
}

template <int NT>
__global__ __launch_bounds__(NTHREADS) void k_tcn_conv(const egp_tcn_desc d) {
    __shared__ Tile<NT> lds;
    const int M = d.T * d.B, n_out = d.C_out;
    const int r0 = blockIdx.x * BM, c0 = blockIdx.y * Tile<NT>::BN;
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[nt][i] = 0.f;

    product<NT>(acc, lds, d.X, d.ldx, d.W, d.C_in, d.taps, d.shift0, d.dshift, d.T, d.B, M, n_out, r0, c0);
    const bool second = d.X2 != nullptr;
    if (second && !d.x2_after_act) {                    // one sum with the main product (the residual branch of a data gradient)
        if (d.W2) product<NT>(acc, lds, d.X2, d.ldx2, d.W2, d.C2, 1, 0, 0, d.T, d.B, M, n_out, r0, c0);
        else for_each_element<NT>(acc, M, n_out, r0, c0, [&](float v, int r, int c) { return v + d.X2[(int64_t)r * d.ldx2 + c]; });
    }
    for_each_element<NT>(acc, M, n_out, r0, c0, [&](float v, int r, int c) {
        if (d.bias) v += d.bias[c];
        if (d.relu) v = fmaxf(v, 0.f);
        if (d.mask) v *= d.mask[(int64_t)r * d.ldmask + c];
        if (d.gate) v = d.gate[(int64_t)r * d.ldgate + c] > 0.f ? v : 0.f;
        if (d.out2) d.out2[(int64_t)r * d.ldout2 + c] = v;
        return v;
    });
    if (second && d.x2_after_act) {                     // the residual of a block's forward pass: on top of the activation
        if (d.W2) product<NT>(acc, lds, d.X2, d.ldx2, d.W2, d.C2, 1, 0, 0, d.T, d.B, M, n_out, r0, c0);
        for_each_element<NT>(acc, M, n_out, r0, c0, [&](float v, int r, int c) {
            if (!d.W2) v += d.X2[(int64_t)r * d.ldx2 + c];
            if (d.b2) v += d.b2[c];
            return fmaxf(v, 0.f);
        });
    }
    for_each_element<NT>(acc, M, n_out, r0, c0, [&](float v, int r, int c) { d.out[(int64_t)r * d.ldout + c] = v; return v; });
}

bool chan_ok(int c) { return c >= 16 && c <= 512 && c % 16 == 0; }
bool vec_ok(const void *p, int64_t ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; }

}  // namespace

extern "C" int egp_tcn_conv_f32(const egp_tcn_desc *d, void *stream) {
    EGP_REQUIRE(d, "descriptor is NULL");
    EGP_REQUIRE(d->T >= 0 && d->B >= 0 && d->T < (1 << 30), "T must be in [0, 2^30), B >= 0");
    EGP_REQUIRE((int64_t)d->T * d->B < ((int64_t)1 << 31) - BM, "T*B must stay below 2^31");
    EGP_REQUIRE(chan_ok(d->C_in) && chan_ok(d->C_out), "C_in and C_out must be multiples of 16 in [16, 512]");
    EGP_REQUIRE(d->taps >= 1 && d->taps <= 7, "1 to 7 taps");
    for (int j = 0; j < d->taps; j++) {
        const int64_t s = (int64_t)d->shift0 + (int64_t)j * d->dshift;
        EGP_REQUIRE(s > -((int64_t)1 << 30) && s < ((int64_t)1 << 30), "tap shift out of range");
    }
    EGP_REQUIRE(d->X && d->W && d->out, "NULL operand");
    EGP_REQUIRE(d->ldx >= d->C_in && vec_ok(d->X, d->ldx) && vec_ok(d->W, 4), "X / W: 16-byte aligned rows, ldx >= C_in");
    EGP_REQUIRE(d->ldout >= d->C_out, "ldout < C_out");
    EGP_REQUIRE(!d->mask || d->ldmask >= d->C_out, "ldmask < C_out");
    EGP_REQUIRE(!d->gate || d->ldgate >= d->C_out, "ldgate < C_out");
    EGP_REQUIRE(!d->out2 || d->ldout2 >= d->C_out, "ldout2 < C_out");
    EGP_REQUIRE(d->x2_after_act == 0 || d->x2_after_act == 1, "x2_after_act must be 0 or 1");
    if (d->X2) {
        EGP_REQUIRE(d->ldx2 >= d->C2, "ldx2 < C2");
        if (d->W2) EGP_REQUIRE(chan_ok(d->C2) && vec_ok(d->X2, d->ldx2) && vec_ok(d->W2, 4), "X2 / W2: C2 a multiple of 16 in [16, 512], 16-byte aligned rows");
        else EGP_REQUIRE(d->C2 == d->C_out && !d->b2, "an identity second term needs C2 == C_out and no b2");
    } else {
        EGP_REQUIRE(!d->W2 && !d->b2 && !d->x2_after_act, "W2 / b2 / x2_after_act without X2");
    }
    const int64_t M = (int64_t)d->T * d->B;
    if (M == 0) return EGP_OK;
    const dim3 block(NTHREADS);
    if (d->C_out > 32) k_tcn_conv<2><<<dim3((unsigned)((M + BM - 1) / BM), (unsigned)((d->C_out + 63) / 64)), block, 0, (hipStream_t)stream>>>(*d);
    else k_tcn_conv<1><<<dim3((unsigned)((M + BM - 1) / BM), 1), block, 0, (hipStream_t)stream>>>(*d);
    EGP_HIP_CHECK(hipGetLastError());
    return EGP_OK;
}
