// Rollout-time policy step in ONE launch:
//   x = [video context row (fp32) | filtered observation (fp64 -> fp32)]  ->  MLP (hidden layers + activation)
//   -> action_mean (Linear) -> action = mean + exp(log_std) * noise  (float32 arithmetic, stored as float64 for
//   the engine), i.e. PolicyGaussian.select_action of models/policy_gaussian.py:19-27 over models/mlp.py:5-25 with
//   the VideoStateNet concatenation of models/video_state_net.py:37-43, for all envs of a group at once.
// During a rollout this chain is ~13 launch-bound torch ops per tick (3 GEMMs of 512 rows, gather, cat, casts).
//
// Round 4: the layer products run on the matrix cores in exact float32 (v_mfma_f32_4x4x1_16b_f32: 16 independent 4 x 4
// outer products per instruction = 4 batch rows x 64 output columns x one input feature; an fmaf chain, bit for bit).
// A workgroup owns R = 4 or 8 batch rows and walks the layers with the activations in LDS. Its NW waves split a layer's
// input features (k) between them; every wave streams its k range of the PACKED weights (egp_mlp_pack_f32: for each
// group of 64 output columns and each quad of input features one 1-KiB block, lane l's 16 bytes = column l at the four
// k of the quad -> one coalesced global_load_dwordx4 per wave and block, PF blocks in flight per column group) and
// reads the rows' activations as broadcast ds_read_b128; the per-wave partial sums meet in LDS, where bias and
// activation are applied in a fixed order (deterministic, independent of the row's position in the batch).
// The weights of the next pass are requested BEFORE the partial sums are written and reduced (they do not depend on the
// activations), and the first layer's before the input rows are gathered: the dependent global round trips of a tick
// (context-row index -> context row, tile statistics -> filtered observation) overlap the weight stream.
//
// ego_forecast (egp_policy_desc.cell, forecast_body below): the state first goes through one step of the state LSTM cell
// (models/rnn.py:29-36, models/video_forecast_net.py:88-93) -- its gate pre-activations are one more layer of the same passes, its
// epilogue the gates -- and x = [context row | h']; h / c are updated in place.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "egp_internal.hpp"
#include "egp_filter_dev.hpp"
#include "egp_act_dev.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The filter's apply pass folded into the policy step (egp_policy_desc's filter block): the observation rows of the tile are
// formed, normalised with the running statistics merged from the tick's tile partials (exactly k_zf_apply's arithmetic: same
// merge order, same expression, float64) and written to next_states[k] / states[k + 1] on their way into the MLP's input -- one
// launch and its dependent memory round trips less on the chain filter -> policy -> env-step of every tick without a reset.
struct PolFilter {
    egp::ZfSrc<double> src;          // rows of the group: observation from (qpos, qvel)
    const double *st_in; double *st_out;
    const double *ws; int n_tiles;
    double clip;
    double *y, *y2;                  // [n][dim] each (y2 may be NULL)
};

// EGP_POLICY_TRACE (tools/probes/policy_trace.py builds the library with it): wall_clock64 stamps (100 MHz) of thread 0 of one workgroup
#ifdef EGP_POLICY_TRACE
__device__ long long g_pol_trace[64];
#define POL_TR(i) do { if (blockIdx.x == EGP_POLICY_TRACE && threadIdx.x == 0) g_pol_trace[i] = wall_clock64(); } while (0)
// (the prologue of a wave that holds state columns: stamps 32..39 of thread 128)
#define POL_TR_S(i) do { if (blockIdx.x == EGP_POLICY_TRACE && threadIdx.x == 128) g_pol_trace[32 + (i)] = wall_clock64(); } while (0)
#else
#define POL_TR(i) do { } while (0)
#define POL_TR_S(i) do { } while (0)
#endif

constexpr int POL_MAX_LAYERS = 8;
constexpr int POL_GC = 5;            // column groups (64 outputs each) a pass accumulates in registers: 320 >= the 300-wide layer
constexpr int POL_PS = POL_GC * 64 + 4;   // row stride of a wave's partial sums (floats)

// tile of the policy step, both kernels: rows per workgroup x waves x weight blocks in flight per column group.
// Round-4 sweep on the MI355X (tools/probes/policy_tile_sweep.sh; 512 rows, bench workload): 4x4x2 15.2 us per launch and the
// lowest / least scattered T_sample; 4x8x2 14.9 us; 8-row tiles 19-21 us (twice the MFMAs per workgroup on half the CUs).
constexpr int POL_R = 4, POL_NW = 4, POL_PF = 2;

// The dynamic LDS of a workgroup, for the kernels and for the host's byte count (float offsets; cur is at 0):
//   cur[R][xs] | nxt[R][xs] | part[NW][R][POL_PS] | every layer's bias | exp(log_std) | the rows' noise | the kernel's own tail:
//   the cell's c rows (`cell_floats` = R x hidden size; the forecast step), then the filter's merged (mean, 1 / std) doubles
//   (`ms_doubles` = 2 x obs dim) behind a pad to an even float -- 8-byte aligned; the pad float is always reserved
struct PolCarve {
    int nxt, part, bias, sd, noise, tail, ms, end;
};
template <int R, int NW>
__host__ __device__ __forceinline__ PolCarve pol_carve(int xs, int sum_out4, int out_last, int cell_floats = 0, int ms_doubles = 0) {
    const int out4 = (out_last + 3) & ~3;
    PolCarve c;
    c.nxt = R * xs; c.part = 2 * R * xs; c.bias = c.part + NW * R * POL_PS;
    c.sd = c.bias + sum_out4; c.noise = c.sd + out4; c.tail = c.noise + R * out4;
    c.ms = (c.tail + cell_floats + 1) & ~1;
    c.end = c.tail + cell_floats + 1 + 2 * ms_doubles;
    return c;
}

struct PolLayers {
    const float *wp[POL_MAX_LAYERS];     // packed weights (egp_mlp_pack_f32)
    const float *bias[POL_MAX_LAYERS];
    int in_dim[POL_MAX_LAYERS], out_dim[POL_MAX_LAYERS];
    int n;                                // hidden layers + the output layer
    int sum_out4;                         // sum of the output widths, each rounded up to 4 (the LDS copy of the biases)
    int warm_lines;                       // 128-byte lines of the packed weights when the layers' buffers follow each other in memory, else 0
};

__device__ __forceinline__ float pol_act(float v, int kind) {
    if (kind == 1) return fmaxf(v, 0.0f);                 // relu
    if (kind == 2) return egp_act_sigmoid(v);             // sigmoid
    return egp_act_tanh(v);                               // tanh  (egp_act_dev.hpp: the formulas the update's epilogues use)
}

// nn.Linear weight W[out][in] (row stride ldw) -> packed[(g * nkq + kq) * 64 + lane][kk] = W[64 g + lane][4 kq + kk], zero outside
__global__ void k_mlp_pack(const float *__restrict__ W, long ldw, int in_dim, int out_dim, float *__restrict__ dst, long total) {
    const int nkq = (in_dim + 3) >> 2;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int kk = (int)(e & 3), lane = (int)((e >> 2) & 63);
        const long blk = e >> 8;
        const int kq = (int)(blk % nkq), g = (int)(blk / nkq);
        const int o = 64 * g + lane, i = 4 * kq + kk;
        dst[e] = (o < out_dim && i < in_dim) ? W[(long)o * ldw + i] : 0.0f;
    }
}

// The wave's weight blocks of one pass: PF quads x up to POL_GC column groups in flight.
template <int PF>
struct PolStage {
    f32x4 w[PF][POL_GC];
};

// request the blocks of quads kq .. kq + PF - 1 (clamped into the wave's range) of column groups g0 .. g0 + ng - 1 (clamped)
// (a pass over ONE column group -- the output layer -- uses the POL_GC slots of a stage for POL_GC different quads: PF x POL_GC quads
//  in flight instead of PF; with PF of them the 50 quads of the 200 -> 52 layer were a chain of L2 round trips, 1.8 of the step's 15 us)
template <int PF>
__device__ __forceinline__ void pol_preload(PolStage<PF> &st, const float *__restrict__ wl, int nkq, int g0, int ng, int kq0, int kq1, int lane) {
#pragma unroll
    for (int s = 0; s < PF; ++s) {
#pragma unroll
        for (int g = 0; g < POL_GC; ++g) {
            const int k = min(ng == 1 ? kq0 + s * POL_GC + g : kq0 + s, kq1 - 1);
            const int gg = g0 + min(g, ng - 1);
            st.w[s][g] = *reinterpret_cast<const f32x4 *>(wl + (((long)gg * nkq + k) * 64 + lane) * 4);
        }
    }
}

// One pass: acc[g][h] += W[cols of group g0 + g][k range of the wave] * x[rows 4 h .. 4 h + 3][k range]. Straight-line loop body
// (every load is unconditional with a clamped address, quads past the wave's range multiply zeros), so the compiler's
// counted waits keep PF blocks per group in flight.
template <int NG, int R, int PF>
__device__ __forceinline__ void pol_pass(PolStage<PF> &st, const float *__restrict__ wl, int nkq, int g0, int kq0, int kq1, const float *x, int xs,
                                         int lane, f32x4 (&acc)[POL_GC][R / 4]) {
    const float *xr = x + (lane & 3) * xs;
    const float *wb = wl + (((long)g0 * nkq) * 64 + lane) * 4;
    const long gstride = (long)nkq * 256;
    if constexpr (NG == 1) {                             // one column group: the stage's slots hold PF x POL_GC consecutive quads
        constexpr int D = PF * POL_GC;
        for (int kq = kq0; kq < kq1; kq += D) {
#pragma unroll
            for (int s = 0; s < PF; ++s)
#pragma unroll
                for (int g = 0; g < POL_GC; ++g) {
                    const int k = kq + s * POL_GC + g;
                    const bool live = k < kq1;
                    const int kc = live ? k : kq1 - 1;
                    f32x4 b[R / 4];
#pragma unroll
                    for (int h = 0; h < R / 4; ++h) {
                        const f32x4 v = *reinterpret_cast<const f32x4 *>(xr + 4 * h * xs + 4 * kc);
                        b[h][0] = live ? v[0] : 0.0f; b[h][1] = live ? v[1] : 0.0f; b[h][2] = live ? v[2] : 0.0f; b[h][3] = live ? v[3] : 0.0f;
                    }
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                        for (int h = 0; h < R / 4; ++h)
                            acc[0][h] = __builtin_amdgcn_mfma_f32_4x4x1f32(st.w[s][g][kk], b[h][kk], acc[0][h], 0, 0, 0);
                    const int kn = min(k + D, kq1 - 1);
                    st.w[s][g] = *reinterpret_cast<const f32x4 *>(wb + (long)kn * 256);
                }
        }
        return;
    }
    for (int kq = kq0; kq < kq1; kq += PF) {
#pragma unroll
        for (int s = 0; s < PF; ++s) {
            const int k = kq + s;
            const bool live = k < kq1;
            const int kc = live ? k : kq1 - 1;
            f32x4 b[R / 4];
#pragma unroll
            for (int h = 0; h < R / 4; ++h) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(xr + 4 * h * xs + 4 * kc);
                b[h][0] = live ? v[0] : 0.0f; b[h][1] = live ? v[1] : 0.0f; b[h][2] = live ? v[2] : 0.0f; b[h][3] = live ? v[3] : 0.0f;
            }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int g = 0; g < NG; ++g)
#pragma unroll
                    for (int h = 0; h < R / 4; ++h)
                        acc[g][h] = __builtin_amdgcn_mfma_f32_4x4x1f32(st.w[s][g][kk], b[h][kk], acc[g][h], 0, 0, 0);
            const int kn = min(k + PF, kq1 - 1);
#pragma unroll
            for (int g = 0; g < NG; ++g) st.w[s][g] = *reinterpret_cast<const f32x4 *>(wb + g * gstride + (long)kn * 256);
        }
    }
}

// a wave's share [kq0, kq1) of a layer's nkq input quads (wave scalar: the k loops' bounds live in SGPRs)
struct PolSplit {
    int nkq, kq0, kq1;
};
template <int NW>
__device__ __forceinline__ PolSplit pol_split(int in_dim, int wave) {
    const int nkq = (in_dim + 3) >> 2;
    return PolSplit{nkq, wave * nkq / NW, (wave + 1) * nkq / NW};
}

// the wave's first blocks of the pass over column groups g0 .. of layer l
template <int NW, int PF>
__device__ __forceinline__ void pol_preload_pass(PolStage<PF> &st, const PolLayers &L, int l, int g0, int wave, int lane) {
    const PolSplit k = pol_split<NW>(L.in_dim[l], wave);
    pol_preload<PF>(st, L.wp[l], k.nkq, g0, min(POL_GC, ((L.out_dim[l] + 63) >> 6) - g0), k.kq0, max(k.kq1, k.kq0 + 1), lane);
}

// L2 warm-up. A kernel starts with a cold L2 on every XCD (the per-XCD L2s are invalidated at kernel boundaries), so the
// first touch of a weight line costs a trip to the memory side (~0.7 us) and a wave's PF x POL_GC KiB in flight turn the
// weight stream into a chain of such trips. The workgroups of one XCD (round-robin dispatch: blockIdx & 7) therefore each
// touch a DIFFERENT slice of the packed weights right away -- one dword per 128-byte line, all requests in flight at once --
// while the input rows are gathered; by the time the k loops start, the XCD's L2 holds every layer and the stream runs at
// L2-hit latency. (Pure prefetch: results are never used; up to POL_WARM x T lines per workgroup; needs the layers' packed
// buffers back to back in memory -- FusedGaussianPolicy allocates them so -- else warm_lines = 0 and one line is touched.)
constexpr int POL_WARM = 8;
template <int T>
__device__ __forceinline__ void pol_warm_request(const PolLayers &L, int tid, float (&warm)[POL_WARM]) {
    const int per_xcd = (gridDim.x + 7) >> 3, me = blockIdx.x >> 3;
    const int lo = (int)((long)L.warm_lines * me / per_xcd), hi = (int)((long)L.warm_lines * (me + 1) / per_xcd);
#pragma unroll
    for (int u = 0; u < POL_WARM; ++u) {
        const int i = min(lo + tid + u * T, max(hi - 1, 0));
        warm[u] = L.wp[0][(long)i * 32];
    }
}
// (behind the inputs' barrier the warm-up loads have long landed; their registers are free from here on)
__device__ __forceinline__ void pol_warm_sink(const float (&warm)[POL_WARM]) {
    float sink = 0.0f;
#pragma unroll
    for (int u = 0; u < POL_WARM; ++u) sink += warm[u];
    asm volatile("" ::"v"(sink));
}

// What the forecast step's layer 0 -- the state LSTM's gates -- needs in its epilogue (see forecast_body)
struct PolCell {
    const float *s_c;                // c rows in LDS [R][hs]
    float *h_io, *c_io; long hc_stride;
    int hs, ctx_dim;
};

// The layers, one pass per chunk of POL_GC x 64 output columns: `cur` holds the workgroup's input rows, `st` the wave's first
// blocks of layer 0, `split` its share of layer 0's quads. Epilogue of a pass: bias + the waves' partial sums in fixed order
// (deterministic), then the activation into `nxt` (hidden layer), the Gaussian head (last layer) or, CELL0, layer 0's gates:
// h' behind the context columns that the prologue has put into `nxt`, h' / c' to the caller's rows. `critic` (BOTH kernels only, a
// workgroup-uniform flag; constant false elsewhere): the last layer is a value head -- no Gaussian head, no float64 action; its
// float32 output goes where the actor's goes with `mean_out`.
template <int R, int NW, int PF, bool CELL0, bool BOTH = false>
__device__ __forceinline__ void pol_layers(float *cur, float *nxt, float *part, const float *s_bias, const float *s_sd, const float *s_noise,
                                           PolStage<PF> &st, PolSplit split, const PolLayers &L, int act_kind, int xs, int r0, int n, int wave,
                                           const float *__restrict__ noise, double *__restrict__ action, float *__restrict__ mean_out,
                                           const PolCell &C, bool critic_flag = false) {
    constexpr int T = NW * 64, PS = POL_PS;
    const bool critic = BOTH && critic_flag;
    const int tid = threadIdx.x, lane = tid & 63;
    int bias_off = 0;
    for (int l = 0; l < L.n; ++l) {
        const int out = L.out_dim[l];
        const int ng_all = (out + 63) >> 6;
        const bool last = l == L.n - 1;
        const float *wl = L.wp[l];
        for (int g0 = 0; g0 < ng_all; g0 += POL_GC) {
            const int ng = min(POL_GC, ng_all - g0);
            f32x4 acc[POL_GC][R / 4];
#pragma unroll
            for (int g = 0; g < POL_GC; ++g)
#pragma unroll
                for (int h = 0; h < R / 4; ++h) acc[g][h] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (split.kq1 > split.kq0) {
                const int nkq = split.nkq, kq0 = split.kq0, kq1 = split.kq1;
                switch (ng) {
                    case 1: pol_pass<1, R, PF>(st, wl, nkq, g0, kq0, kq1, cur, xs, lane, acc); break;
                    case 2: pol_pass<2, R, PF>(st, wl, nkq, g0, kq0, kq1, cur, xs, lane, acc); break;
                    case 3: pol_pass<3, R, PF>(st, wl, nkq, g0, kq0, kq1, cur, xs, lane, acc); break;
                    case 4: pol_pass<4, R, PF>(st, wl, nkq, g0, kq0, kq1, cur, xs, lane, acc); break;
                    default: pol_pass<5, R, PF>(st, wl, nkq, g0, kq0, kq1, cur, xs, lane, acc); break;
                }
            }
            POL_TR(3 + 4 * l);
            // the next pass's first blocks: same layer's next column chunk, or the next layer
            {
                int nl = l, ng0 = g0 + POL_GC;
                if (ng0 >= ng_all) { nl = l + 1; ng0 = 0; }
                if (nl < L.n) pol_preload_pass<NW, PF>(st, L, nl, ng0, wave, lane);
            }
            // partial sums -> LDS: register i of lane 4 b + j = out[row 4 h + j][column 64 g + 4 b + i]
#pragma unroll
            for (int g = 0; g < POL_GC; ++g)
                if (g < ng) {
#pragma unroll
                    for (int h = 0; h < R / 4; ++h)
                        *reinterpret_cast<f32x4 *>(part + ((wave * R) + 4 * h + (lane & 3)) * PS + 64 * g + (lane & ~3)) = acc[g][h];
                }
            POL_TR(4 + 4 * l);
            __syncthreads();
            POL_TR(5 + 4 * l);
            const int c_base = 64 * g0;
            const int cw = min(out - c_base, POL_GC * 64);               // real columns of this chunk
            if (CELL0 && l == 0) {
                // gate epilogue: one thread per unit, columns 4 u .. 4 u + 3 = (i, f, g, o); fixed summation order
                for (int j = tid; j < (cw >> 2); j += T) {
                    const int u = (c_base >> 2) + j;
                    const f32x4 bv = *reinterpret_cast<const f32x4 *>(s_bias + 4 * u);
                    f32x4 v[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) v[r] = bv;
#pragma unroll
                    for (int w = 0; w < NW; ++w)
#pragma unroll
                        for (int r = 0; r < R; ++r) v[r] += *reinterpret_cast<const f32x4 *>(part + (w * R + r) * PS + 4 * j);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const float gi = pol_act(v[r][0], 2), gf = pol_act(v[r][1], 2), gg = tanhf(v[r][2]), go = pol_act(v[r][3], 2);
                        const float cn = gf * C.s_c[r * C.hs + u] + gi * gg;
                        const float hn = go * tanhf(cn);
                        nxt[r * xs + C.ctx_dim + u] = hn;
                        const int row = r0 + r;
                        if (row < n) {
                            C.h_io[(long)row * C.hc_stride + u] = hn;
                            C.c_io[(long)row * C.hc_stride + u] = cn;
                        }
                    }
                }
            } else {
                const int cw4 = last ? cw : min((cw + 3) & ~3, ng * 64);      // hidden layers: the pad columns of the last quad become zeros
                for (int c = tid; c < cw4; c += T) {
                    const int col = c_base + c;
                    const bool real = c < cw;
                    const float bv = real ? s_bias[bias_off + col] : 0.0f;
                    float v[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) v[r] = bv;
#pragma unroll
                    for (int w = 0; w < NW; ++w)                         // fixed order: deterministic
#pragma unroll
                        for (int r = 0; r < R; ++r) v[r] += part[(w * R + r) * PS + c];
                    if (!last) {
#pragma unroll
                        for (int r = 0; r < R; ++r) nxt[r * xs + col] = real ? pol_act(v[r], act_kind) : 0.0f;
                    } else if (critic) {
#pragma unroll
                        for (int r = 0; r < R; ++r)
                            if (r0 + r < n) mean_out[(long)(r0 + r) * out + col] = v[r];
                    } else {
                        const float sd = noise ? s_sd[col] : 0.0f;
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const int row = r0 + r;
                            if (row >= n) continue;
                            const float a = noise ? fmaf(sd, s_noise[r * out + col], v[r]) : v[r];
                            action[(long)row * out + col] = (double)a;
                            if (mean_out) mean_out[(long)row * out + col] = v[r];
                        }
                    }
                }
            }
            __syncthreads();
            POL_TR(6 + 4 * l);
        }
        bias_off += (out + 3) & ~3;
        if (!last) {
            split = pol_split<NW>(L.in_dim[l + 1], wave);
            float *t = cur; cur = nxt; nxt = t;
        }
    }
}

// `stage_src` / `stage_dst` (optional): the tick's flag slab. The rollout stages the integer flags and context-row indices of a
// tick in pinned host memory; instead of a copy-engine transfer in front of this kernel (one more dependent operation, ~6 us,
// on the chain filter -> policy -> env-step of every tick) the workgroups copy the slab to its device copy themselves -- the
// kernels that run after the env-step (reward, filter) read it there -- and take their own rows' indices (`t_idx`, which then
// points into the pinned slab) with ONE load per row.
// BOTH (k_policy_value_w4): the workgroups with blockIdx.y != 0 take the same rows through a value stack (`critic`); the filter's
// outputs (y / y2, st_out) are left to the actor's workgroups.
template <int R, int NW, int PF, bool FILTER, bool BOTH = false>
__device__ __forceinline__ void policy_body(const float *__restrict__ ctx_rows, long ctx_row_stride, int ctx_dim,
                                  const long long *__restrict__ t_idx, const double *__restrict__ state, int state_dim, int n,
                                  const PolLayers &L, int act_kind, int xs, const float *__restrict__ log_std,
                                  const float *__restrict__ noise, double *__restrict__ action, float *__restrict__ mean_out,
                                  const unsigned *__restrict__ stage_src, unsigned *__restrict__ stage_dst, int stage_words,
                                  const PolFilter &F) {
    constexpr int T = NW * 64;
    const bool critic = BOTH && blockIdx.y != 0;
    extern __shared__ __attribute__((aligned(16))) float s_f[];     // see PolCarve; the tail: mean, 1 / std of the filter (2 dim doubles)
    const int out_last = L.out_dim[L.n - 1];
    const PolCarve lds = pol_carve<R, NW>(xs, L.sum_out4, out_last);
    float *cur = s_f, *nxt = s_f + lds.nxt, *part = s_f + lds.part;
    // small operands of the epilogues, fetched once in the prologue (a global load in an epilogue is a cold round trip on the chain):
    // every layer's bias | exp(log_std) | the rows' noise
    float *s_bias = s_f + lds.bias, *s_sd = s_f + lds.sd, *s_noise = s_f + lds.noise;
    double *s_ms = reinterpret_cast<double *>(s_f + lds.ms);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (scalar: the k loops' bounds live in SGPRs)
    const int r0 = blockIdx.x * R;
    const int in0 = ctx_dim + state_dim;

    POL_TR(0);
    // the rows' context-row indices first: the longest dependent chain of the prologue (index -> context row) starts here
    long tix[R];
#pragma unroll
    for (int r = 0; r < R; ++r) tix[r] = (long)t_idx[min(r0 + r, n - 1)];
    // One input column per thread (in0 <= T, the shipped 128 + 115 on 256 threads): the thread that normalises state column c
    // merges that column's statistics itself -- no LDS hop and no barrier between the filter's two phases, and the waves that
    // gather the context columns do not wait for the merge. (Waves hold context columns, state columns or straddle the
    // boundary: `state_wave` is wave-uniform.)
    const int in0p = (in0 + 3) & ~3;
    const bool own_col = in0p <= T;
    const bool state_wave = own_col && wave * 64 + 63 >= ctx_dim && wave * 64 < in0;
    const bool mine = tid >= ctx_dim && tid < in0;
    const int c_own = min(max(tid - ctx_dim, 0), state_dim - 1);
    // ... and the filter's loads next, ahead of the weight traffic below in the memory queue (loads return in order): the
    // statistics' tile partials and the rows' raw state, which do not depend on each other -- one cold round trip for both
    egp::ZfWaveMerge M;
    egp::ZfSrc<double>::Rows<R> pend;
    if constexpr (FILTER) {
        if (state_wave) {
            M.begin(state_dim, F.st_in, c_own);
            M.load(state_dim, F.n_tiles, F.ws, c_own, 0);
            pend = F.src.template load_rows<R>(r0, n, c_own);
        }
    }
    // the L2 warm-up (pol_warm_request), while the input rows are gathered
    float warm[POL_WARM];
    pol_warm_request<T>(L, tid, warm);
    // the first layer's own first blocks
    PolStage<PF> st;
    pol_preload_pass<NW, PF>(st, L, 0, 0, wave, lane);
    // the context columns (waiting for the indices requested first; everything above stays in flight)
    long ctx_off[R];                      // every thread resolves its rows' context offsets itself: no LDS hop + barrier between the two dependent loads
#pragma unroll
    for (int r = 0; r < R; ++r) ctx_off[r] = (long)min(r0 + r, n - 1) * ctx_row_stride + tix[r] * ctx_dim;
    float v_in[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v_in[r] = 0.0f;
    if (own_col && wave * 64 < ctx_dim) {
        if (tid < ctx_dim) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (r0 + r < n) v_in[r] = ctx_rows[ctx_off[r] + tid];
        }
    }
    // The small operands of the epilogues (every layer's bias | exp(log_std) | the rows' noise: one LDS range from s_bias on):
    // requested here into registers and parked in LDS behind the inputs' barrier -- a load followed by its LDS store right
    // here would stall every wave until the weight loads queued in front of it have landed.
    constexpr int POL_SMALL = 4;
    const int osd4 = (out_last + 3) & ~3;
    const int small_n = L.sum_out4 + (noise ? osd4 + R * out_last : 0);
    // (where LDS float f of the range comes from, without touching memory: 0 padding, 1 value, 2 exp(value), 3 zero)
    auto small_source = [&](int f, const float *&src) -> int {
        src = L.bias[0];
        if (f >= small_n) return 0;
        if (f < L.sum_out4) {
            int off = 0, kind = 0;
            for (int l = 0; l < L.n; ++l) {
                const int j = f - off;
                const bool hit = j >= 0 && j < L.out_dim[l];
                src = hit ? L.bias[l] + j : src;
                kind = hit ? 1 : kind;
                off += (L.out_dim[l] + 3) & ~3;
            }
            return kind;
        }
        const int j = f - L.sum_out4;
        if (j < osd4) {
            src = j < out_last ? log_std + j : src;
            return j < out_last ? 2 : 0;
        }
        const int e = j - osd4, r = e / out_last;
        const bool live = r0 + r < n;
        src = live ? noise + (long)(r0 + r) * out_last + (e - r * out_last) : src;
        return live ? 1 : 3;
    };
    float small_v[POL_SMALL];
    int small_kind[POL_SMALL];
#pragma unroll
    for (int u = 0; u < POL_SMALL; ++u) {
        const float *src;
        small_kind[u] = small_source(tid + u * T, src);
        small_v[u] = *src;                        // (unconditional: a load under a branch is waited for at the branch's end)
    }

    if constexpr (FILTER) if (!own_col) {   // k_zf_apply's first phase: the merged statistics, every workgroup for itself
        const int dim = state_dim;
        for (int c = tid; c < dim; c += T) {
            double cnt, mean, S;
            egp::zf_merge_column(dim, F.n_tiles, F.ws, F.st_in, c, cnt, mean, S);
            if (!critic && blockIdx.x == 0) {
                F.st_out[1 + c] = mean;
                F.st_out[1 + dim + c] = S;
                if (c == 0) F.st_out[0] = cnt;
            }
            const double var = cnt > 1.0 ? S / (cnt - 1.0) : mean * mean;
            s_ms[c] = mean;
            s_ms[dim + c] = 1.0 / (sqrt(var) + 1e-8);
        }
    }
    POL_TR(1);
    if (stage_src)
        for (int i = blockIdx.x * T + tid; i < stage_words; i += gridDim.x * T) stage_dst[i] = stage_src[i];
    if (own_col) {
        const int k = tid;
        float (&v)[R] = v_in;
        if (state_wave) {
            const int c = c_own;
            if constexpr (FILTER) {
                POL_TR_S(0);
                M.merge(F.n_tiles, 0);
                POL_TR_S(1);
                for (int q0 = 8; q0 < F.n_tiles; q0 += 8) {
                    M.load(state_dim, F.n_tiles, F.ws, c, q0);
                    M.merge(F.n_tiles, q0);
                }
                const double cnt = M.cnt, mean = M.mean, S = M.S;
                if (!critic && blockIdx.x == 0 && mine) {
                    F.st_out[1 + c] = mean;
                    F.st_out[1 + state_dim + c] = S;
                    if (c == 0) F.st_out[0] = cnt;
                }
                const double var = cnt > 1.0 ? S / (cnt - 1.0) : mean * mean;
                const double istd = 1.0 / (sqrt(var) + 1e-8);
                POL_TR_S(2);
                F.src.template finish_rows<R>(pend, r0, n, c);
                const double (&raw)[R] = pend.own;
                POL_TR_S(3);
                if (mine) {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int row = r0 + r;
                        if (row < n) {
                            double x = (raw[r] - mean) * istd;
                            if (F.clip > 0.0) x = fmin(fmax(x, -F.clip), F.clip);
                            if (!critic) {
                                const long e = (long)row * state_dim + c;
                                F.y[e] = x;
                                if (F.y2) F.y2[e] = x;
                            }
                            v[r] = (float)x;
                        }
                    }
                }
            } else if (mine) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (r0 + r < n) v[r] = (float)state[(long)(r0 + r) * state_dim + c];
            }
        }
        POL_TR_S(4);
        if (k < in0p) {
#pragma unroll
            for (int r = 0; r < R; ++r) cur[r * xs + k] = v[r];
        }
        POL_TR_S(5);
    } else {
    if constexpr (FILTER) __syncthreads();            // the merged statistics (s_ms) are read by the staging loop below
    for (int k = tid; k < in0p; k += T) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = r0 + r;
            float v = 0.0f;
            if (row < n && k < in0) {
                if (k < ctx_dim) {
                    v = ctx_rows[ctx_off[r] + k];
                } else if constexpr (FILTER) {            // k_zf_apply's second phase for this element
                    const int c = k - ctx_dim;
                    double x = ((double)F.src.at(row, c) - s_ms[c]) * s_ms[state_dim + c];
                    if (F.clip > 0.0) x = fmin(fmax(x, -F.clip), F.clip);
                    if (!critic) {
                        const long e = (long)row * state_dim + c;
                        F.y[e] = x;
                        if (F.y2) F.y2[e] = x;
                    }
                    v = (float)x;
                } else {
                    v = (float)state[(long)row * state_dim + (k - ctx_dim)];
                }
            }
            cur[r * xs + k] = v;
        }
    }
    }
    // the small operands into LDS (their loads have landed with the inputs'); the rest of a range beyond POL_SMALL x T floats directly
#pragma unroll
    for (int u = 0; u < POL_SMALL; ++u)
        if (small_kind[u]) s_bias[tid + u * T] = small_kind[u] == 2 ? expf(small_v[u]) : (small_kind[u] == 3 ? 0.0f : small_v[u]);
    for (int f = tid + POL_SMALL * T; f < small_n; f += T) {
        const float *src;
        const int kind = small_source(f, src);
        const float val = *src;
        if (kind) s_bias[f] = kind == 2 ? expf(val) : (kind == 3 ? 0.0f : val);
    }
    // (the barrier for the staged inputs in LDS only: __syncthreads() would also wait for the acknowledgement of the filtered
    //  rows' global stores above -- a trip to the memory side on the critical path; nothing in this kernel reads them back)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    pol_warm_sink(warm);
    POL_TR(2);

    pol_layers<R, NW, PF, false, BOTH>(cur, nxt, part, s_bias, s_sd, s_noise, st, pol_split<NW>(L.in_dim[0], wave), L, act_kind, xs, r0, n, wave,
                                       noise, action, mean_out, PolCell{}, critic);
}

// Registers: no cap. A resident K1 workgroup keeps one 346-register wave on every SIMD of its CU for the length of an env-step
// (160 left); with 2 groups the OTHER group's K1 occupies half the CUs while this group's policy step runs. A policy workgroup
// that needs more than 160 registers per SIMD cannot be placed beside a K1 wave and goes to the K1-free CUs -- which is where it
// runs fastest anyway (no polling waves competing for issue slots), so the prefetch depth is chosen for speed, not for fitting.
template <int R, int PF, bool FILTER>
__global__ __launch_bounds__(256) void k_policy_gaussian_w4(const float *__restrict__ ctx_rows, long ctx_row_stride, int ctx_dim,
                                                            const long long *__restrict__ t_idx, const double *__restrict__ state,
                                                            int state_dim, int n, PolLayers L, int act_kind, int xs,
                                                            const float *__restrict__ log_std, const float *__restrict__ noise,
                                                            double *__restrict__ action, float *__restrict__ mean_out,
                                                            const unsigned *__restrict__ stage_src, unsigned *__restrict__ stage_dst,
                                                            int stage_words, PolFilter F) {
    policy_body<R, 4, PF, FILTER>(ctx_rows, ctx_row_stride, ctx_dim, t_idx, state, state_dim, n, L, act_kind, xs, log_std, noise, action, mean_out,
                                  stage_src, stage_dst, stage_words, F);
}

// Actor and critic of a tick in one launch (egp_policy_desc.vlayers): a second grid dimension selects the net. Workgroup
// (x, 0) is k_policy_gaussian_w4 for rows x R ..: observation -> filter (frozen statistics) -> [policy ctx row | state] -> MLP ->
// Gaussian head, and it alone writes y / y2 / st_out. Workgroup (x, 1) takes the same rows through the value stack --
// [value ctx row | state] -> MLP -> value_head, one float32 per row -- and repeats the cheap frozen normalisation for itself, so
// no workgroup waits for another. Each net has its own layers, context slab, row stride, context width, activation and row
// stride in LDS (the launch's dynamic LDS is the larger of the two carve-ups); `t_idx` is shared. One copy of policy_body serves
// both kinds of workgroup (a workgroup-uniform flag skips the filter's stores and picks the last layer's epilogue); the actor's
// workgroups do the arithmetic of k_policy_gaussian_w4<R, PF, FILTER> on the same values: bit-identical actions.
struct PolNet {
    const float *ctx_rows; long ctx_row_stride; int ctx_dim;
    int act_kind, xs;
    PolLayers L;
};
struct PolNets { PolNet net[2]; };          // actor, critic: indexed with blockIdx.y where it lies, in the kernel's argument segment
template <int R, int PF, bool FILTER>
__global__ __launch_bounds__(256) void k_policy_value_w4(PolNets P, const long long *__restrict__ t_idx, const double *__restrict__ state,
                                                         int state_dim, int n, const float *__restrict__ log_std, const float *__restrict__ noise,
                                                         double *__restrict__ action, float *__restrict__ mean_out, float *__restrict__ value_out,
                                                         PolFilter F) {
    const bool critic = blockIdx.y != 0;
    const PolNet &N = P.net[blockIdx.y];
    policy_body<R, 4, PF, FILTER, true>(N.ctx_rows, N.ctx_row_stride, N.ctx_dim, t_idx, state, state_dim, n, N.L, N.act_kind, N.xs,
                                        critic ? nullptr : log_std, critic ? nullptr : noise, action, critic ? value_out : mean_out, nullptr, nullptr, 0, F);
}

// ---------------------------------------------------------------------------------------------------------------- forecast
// The ego_forecast policy step (egp_policy_desc.cell): the state goes through one step of the state LSTM
// (models/rnn.py:29-36 in step mode, as models/video_forecast_net.py:88-93 calls it) before it joins the video context:
//   pre = [W_ih | W_hh] [s | h] + (b_ih + b_hh);  c' = sigmoid(f) c + sigmoid(i) tanh(g);  h' = sigmoid(o) tanh(c');  x = [ctx | h']
// The gate pre-activations are layer 0 of the same pass machinery (L.wp[0]: the cell, input [s | h] in `cur`, 4 Hs outputs with
// the four gates of a unit in adjacent columns 4 u .. 4 u + 3, so a pass of POL_GC x 64 columns holds 80 whole units and the gate
// epilogue is one 16-byte LDS read per wave partial); its epilogue writes h' behind the context columns that the prologue has
// gathered into `nxt` -- the MLP's input -- and h' / c' back to the caller's rows. Layers 1 .. L.n - 1 are the MLP and the head.
// In place: a workgroup's h / c rows are read in the prologue (into LDS) and written in layer 0's epilogue, behind barriers;
// no workgroup touches another's rows, and rows >= n are neither read nor written.
// FILTER (the descriptor's filter block): the state columns are the observations of (qpos, qvel) pushed through the filter's apply
// pass on their way into `cur` (see PolFilter) -- k_zf_apply's two phases in its plain form: every workgroup merges the tile
// partials into the running statistics for itself (F.n_tiles == 0: the statistics as they stand, the frozen filter of an
// evaluation), one column per thread and round, then normalises its rows element by element. `state` is unused then.
template <int R, int NW, int PF, bool FILTER>
__device__ __forceinline__ void forecast_body(const float *__restrict__ ctx_rows, long ctx_row_stride, int ctx_dim,
                                              const long long *__restrict__ t_idx, const double *__restrict__ state, int state_dim,
                                              float *h_io, float *c_io, long hc_stride, int hs, int n,
                                              const PolLayers &L, int act_kind, int xs, const float *__restrict__ log_std,
                                              const float *__restrict__ noise, double *__restrict__ action, float *__restrict__ mean_out,
                                              const PolFilter &F) {
    constexpr int T = NW * 64;
    extern __shared__ __attribute__((aligned(16))) float s_f[];     // see PolCarve; the tail: c[R][hs], then the filter's mean, 1 / std
    const int out_last = L.out_dim[L.n - 1];
    const PolCarve lds = pol_carve<R, NW>(xs, L.sum_out4, out_last, R * hs, FILTER ? 2 * state_dim : 0);
    float *cur = s_f, *nxt = s_f + lds.nxt, *part = s_f + lds.part;
    float *s_bias = s_f + lds.bias, *s_sd = s_f + lds.sd, *s_noise = s_f + lds.noise, *s_c = s_f + lds.tail;
    double *s_ms = reinterpret_cast<double *>(s_f + lds.ms);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = blockIdx.x * R;
    const int in_c = state_dim + hs, in_cp = (in_c + 3) & ~3;        // the cell's input [s | h]
    const int in_m = ctx_dim + hs, in_mp = (in_m + 3) & ~3;          // the MLP's input [ctx | h']

    // the rows' context-row indices first: index -> context row is the longest dependent chain of the prologue
    long tix[R];
#pragma unroll
    for (int r = 0; r < R; ++r) tix[r] = ctx_dim > 0 ? (long)t_idx[min(r0 + r, n - 1)] : 0;
    // L2 warm-up over the packed weights (cell + MLP in one range)
    float warm[POL_WARM];
    pol_warm_request<T>(L, tid, warm);
    // the cell's own first blocks
    PolStage<PF> st;
    pol_preload_pass<NW, PF>(st, L, 0, 0, wave, lane);
    if constexpr (FILTER) {         // k_zf_apply's first phase: the merged statistics, every workgroup for itself
        const int dim = state_dim;
        for (int c = tid; c < dim; c += T) {
            double cnt, mean, S;
            egp::zf_merge_column(dim, F.n_tiles, F.ws, F.st_in, c, cnt, mean, S);
            if (blockIdx.x == 0 && F.st_out) {
                F.st_out[1 + c] = mean;
                F.st_out[1 + dim + c] = S;
                if (c == 0) F.st_out[0] = cnt;
            }
            const double var = cnt > 1.0 ? S / (cnt - 1.0) : mean * mean;
            s_ms[c] = mean;
            s_ms[dim + c] = 1.0 / (sqrt(var) + 1e-8);
        }
        __syncthreads();
    }
    // inputs: cur = [s | h | 0], nxt = [ctx | (h' later) | 0], s_c = c; rows >= n are zeros
    for (int k = tid; k < in_cp; k += T) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = r0 + r;
            float v = 0.0f;
            if (row < n && k < in_c) {
                if (k >= state_dim) {
                    v = h_io[(long)row * hc_stride + (k - state_dim)];
                } else if constexpr (FILTER) {        // k_zf_apply's second phase for this element
                    double x = ((double)F.src.at(row, k) - s_ms[k]) * s_ms[state_dim + k];
                    if (F.clip > 0.0) x = fmin(fmax(x, -F.clip), F.clip);
                    const long e = (long)row * state_dim + k;
                    F.y[e] = x;
                    if (F.y2) F.y2[e] = x;
                    v = (float)x;
                } else {
                    v = (float)state[(long)row * state_dim + k];
                }
            }
            cur[r * xs + k] = v;
        }
    }
    for (int k = tid; k < hs; k += T) {
#pragma unroll
        for (int r = 0; r < R; ++r) s_c[r * hs + k] = r0 + r < n ? c_io[(long)(r0 + r) * hc_stride + k] : 0.0f;
    }
    for (int k = tid; k < in_mp; k += T) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = r0 + r;
            nxt[r * xs + k] = (row < n && k < ctx_dim) ? ctx_rows[(long)row * ctx_row_stride + tix[r] * ctx_dim + k] : 0.0f;
        }
    }
    // the small operands of the epilogues: every layer's bias | exp(log_std) | the rows' noise
    {
        int off = 0;
        for (int l = 0; l < L.n; ++l) {
            const int o = L.out_dim[l];
            for (int j = tid; j < o; j += T) s_bias[off + j] = L.bias[l][j];
            off += (o + 3) & ~3;
        }
        if (noise) {
            for (int j = tid; j < out_last; j += T) s_sd[j] = expf(log_std[j]);
            for (int e = tid; e < R * out_last; e += T) {
                const int r = e / out_last;
                s_noise[e] = r0 + r < n ? noise[(long)(r0 + r) * out_last + (e - r * out_last)] : 0.0f;
            }
        }
    }
    __syncthreads();
    pol_warm_sink(warm);

    pol_layers<R, NW, PF, true>(cur, nxt, part, s_bias, s_sd, s_noise, st, pol_split<NW>(L.in_dim[0], wave), L, act_kind, xs, r0, n, wave,
                                noise, action, mean_out, PolCell{s_c, h_io, c_io, hc_stride, hs, ctx_dim});
}

template <int R, int PF, bool FILTER>
__global__ __launch_bounds__(256) void k_policy_forecast_w4(const float *__restrict__ ctx_rows, long ctx_row_stride, int ctx_dim,
                                                            const long long *__restrict__ t_idx, const double *__restrict__ state,
                                                            int state_dim, float *h_io, float *c_io, long hc_stride, int hs, int n,
                                                            PolLayers L, int act_kind, int xs, const float *__restrict__ log_std,
                                                            const float *__restrict__ noise, double *__restrict__ action,
                                                            float *__restrict__ mean_out, PolFilter F) {
    forecast_body<R, 4, PF, FILTER>(ctx_rows, ctx_row_stride, ctx_dim, t_idx, state, state_dim, h_io, c_io, hc_stride, hs, n, L, act_kind, xs,
                                    log_std, noise, action, mean_out, F);
}

}  // namespace

#ifdef EGP_POLICY_TRACE
extern "C" int egp_policy_trace_read(long long *out64) {
    return hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_pol_trace), sizeof(long long) * 64) == hipSuccess ? 0 : -1;
}
#endif

// Packed form of an nn.Linear weight for the policy step: egp_mlp_pack_floats(in, out) floats.
extern "C" int64_t egp_mlp_pack_floats(int32_t in_dim, int32_t out_dim) {
    if (in_dim <= 0 || out_dim <= 0) return 0;
    return (int64_t)((out_dim + 63) / 64) * ((in_dim + 3) / 4) * 256;
}

extern "C" int egp_mlp_pack_f32(const float *weight, int64_t ldw, int32_t in_dim, int32_t out_dim, float *packed, void *stream) {
    EGP_REQUIRE(weight && packed && in_dim > 0 && out_dim > 0 && ldw >= in_dim, "bad weight");
    const long total = (long)egp_mlp_pack_floats(in_dim, out_dim);
    const int threads = 256;
    const long blocks = (total + threads - 1) / threads;
    k_mlp_pack<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(threads), 0, (hipStream_t)stream>>>(weight, (long)ldw, in_dim, out_dim, packed, total);
    return after_launch("k_mlp_pack");
}

// The kernels' layer table from `front` (optional: the forecast step's cell) and layers[0 .. n_layers), validated. `in0`: width of
// the MLP's input, `chain_msg`: the caller's wording for a break in the dims chain. *kmax: the widest activation row.
static int pol_layer_table(const egp_mlp_layer *front, const egp_mlp_layer *layers, int n_layers, int in0, const char *chain_msg, PolLayers &L,
                           int *kmax) {
    L.n = 0; L.sum_out4 = 0;
    long lines = 0;
    bool contiguous = true;
    const float *follow = nullptr;                    // where the next layer's packed weights start if the buffers follow each other
    auto append = [&](const egp_mlp_layer &y) {
        L.wp[L.n] = y.wt; L.bias[L.n] = y.bias; L.in_dim[L.n] = y.in_dim; L.out_dim[L.n] = y.out_dim;
        ++L.n;
        L.sum_out4 += (y.out_dim + 3) & ~3;
        const long floats = egp_mlp_pack_floats(y.in_dim, y.out_dim);
        if (follow && y.wt != follow) contiguous = false;
        follow = y.wt + floats;
        lines += floats / 32;
    };
    if (front) append(*front);                        // (checked by the caller, with messages of its own)
    int prev = in0;
    *kmax = front && front->in_dim > in0 ? front->in_dim : in0;
    for (int l = 0; l < n_layers; ++l) {
        EGP_REQUIRE(layers[l].wt && layers[l].bias, "NULL layer");
        EGP_REQUIRE(((uintptr_t)layers[l].wt & 15) == 0, "packed weights must be 16-byte aligned");
        EGP_REQUIRE(layers[l].in_dim == prev && layers[l].out_dim > 0, chain_msg);
        append(layers[l]);
        prev = layers[l].out_dim;
        if (prev > *kmax) *kmax = prev;
    }
    EGP_REQUIRE(*kmax <= 2048, "layer wider than 2048");
    L.warm_lines = contiguous && lines < (1l << 30) ? (int)lines : 0;
    return EGP_OK;
}

// Activation row stride and dynamic LDS bytes of a launch: PolCarve's ranges, the kernel's own tail included (see pol_carve).
static int pol_lds(const PolLayers &L, int kmax, int cell_floats, int ms_doubles, int *xs, size_t *lds) {
    *xs = ((kmax + 31) & ~31) + 4;                    // rows 0..3 of a broadcast read sit on different banks
    *lds = (size_t)pol_carve<POL_R, POL_NW>(*xs, L.sum_out4, L.out_dim[L.n - 1], cell_floats, ms_doubles).end * sizeof(float);
    EGP_REQUIRE(*lds <= 150 * 1024, "layers too wide for the LDS tile");
    return EGP_OK;
}

// The PolFilter of a descriptor's filter block (zf_in != NULL). `need_out`: the kernel stores to zf_out without a null check (every
// step but the forecast one). Frozen statistics (zf_workspace == NULL): no tiles, and ws = zf_in -- the plain step's wave merge
// loads tile 0 unconditionally and discards it (`zf_in` has a tile partial's layout); zf_merge_column never reads ws then.
static int pol_filter(const egp_policy_desc *d, bool need_out, PolFilter &f) {
    EGP_REQUIRE(d->ctx && d->qpos && d->qvel && d->y && (d->zf_out || !need_out) && d->zf_in != d->zf_out,
                "NULL pointer / zf_out must differ from zf_in");
    EGP_REQUIRE(!d->zf_workspace || (d->zf_out && d->n <= 64 * egp::ZF_FUSED_TILES),
                "merged statistics: zf_out is required and at most egp_obs_zfilter_split_max_rows() rows");
    const auto &dm = d->ctx->dm;
    EGP_REQUIRE(!dm.obs_phase || d->phase_t, "the model has obs_phase: phase_t (the rows' cur_t) is required");
    int rpt, nt = 0;
    if (d->zf_workspace) egp::zf_tiling(d->n, &rpt, &nt);
    f.src = egp::ZfSrc<double>{nullptr, d->qpos, d->qvel, dm.nq, dm.nv, dm.obs_dim, egp::obs_opt_of(dm), d->phase_t};
    f.st_in = d->zf_in; f.st_out = d->zf_out; f.ws = d->zf_workspace ? (const double *)d->zf_workspace : d->zf_in; f.n_tiles = nt;
    f.clip = d->clip; f.y = d->y; f.y2 = d->y2;
    return EGP_OK;
}

// Every form of the policy step (include/egopose_hip.h: egp_policy_desc): validated once, then one launch of the plain kernel, of
// the forecast kernel (d->cell: one step of the state LSTM cell in front, see forecast_body) or of the actor + critic kernel
// (d->vlayers, k_policy_value_w4), each with the filter's apply pass in front (d->zf_in, see PolFilter) or without.
extern "C" int egp_policy_step_f32(const egp_policy_desc *d, void *stream) {
    EGP_REQUIRE(d, "desc is NULL");
    EGP_REQUIRE(d->n >= 0, "n < 0");
    EGP_REQUIRE(d->stage_bytes >= 0 && d->stage_bytes % 4 == 0 && d->stage_bytes < (1ll << 31) && (d->stage_bytes == 0 || (d->stage_src && d->stage_dst)),
                "bad staging slab");
    if (d->n == 0) return EGP_OK;
    const bool cell = d->cell, both = d->vlayers, flt = d->zf_in;
    EGP_REQUIRE(!cell || !both, "cell with vlayers: no kernel runs the LSTM cell and the critic together");
    EGP_REQUIRE(d->stage_bytes == 0 || (!cell && !both), "a staging slab rides in the plain step only (no cell, no vlayers)");
    EGP_REQUIRE(!both || !d->zf_workspace, "the actor + critic step normalises with frozen statistics only (zf_workspace == NULL)");
    PolFilter F{};
    if (flt)
        if (int rc = pol_filter(d, !cell, F)) return rc;
    const int n = d->n, ctx_dim = d->ctx_dim, state_dim = flt ? d->ctx->dm.obs_dim : d->state_dim;
    EGP_REQUIRE((d->state || flt) && d->layers && d->action && (cell || (d->ctx_rows && d->t_idx)) && (!both || (d->vctx_rows && d->value_out)), "NULL pointer");
    EGP_REQUIRE(!cell || (d->h && d->c && d->h != d->c), "NULL pointer (or h == c)");
    EGP_REQUIRE(!cell || (ctx_dim >= 0 && (ctx_dim == 0 || (d->ctx_rows && d->t_idx))), "bad context");
    EGP_REQUIRE(!d->noise || d->log_std, "noise needs log_std");
    EGP_REQUIRE(d->n_layers >= 1 && d->n_layers + (cell ? 1 : 0) <= POL_MAX_LAYERS,
                cell ? "1..7 layers (hidden layers + output layer) behind the cell" : "1..8 layers (hidden layers + output layer)");
    EGP_REQUIRE(d->activation >= 0 && d->activation <= 2, "activation: 0 tanh, 1 relu, 2 sigmoid");
    int hs = 0;
    if (cell) {
        const egp_mlp_layer *cl = d->cell;
        EGP_REQUIRE(cl->wt && cl->bias && ((uintptr_t)cl->wt & 15) == 0, "cell: NULL or misaligned packed weights");
        EGP_REQUIRE(cl->out_dim >= 4 && cl->out_dim % 4 == 0 && cl->out_dim <= 2048, "cell: out_dim = 4 x hidden size, at most 2048");
        hs = cl->out_dim / 4;
        EGP_REQUIRE(state_dim >= 1 && cl->in_dim == state_dim + hs && cl->in_dim <= 2048, "cell: in_dim = state_dim + hidden size, at most 2048");
        EGP_REQUIRE(d->hc_row_stride >= hs, "h / c row stride below the hidden size");
    } else {
        EGP_REQUIRE(ctx_dim >= 0 && state_dim >= 0 && ctx_dim + state_dim > 0, "bad input dims");
    }
    PolLayers L;
    int kmax, xs;
    size_t lds;
    if (int rc = pol_layer_table(d->cell, d->layers, d->n_layers, ctx_dim + (cell ? hs : state_dim),
                                 cell ? "layer dims do not chain (first layer: ctx_dim + hidden size)"
                                      : both ? "policy layer dims do not chain" : "layer dims do not chain", L, &kmax)) return rc;
    // the tail: the cell's c rows, and with the filter its merged mean | 1 / std (behind the pad float)
    const int ms = flt ? 2 * state_dim : 0;
    if (int rc = pol_lds(L, kmax, POL_R * hs, ms, &xs, &lds)) return rc;
    const dim3 block(POL_NW * 64);
    dim3 grid((n + POL_R - 1) / POL_R);
    const long long *t_idx = (const long long *)d->t_idx;
#define POL_GO(KERNEL, ...) do {                                                                                        \
        if (flt) KERNEL<POL_R, POL_PF, true><<<grid, block, lds, (hipStream_t)stream>>>(__VA_ARGS__);                    \
        else KERNEL<POL_R, POL_PF, false><<<grid, block, lds, (hipStream_t)stream>>>(__VA_ARGS__);                       \
    } while (0)
    if (!cell && !both) {
        POL_GO(k_policy_gaussian_w4, d->ctx_rows, (long)d->ctx_row_stride, ctx_dim, t_idx, d->state, state_dim, n, L, d->activation, xs, d->log_std,
               d->noise, d->action, d->mean_out, d->stage_bytes ? (const unsigned *)d->stage_src : nullptr, (unsigned *)d->stage_dst,
               (int)(d->stage_bytes / 4), F);
        return after_launch("k_policy_gaussian");
    }
    if (cell) {
        POL_GO(k_policy_forecast_w4, d->ctx_rows, (long)d->ctx_row_stride, ctx_dim, t_idx, d->state, state_dim, d->h, d->c, (long)d->hc_row_stride, hs, n,
               L, d->activation, xs, d->log_std, d->noise, d->action, d->mean_out, F);
        return after_launch("k_policy_forecast");
    }
    // the critic's own layer table and carve-up; the launch's dynamic LDS is the larger of the two
    EGP_REQUIRE(d->n_vlayers >= 1 && d->n_vlayers <= POL_MAX_LAYERS, "1..8 layers per net (hidden layers + output layer)");
    EGP_REQUIRE(d->vactivation >= 0 && d->vactivation <= 2, "activation: 0 tanh, 1 relu, 2 sigmoid");
    EGP_REQUIRE(d->vctx_dim >= 0 && d->ctx_row_stride >= 0 && d->vctx_row_stride >= 0, "bad context dims");
    PolNets P{{{d->ctx_rows, (long)d->ctx_row_stride, ctx_dim, d->activation, xs, L},
               {d->vctx_rows, (long)d->vctx_row_stride, d->vctx_dim, d->vactivation, 0, {}}}};
    PolNet &V = P.net[1];
    size_t lds_v;
    if (int rc = pol_layer_table(nullptr, d->vlayers, d->n_vlayers, d->vctx_dim + state_dim, "value layer dims do not chain", V.L, &kmax)) return rc;
    if (int rc = pol_lds(V.L, kmax, 0, ms, &V.xs, &lds_v)) return rc;
    EGP_REQUIRE(d->vlayers[d->n_vlayers - 1].out_dim == 1, "the value net's last layer is the value head (out_dim 1)");
    if (lds_v > lds) lds = lds_v;
    grid.y = 2;
    POL_GO(k_policy_value_w4, P, t_idx, d->state, state_dim, n, d->log_std, d->noise, d->action, d->mean_out, d->value_out, F);
#undef POL_GO
    return after_launch("k_policy_value");
}
