// K3 (observations), K4 (body quaternions), the batched quaternion operations (k_quat_op) and K6 (the running filter), with their
// C-ABI entry points egp_obs_* / egp_body_quat_* / egp_quat_op_* / egp_zfilter_* / egp_obs_zfilter_* declared in
// include/egopose_hip.h. K6 reads the observations of the drained state through ZfSrc (egp_filter_dev.hpp), so it lives with K3.
//
// Every per-env array is env-major and row-contiguous (qpos[n][nq], qvel[n][nv], obs[n][obs_dim]); consecutive lanes touch
// consecutive addresses of one row (or of adjacent rows).
//   K3 k_obs / k_obs_rows   one thread per output element / a workgroup per 64 rows (large batches).
//   K4 k_body_quat          one thread per body.
//   K6 k_zf_partial         per-tile (count, mean, M2) partials; k_zf_merge: Chan merge of many tiles; k_zf_apply: normalise
//                           (and merge a few tiles itself).
#include <hip/hip_runtime.h>
#include <math.h>

#include "egp_internal.hpp"
#include "egp_quat.hpp"
#include "egp_filter_dev.hpp"

namespace egp {

// ============================================================================================ K4
// get_body_quat (ego_pose/envs/humanoid_v1.py:113-125)
template <typename T>
__global__ __launch_bounds__(256) void k_body_quat(DevModel m, const T *__restrict__ qpos, int n,
                                                   T *__restrict__ bquat) {
    __shared__ int s_start[EGP_MAX_BODY], s_ndof[EGP_MAX_BODY];
    if (threadIdx.x < m.nbody) {
        s_start[threadIdx.x] = m.body_qpos_start[threadIdx.x];
        s_ndof[threadIdx.x] = m.body_ndof[threadIdx.x];
    }
    __syncthreads();
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)n * m.nbody) return;
    const int env = gid / m.nbody, b = gid % m.nbody;
    const T *q = qpos + (long)env * m.nq;
    Q4<T> o;
    if (b == 0) {
        o.w = q[3]; o.x = q[4]; o.y = q[5]; o.z = q[6];
    } else {
        const int s = s_start[b], nd = s_ndof[b];
        const T e0 = nd > 0 ? q[s] : T(0), e1 = nd > 1 ? q[s + 1] : T(0), e2 = nd > 2 ? q[s + 2] : T(0);
        o = q_from_euler_sxyz<T>(e0, e1, e2);
    }
    T *dst = bquat + gid * 4;
    dst[0] = o.w; dst[1] = o.x; dst[2] = o.y; dst[3] = o.z;
}

// ============================================================================================ K3
// (ObsOpt, obs_element: egp_filter_dev.hpp)

template <typename T>
__global__ __launch_bounds__(256) void k_obs(DevModel m, const T *__restrict__ qpos, const T *__restrict__ qvel,
                                             const int *__restrict__ phase_t, int n, T *__restrict__ obs) {
    const int od = m.obs_dim;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)n * od) return;
    const int env = gid / od, c = gid % od;
    obs[gid] = obs_element<T>(qpos + (long)env * m.nq, qvel + (long)env * m.nv, obs_opt_of(m), c, m.obs_phase ? phase_t[env] : 0);
}

// Large batches (the HBM-resident form): with one thread per element the wave that holds a row's root quaternion columns pays the
// whole de-heading (two float64 divisions, a square root) and the one with the root velocity columns the rotation -- ~600 cycles
// of divergent float64 work per wave for 1 KiB of traffic: 65 536 rows took 47 us at 32 % of the HBM roofline, vector-ALU bound (now 23 us, 65 %; 262 144 rows, beyond the 256 MB cache: 52 %).
// Here a workgroup takes 64 rows. First the columns that need arithmetic (heading, de-headed quaternion, root velocity, phase:
// at most 9): one wave per column, one lane per row, obs_element itself (same bits) into LDS -- every lane of the wave works.
// Then the rows stream through: 128 threads per row, 8-byte loads and stores of consecutive columns, the special ones from LDS.
constexpr int OBS_ROWS = 64;
template <typename T>
__global__ __launch_bounds__(256) void k_obs_rows(DevModel m, const T *__restrict__ qpos, const T *__restrict__ qvel,
                                                  const int *__restrict__ phase_t, int n, T *__restrict__ obs) {
    __shared__ T s_spec[9][OBS_ROWS];
    const ObsOpt o = obs_opt_of(m);
    const int od = m.obs_dim, h = o.heading ? 1 : 0;
    const int n_vel = o.vel == 0 ? o.nv : (o.vel == 1 ? 6 : 0);
    // special column s -> its index in the row (-1: not present)
    auto spec_col = [&](int s) {
        if (s == 0) return o.heading ? 0 : -1;
        if (s <= 4) return o.keep ? -1 : h + s;
        if (s <= 7) return n_vel >= 3 ? h + o.np + (s - 5) : -1;
        return o.phase ? h + o.np + n_vel : -1;
    };
    const long r0 = (long)blockIdx.x * OBS_ROWS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s = wave; s < 9; s += 4) {                       // (wave-uniform: one column per wave and round)
        const int c = spec_col(s);
        if (c < 0) continue;
        const long r = min(r0 + lane, (long)n - 1);
        s_spec[s][lane] = obs_element<T>(qpos + r * m.nq, qvel + r * m.nv, o, c, o.phase ? phase_t[r] : 0);
    }
    __syncthreads();
    const int c = threadIdx.x & 127, half = threadIdx.x >> 7;
    if (c >= od) return;
    int sp = -1;
#pragma unroll
    for (int s = 0; s < 9; ++s) sp = spec_col(s) == c ? s : sp;
    const int cc = c - h;
    const bool from_q = cc < o.np;
    const int src = from_q ? cc + 2 : cc - o.np;             // (unused for special columns)
#pragma unroll 4
    for (int e = half; e < OBS_ROWS; e += 2) {
        const long r = r0 + e;
        if (r >= n) break;
        T v;
        if (sp >= 0) v = s_spec[sp][e];
        else v = from_q ? qpos[r * m.nq + src] : qvel[r * m.nv + src];
        obs[r * od + c] = v;
    }
}

// ============================================================================================ K6
// RunningStat / ZFilter (utils/zfilter.py:7-67), batched.
// partial layout per tile p: ws[p*(1+2*dim)] = count, then mean[dim], then M2[dim]  (float64)
// (ZfSrc, zf_merge_column: egp_filter_dev.hpp)

// tile statistics: a workgroup is G = blockDim / 128 row groups x 128 columns. A thread takes its group's share of the
// tile's rows in chunks of 8 (8 independent loads in flight, then an exact two-pass mean / M2 of the chunk, Chan-merged
// into the thread's running statistics); the groups' results meet in LDS and group 0 merges them in row order. With
// 1 024 threads and 64-row tiles every thread has ONE round of loads and a 512-env tick leaves 8 partials -- few
// enough for k_zf_apply to merge them itself (one launch and its memory round trips less on the tick's critical path).
// ROWS: the source is the drained state (src.x == nullptr) and takes ZfSrc's rows form; else src.at() per element
// (two instantiations, two kernels: one function with both paths needs more than the 128 registers of a 1 024-thread workgroup)
template <typename T, bool ROWS>
__device__ __forceinline__ void zf_partial_body(const ZfSrc<T> &src, const int *__restrict__ active, int n, int dim,
                                                int rows_per_tile, double *__restrict__ ws, int p) {
    __shared__ double s_mean[8][128], s_m2[8][128], s_cnt[8];
    const int G = blockDim.x >> 7, g = threadIdx.x >> 7, lc = threadIdx.x & 127;
    const int r0 = p * rows_per_tile, r1 = min(n, r0 + rows_per_tile);
    // row group g takes the tile's 8-row chunks g, g + G, g + 2 G, ...: at any time the workgroup reads 8 G consecutive rows (with a
    // contiguous share per group -- 256 rows each in a 2 048-row tile -- a workgroup kept 16 streams a quarter of a megabyte apart
    // going; 64-row tiles, the rollout's, have one chunk per group either way: same partials bit for bit)
    const int g0 = r0 + 8 * g, g1 = r1, g_step = 8 * G;
    double *out = ws + (long)p * (1 + 2 * dim);
    for (int cb = 0; cb < dim; cb += 128) {
        const int c = cb + lc;
        double cnt = 0.0, mean = 0.0, m2 = 0.0;
        // (rows of the drained state: every load of the chunk's 8 rows in flight at once and the rows' quaternion work shared
        //  out over the wave's lanes -- ZfSrc::load_rows / finish_rows, wave-uniform here: a wave is 64 columns of ONE row group;
        //  with src.at() per row the chunk was 8 dependent rounds of flag -> branch -> loads -> arithmetic)
        if (ROWS || c < dim)
            for (int rb = g0; rb < g1; rb += g_step) {
                double v[8];
                unsigned on = 0;          // bit i: row rb + i counts
                int k = 0;
                if constexpr (ROWS) {
                    // (two half-chunks of 4 rows: the 8-row form needs more than the 128 registers a thread of this workgroup has)
                    const int cl = min(c, dim - 1);
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        typename ZfSrc<T>::template Rows<4> P = src.template load_rows<4>(rb + 4 * h, n, cl);
                        int flag[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) flag[i] = 1;
                        if (active) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) flag[i] = active[min(rb + 4 * h + i, n - 1)];
                        }
                        src.template finish_rows<4>(P, rb + 4 * h, n, cl);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const bool o_ = rb + 4 * h + i < g1 && flag[i] && c < dim;
                            on |= (unsigned)o_ << (4 * h + i);
                            v[4 * h + i] = o_ ? (double)P.own[i] : 0.0;
                            k += o_;
                        }
                    }
                } else {
                    // (requesting the next chunk before this one's arithmetic was tried in round 6: the 1 024-thread workgroup's 128
                    //  registers do not hold it -- 305 -> 400 us at 1 M rows, 16 -> 34 us at 1 024)
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int r = rb + i;
                        const bool o_ = r < g1 && (!active || active[r]);
                        on |= (unsigned)o_ << i;
                        v[i] = o_ ? (double)src.at(r, c) : 0.0;
                        k += o_;
                    }
                }
                if (k == 0) continue;
                double sum = 0.0;
#pragma unroll
                for (int i = 0; i < 8; ++i) sum += v[i];
                const double mb = sum / k;
                double sb = 0.0;
#pragma unroll
                for (int i = 0; i < 8; ++i) sb += (on >> i) & 1 ? (v[i] - mb) * (v[i] - mb) : 0.0;
                if (cnt == 0.0) {
                    cnt = k; mean = mb; m2 = sb;
                } else {
                    const double tot = cnt + k, d = mb - mean;
                    m2 += sb + d * d * (cnt * k / tot);
                    mean += d * (k / tot);
                    cnt = tot;
                }
            }
        s_mean[g][lc] = mean;
        s_m2[g][lc] = m2;
        if (lc == 0 && cb == 0) s_cnt[g] = cnt;          // (the count is the same for every column)
        __syncthreads();
        if (g == 0 && c < dim) {
            double C = s_cnt[0], M = s_mean[0][lc], S = s_m2[0][lc];
            for (int j = 1; j < G; ++j) {
                const double nb = s_cnt[j];
                if (nb > 0.0) {
                    if (C == 0.0) {
                        C = nb; M = s_mean[j][lc]; S = s_m2[j][lc];
                    } else {
                        const double d = s_mean[j][lc] - M, tot = C + nb;
                        S = S + s_m2[j][lc] + d * d * (C * nb / tot);
                        M = M + d * (nb / tot);
                        C = tot;
                    }
                }
            }
            out[1 + c] = M;
            out[1 + dim + c] = S;
            if (c == 0) out[0] = C;
        }
        __syncthreads();
    }
}

template <typename T, bool ROWS>
__global__ __launch_bounds__(1024) void k_zf_partial(ZfSrc<T> src, const int *__restrict__ active, int n, int dim,
                                                    int rows_per_tile, double *__restrict__ ws) {
    zf_partial_body<T, ROWS>(src, active, n, dim, rows_per_tile, ws, blockIdx.x);
}
template <typename T>
static void launch_zf_partial(const ZfSrc<T> &src, const int *active, int n, int dim, int rpt, int nt, double *ws, hipStream_t stream) {
    if (src.x == nullptr)
        k_zf_partial<T, true><<<dim3(nt), dim3(1024), 0, stream>>>(src, active, n, dim, rpt, ws);
    else
        k_zf_partial<T, false><<<dim3(nt), dim3(1024), 0, stream>>>(src, active, n, dim, rpt, ws);
}

// one block: the merged state of a batch with many tiles (few tiles: k_zf_apply merges them itself). 8 tile groups x 128
// columns: group g merges its contiguous eighth of the tiles in order, then group 0 merges the eight results in order
// through LDS -- eight times fewer dependent rounds of loads than one pass over all tiles (90 -> 15 us for 512 tiles).
// Large batches (round 3): ONE block merging 512 partials took 31 of K6's 70 us at 65 536 rows. Now gridDim.x blocks each
// merge a contiguous share of the tiles into a partial record of their own (st_in == nullptr: block b writes record b of
// st_out, layout as ws) and the apply kernel merges those <= 16 records into the running state itself, as it does for small batches.
__global__ __launch_bounds__(1024) void k_zf_merge(int dim, int n_tiles_all, const double *__restrict__ ws_all,
                                                   const double *__restrict__ st_in, double *__restrict__ st_out_all) {
    __shared__ double s_n[8], s_mean[8][128], s_S[8][128];
    const int g = threadIdx.x >> 7, lc = threadIdx.x & 127;
    const int share = (n_tiles_all + gridDim.x - 1) / gridDim.x;
    const int t0 = blockIdx.x * share, n_tiles = max(0, min(n_tiles_all, t0 + share) - t0);
    const double *ws = ws_all + (long)t0 * (1 + 2 * dim);
    double *st_out = st_out_all + (st_in ? 0 : (long)blockIdx.x * (1 + 2 * dim));
    const int per = (n_tiles + 7) / 8, q0 = g * per, q1 = min(n_tiles, q0 + per);
    for (int cb = 0; cb < dim; cb += 128) {
        const int c = cb + lc;
        double cnt = 0.0, mean = 0.0, S = 0.0;
        if (c < dim && q0 < q1) {
            for (int qa = q0; qa < q1; qa += 8) {
                double nb[8], mb[8], Sb[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int q = qa + i;
                    const double *pp = ws + (long)(q < q1 ? q : q0) * (1 + 2 * dim);
                    nb[i] = q < q1 ? pp[0] : 0.0;
                    mb[i] = pp[1 + c];
                    Sb[i] = pp[1 + dim + c];
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (nb[i] > 0.0) {
                        if (cnt == 0.0) {
                            cnt = nb[i]; mean = mb[i]; S = Sb[i];
                        } else {
                            const double d = mb[i] - mean, tot = cnt + nb[i];
                            S = S + Sb[i] + d * d * (cnt * nb[i] / tot);
                            mean = mean + d * (nb[i] / tot);
                            cnt = tot;
                        }
                    }
                }
            }
        }
        s_mean[g][lc] = mean; s_S[g][lc] = S;
        if (lc == 0 && cb == 0) s_n[g] = cnt;            // (the count is the same for every column)
        __syncthreads();
        if (g == 0 && c < dim) {
            double C = st_in ? st_in[0] : 0.0, M = st_in ? st_in[1 + c] : 0.0, SS = st_in ? st_in[1 + dim + c] : 0.0;
            for (int j = 0; j < 8; ++j) {
                const double nb = s_n[j];
                if (nb > 0.0) {
                    if (C == 0.0) {
                        C = nb; M = s_mean[j][lc]; SS = s_S[j][lc];
                    } else {
                        const double d = s_mean[j][lc] - M, tot = C + nb;
                        SS = SS + s_S[j][lc] + d * d * (C * nb / tot);
                        M = M + d * (nb / tot);
                        C = tot;
                    }
                }
            }
            st_out[1 + c] = M;
            st_out[1 + dim + c] = SS;
            if (c == 0) st_out[0] = C;
        }
        __syncthreads();
    }
}

// y = clip((x - mean) / (std + 1e-8)) with the statistics in `st` (identity: raw copy)
template <typename T>
// `ws` != nullptr: `st` is the state BEFORE this batch and every block merges the batch's n_tiles partials into it for
// itself (same operations in the same order: identical in every block); block 0 writes the new state to st_out
__global__ __launch_bounds__(128) void k_zf_apply(ZfSrc<T> src, int n, int dim, int rows_per_block, const double *__restrict__ st,
                                                  double clip, T *__restrict__ y, T *__restrict__ y2,
                                                  const int *__restrict__ write_mask, int identity,
                                                  const double *__restrict__ ws, int n_tiles, double *__restrict__ st_out) {
    extern __shared__ double s_ms[];   // mean[dim], inv[dim]
    for (int c = threadIdx.x; c < dim; c += blockDim.x) {
        if (identity) { s_ms[c] = 0.0; s_ms[dim + c] = 1.0; continue; }
        double cnt, mean, S;
        if (ws) {
            zf_merge_column(dim, n_tiles, ws, st, c, cnt, mean, S);
            if (blockIdx.x == 0) {
                st_out[1 + c] = mean;
                st_out[1 + dim + c] = S;
                if (c == 0) st_out[0] = cnt;
            }
        } else {
            cnt = st[0]; mean = st[1 + c]; S = st[1 + dim + c];
        }
        const double var = cnt > 1.0 ? S / (cnt - 1.0) : mean * mean;
        s_ms[c] = mean;
        s_ms[dim + c] = 1.0 / (sqrt(var) + 1e-8);
    }
    __syncthreads();
    const int r0 = blockIdx.x * rows_per_block, r1 = min(n, r0 + rows_per_block);
    if (src.x == nullptr && dim <= (int)blockDim.x) {
        // rows of the drained state, one column per thread: ZfSrc's rows form (every load of 4 rows in flight at once, the rows'
        // quaternion work shared out over the wave's lanes) instead of one src.at() -- branch, loads, arithmetic -- per element
        const int c = min((int)threadIdx.x, dim - 1);
        const bool mine = (int)threadIdx.x < dim;
        const double mean = s_ms[c], inv = s_ms[dim + c];
        for (int rb = r0; rb < r1; rb += 4) {
            typename ZfSrc<T>::template Rows<4> P = src.template load_rows<4>(rb, n, c);
            int keep[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) keep[i] = 1;
            if (write_mask) {
#pragma unroll
                for (int i = 0; i < 4; ++i) keep[i] = write_mask[min(rb + i, n - 1)];
            }
            src.template finish_rows<4>(P, rb, n, c);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = rb + i;
                if (r < r1 && mine && keep[i]) {
                    double v = ((double)P.own[i] - mean) * inv;
                    if (clip > 0.0 && !identity) v = fmin(fmax(v, -clip), clip);
                    const long e = (long)r * dim + c;
                    y[e] = (T)v;
                    if (y2) y2[e] = (T)v;
                }
            }
        }
        return;
    }
    if (src.x != nullptr && dim <= (int)blockDim.x && !write_mask) {
        // a plain matrix, one column per thread, eight rows' loads in flight: no per-element division by `dim` (the flat loop below
        // spent 64-bit e / dim and e % dim on every element: 603 us over 1 M rows of 115 where this form takes ~400)
        const int c = threadIdx.x;
        if (c >= dim) return;
        const double mean = s_ms[c], inv = s_ms[dim + c];
        const bool clamp = clip > 0.0 && !identity;
        for (int rb = r0; rb < r1; rb += 8) {
            double v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = rb + i < r1 ? (double)src.x[(long)(rb + i) * dim + c] : 0.0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (rb + i >= r1) break;
                double w = (v[i] - mean) * inv;
                if (clamp) w = fmin(fmax(w, -clip), clip);
                const long e = (long)(rb + i) * dim + c;
                y[e] = (T)w;
                if (y2) y2[e] = (T)w;
            }
        }
        return;
    }
    const long e0 = (long)r0 * dim, e1 = (long)r1 * dim;
    for (long e = e0 + threadIdx.x; e < e1; e += blockDim.x) {
        const int c = e % dim;
        const long r = e / dim;
        if (write_mask && !write_mask[r]) continue;
        double v = ((double)src.at(r, c) - s_ms[c]) * s_ms[dim + c];
        if (clip > 0.0 && !identity) v = fmin(fmax(v, -clip), clip);
        y[e] = (T)v;
        if (y2) y2[e] = (T)v;
    }
}

}  // namespace egp

using namespace egp;

template <typename T>
static int launch_body_quat(egp_ctx *ctx, const T *qpos, int n, T *bquat, void *stream) {
    EGP_REQUIRE(ctx, "ctx is NULL");
    EGP_REQUIRE(n >= 0, "n < 0");
    if (n == 0) return EGP_OK;
    EGP_REQUIRE(qpos && bquat, "NULL pointer");
    const long total = (long)n * ctx->dm.nbody;
    k_body_quat<T><<<dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(ctx->dm, qpos, n, bquat);
    return after_launch("k_body_quat");
}

// ---------------------------------------------------------------------------------------------------------------
// a7: the quaternion algebra of egp_quat.hpp as a batched entry point of its own (one thread per row). The rollout
// kernels inline these functions; this launch exists so that callers (and the parity tests against the reference's
// utils/transformation.py / utils/math.py vectors) can reach each of them directly.
template <typename T>
__global__ __launch_bounds__(256) void k_quat_op(int op, const T *__restrict__ a, const T *__restrict__ b, int n, T *__restrict__ o) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    auto ldq = [](const T *p) { Q4<T> q; q.w = p[0]; q.x = p[1]; q.y = p[2]; q.z = p[3]; return q; };
    auto stq = [](T *p, const Q4<T> &q) { p[0] = q.w; p[1] = q.x; p[2] = q.y; p[3] = q.z; };
    switch (op) {
    case EGP_QUAT_MUL: stq(o + 4 * i, qmul(ldq(a + 4 * i), ldq(b + 4 * i))); break;
    case EGP_QUAT_INV: stq(o + 4 * i, qinv(ldq(a + 4 * i))); break;
    case EGP_QUAT_FROM_EULER_SXYZ: stq(o + 4 * i, q_from_euler_sxyz<T>(a[3 * i], a[3 * i + 1], a[3 * i + 2])); break;
    case EGP_QUAT_HEADING_Q: stq(o + 4 * i, heading_q(ldq(a + 4 * i))); break;
    case EGP_QUAT_DE_HEADING: stq(o + 4 * i, de_heading(ldq(a + 4 * i))); break;
    case EGP_QUAT_TRANSFORM_VEC_ROOT:
    case EGP_QUAT_TRANSFORM_VEC_HEADING: {
        Q4<T> q = ldq(b + 4 * i);
        if (op == EGP_QUAT_TRANSFORM_VEC_HEADING) q = heading_q(q);
        V3<T> v; v.x = a[3 * i]; v.y = a[3 * i + 1]; v.z = a[3 * i + 2];
        const V3<T> r = rotate_T(q, v);
        o[3 * i] = r.x; o[3 * i + 1] = r.y; o[3 * i + 2] = r.z;
        break;
    }
    case EGP_QUAT_ROTATION: {
        V3<T> ax; T an;
        rot_axis_angle(ldq(a + 4 * i), &ax, &an);
        o[4 * i] = ax.x; o[4 * i + 1] = ax.y; o[4 * i + 2] = ax.z; o[4 * i + 3] = an;
        break;
    }
    case EGP_QUAT_DIFF_HALF_ANGLE: o[i] = half_angle(qmul(ldq(a + 4 * i), qinv(ldq(b + 4 * i)))); break;
    default: break;
    }
}

template <typename T>
static int launch_quat_op(int op, const T *a, const T *b, int n, T *out, void *stream) {
    EGP_REQUIRE(op >= 0 && op < EGP_QUAT_N_OPS, "unknown quaternion op");
    EGP_REQUIRE(n >= 0, "n < 0");
    if (n == 0) return EGP_OK;
    const bool two = op == EGP_QUAT_MUL || op == EGP_QUAT_TRANSFORM_VEC_ROOT || op == EGP_QUAT_TRANSFORM_VEC_HEADING ||
                     op == EGP_QUAT_DIFF_HALF_ANGLE;
    EGP_REQUIRE(a && out && (b || !two), "NULL pointer");
    k_quat_op<T><<<dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(op, a, b, n, out);
    return after_launch("k_quat_op");
}

template <typename T>
static int launch_obs(egp_ctx *ctx, const T *qpos, const T *qvel, const int *phase_t, int n, T *obs, void *stream) {
    EGP_REQUIRE(ctx, "ctx is NULL");
    EGP_REQUIRE(n >= 0, "n < 0");
    if (n == 0) return EGP_OK;
    EGP_REQUIRE(qpos && qvel && obs, "NULL pointer");
    EGP_REQUIRE(!ctx->dm.obs_phase || phase_t, "the model has obs_phase: phase_t (the rows' cur_t) is required");
    const long total = (long)n * ctx->dm.obs_dim;
    if (n >= 32768 && ctx->dm.obs_dim <= 128) {        // whole rounds of the chip: the row-streaming form (k_obs_rows); below, launch-bound either way
        k_obs_rows<T><<<dim3((n + OBS_ROWS - 1) / OBS_ROWS), dim3(256), 0, (hipStream_t)stream>>>(ctx->dm, qpos, qvel, phase_t, n, obs);
        return after_launch("k_obs_rows");
    }
    k_obs<T><<<dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(ctx->dm, qpos, qvel, phase_t, n, obs);
    return after_launch("k_obs");
}

template <typename T>
static int launch_zfilter_src(const ZfSrc<T> &src, const int *active, int n, int dim, const double *st_in, double *st_out, int update,
                              double clip, T *y, T *y2, const int *write_mask, void *ws, void *stream) {
    const int identity = st_in == nullptr;
    EGP_REQUIRE(n >= 0 && dim > 0 && dim <= 4096, "bad n/dim");
    EGP_REQUIRE(n == 0 || y, "NULL output");
    EGP_REQUIRE(identity || !update || (st_out && ws && st_out != st_in), "update needs workspace and a distinct state_out");
    if (identity) update = 0;
    if (n == 0) {
        if (update) EGP_HIP_CHECK(hipMemcpyAsync(st_out, st_in, (1 + 2 * (size_t)dim) * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return EGP_OK;
    }
    int rpt, nt;
    zf_tiling(n, &rpt, &nt);
    // <= 16 tiles: the apply kernel merges them itself (2 launches). Up to 256 tiles: one block merges them into the new state
    // (a few rounds of loads). Beyond (>= 32 k rows): 16 blocks reduce the tiles to 16 records, which the apply kernel's
    // (16-row) blocks merge themselves -- the single block took 31 of K6's 70 us at 65 536 rows.
    const bool direct = update && nt <= ZF_FUSED_TILES;
    const bool two_level = update && nt > 256;
    const double *records = nullptr;                            // what the apply kernel merges into the running state, if anything
    int n_records = 0;
    if (update) {
        // (1 024 threads = one round of loads per thread: in the rollout 16.9 us per call against 20.1 with 512 and 33.6 with 256)
        launch_zf_partial<T>(src, active, n, dim, rpt, nt, (double *)ws, (hipStream_t)stream);
        if (direct) {
            records = (const double *)ws; n_records = nt;
        } else if (two_level) {
            double *lvl1 = (double *)ws + (size_t)nt * (1 + 2 * dim);            // behind the tiles in the workspace
            k_zf_merge<<<dim3(ZF_FUSED_TILES), dim3(1024), 0, (hipStream_t)stream>>>(dim, nt, (const double *)ws, nullptr, lvl1);
            records = lvl1; n_records = ZF_FUSED_TILES;
        } else {
            k_zf_merge<<<dim3(1), dim3(1024), 0, (hipStream_t)stream>>>(dim, nt, (const double *)ws, st_in, st_out);
        }
        int rc = after_launch("k_zf_partial/merge");
        if (rc != EGP_OK) return rc;
    }
    const int rows_per_block = direct ? 8 : (n <= 8192 ? 2 : 16);     // small batches: enough blocks to cover the latency
    k_zf_apply<T><<<dim3((n + rows_per_block - 1) / rows_per_block), dim3(128), 2 * dim * sizeof(double), (hipStream_t)stream>>>(
        src, n, dim, rows_per_block, update && !records ? st_out : st_in, clip, y, y2, write_mask, identity, records, n_records, st_out);
    return after_launch("k_zf_apply");
}

template <typename T>
static int launch_zfilter(const T *x, const int *active, int n, int dim, const double *st_in, double *st_out, int update,
                          double clip, T *y, void *ws, void *stream) {
    EGP_REQUIRE(st_in && (n == 0 || (x && y)), "NULL pointer");
    ZfSrc<T> src{x, nullptr, nullptr, 0, 0, dim, ObsOpt{0, 0, 0, 0, 0, 0}};
    return launch_zfilter_src<T>(src, active, n, dim, st_in, st_out, update, clip, y, nullptr, nullptr, ws, stream);
}

template <typename T>
static int launch_obs_zfilter(egp_ctx *ctx, const T *qpos, const T *qvel, const int *phase_t, const int *active, int n, const double *st_in, double *st_out,
                              double clip, T *y, T *y2, int write_only_active, void *ws, void *stream) {
    EGP_REQUIRE(ctx, "ctx is NULL");
    EGP_REQUIRE(n == 0 || (qpos && qvel), "NULL pointer");
    EGP_REQUIRE(!write_only_active || active, "write_only_active needs the active mask");
    EGP_REQUIRE(n == 0 || !ctx->dm.obs_phase || phase_t, "the model has obs_phase: phase_t (the rows' cur_t) is required");
    const int dim = ctx->dm.obs_dim;
    ZfSrc<T> src{nullptr, qpos, qvel, ctx->dm.nq, ctx->dm.nv, dim, obs_opt_of(ctx->dm), phase_t};
    return launch_zfilter_src<T>(src, active, n, dim, st_in, st_out, 1, clip, y, y2, write_only_active ? active : nullptr, ws, stream);
}

extern "C" {

int egp_body_quat_f64(egp_ctx *c, const double *q, int32_t n, double *o, void *s) { return launch_body_quat<double>(c, q, n, o, s); }
int egp_body_quat_f32(egp_ctx *c, const float *q, int32_t n, float *o, void *s) { return launch_body_quat<float>(c, q, n, o, s); }
int egp_quat_op_f64(int32_t op, const double *a, const double *b, int32_t n, double *o, void *s) { return launch_quat_op<double>(op, a, b, n, o, s); }
int egp_quat_op_f32(int32_t op, const float *a, const float *b, int32_t n, float *o, void *s) { return launch_quat_op<float>(op, a, b, n, o, s); }
int egp_obs_f64(egp_ctx *c, const double *q, const double *v, const int32_t *phase_t, int32_t n, double *o, void *s) { return launch_obs<double>(c, q, v, phase_t, n, o, s); }
int egp_obs_f32(egp_ctx *c, const float *q, const float *v, const int32_t *phase_t, int32_t n, float *o, void *s) { return launch_obs<float>(c, q, v, phase_t, n, o, s); }

int64_t egp_zfilter_workspace_bytes(int32_t n, int32_t dim) {
    int rpt, nt;
    zf_tiling(n > 0 ? n : 1, &rpt, &nt);
    return ((int64_t)nt + ZF_FUSED_TILES) * (1 + 2 * (int64_t)dim) * sizeof(double);      // the tiles + the level-1 records
}
int egp_zfilter_f64(const double *x, const int32_t *active, int32_t n, int32_t dim, const double *si, double *so,
                    int32_t update, double clip, double *y, void *ws, void *s) {
    return launch_zfilter<double>(x, active, n, dim, si, so, update, clip, y, ws, s);
}
int egp_zfilter_f32(const float *x, const int32_t *active, int32_t n, int32_t dim, const double *si, double *so,
                    int32_t update, double clip, float *y, void *ws, void *s) {
    return launch_zfilter<float>(x, active, n, dim, si, so, update, clip, y, ws, s);
}

/* K3+K6 fused: observations of the drained state (get_full_obs) pushed through the running filter in one call.
 *   active [n] (optional): rows that update the statistics; write_only_active: only those rows are written.
 *   state_in == NULL: no filter (raw observations). y2 (optional) receives a second copy of the output. */
int egp_obs_zfilter_f64(egp_ctx *c, const double *qpos, const double *qvel, const int32_t *phase_t, const int32_t *active, int32_t n, const double *si,
                        double *so, double clip, double *y, double *y2, int32_t write_only_active, void *ws, void *s) {
    return launch_obs_zfilter<double>(c, qpos, qvel, phase_t, active, n, si, so, clip, y, y2, write_only_active, ws, s);
}
int egp_obs_zfilter_f32(egp_ctx *c, const float *qpos, const float *qvel, const int32_t *phase_t, const int32_t *active, int32_t n, const double *si,
                        double *so, double clip, float *y, float *y2, int32_t write_only_active, void *ws, void *s) {
    return launch_obs_zfilter<float>(c, qpos, qvel, phase_t, active, n, si, so, clip, y, y2, write_only_active, ws, s);
}
// egp_obs_zfilter_f64 in two calls, for batches of at most egp_obs_zfilter_split_max_rows() rows (the apply pass merges the tile
// statistics itself there): _stats = the first launch, _apply = the second, same kernels with the same arguments. Whoever runs
// the apply pass may instead be the policy step of the next tick (egp_policy_step_f32 with the descriptor's filter block).
int32_t egp_obs_zfilter_split_max_rows(void) { return 64 * ZF_FUSED_TILES; }
int egp_obs_zfilter_stats_f64(egp_ctx *ctx, const double *qpos, const double *qvel, const int32_t *phase_t, const int32_t *active, int32_t n, void *ws, void *stream) {
    EGP_REQUIRE(ctx && ws, "NULL pointer");
    EGP_REQUIRE(n > 0 && n <= 64 * ZF_FUSED_TILES && qpos && qvel, "1 .. egp_obs_zfilter_split_max_rows() rows");
    EGP_REQUIRE(!ctx->dm.obs_phase || phase_t, "the model has obs_phase: phase_t (the rows' cur_t) is required");
    const int dim = ctx->dm.obs_dim;
    ZfSrc<double> src{nullptr, qpos, qvel, ctx->dm.nq, ctx->dm.nv, dim, obs_opt_of(ctx->dm), phase_t};
    int rpt, nt;
    zf_tiling(n, &rpt, &nt);
    launch_zf_partial<double>(src, active, n, dim, rpt, nt, (double *)ws, (hipStream_t)stream);
    return after_launch("k_zf_partial");
}
int egp_obs_zfilter_apply_f64(egp_ctx *ctx, const double *qpos, const double *qvel, const int32_t *phase_t, int32_t n, const double *st_in, double *st_out,
                              double clip, double *y, double *y2, void *ws, void *stream) {
    EGP_REQUIRE(ctx && ws && st_in && st_out && st_in != st_out && y, "NULL pointer / state_out must differ from state_in");
    EGP_REQUIRE(n > 0 && n <= 64 * ZF_FUSED_TILES && qpos && qvel, "1 .. egp_obs_zfilter_split_max_rows() rows");
    EGP_REQUIRE(!ctx->dm.obs_phase || phase_t, "the model has obs_phase: phase_t (the rows' cur_t) is required");
    const int dim = ctx->dm.obs_dim;
    ZfSrc<double> src{nullptr, qpos, qvel, ctx->dm.nq, ctx->dm.nv, dim, obs_opt_of(ctx->dm), phase_t};
    int rpt, nt;
    zf_tiling(n, &rpt, &nt);
    k_zf_apply<double><<<dim3((n + 7) / 8), dim3(128), 2 * dim * sizeof(double), (hipStream_t)stream>>>(
        src, n, dim, 8, st_in, clip, y, y2, nullptr, 0, (const double *)ws, nt, st_out);
    return after_launch("k_zf_apply");
}

}  // extern "C"
