// egp_update.hip -- the element-wise tail of a PPO epoch: both losses with their gradients w.r.t. the nets' outputs in one
// launch, and gradient-norm clip + Adam over flat parameter buffers in two.
//
//   k_ppo_loss   agents/agent_pg.py:19-26 (critic MSE), agents/agent_ppo.py:58-65 (clipped surrogate) over
//                core/distributions.py:6-25 / utils/math.py:14-17 (diagonal Gaussian log-density), plus what autograd would
//                send back to `values_pred` and `action_mean`
//   k_ppo_stats  the update monitor (no reference counterpart): KL estimators, clip fraction, ratio range, explained-variance moments
//                and non-finite rows of an epoch as one record of float64 raw sums, from k_ppo_loss's own row_logp
//   k_minibatch_plan / k_ppo_loss_mb   the mini-batch epochs (agents/agent_ppo.py:24-44): the epoch's shuffle as one gather of the
//                update's columns + per-window exploration-row counts, and k_ppo_loss for one window with data-independent shapes
//   k_sqnorm     torch.nn.utils.clip_grad_norm_'s total norm (agents/agent_ppo.py:53-56)
//   k_adam       torch.optim.Adam.step for every parameter group of both optimizers (agent_ppo.py:24-30)
//
// The loss and optimizer kernels are one pass over their operands (HBM-bound, a few MB): what they replace is ~45 launch-bound library kernels per
// epoch. Reductions are float64 in a fixed order: per-workgroup partials, summed in index order by a one-workgroup launch.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "egp_internal.hpp"

namespace {

constexpr int LOSS_BLOCK = 256;
constexpr int LOSS_GROUP = 16;                 // lanes per policy row
constexpr int LOSS_MAX_BLOCKS = 1024;
constexpr int LOSS_MAX_ACT = 256;              // action width limit (d_log_std accumulators per lane: act_dim / 16)

struct LossArgs {
    int n, n_pol, act_dim;
    const long long *rows;
    const float *pred, *returns, *mean, *actions, *log_std, *adv;
    long ld_mean, ld_act, ld_dmean;
    float *fixed_logp;
    int write_fixed;
    double clip_eps, inv_n_val, inv_n_exp;
    float *d_pred, *d_mean, *d_log_std;
    double *losses;
    double *part;              // [gridDim.x][2 + act_dim]: value-loss sum, surrogate sum, d_log_std sums
    unsigned *counter;
    int pol_blocks;            // blocks [0, pol_blocks) take policy rows, the rest value elements
};

__device__ __forceinline__ double block_sum(double v, double *s_red) {
    // fixed tree over the 256 threads: lane butterflies inside a wave, then the four wave sums in order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
    return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// ---- the per-row arithmetic of the surrogate, shared by k_ppo_loss and k_ppo_loss_mb. A 16-lane group owns a row; lane l
// takes action dimensions l, l + 16, ... (`ok` = the group has a row: lanes without one run along for the shuffles).
constexpr int LOSS_MAXD = LOSS_MAX_ACT / LOSS_GROUP;

// log-density of the row under N(mean, exp(log_std)), summed over the group; leaves z_j = (a_j - mean_j) / std_j and 1 / std_j
__device__ __forceinline__ float row_logp(bool ok, int l, int act_dim, const float *__restrict__ act_row, const float *__restrict__ mean_row,
                                          const float *__restrict__ log_std, float (&z)[LOSS_MAXD], float (&istd)[LOSS_MAXD]) {
    const float half_log_2pi = 0.91893853320467274178f;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < LOSS_MAXD; ++k) {
        const int j = l + LOSS_GROUP * k;
        z[k] = 0.f; istd[k] = 0.f;
        if (ok && j < act_dim) {
            const float ls = log_std[j];
            istd[k] = expf(-ls);
            z[k] = (act_row[j] - mean_row[j]) * istd[k];
            // normal_log_density per element: -z^2 / 2 - 0.5 log(2 pi) - log_std
            acc += -0.5f * z[k] * z[k] - half_log_2pi - ls;
        }
    }
#pragma unroll
    for (int off = LOSS_GROUP / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, LOSS_GROUP);
    return acc;
}

// surr = min(ratio A, clamp(ratio, lo, hi) A) -> `surr`; returns d loss / d logp for loss = -inv_n_exp * sum surr (neg_inv = -inv_n_exp)
__device__ __forceinline__ float row_surrogate(bool ok, float logp, float fixed, float adv, float lo, float hi, float neg_inv, float &surr) {
    const float ratio = expf(logp - fixed);
    const float clamped = fminf(fmaxf(ratio, lo), hi);
    const float surr1 = ratio * adv, surr2 = clamped * adv;
    surr = fminf(surr1, surr2);
    // d surr / d ratio with torch.min's tie rule (half each way) and clamp's sub-gradient (1 inside [lo, hi], ends included)
    const float inside = (ratio >= lo && ratio <= hi) ? 1.f : 0.f;
    float g_ratio;
    if (surr1 < surr2) g_ratio = adv;
    else if (surr1 > surr2) g_ratio = adv * inside;
    else g_ratio = 0.5f * adv + 0.5f * adv * inside;
    // loss = -inv_n_exp * sum surr;  d loss / d logp = -inv_n_exp * g_ratio * ratio
    return ok ? neg_inv * g_ratio * ratio : 0.f;
}

// d logp / d mean_j = z_j / std_j -> the row of d_mean;  d logp / d log_std_j = z_j^2 - 1 -> the lane's running sums
__device__ __forceinline__ void row_grads(bool ok, int l, int act_dim, float g_logp, const float (&z)[LOSS_MAXD], const float (&istd)[LOSS_MAXD],
                                          float *__restrict__ d_mean_row, float (&dls)[LOSS_MAXD]) {
#pragma unroll
    for (int k = 0; k < LOSS_MAXD; ++k) {
        const int j = l + LOSS_GROUP * k;
        if (ok && j < act_dim) {
            d_mean_row[j] = g_logp * z[k] * istd[k];
            dls[k] += g_logp * (z[k] * z[k] - 1.f);
        }
    }
}

__global__ __launch_bounds__(LOSS_BLOCK) void k_ppo_loss(LossArgs a) {
    __shared__ double s_red[4];
    __shared__ float s_grp[LOSS_BLOCK / LOSS_GROUP][LOSS_MAX_ACT];        // d_log_std sums of the block's 16 row groups
    const int t = threadIdx.x;
    double v_sum = 0.0, s_sum = 0.0;
    const bool want_dls = a.d_log_std != nullptr;
    if (want_dls) {
        for (int j = t; j < (LOSS_BLOCK / LOSS_GROUP) * LOSS_MAX_ACT; j += LOSS_BLOCK) (&s_grp[0][0])[j] = 0.f;
        __syncthreads();
    }
    if ((int)blockIdx.x >= a.pol_blocks) {
        // ---- critic: (pred - returns)^2, d_pred = 2 (pred - returns) / n_val
        const int vb = blockIdx.x - a.pol_blocks, nvb = gridDim.x - a.pol_blocks;
        const float two_inv = (float)(2.0 * a.inv_n_val);
        for (long i = (long)vb * LOSS_BLOCK + t; i < a.n; i += (long)nvb * LOSS_BLOCK) {
            const float d = a.pred[i] - a.returns[i];
            v_sum += (double)d * (double)d;
            if (a.d_pred) a.d_pred[i] = two_inv * d;
        }
    } else {
        // ---- actor: a 16-lane group per row, lane l takes action dimensions l, l + 16, ...
        const int grp = t / LOSS_GROUP, l = t % LOSS_GROUP;
        constexpr int GPB = LOSS_BLOCK / LOSS_GROUP;
        constexpr int MAXD = LOSS_MAXD;
        float dls[MAXD];
#pragma unroll
        for (int k = 0; k < MAXD; ++k) dls[k] = 0.f;
        const float lo = (float)(1.0 - a.clip_eps), hi = (float)(1.0 + a.clip_eps);
        const float neg_inv = (float)(-a.inv_n_exp);
        for (long r0 = (long)blockIdx.x * GPB; r0 < a.n_pol; r0 += (long)a.pol_blocks * GPB) {
            const long i = r0 + grp;
            const bool ok = i < a.n_pol;
            const long s = ok ? (a.rows ? (long)a.rows[i] : i) : 0;
            float z[LOSS_MAXD], istd[LOSS_MAXD];
            const float logp = row_logp(ok, l, a.act_dim, a.actions + s * a.ld_act, a.mean + i * a.ld_mean, a.log_std, z, istd);
            float fixed = logp;
            if (ok) {
                if (a.write_fixed) { if (l == 0) a.fixed_logp[i] = logp; }
                else fixed = a.fixed_logp[i];
            }
            float surr;
            const float g_logp = row_surrogate(ok, logp, fixed, ok ? a.adv[s] : 0.f, lo, hi, neg_inv, surr);
            if (ok && l == 0) s_sum += (double)surr;
            row_grads(ok, l, a.act_dim, g_logp, z, istd, a.d_mean + i * a.ld_dmean, dls);
        }
        if (want_dls) {
#pragma unroll
            for (int k = 0; k < MAXD; ++k) {
                const int j = l + LOSS_GROUP * k;
                if (j < a.act_dim) s_grp[grp][j] = dls[k];
            }
        }
    }
    const double vs = block_sum(v_sum, s_red);
    const double ss = block_sum(s_sum, s_red);
    double *mine = a.part + (long)blockIdx.x * (2 + a.act_dim);
    if (t == 0) { mine[0] = vs; mine[1] = ss; }
    if (want_dls) {
        __syncthreads();
        for (int j = t; j < a.act_dim; j += LOSS_BLOCK) {        // the 16 row groups in index order
            double d = 0.0;
            for (int g = 0; g < LOSS_BLOCK / LOSS_GROUP; ++g) d += (double)s_grp[g][j];
            mine[2 + j] = d;
        }
    }
}

// The partials -> losses[2] (and d_log_std): one workgroup, index order. A launch of its own rather than "whoever finishes
// last": a device-scope release / acquire per workgroup writes back and invalidates the XCD's whole L2 on this chip -- the
// loss kernel took 170 us with that pattern and 1 100 workgroups, against the ~30 us its 84 MB of traffic need.
__global__ __launch_bounds__(LOSS_BLOCK) void k_ppo_loss_final(LossArgs a, int nb) {
    __shared__ double s_red[4];
    const int t = threadIdx.x, stride = 2 + a.act_dim;
    double v = 0.0, s = 0.0;
    for (int b = t; b < nb; b += LOSS_BLOCK) {               // 256 interleaved slices, combined by block_sum's fixed tree
        const double *p = a.part + (long)b * stride;
        v += p[0];
        s += p[1];
    }
    v = block_sum(v, s_red);
    s = block_sum(s, s_red);
    if (t == 0) {
        a.losses[0] = v * a.inv_n_val;
        a.losses[1] = -s * a.inv_n_exp;
    }
    if (a.d_log_std) {
        for (int j = t; j < a.act_dim; j += LOSS_BLOCK) {
            double d = 0.0;
            for (int b = 0; b < a.pol_blocks; ++b) d += a.part[(long)b * stride + 2 + j];
            a.d_log_std[j] = (float)d;
        }
    }
}

// ------------------------------------------------------------------------------------------------ update monitor
// k_ppo_stats: what a PPO user reads off an epoch -- KL estimators, clip fraction, ratio range of the policy rows (logp from
// row_logp, the float32 log-ratio as row_surrogate forms it, everything after that in float64), the moments of returns and
// residuals for the critic's explained variance, and the number of sample rows with a non-finite operand -- as RAW sums, so that
// ranks combine by adding. A launch of its own: k_ppo_loss, its registers and its bits stay as they are. Same shape as the loss
// launch: blocks [0, pol_blocks) take policy rows (16 lanes per row), the rest value elements; per-workgroup float64
// partials, then one workgroup adds them in index order (k_ppo_stats_final).
constexpr int STATS_PART = 12;                 // doubles per workgroup: k1, k3, clipped, min r, max r, sum y, y^2, d, d^2, non-finite (+ 2 pad)

struct StatsArgs {
    int n, n_pol, act_dim;
    const long long *rows;
    const float *pred, *returns, *mean, *actions, *log_std, *adv, *fixed_logp;
    long ld_mean, ld_act;
    double clip_eps;
    float *logp_out;
    double *record;
    double *part;              // [gridDim.x][STATS_PART]
    int pol_blocks;
};

__device__ __forceinline__ double block_min(double v, double *s_red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_down(v, off, 64));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
    return fmin(fmin(s_red[0], s_red[1]), fmin(s_red[2], s_red[3]));
}

__device__ __forceinline__ double block_max(double v, double *s_red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
    return fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
}

// expm1(x) - x, the k3 term, without the cancellation of the subtraction for small |x| (the usual case: x is an epoch's log-ratio):
// x^2 (1/2 + x/6 + ... + x^14 / 16!) below 0.5 (the first term left out is under 2^-56 of the sum there) -- never negative.
__device__ __forceinline__ double k3_term(double x) {
    if (!(fabs(x) < 0.5)) return expm1(x) - x;
    const double c[15] = {1.0 / 2, 1.0 / 6, 1.0 / 24, 1.0 / 120, 1.0 / 720, 1.0 / 5040, 1.0 / 40320, 1.0 / 362880, 1.0 / 3628800,
                          1.0 / 39916800, 1.0 / 479001600, 1.0 / 6227020800.0, 1.0 / 87178291200.0, 1.0 / 1307674368000.0,
                          1.0 / 20922789888000.0};
    double p = c[14];
#pragma unroll
    for (int k = 13; k >= 0; --k) p = fma(x, p, c[k]);
    return (x * x) * p;
}

__global__ __launch_bounds__(LOSS_BLOCK) void k_ppo_stats(StatsArgs a) {
    __shared__ double s_red[4];
    const int t = threadIdx.x;
    double k1 = 0.0, k3 = 0.0, clipped = 0.0, rmin = INFINITY, rmax = -INFINITY;
    double sy = 0.0, syy = 0.0, sd = 0.0, sdd = 0.0, bad = 0.0;
    if ((int)blockIdx.x >= a.pol_blocks) {
        // ---- critic: moments of y = returns and d = returns - pred; a row with a non-finite pred / returns is counted here
        const int vb = blockIdx.x - a.pol_blocks, nvb = gridDim.x - a.pol_blocks;
        for (long i = (long)vb * LOSS_BLOCK + t; i < a.n; i += (long)nvb * LOSS_BLOCK) {
            const float p = a.pred[i], y = a.returns[i];
            const double yd = (double)y, dd = (double)y - (double)p;
            sy += yd; syy += yd * yd;
            sd += dd; sdd += dd * dd;
            if (!(isfinite(p) && isfinite(y))) bad += 1.0;
        }
    } else {
        // ---- actor: a 16-lane group per row, as k_ppo_loss; lane 0 of the group carries the row's terms
        const int grp = t / LOSS_GROUP, l = t % LOSS_GROUP;
        constexpr int GPB = LOSS_BLOCK / LOSS_GROUP;
        for (long r0 = (long)blockIdx.x * GPB; r0 < a.n_pol; r0 += (long)a.pol_blocks * GPB) {
            const long i = r0 + grp;
            const bool ok = i < a.n_pol;
            const long s = ok ? (a.rows ? (long)a.rows[i] : i) : 0;
            float z[LOSS_MAXD], istd[LOSS_MAXD];
            const float logp = row_logp(ok, l, a.act_dim, a.actions + s * a.ld_act, a.mean + i * a.ld_mean, a.log_std, z, istd);
            if (ok && l == 0) {
                if (a.logp_out) a.logp_out[i] = logp;
                const float lrf = logp - a.fixed_logp[i];              // the float32 log-ratio row_surrogate exponentiates
                const double lr = (double)lrf;
                const double r = exp(lr);
                k1 -= lr;
                k3 += k3_term(lr);
                if (fabs(r - 1.0) > a.clip_eps) clipped += 1.0;
                rmin = fmin(rmin, r);
                rmax = fmax(rmax, r);
                // the sample row is counted once: by the critic's blocks when its pred / returns is non-finite, else here
                const bool v_ok = s >= a.n || (isfinite(a.pred[s]) && isfinite(a.returns[s]));
                if (v_ok && !(isfinite(a.adv[s]) && isfinite(logp))) bad += 1.0;
            }
        }
    }
    double *mine = a.part + (long)blockIdx.x * STATS_PART;
    const double v[10] = {block_sum(k1, s_red), block_sum(k3, s_red), block_sum(clipped, s_red), block_min(rmin, s_red), block_max(rmax, s_red),
                          block_sum(sy, s_red), block_sum(syy, s_red), block_sum(sd, s_red), block_sum(sdd, s_red), block_sum(bad, s_red)};
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < 10; ++k) mine[k] = v[k];
    }
}

// the partials of `nb` workgroups -> the record (layout: include/egopose_hip.h); nb = 0 writes the record of an empty batch
__global__ __launch_bounds__(LOSS_BLOCK) void k_ppo_stats_final(StatsArgs a, int nb) {
    __shared__ double s_red[4];
    const int t = threadIdx.x;
    double acc[10] = {0.0, 0.0, 0.0, INFINITY, -INFINITY, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = t; b < nb; b += LOSS_BLOCK) {               // 256 interleaved slices, combined by the fixed trees below
        const double *p = a.part + (long)b * STATS_PART;
#pragma unroll
        for (int k = 0; k < 10; ++k) acc[k] = k == 3 ? fmin(acc[k], p[k]) : (k == 4 ? fmax(acc[k], p[k]) : acc[k] + p[k]);
    }
    double tot[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) tot[k] = k == 3 ? block_min(acc[k], s_red) : (k == 4 ? block_max(acc[k], s_red) : block_sum(acc[k], s_red));
    if (t == 0) {
        double *o = a.record;
        o[EGP_PPO_STATS_N_POL] = (double)a.n_pol;
        o[EGP_PPO_STATS_K1] = tot[0];
        o[EGP_PPO_STATS_K3] = tot[1];
        o[EGP_PPO_STATS_CLIPPED] = tot[2];
        o[EGP_PPO_STATS_RATIO_MIN] = tot[3];
        o[EGP_PPO_STATS_RATIO_MAX] = tot[4];
        o[EGP_PPO_STATS_N] = (double)a.n;
        o[EGP_PPO_STATS_SUM_Y] = tot[5];
        o[EGP_PPO_STATS_SUM_YY] = tot[6];
        o[EGP_PPO_STATS_SUM_D] = tot[7];
        o[EGP_PPO_STATS_SUM_DD] = tot[8];
        o[EGP_PPO_STATS_NONFINITE] = tot[9];
        // entropy of N(., diag exp(2 log_std)) with a state-independent log_std: sum_j log_std_j + act_dim / 2 * log(2 pi e)
        double e = a.log_std ? 0.0 : (double)NAN;              // (no log_std: only allowed without policy rows)
        if (a.log_std)
            for (int j = 0; j < a.act_dim; ++j) e += (double)a.log_std[j];
        o[EGP_PPO_STATS_ENTROPY] = e + 0.5 * (double)a.act_dim * 2.8378770664093453;
    }
}

// ------------------------------------------------------------------------------------------------ mini-batch epochs
// agents/agent_ppo.py:24-44: every epoch shuffles the batch, then takes optimizer steps on windows of opt_batch_size rows. A
// window is a few dozen rows, so everything here is launch latency: one launch lays the epoch out (k_minibatch_plan), one launch
// per window forms both losses (k_ppo_loss_mb), and the number of exploration rows of a window never leaves the device.

constexpr int PLAN_BLOCK = 256;
constexpr int PLAN_MAX_BLOCKS = 1024;

struct PlanArgs {
    int n, state_dim, act_dim, batch, n_win;
    const long long *perm;
    const float *states, *actions, *returns, *adv, *fixed_logp, *exps;
    long ld_states, ld_act;
    float *o_states, *o_actions, *o_returns, *o_adv, *o_fixed_logp, *o_exps;
    int *mb_n_exp;
    int wide_states, wide_act;
};

// rows of `width` floats: dst row r = src row perm[r]; the grid strides over the (row, column) elements
template <typename V>
__device__ __forceinline__ void plan_copy_rows(const PlanArgs &a, const float *__restrict__ src, long ld_src, float *__restrict__ dst, int width) {
    constexpr int W = (int)(sizeof(V) / sizeof(float));
    const int wv = width / W;
    const long total = (long)a.n * wv;
    for (long e = (long)blockIdx.x * PLAN_BLOCK + threadIdx.x; e < total; e += (long)gridDim.x * PLAN_BLOCK) {
        const long r = e / wv;
        const int c = (int)(e - r * wv);
        const long long sr = a.perm[r];
        if (sr < 0 || sr >= a.n) continue;                       // (not a permutation: the row is left alone, nothing is read out of range)
        *reinterpret_cast<V *>(dst + r * width + (long)c * W) = *reinterpret_cast<const V *>(src + sr * ld_src + (long)c * W);
    }
}

__global__ __launch_bounds__(PLAN_BLOCK) void k_minibatch_plan(PlanArgs a) {
    __shared__ int s_cnt[PLAN_BLOCK / 64];
    if (a.wide_states) plan_copy_rows<float4>(a, a.states, a.ld_states, a.o_states, a.state_dim);
    else plan_copy_rows<float>(a, a.states, a.ld_states, a.o_states, a.state_dim);
    if (a.wide_act) plan_copy_rows<float4>(a, a.actions, a.ld_act, a.o_actions, a.act_dim);
    else plan_copy_rows<float>(a, a.actions, a.ld_act, a.o_actions, a.act_dim);
    for (long r = (long)blockIdx.x * PLAN_BLOCK + threadIdx.x; r < a.n; r += (long)gridDim.x * PLAN_BLOCK) {
        const long long sr = a.perm[r];
        if (sr < 0 || sr >= a.n) continue;
        a.o_returns[r] = a.returns[sr];
        a.o_adv[r] = a.adv[sr];
        a.o_fixed_logp[r] = a.fixed_logp[sr];
        a.o_exps[r] = a.exps[sr];
    }
    // exploration rows per window: windows stride over the workgroups, a window's rows over the workgroup's threads; each wave
    // counts with ballot + popcount and the four wave counts are added in order. Every entry is written: nothing to zero first.
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int w = blockIdx.x; w < a.n_win; w += gridDim.x) {
        const long begin = (long)w * a.batch;
        const long end = begin + a.batch < a.n ? begin + a.batch : a.n;
        int cnt = 0;
        for (long r0 = begin; r0 < end; r0 += PLAN_BLOCK) {          // (uniform trip count: the ballot sees whole waves)
            const long r = r0 + threadIdx.x;
            bool on = false;
            if (r < end) {
                const long long sr = a.perm[r];
                on = sr >= 0 && sr < a.n && a.exps[sr] != 0.f;
            }
            cnt += __popcll(__ballot(on));
        }
        __syncthreads();
        if (lane == 0) s_cnt[wave] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) a.mb_n_exp[w] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    }
}

constexpr int MB_BLOCK = 512;                      // one workgroup per window: 32 row groups of 16 lanes
constexpr int MB_GROUPS = MB_BLOCK / LOSS_GROUP;
constexpr int MB_WAVES = MB_BLOCK / 64;

struct LossMbArgs {
    int n, act_dim;
    const float *pred, *returns, *mean, *actions, *log_std, *adv, *fixed_logp, *exps;
    long ld_mean, ld_act, ld_dmean;
    const int *n_exp;
    double clip_eps;
    float *d_pred, *d_mean, *d_log_std;
    double *losses;
};

__device__ __forceinline__ double block_sum_mb(double v, double *s_red) {
    // as block_sum, for the MB_BLOCK threads of k_ppo_loss_mb: lane butterflies, then the eight wave sums in index order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < MB_WAVES; ++w) tot += s_red[w];
    return tot;
}

// Both losses of ONE window of the permuted batch, with fixed shapes: the policy head was evaluated on every row, the rows with
// exps == 0 get d_mean = 0 (exact zeros in every weight gradient: what leaving them out of the batch gives) and stay out of the
// surrogate's sums; its mean divides by the count k_minibatch_plan left on the device. A window is a few thousand rows at most,
// so one workgroup walks it and adds its own partials in index order: no workspace, no second launch.
__global__ __launch_bounds__(MB_BLOCK) void k_ppo_loss_mb(LossMbArgs a) {
    __shared__ double s_red[MB_WAVES];
    __shared__ float s_grp[MB_GROUPS][LOSS_MAX_ACT];
    const int t = threadIdx.x;
    const bool want_dls = a.d_log_std != nullptr;
    // ---- critic
    double v_sum = 0.0;
    const double inv_n_val = 1.0 / (double)(a.n > 0 ? a.n : 1);
    const float two_inv = (float)(2.0 * inv_n_val);
    for (int i = t; i < a.n; i += MB_BLOCK) {
        const float d = a.pred[i] - a.returns[i];
        v_sum += (double)d * (double)d;
        a.d_pred[i] = two_inv * d;
    }
    // ---- actor
    const int cnt = *a.n_exp;
    const double inv_n_exp = 1.0 / (double)cnt;                 // an empty window: 1 / 0, the surrogate loss below is 0 * inf = NaN (torch's empty .mean())
    const int grp = t / LOSS_GROUP, l = t % LOSS_GROUP;
    float dls[LOSS_MAXD];
#pragma unroll
    for (int k = 0; k < LOSS_MAXD; ++k) dls[k] = 0.f;
    const float lo = (float)(1.0 - a.clip_eps), hi = (float)(1.0 + a.clip_eps);
    const float neg_inv = (float)(-inv_n_exp);
    double s_sum = 0.0;
    for (int r0 = 0; r0 < a.n; r0 += MB_GROUPS) {
        const long i = r0 + grp;
        const bool in = i < a.n;
        const bool ok = in && a.exps[i] != 0.f;
        const long s = in ? i : 0;
        float z[LOSS_MAXD], istd[LOSS_MAXD];
        const float logp = row_logp(ok, l, a.act_dim, a.actions + s * a.ld_act, a.mean + s * a.ld_mean, a.log_std, z, istd);
        float surr;
        const float g_logp = row_surrogate(ok, logp, ok ? a.fixed_logp[i] : logp, ok ? a.adv[i] : 0.f, lo, hi, neg_inv, surr);
        if (ok && l == 0) s_sum += (double)surr;
        row_grads(ok, l, a.act_dim, g_logp, z, istd, a.d_mean + s * a.ld_dmean, dls);
        if (in && !ok)
            for (int j = l; j < a.act_dim; j += LOSS_GROUP) a.d_mean[i * a.ld_dmean + j] = 0.f;
    }
    const double vs = block_sum_mb(v_sum, s_red);
    const double ss = block_sum_mb(s_sum, s_red);
    if (t == 0) {
        a.losses[0] = vs * inv_n_val;
        a.losses[1] = -ss * inv_n_exp;
    }
    if (want_dls) {
#pragma unroll
        for (int k = 0; k < LOSS_MAXD; ++k) {
            const int j = l + LOSS_GROUP * k;
            if (j < a.act_dim) s_grp[grp][j] = dls[k];
        }
        __syncthreads();
        for (int j = t; j < a.act_dim; j += MB_BLOCK) {          // the 32 row groups in index order
            double d = 0.0;
            for (int g = 0; g < MB_GROUPS; ++g) d += (double)s_grp[g][j];
            a.d_log_std[j] = (float)d;
        }
    }
}

// ------------------------------------------------------------------------------------------------ clip + Adam
constexpr int ADAM_BLOCK = 256;
constexpr int NORM_BLOCKS = 256;               // partials per clip group

struct AdamSeg {
    long begin, end;
    double lr, beta1, beta2, eps, wd, bias1, bias2, max_norm;
    int clip_group;
};
struct AdamArgs {
    int n_seg;
    AdamSeg seg[EGP_ADAM_MAX_SEGMENTS];
    double *part;              // [EGP_ADAM_MAX_SEGMENTS + 1][NORM_BLOCKS] squared-norm partials per clip group
    double *norms_out;         // [EGP_ADAM_MAX_SEGMENTS + 1] or null
};

// squared 2-norm of the gradient of every clip group: blockIdx.y = group (1-based), NORM_BLOCKS partials each
template <typename TG>
__global__ __launch_bounds__(ADAM_BLOCK) void k_sqnorm(AdamArgs a, const TG *__restrict__ grad) {
    __shared__ double s_red[4];
    const int group = blockIdx.y + 1;
    double acc = 0.0;
    for (int s = 0; s < a.n_seg; ++s) {
        if (a.seg[s].clip_group != group) continue;
        for (long i = a.seg[s].begin + (long)blockIdx.x * ADAM_BLOCK + threadIdx.x; i < a.seg[s].end; i += (long)NORM_BLOCKS * ADAM_BLOCK) {
            const double g = (double)grad[i];
            acc += g * g;
        }
    }
    const double tot = block_sum(acc, s_red);
    if (threadIdx.x == 0) a.part[(long)group * NORM_BLOCKS + blockIdx.x] = tot;
}

template <typename TP, typename TG>
__global__ __launch_bounds__(ADAM_BLOCK) void k_adam(AdamArgs a, const TG *__restrict__ grad, TP *__restrict__ param, TP *__restrict__ m,
                                                     TP *__restrict__ v, float *__restrict__ shadow, long total) {
    __shared__ double s_red[4];
    __shared__ double s_coef[EGP_ADAM_MAX_SEGMENTS + 1];
    // every block derives the clip coefficients itself from the partials (the same operations in the same order everywhere)
    for (int g = 1; g <= EGP_ADAM_MAX_SEGMENTS; ++g) {
        bool used = false;
        for (int s = 0; s < a.n_seg; ++s) used |= a.seg[s].clip_group == g;
        if (!used) { if (threadIdx.x == 0) s_coef[g] = 1.0; continue; }       // (uniform branch: `used` depends on kernel arguments only)
        double max_norm = 0.0;
        for (int s = 0; s < a.n_seg; ++s) if (a.seg[s].clip_group == g) max_norm = a.seg[s].max_norm;
        const double p = threadIdx.x < NORM_BLOCKS ? a.part[(long)g * NORM_BLOCKS + threadIdx.x] : 0.0;
        const double norm = sqrt(block_sum(p, s_red));
        if (threadIdx.x == 0) {
            s_coef[g] = fmin(1.0, max_norm / (norm + 1e-6));                  // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1)
            if (a.norms_out && blockIdx.x == 0) a.norms_out[g] = norm;
        }
    }
    if (threadIdx.x == 0) s_coef[0] = 1.0;
    __syncthreads();
    for (long i = (long)blockIdx.x * ADAM_BLOCK + threadIdx.x; i < total; i += (long)gridDim.x * ADAM_BLOCK) {
        int s = 0;
        while (s < a.n_seg && !(i >= a.seg[s].begin && i < a.seg[s].end)) ++s;
        if (s == a.n_seg) continue;                                           // an element outside every stepped segment
        const AdamSeg &sg = a.seg[s];
        const TP coef = (TP)s_coef[sg.clip_group];
        const TP p = param[i];
        TP g = (TP)grad[i] * coef;
        if (sg.wd != 0.0) g += (TP)sg.wd * p;
        const TP b1 = (TP)sg.beta1, b2 = (TP)sg.beta2;
        const TP mm = m[i] + (g - m[i]) * ((TP)1 - b1);                        // lerp(exp_avg, grad, 1 - beta1)
        const TP vv = b2 * v[i] + ((TP)1 - b2) * g * g;
        const TP step_size = (TP)(sg.lr / sg.bias1);
        const TP denom = (TP)sqrt((double)vv) / (TP)sqrt(sg.bias2) + (TP)sg.eps;
        const TP pn = p - step_size * (mm / denom);
        m[i] = mm;
        v[i] = vv;
        param[i] = pn;
        if (shadow) shadow[i] = (float)pn;
    }
}

template <typename TP, typename TG>
int adam_launch(int n_seg, const egp_adam_segment *seg, const TG *grad, TP *param, TP *m, TP *v, float *shadow, void *workspace,
                double *norms_out, void *stream) {
    EGP_REQUIRE(n_seg >= 0 && n_seg <= EGP_ADAM_MAX_SEGMENTS, "n_seg out of range");
    if (n_seg == 0) return EGP_OK;
    EGP_REQUIRE(seg && grad && param && m && v && workspace, "NULL pointer");
    AdamArgs a{};
    a.n_seg = n_seg;
    a.part = (double *)workspace;
    a.norms_out = norms_out;
    long lo = -1, hi = 0;
    int max_group = 0;
    for (int s = 0; s < n_seg; ++s) {
        const egp_adam_segment &q = seg[s];
        EGP_REQUIRE(q.begin >= 0 && q.end >= q.begin, "bad segment range");
        EGP_REQUIRE(q.clip_group >= 0 && q.clip_group <= EGP_ADAM_MAX_SEGMENTS, "clip_group out of range");
        EGP_REQUIRE(q.clip_group == 0 || q.max_norm > 0.0, "a clipped segment needs max_norm > 0");
        EGP_REQUIRE(q.bias1 > 0.0 && q.bias2 > 0.0, "bias corrections must be positive (step >= 1)");
        a.seg[s] = AdamSeg{(long)q.begin, (long)q.end, q.lr, q.beta1, q.beta2, q.eps, q.weight_decay, q.bias1, q.bias2, q.max_norm, q.clip_group};
        if (q.end > q.begin) {
            lo = lo < 0 ? (long)q.begin : (q.begin < lo ? (long)q.begin : lo);
            hi = q.end > hi ? (long)q.end : hi;
        }
        max_group = q.clip_group > max_group ? q.clip_group : max_group;
    }
    if (hi <= 0 || lo < 0) return EGP_OK;
    hipStream_t st = (hipStream_t)stream;
    if (max_group > 0) {
        k_sqnorm<TG><<<dim3(NORM_BLOCKS, max_group), dim3(ADAM_BLOCK), 0, st>>>(a, grad);
        int rc = after_launch("k_sqnorm");
        if (rc != EGP_OK) return rc;
    }
    const long blocks = std::min<long>((hi + ADAM_BLOCK - 1) / ADAM_BLOCK, 2048);
    k_adam<TP, TG><<<dim3((unsigned)blocks), dim3(ADAM_BLOCK), 0, st>>>(a, grad, param, m, v, shadow, hi);
    return after_launch("k_adam");
}

}  // namespace

extern "C" {

int64_t egp_ppo_loss_workspace_bytes(int32_t n, int32_t n_pol, int32_t act_dim) {
    (void)n; (void)n_pol;
    return (int64_t)(2 * LOSS_MAX_BLOCKS) * (2 + (act_dim > 0 ? act_dim : 0)) * (int64_t)sizeof(double) + 64;
}

int egp_ppo_loss_f32(const egp_ppo_loss_desc *d, void *stream) {
    EGP_REQUIRE(d, "descriptor is NULL");
    EGP_REQUIRE(d->n >= 0 && d->n_pol >= 0 && d->act_dim >= 0 && d->act_dim <= LOSS_MAX_ACT, "bad sizes (act_dim <= 256)");
    EGP_REQUIRE(d->losses && d->workspace, "NULL losses / workspace");
    EGP_REQUIRE(d->n == 0 || (d->pred && d->returns), "NULL critic operand");
    EGP_REQUIRE(d->n_pol == 0 || (d->mean && d->actions && d->log_std && d->adv && d->fixed_logp && d->d_mean), "NULL actor operand");
    LossArgs a{};
    a.n = d->n; a.n_pol = d->n_pol; a.act_dim = d->act_dim;
    a.rows = (const long long *)d->rows;
    a.pred = d->pred; a.returns = d->returns; a.mean = d->mean; a.actions = d->actions; a.log_std = d->log_std; a.adv = d->adv;
    a.ld_mean = d->ld_mean; a.ld_act = d->ld_act; a.ld_dmean = d->ld_dmean;
    a.fixed_logp = d->fixed_logp; a.write_fixed = d->write_fixed;
    a.clip_eps = d->clip_eps; a.inv_n_val = d->inv_n_val; a.inv_n_exp = d->inv_n_exp;
    a.d_pred = d->d_pred; a.d_mean = d->d_mean; a.d_log_std = d->d_log_std;
    a.losses = d->losses;
    a.counter = nullptr;
    a.part = (double *)d->workspace;                        // [workgroups][2 + act_dim] partial sums
    constexpr int GPB = LOSS_BLOCK / LOSS_GROUP;
    long pb = ((long)d->n_pol + 4 * GPB - 1) / (4 * GPB);          // ~4 passes of 16 rows per block
    pb = pb < 1 ? (d->n_pol > 0 ? 1 : 0) : (pb > LOSS_MAX_BLOCKS ? LOSS_MAX_BLOCKS : pb);
    long vb = ((long)d->n + 4 * LOSS_BLOCK - 1) / (4 * LOSS_BLOCK);
    vb = vb < 1 ? (d->n > 0 ? 1 : 0) : (vb > LOSS_MAX_BLOCKS ? LOSS_MAX_BLOCKS : vb);
    if (pb + vb == 0) {
        // nothing to sum: both losses are zero
        hipError_t e = hipMemsetAsync(d->losses, 0, 2 * sizeof(double), (hipStream_t)stream);
        if (e != hipSuccess) { egp::set_error("hipMemsetAsync failed: %s", hipGetErrorString(e)); return EGP_E_HIP; }
        return EGP_OK;
    }
    a.pol_blocks = (int)pb;
    k_ppo_loss<<<dim3((unsigned)(pb + vb)), dim3(LOSS_BLOCK), 0, (hipStream_t)stream>>>(a);
    int rc = after_launch("k_ppo_loss");
    if (rc != EGP_OK) return rc;
    k_ppo_loss_final<<<dim3(1), dim3(LOSS_BLOCK), 0, (hipStream_t)stream>>>(a, (int)(pb + vb));
    return after_launch("k_ppo_loss_final");
}

int64_t egp_ppo_stats_workspace_bytes(int32_t n, int32_t n_pol, int32_t act_dim) {
    (void)n; (void)n_pol; (void)act_dim;
    return (int64_t)(2 * LOSS_MAX_BLOCKS) * STATS_PART * (int64_t)sizeof(double) + 64;
}

int egp_ppo_stats_f32(const egp_ppo_stats_desc *d, void *stream) {
    EGP_REQUIRE(d, "descriptor is NULL");
    EGP_REQUIRE(d->n >= 0 && d->n_pol >= 0 && d->act_dim >= 0 && d->act_dim <= LOSS_MAX_ACT, "bad sizes (act_dim <= 256)");
    EGP_REQUIRE(d->record && d->workspace, "NULL record / workspace");
    EGP_REQUIRE(d->n == 0 || (d->pred && d->returns), "NULL critic operand");
    EGP_REQUIRE(d->n_pol == 0 || (d->mean && d->actions && d->log_std && d->adv && d->fixed_logp), "NULL actor operand");
    EGP_REQUIRE(d->n_pol <= 1 || (d->ld_mean >= d->act_dim && d->ld_act >= d->act_dim), "row stride smaller than the row");
    EGP_REQUIRE(d->clip_eps >= 0.0, "clip_eps must not be negative (or NaN)");
    StatsArgs a{};
    a.n = d->n; a.n_pol = d->n_pol; a.act_dim = d->act_dim;
    a.rows = (const long long *)d->rows;
    a.pred = d->pred; a.returns = d->returns; a.mean = d->mean; a.actions = d->actions; a.log_std = d->log_std; a.adv = d->adv;
    a.fixed_logp = d->fixed_logp;
    a.ld_mean = d->ld_mean; a.ld_act = d->ld_act;
    a.clip_eps = d->clip_eps;
    a.logp_out = d->logp_out;
    a.record = d->record;
    a.part = (double *)d->workspace;
    constexpr int GPB = LOSS_BLOCK / LOSS_GROUP;
    long pb = ((long)d->n_pol + 4 * GPB - 1) / (4 * GPB);          // the loss launch's grid: ~4 passes per block
    pb = pb < 1 ? (d->n_pol > 0 ? 1 : 0) : (pb > LOSS_MAX_BLOCKS ? LOSS_MAX_BLOCKS : pb);
    long vb = ((long)d->n + 4 * LOSS_BLOCK - 1) / (4 * LOSS_BLOCK);
    vb = vb < 1 ? (d->n > 0 ? 1 : 0) : (vb > LOSS_MAX_BLOCKS ? LOSS_MAX_BLOCKS : vb);
    a.pol_blocks = (int)pb;
    if (pb + vb > 0) {
        k_ppo_stats<<<dim3((unsigned)(pb + vb)), dim3(LOSS_BLOCK), 0, (hipStream_t)stream>>>(a);
        int rc = after_launch("k_ppo_stats");
        if (rc != EGP_OK) return rc;
    }
    k_ppo_stats_final<<<dim3(1), dim3(LOSS_BLOCK), 0, (hipStream_t)stream>>>(a, (int)(pb + vb));
    return after_launch("k_ppo_stats_final");
}

int egp_minibatch_plan_f32(const egp_minibatch_plan_desc *d, void *stream) {
    EGP_REQUIRE(d, "descriptor is NULL");
    EGP_REQUIRE(d->n >= 0 && d->state_dim >= 1 && d->act_dim >= 1 && d->batch >= 1, "bad sizes (n >= 0, state_dim / act_dim / batch >= 1)");
    if (d->n == 0) return EGP_OK;
    EGP_REQUIRE(d->perm && d->states && d->actions && d->returns && d->adv && d->fixed_logp && d->exps, "NULL source column");
    EGP_REQUIRE(d->out_states && d->out_actions && d->out_returns && d->out_adv && d->out_fixed_logp && d->out_exps && d->mb_n_exp,
                "NULL destination");
    EGP_REQUIRE(d->ld_states >= d->state_dim && d->ld_act >= d->act_dim, "row stride smaller than the row");
    PlanArgs a{};
    a.n = d->n; a.state_dim = d->state_dim; a.act_dim = d->act_dim; a.batch = d->batch;
    a.n_win = (int)(((long)d->n + d->batch - 1) / d->batch);
    a.perm = (const long long *)d->perm;
    a.states = d->states; a.actions = d->actions; a.returns = d->returns; a.adv = d->adv; a.fixed_logp = d->fixed_logp; a.exps = d->exps;
    a.ld_states = d->ld_states; a.ld_act = d->ld_act;
    a.o_states = d->out_states; a.o_actions = d->out_actions; a.o_returns = d->out_returns; a.o_adv = d->out_adv;
    a.o_fixed_logp = d->out_fixed_logp; a.o_exps = d->out_exps;
    a.mb_n_exp = d->mb_n_exp;
    // 16-byte moves when every row base on both sides is 16-byte aligned, single floats otherwise
    auto wide = [](const void *src, long ld, const void *dst, int width) {
        return width % 4 == 0 && ld % 4 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0;
    };
    a.wide_states = wide(d->states, a.ld_states, d->out_states, d->state_dim) ? 1 : 0;
    a.wide_act = wide(d->actions, a.ld_act, d->out_actions, d->act_dim) ? 1 : 0;
    const int widest = d->state_dim > d->act_dim ? d->state_dim : d->act_dim;
    long blocks = ((long)d->n * (a.wide_states ? widest / 4 : widest) + PLAN_BLOCK - 1) / PLAN_BLOCK;
    blocks = blocks < 1 ? 1 : (blocks > PLAN_MAX_BLOCKS ? PLAN_MAX_BLOCKS : blocks);
    k_minibatch_plan<<<dim3((unsigned)blocks), dim3(PLAN_BLOCK), 0, (hipStream_t)stream>>>(a);
    return after_launch("k_minibatch_plan");
}

int egp_ppo_loss_mb_f32(const egp_ppo_loss_mb_desc *d, void *stream) {
    EGP_REQUIRE(d, "descriptor is NULL");
    EGP_REQUIRE(d->n >= 1 && d->n <= EGP_PPO_LOSS_MB_MAX_ROWS, "a window has 1 .. EGP_PPO_LOSS_MB_MAX_ROWS rows");
    EGP_REQUIRE(d->act_dim >= 1 && d->act_dim <= LOSS_MAX_ACT, "bad act_dim (1 .. 256)");
    EGP_REQUIRE(d->pred && d->returns && d->mean && d->actions && d->log_std && d->adv && d->fixed_logp && d->exps && d->n_exp, "NULL operand");
    EGP_REQUIRE(d->d_pred && d->d_mean && d->losses, "NULL result");
    EGP_REQUIRE(d->ld_mean >= d->act_dim && d->ld_act >= d->act_dim && d->ld_dmean >= d->act_dim, "row stride smaller than the row");
    LossMbArgs a{};
    a.n = d->n; a.act_dim = d->act_dim;
    a.pred = d->pred; a.returns = d->returns; a.mean = d->mean; a.actions = d->actions; a.log_std = d->log_std; a.adv = d->adv;
    a.fixed_logp = d->fixed_logp; a.exps = d->exps;
    a.ld_mean = d->ld_mean; a.ld_act = d->ld_act; a.ld_dmean = d->ld_dmean;
    a.n_exp = d->n_exp;
    a.clip_eps = d->clip_eps;
    a.d_pred = d->d_pred; a.d_mean = d->d_mean; a.d_log_std = d->d_log_std;
    a.losses = d->losses;
    k_ppo_loss_mb<<<dim3(1), dim3(MB_BLOCK), 0, (hipStream_t)stream>>>(a);
    return after_launch("k_ppo_loss_mb");
}

int64_t egp_adam_workspace_bytes(void) { return (int64_t)(EGP_ADAM_MAX_SEGMENTS + 1) * NORM_BLOCKS * (int64_t)sizeof(double); }

int egp_adam_step_f32(int32_t n_seg, const egp_adam_segment *seg, const float *grad, float *param, float *exp_avg, float *exp_avg_sq,
                      void *workspace, double *norms_out, void *stream) {
    return adam_launch<float, float>(n_seg, seg, grad, param, exp_avg, exp_avg_sq, nullptr, workspace, norms_out, stream);
}
int egp_adam_step_f64(int32_t n_seg, const egp_adam_segment *seg, const float *grad, double *param, double *exp_avg, double *exp_avg_sq,
                      float *shadow, void *workspace, double *norms_out, void *stream) {
    return adam_launch<double, float>(n_seg, seg, grad, param, exp_avg, exp_avg_sq, shadow, workspace, norms_out, stream);
}
int egp_adam_step_f64g(int32_t n_seg, const egp_adam_segment *seg, const double *grad, double *param, double *exp_avg, double *exp_avg_sq,
                       void *workspace, double *norms_out, void *stream) {
    return adam_launch<double, double>(n_seg, seg, grad, param, exp_avg, exp_avg_sq, nullptr, workspace, norms_out, stream);
}

}  // extern "C"
