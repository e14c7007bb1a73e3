// K1, one launch per substep: the stable-PD torque (compute_torque / compute_desired_accel,
// ego_pose/envs/humanoid_v1.py:130-156, + clip :172) with the C-ABI entry points egp_pd_torque_{f64,f32} and the engine's
// strided launch.
//
// One 64-lane wavefront per env; the shared skeleton tables (the dof tree's dense -> sparse map, the PD gains) and the env's
// sparse inertia row are staged in LDS. The kernel is chosen by the context's pd_variant:
//   0  k_pd_torque_grid58   the tree-ordered elimination on a 4 x 16 lane grid (egp_pd_grid.hpp): default for the humanoid
//   3  k_pd_torque_tree58   its predecessor: lane i owns row i, the 58 x 58 system in VGPRs, pivots leaves -> root (egp_pd_dev.hpp)
//   2  k_pd_torque_reg58    dense in-register Gauss-Jordan with v_readlane broadcasts: any dof tree with nv == 58
//   1  k_pd_torque_lds      the system in LDS: any nv <= 64
// and k_torque_direct stands in for all of them when cfg.action_type is 'torque'.
#include <hip/hip_runtime.h>
#include <math.h>

#include "egp_internal.hpp"
#include "egp_pd_dev.hpp"
#include "egp_pd_grid.hpp"

namespace egp {

// ============================================================================================ K1
template <typename TIO>
__global__ __launch_bounds__(256) void k_pd_torque_reg58(DevModel m, PdLd ld, const TIO *__restrict__ qpos,
                                                         const TIO *__restrict__ qvel, const TIO *__restrict__ action,
                                                         const TIO *__restrict__ qM, const TIO *__restrict__ C, int n,
                                                         TIO *__restrict__ torque, TIO *__restrict__ torque_raw) {
    __shared__ short s_map[PD_NV * PD_NV];        // dense (i,j) -> qM index: the dof tree, staged once per block
    __shared__ double s_qM[4][PD_NM_MAX];         // this wave's sparse inertia
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < PD_NV * PD_NV; i += 256) s_map[i] = m.m_map[i];
    const long env = (long)blockIdx.x * 4 + wave;
    const bool valid = env < n;
    if (valid) {
        const TIO *src = qM + env * ld.qM;
        for (int i = lane; i < m.nM; i += 64) s_qM[wave][i] = (double)src[i];
    }
    __syncthreads();
    if (!valid) return;
    const int row = lane < PD_NV ? lane : PD_NV - 1;   // spare lanes shadow the last row
    double kp, kd, eq, qv, b;
    pd_rhs<TIO>(m, ld, qpos, qvel, action, C, env, row, kp, kd, eq, qv, b);
    const double kd_dt = kd * m.sub_dt;
    // mj_fullM: lane `row` gathers its dense row from the sparse chain layout; + Kd*dt on the diagonal
    double a[PD_NV];
#pragma unroll
    for (int j = 0; j < PD_NV; ++j) {
        const int id = s_map[row * PD_NV + j];
        double v = id >= 0 ? s_qM[wave][id] : 0.0;
        a[j] = v + (j == row ? kd_dt : 0.0);
    }
    // Gauss-Jordan without pivoting (matrix is SPD): after step k column k is zero off the diagonal.
    double dinv = 0.0;
#pragma unroll
    for (int k = 0; k < PD_NV; ++k) {
        const double pk = readlane_f64(a[k], k);
        const double inv = 1.0 / pk;
        const bool me = row == k;
        const double f = me ? 0.0 : a[k] * inv;
        dinv = me ? inv : dinv;
#pragma unroll
        for (int j = k + 1; j < PD_NV; ++j) {
            const double r = readlane_f64(a[j], k);
            a[j] = fma(-f, r, a[j]);
        }
        const double bk = readlane_f64(b, k);
        b = fma(-f, bk, b);
    }
    const double qacc = b * dinv;
    pd_store<TIO>(m, env, row, lane < PD_NV, kp, kd, eq, qv, qacc, torque, torque_raw);
}

// Tree-ordered elimination, lane i owns row i (tree_eliminate: egp_pd_dev.hpp).
template <typename TIO>
__global__ __launch_bounds__(256) void k_pd_torque_tree58(DevModel m, PdLd ld, const TIO *__restrict__ qpos,
                                                          const TIO *__restrict__ qvel, const TIO *__restrict__ action,
                                                          const TIO *__restrict__ qM, const TIO *__restrict__ C, int n,
                                                          TIO *__restrict__ torque, TIO *__restrict__ torque_raw, PdDone done) {
    __shared__ short s_map[PD_NV * PD_NV];
    __shared__ double s_qM[4][PD_NM_MAX];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long env = (long)blockIdx.x * 4 + wave;
    const bool valid = env < n;
    const int row = lane < PD_NV ? lane : PD_NV - 1;
    // the state row may live in pinned host memory (zero-copy engine): issue those loads first so the PCIe round
    // trip overlaps the LDS fills below
    const int act = row >= 6 ? row - 6 : 0;
    TIO r_q = TIO(0), r_v = TIO(0), r_c = TIO(0), r_a = TIO(0);
    if (valid) {
        r_q = qpos[env * ld.qpos + 7 + act];
        r_v = qvel[env * ld.qvel + row];
        r_c = C[env * ld.bias + row];
        r_a = action[env * ld.action + act];
    }
    // per-dof constants, also up front (each dependent global load costs a full memory round trip at 2 waves/CU)
    const double c_kp = m.jkp[act], c_kd = m.jkd[act], c_ref = m.a_ref[act], c_scale = m.a_scale[act], c_lim = m.torque_lim[act];
    // LDS fills with every load of a thread in flight at once (the rolled loops waited for each load in turn)
    {
        constexpr int MAP_IT = (PD_NV * PD_NV + 255) / 256;
        short t_map[MAP_IT];
#pragma unroll
        for (int k = 0; k < MAP_IT; ++k) {
            const int i = threadIdx.x + 256 * k;
            t_map[k] = i < PD_NV * PD_NV ? m.m_map[i] : (short)0;
        }
        constexpr int QM_IT = PD_NM_MAX / 64;
        TIO t_qM[QM_IT];
        const TIO *src = qM + (valid ? env : 0) * ld.qM;
#pragma unroll
        for (int k = 0; k < QM_IT; ++k) {
            const int i = lane + 64 * k;
            t_qM[k] = (valid && i < m.nM) ? src[i] : TIO(0);
        }
#pragma unroll
        for (int k = 0; k < MAP_IT; ++k) {
            const int i = threadIdx.x + 256 * k;
            if (i < PD_NV * PD_NV) s_map[i] = t_map[k];
        }
#pragma unroll
        for (int k = 0; k < QM_IT; ++k) s_qM[wave][lane + 64 * k] = (double)t_qM[k];
    }
    __syncthreads();
    if (valid) {
        // same arithmetic as pd_rhs / pd_store
        double kp = 0.0, kd = 0.0, eq = 0.0;
        if (row >= 6) {
            kp = c_kp;
            kd = c_kd;
            const double target = c_ref + (double)r_a * c_scale;
            eq = (double)r_q - target;
        }
        const double qv = (double)r_v;
        double b = -(double)r_c - kp * eq - kd * qv;
        const double kd_dt = kd * m.sub_dt;
        double a[PD_NV];
#pragma unroll
        for (int j = 0; j < PD_NV; ++j) {
            const int id = s_map[row * PD_NV + j];
            double v = id >= 0 ? s_qM[wave][id] : 0.0;
            a[j] = v + (j == row ? kd_dt : 0.0);
        }
        double dinv = 0.0;
        tree_eliminate<PD_NV - 1>(a, b, dinv, row);
        const double qacc = b * dinv;
        if (lane < PD_NV && row >= 6) {
            const double ev = qv + qacc * m.sub_dt;
            const double tau = -kp * eq - kd * ev;
            const double tc = fmin(fmax(tau, -c_lim), c_lim);
            torque[env * m.nu + act] = (TIO)tc;
            if (torque_raw) torque_raw[env * m.nu + act] = (TIO)tau;
        }
    }
    if (done.counter) {
        // completion signal for a host that polls pinned memory instead of synchronising the stream: every wave
        // releases its torques system-wide, the block counts in; the last one publishes the launch's sequence number
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) {
            __threadfence_system();
            const unsigned prev = atomicAdd(done.counter, 1u);
            if (prev == gridDim.x - 1) {
                *done.counter = 0u;
                __threadfence_system();
                __hip_atomic_store(done.host_flag, done.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// cfg.action_type == 'torque' (humanoid_v1.py:167-172): torque = clip(a_ref + action * a_scale, +-torque_lim); nothing of
// the state enters. Same launch geometry and completion signal as the PD kernels it stands in for (4 envs per block).
template <typename TIO>
__global__ __launch_bounds__(256) void k_torque_direct(DevModel m, PdLd ld, const TIO *__restrict__ action, int n,
                                                       TIO *__restrict__ torque, TIO *__restrict__ torque_raw, PdDone done) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long env = (long)blockIdx.x * 4 + wave;
    if (env < n && lane < m.nu) {
        const double tau = m.a_ref[lane] + (double)action[env * ld.action + lane] * m.a_scale[lane];
        const double lim = m.torque_lim[lane];
        torque[env * m.nu + lane] = (TIO)fmin(fmax(tau, -lim), lim);
        if (torque_raw) torque_raw[env * m.nu + lane] = (TIO)tau;
    }
    if (done.counter) {
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) {
            __threadfence_system();
            const unsigned prev = atomicAdd(done.counter, 1u);
            if (prev == gridDim.x - 1) {
                *done.counter = 0u;
                __threadfence_system();
                __hip_atomic_store(done.host_flag, done.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// Generic path (any nv <= 64): one wavefront per env, system in LDS.
template <typename TIO>
__global__ __launch_bounds__(64) void k_pd_torque_lds(DevModel m, PdLd ld, const TIO *__restrict__ qpos,
                                                      const TIO *__restrict__ qvel, const TIO *__restrict__ action,
                                                      const TIO *__restrict__ qM, const TIO *__restrict__ C, int n,
                                                      TIO *__restrict__ torque, TIO *__restrict__ torque_raw) {
    extern __shared__ double s_dyn[];
    const int nv = m.nv, lda = nv + 1;
    double *A = s_dyn;            // [nv][ld]
    double *rhs = s_dyn + nv * lda; // [nv]
    const int lane = threadIdx.x;
    const long env = blockIdx.x;
    const int row = lane < nv ? lane : nv - 1;
    for (int i = lane; i < nv * lda; i += 64) A[i] = 0.0;
    __syncthreads();
    for (int i = lane; i < m.nM; i += 64) {
        const int r = m.m_row[i], c = m.m_col[i];
        const double v = (double)qM[env * ld.qM + i];
        A[r * lda + c] = v;
        A[c * lda + r] = v;
    }
    __syncthreads();
    double kp, kd, eq, qv, b;
    pd_rhs<TIO>(m, ld, qpos, qvel, action, C, env, row, kp, kd, eq, qv, b);
    if (lane < nv) {
        A[row * lda + row] += kd * m.sub_dt;
        rhs[row] = b;
    }
    __syncthreads();
    for (int k = 0; k < nv; ++k) {
        const double pk = A[k * lda + k];
        if (lane < nv && row != k) {
            const double f = A[row * lda + k] / pk;
            for (int j = k + 1; j < nv; ++j) A[row * lda + j] -= f * A[k * lda + j];
            rhs[row] -= f * rhs[k];
        }
        __syncthreads();
    }
    const double qacc = rhs[row] / A[row * lda + row];
    pd_store<TIO>(m, env, row, lane < nv, kp, kd, eq, qv, qacc, torque, torque_raw);
}

}  // namespace egp

using namespace egp;

template <typename T>
static int launch_pd(egp_ctx *ctx, const PdLd &ld, const T *qpos, const T *qvel, const T *action, const T *qM, const T *C, int n,
                     T *torque, T *torque_raw, hipStream_t stream, PdDone done = PdDone{nullptr, nullptr, 0}) {
    EGP_REQUIRE(ctx, "ctx is NULL");
    EGP_REQUIRE(n >= 0, "n < 0");
    if (n == 0) return EGP_OK;
    if (ctx->dm.action_torque) {        // action_type 'torque': no state, no inertia
        EGP_REQUIRE(action && torque, "NULL pointer");
        k_torque_direct<T><<<dim3((n + 3) / 4), dim3(256), 0, stream>>>(ctx->dm, ld, action, n, torque, torque_raw, done);
        return after_launch("k_torque_direct");
    }
    EGP_REQUIRE(qpos && qvel && action && qM && C && torque, "NULL pointer");
    if (ctx->pd_variant == 0 && ctx->pd_grid) {
        k_pd_torque_grid58<T><<<dim3((n + 3) / 4), dim3(256), 0, stream>>>(ctx->dm, ld, ctx->pd_grid_off, qpos, qvel, action, qM, C, n, torque, torque_raw, done);
        return after_launch("k_pd_torque_grid58");
    }
    if (ctx->pd_variant == 0) {
        k_pd_torque_tree58<T><<<dim3((n + 3) / 4), dim3(256), 0, stream>>>(ctx->dm, ld, qpos, qvel, action, qM, C, n, torque, torque_raw, done);
        return after_launch("k_pd_torque_tree58");
    }
    if (ctx->pd_variant == 2) {
        k_pd_torque_reg58<T><<<dim3((n + 3) / 4), dim3(256), 0, stream>>>(ctx->dm, ld, qpos, qvel, action, qM, C, n, torque, torque_raw);
        return after_launch("k_pd_torque_reg58");
    }
    const int nv = ctx->dm.nv;
    const size_t lds = ((size_t)nv * (nv + 1) + nv) * sizeof(double);
    k_pd_torque_lds<T><<<dim3(n), dim3(64), lds, stream>>>(ctx->dm, ld, qpos, qvel, action, qM, C, n, torque, torque_raw);
    return after_launch("k_pd_torque_lds");
}

static inline PdLd dense_ld(const egp_ctx *c) { return PdLd{c->dm.nq, c->dm.nv, c->dm.nu, c->dm.nM, c->dm.nv}; }

// engine entry: inputs live in the engine's staging layouts (row strides in doubles)
int egp_launch_pd_torque_strided(egp_ctx *ctx, const double *qpos, long ld_qpos, const double *qvel, long ld_qvel,
                                 const double *bias, long ld_bias, const double *qM, long ld_qM, const double *action,
                                 int32_t n, double *torque, hipStream_t stream, unsigned *done_counter,
                                 unsigned long long *host_flag, unsigned long long seq) {
    PdLd ld{ld_qpos, ld_qvel, ctx->dm.nu, ld_qM, ld_bias};
    PdDone done{ctx->pd_variant == 0 ? done_counter : nullptr, host_flag, seq};
    return launch_pd<double>(ctx, ld, qpos, qvel, action, qM, bias, n, torque, nullptr, stream, done);
}

extern "C" {

int egp_pd_torque_f64(egp_ctx *c, const double *qpos, const double *qvel, const double *action, const double *qM,
                      const double *bias, int32_t n, double *torque, double *torque_raw, void *s) {
    EGP_REQUIRE(c, "ctx is NULL");
    return launch_pd<double>(c, dense_ld(c), qpos, qvel, action, qM, bias, n, torque, torque_raw, (hipStream_t)s);
}
int egp_pd_torque_f32(egp_ctx *c, const float *qpos, const float *qvel, const float *action, const float *qM,
                      const float *bias, int32_t n, float *torque, float *torque_raw, void *s) {
    EGP_REQUIRE(c, "ctx is NULL");
    return launch_pd<float>(c, dense_ld(c), qpos, qvel, action, qM, bias, n, torque, torque_raw, (hipStream_t)s);
}

}  // extern "C"
