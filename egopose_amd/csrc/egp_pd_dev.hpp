// Device pieces shared by the K1 translation units (egp_pd.hip: one launch per substep; egp_pd_server.hip: the resident form)
// and the lane-grid kernel's header (egp_pd_grid.hpp): the launch descriptors, the 64-bit cross-lane read, the compiled-in
// humanoid dof tree with the tree-ordered elimination on "lane i owns row i", and the stable-PD right-hand side and torque.
//
// compute_torque / compute_desired_accel (ego_pose/envs/humanoid_v1.py:130-156) + clip (:172)
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "egp_internal.hpp"

namespace egp {

__device__ __forceinline__ double readlane_f64(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// row strides (in elements) of the five K1 inputs: dense C-ABI arrays use (nq, nv, nu, nM, nv); the
// rollout engine passes its packed per-env staging row instead
struct PdLd { long qpos, qvel, action, qM, bias; };
// optional completion signal of a K1 launch (counter in HBM, flag in pinned host memory)
struct PdDone { unsigned *counter; unsigned long long *host_flag; unsigned long long seq; };

// Fast path for the humanoid (nv == 58): 4 envs per 256-thread block, one wavefront each.
constexpr int PD_NV = 58;
constexpr int PD_NM_MAX = 960;   // >= nM (910)

// Stable PD (humanoid_v1.py:130-144), per dof: the right-hand side of (M + Kd dt) qacc = -C - Kp eq - Kd qvel, and the torque
// from the solved acceleration. The expression order is part of the result (bit-identical across the kernels).
// Two forms of the same arithmetic. pd_rhs<TIO> / pd_store<TIO> read the dof's inputs from the arrays and write its torque
// themselves: k_pd_torque_reg58 and k_pd_torque_lds. The scalar pd_rhs / pd_torque take values the kernel already holds in
// registers: the three resident kernels (k_pd_server_tree58*). k_pd_torque_tree58 and k_pd_torque_grid58 write the same
// expressions out in their bodies, next to the loads they issue early.
template <typename TIO>
__device__ __forceinline__ void pd_rhs(const DevModel &m, const PdLd &ld, const TIO *qpos, const TIO *qvel, const TIO *action,
                                       const TIO *C, long env, int row, double &kp, double &kd, double &eq,
                                       double &qv, double &b) {
    kp = 0.0; kd = 0.0; eq = 0.0;
    if (row >= 6) {
        const int a = row - 6;
        kp = m.jkp[a];
        kd = m.jkd[a];
        const double target = m.a_ref[a] + (double)action[env * ld.action + a] * m.a_scale[a];
        eq = (double)qpos[env * ld.qpos + 7 + a] - target;
    }
    qv = (double)qvel[env * ld.qvel + row];
    b = -(double)C[env * ld.bias + row] - kp * eq - kd * qv;
}

template <typename TIO>
__device__ __forceinline__ void pd_store(const DevModel &m, long env, int row, bool owner, double kp, double kd,
                                         double eq, double qv, double qacc, TIO *torque, TIO *torque_raw) {
    if (owner && row >= 6) {
        const int a = row - 6;
        const double ev = qv + qacc * m.sub_dt;
        const double tau = -kp * eq - kd * ev;
        const double lim = m.torque_lim[a];
        const double tc = fmin(fmax(tau, -lim), lim);
        torque[env * m.nu + a] = (TIO)tc;
        if (torque_raw) torque_raw[env * m.nu + a] = (TIO)tau;
    }
}

__device__ __forceinline__ double pd_rhs(double r_c, double kp, double eq, double kd, double r_v) { return -r_c - kp * eq - kd * r_v; }
__device__ __forceinline__ double pd_torque(double kp, double eq, double kd, double r_v, double qacc, double sub_dt) {
    const double ev = r_v + qacc * sub_dt;
    return -kp * eq - kd * ev;
}

// Tree-ordered elimination (default for the humanoid): lane i owns row i, and the dofs are eliminated
// leaves -> root (descending index). When dof k is the pivot, every descendant column of row k has already
// been zeroed, so row k is non-zero only on k's ANCESTOR columns: a pivot step updates |anc(k)| columns
// instead of all remaining ones (852 + 58 row updates instead of 1711 + 58; MuJoCo's L^T D L sparsity,
// no fill-in). The ancestor chains are compile-time tables (egp_tree58.inc, generated from the skeleton asset),
// so every register index stays static; egp_create checks the runtime dof tree against them.
#include "egp_tree58.inc"

__device__ __forceinline__ double fast_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);          // v_rcp_f64 + two Newton steps: <= 1 ulp for normal x
    double e = fma(-x, r, 1.0);
    r = fma(r, e, r);
    e = fma(-x, r, 1.0);
    return fma(r, e, r);
}

template <int K, int... T>
__device__ __forceinline__ void tree_pivot_update(double (&a)[PD_NV], double f, std::integer_sequence<int, T...>) {
    if constexpr (sizeof...(T) > 0) {
        // all broadcasts first (v_readlane -> SGPR pairs), then the FMAs: no SGPR-hazard nops in between
        const double r[sizeof...(T)] = {readlane_f64(a[Tree58::ANC[K][T]], K)...};
        __builtin_amdgcn_sched_barrier(0);
        ((a[Tree58::ANC[K][T]] = fma(-f, r[T], a[Tree58::ANC[K][T]])), ...);
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int K>
__device__ __forceinline__ void tree_eliminate(double (&a)[PD_NV], double &b, double &dinv, int row) {
    const double pk = readlane_f64(a[K], K);
    const double inv = fast_rcp(pk);
    const bool me = row == K;
    const double f = me ? 0.0 : a[K] * inv;
    dinv = me ? inv : dinv;
    tree_pivot_update<K>(a, f, std::make_integer_sequence<int, Tree58::NANC[K]>{});
    const double bk = readlane_f64(b, K);
    b = fma(-f, bk, b);
    if constexpr (K > 0) tree_eliminate<K - 1>(a, b, dinv, row);
}

// The same elimination split in two: the matrix work once (the multiplier of pivot K replaces column K of the lane's
// row, like L stored in place), the right-hand side per solve. The operations on b are exactly those of tree_eliminate,
// in the same order, so factor + solve is bit-identical to the one-pass form.
template <int K>
__device__ __forceinline__ void tree_factor(double (&a)[PD_NV], double &dinv, int row) {
    const double pk = readlane_f64(a[K], K);
    const double inv = fast_rcp(pk);
    const bool me = row == K;
    const double f = me ? 0.0 : a[K] * inv;
    dinv = me ? inv : dinv;
    tree_pivot_update<K>(a, f, std::make_integer_sequence<int, Tree58::NANC[K]>{});
    a[K] = f;                       // column K is dead from here on (no later pivot has K among its ancestors)
    if constexpr (K > 0) tree_factor<K - 1>(a, dinv, row);
}

template <int K>
__device__ __forceinline__ void tree_solve(const double (&a)[PD_NV], double &b) {
    const double bk = readlane_f64(b, K);
    b = fma(-a[K], bk, b);
    if constexpr (K > 0) tree_solve<K - 1>(a, b);
}

}  // namespace egp
