// K1, resident form ("K1 server") for the rollout engine: ONE launch covers all frame_skip substeps of an env-step, the
// workgroups wait on go words in pinned host memory. Three kernels with one signature, picked by (device dynamics, envs per
// wavefront) in server_kernel below:
//   k_pd_server_tree58<DYN>          one env per wavefront, 4 per workgroup; DYN: K8 (egp_dynamics_dev.hpp) inside the kernel
//   k_pd_server_tree58_multi<KE>     KE = 2 / 4 envs per wavefront, served in turn; the factors of M + Kd dt kept in LDS
//   k_pd_server_tree58_multi_dyn<KE> KE = 2 with K8 inside
// plus what they share (the host handshake, the epilogue, the torque store, the two-sweep solve), their dynamic-LDS layouts,
// the residency probe and the engine's entry points egp_pd_server_* / egp_launch_pd_server (egp_internal.hpp).
// The tree-ordered elimination and the PD arithmetic are egp_pd_dev.hpp's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>

#include <atomic>
#include <map>
#include <mutex>

#include "egp_internal.hpp"
#include "egp_dynamics_dev.hpp"
#include "egp_pd_dev.hpp"

namespace egp {

// Resident form of the tree kernel for the rollout engine ("K1 server"): ONE launch covers all frame_skip
// substeps of an env-step. The launch is cut into slices of whole blocks, each owned by one host physics thread.
// For every substep a block waits until its slice's `go` word (pinned host memory, written by the owner after it
// advanced the slice's envs) reaches the substep, reads the fresh state rows over PCIe, solves and writes the
// clipped torques straight into the pinned torque rows. There is no completion signal: the owner pre-fills the
// rows with a NaN sentinel before it raises `go` and steps an env as soon as its row holds no sentinel any more
// (clipped torques are never NaN), so the device side needs no fence, no counter and no flag write.
// What stays on the chip across substeps: the dof map, the gains, the action and the sparse inertia rows in LDS
// (re-read from the host rows only when the owner flags that some qM of the slice changed).
// No kernel launch, no stream sync and no group-wide barrier is left on the substep path.
struct PdServe {
    const int *block_slice;               // [gridDim.x]
    const unsigned long long *go;         // [n_slices * 8]  host; value = (substep sequence << 1) | refresh_qM
    unsigned long long base;              // sequence of substep 0 of this env-step
    int n_sub;
    const double *qM_host;                // device alias of the pinned inertia rows (same row stride as qM)
    double *qM_dev;                       // HBM inertia rows, refreshed together with LDS
    int *err;                             // host: set when a wait timed out
    long long timeout_ticks;              // wall_clock64 ticks (100 MHz)
    long long *trace;                     // optional [n_sub * 8] wall_clock64 stamps of block 0 (diagnostics)
    // epilogue (go word reaches base + n_sub: the slice's last physics step is drained): final state -> HBM
    const double *ee_host;                // [n][15] pinned end-effector rows (device alias)
    double *out_qpos, *out_prev_qpos, *out_qvel, *out_ee;   // HBM [n][nq] / [n][nq] / [n][nv] / [n][15]
    int nq, nv;
    int poll_sleep;                       // s_sleep(1) (64 clocks) repeats between two polls of a go word
    const int *active;                    // optional [n] (pinned host): envs with 0 are not stepped this env-step -- their waves
                                          // move no state, torque or epilogue rows (in a rollout's tail that is most of the PCIe traffic)
    const void *dyn;                      // DYN kernels: the egp_dyn::DynTables of the context (device)
    double *bias_dev;                     // DYN kernels: [n][nv] HBM bias rows -- with qM_dev what the env's last mj_step "left behind"
    unsigned *probe;                      // residency probe (egp_pd_server_resident_blocks): count the workgroups on the chip at once and leave
    const int *block_env0;                // multi-env kernels: [gridDim.x + 1] first env of every workgroup (the envs dealt out evenly)
    int row_contig;                       // qpos | qvel | bias are ONE row of nq + 2 nv doubles (the engine's state rows): read it as a
                                          // contiguous stream (see the substep loop)
};

// Poll a word of pinned host memory through the SCALAR memory path (s_load ... glc = always fetch from beyond the
// scalar cache). A vector load that is out on PCIe for ~2 us sits in the CU's in-order vector-memory return queue,
// and with a polling block on every CU that stalled the loads of every other kernel on the chip (a 17 us policy
// kernel took 160 us next to the polling engine); scalar loads do not go through that queue.
__device__ __forceinline__ unsigned long long scalar_poll_u64(const unsigned long long *p) {
    unsigned long long v;
    asm volatile("s_load_dwordx2 %0, %1, 0x0 glc\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory");
    return v;
}

__device__ __forceinline__ double sys_load_f64(const double *p) {
    const unsigned long long u = __hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return __longlong_as_double((long long)u);
}

// Residency probe: every workgroup that gets a place on the chip counts itself in, holds that place until all gridDim.x are there
// (probe[2] is raised) or `timeout_ticks` have passed, and counts itself out; probe[1] ends up as the largest head count any of them
// saw = the workgroups of THIS kernel (its registers, its LDS) the chip really holds at once -- under a CU mask, next to a co-tenant,
// on a part with CUs fused off -- where the occupancy calculator only knows the data sheet. The resident env-step needs that number.
__device__ __forceinline__ void server_residency_probe(const PdServe &sv) {
    if (threadIdx.x == 0) {
        unsigned present = atomicAdd(sv.probe, 1u) + 1u, best = present;
        const long long t0 = wall_clock64();
        for (;;) {
            if (present >= gridDim.x) { atomicExch(sv.probe + 2, 1u); break; }
            if (__hip_atomic_load(sv.probe + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;
            if (wall_clock64() - t0 > sv.timeout_ticks) break;
            __builtin_amdgcn_s_sleep(8);
            present = __hip_atomic_load(sv.probe, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            best = present > best ? present : best;
        }
        atomicMax(sv.probe + 1, best);
        atomicSub(sv.probe, 1u);
    }
}

// The host handshake of the resident kernels. Thread 0 waits until the slice's go word reaches sequence `want` (or for
// `timeout_ticks`), hands the word to the workgroup through `s_go_slot` and, where `trace` is given (block 0's substep waits),
// stamps the start and the end of the wait into trace[0] / trace[1]. The callers alternate between two slots (substep & 1): a wave
// that is still reading substep k's word cannot be overtaken by thread 0 writing substep k + 1's, which lands in the other slot,
// and thread 0 cannot reach substep k + 2's wait before every wave has passed the barrier of k + 1 -- so the ONE barrier in here is
// all a substep needs. A wait that timed out raises sv.err on the host and returns true: the whole workgroup must leave (the
// caller returns; `s_abort` is workgroup-wide and was cleared before the first wait).
__device__ __forceinline__ bool server_wait_go(const PdServe &sv, int slice, unsigned long long want, unsigned long long &s_go_slot,
                                               int &s_abort, long long *trace) {
    if (threadIdx.x == 0) {
        const long long t0 = wall_clock64();
        unsigned long long v;
        for (;;) {
            v = scalar_poll_u64(sv.go + slice * 8);
            if ((v >> 1) >= want) break;
            for (int z = 0; z < sv.poll_sleep; ++z) __builtin_amdgcn_s_sleep(1);
            if (wall_clock64() - t0 > sv.timeout_ticks) { s_abort = 1; break; }
        }
        s_go_slot = v;
        if (trace) { trace[0] = t0; trace[1] = wall_clock64(); }
    }
    __syncthreads();
    if (s_abort) {
        if (threadIdx.x == 0) __hip_atomic_store(sv.err, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        return true;
    }
    return false;
}

// Epilogue of one env, by the wave that served it, after the wait for sequence base + n_sub (the slice's last physics step is
// drained): prev_qpos <- qpos; qpos | qvel | ee_wpos <- the rows the owner left in pinned memory. `qpos` points at the state
// rows' qpos column (offset 0 of the row). The kernels run this slice by slice as the physics threads finish, so the env-step
// ends one PCIe round trip after the last physics call instead of a barrier + a copy launch later.
__device__ __forceinline__ void server_epilogue_env(const PdServe &sv, const PdLd &ld, const double *qpos, const double *qvel, long env,
                                                    int lane) {
    if (lane < sv.nq) {
        const long d = env * sv.nq + lane;
        const double q = sys_load_f64(qpos + env * ld.qpos + lane);
        sv.out_prev_qpos[d] = sv.out_qpos[d];
        sv.out_qpos[d] = q;
    }
    if (lane < sv.nv) sv.out_qvel[env * sv.nv + lane] = sys_load_f64(qvel + env * ld.qvel + lane);
    if (lane < 15) sv.out_ee[env * 15 + lane] = sys_load_f64(sv.ee_host + env * 15 + lane);
}

// clip(value, +-lim) into the pinned torque row. System-scope store: straight to the host's row, nothing lingers in a device
// cache -- the owner steps the env as soon as its row holds no NaN sentinel any more.
__device__ __forceinline__ void store_torque_clipped(double *torque, long index, double value, double lim) {
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(torque + index),
                       (unsigned long long)__double_as_longlong(fmin(fmax(value, -lim), lim)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// An env's inertia row changed on the host: from the pinned row `src` into the wave's LDS row and the HBM copy `dst` (the LDS
// row's padding behind nM is zeroed). All loads are issued before the first store.
__device__ __forceinline__ void refresh_inertia_row(const double *src, double *dst, double *lds_row, int nM, int lane) {
    constexpr int QM_IT = PD_NM_MAX / 64;
    double t_qM[QM_IT];
#pragma unroll
    for (int k = 0; k < QM_IT; ++k) {
        const int i = lane + 64 * k;
        t_qM[k] = i < nM ? sys_load_f64(src + i) : 0.0;
    }
#pragma unroll
    for (int k = 0; k < QM_IT; ++k) {
        const int i = lane + 64 * k;
        lds_row[i] = t_qM[k];
        if (i < nM) dst[i] = t_qM[k];
    }
}

// A solve of the multi-env kernels. They keep the factors of M + Kd dt = L^T D L in LDS in place of the env's sparse inertia row F:
// entry (K, r), r an ancestor of K, holds the multiplier of pivot K in row r, the diagonal entry 1 / D_K. Two sweeps over those
// 852 + 58 numbers: the lane's column of L for the sweep towards the root (entries (K, row), K a descendant: LDS index up(K)), then
// its row for the sweep back (entries (row, K), K an ancestor: lo(K)): 58 reads in flight at once each time, the entries that do
// not exist (and the other sweep's) read a zero slot of the row's padding -- no select, no LDS round trip on the dependent chain
// readlane -> fma (with the reads and a K > row select inside the sweeps a solve took 13, then 4 us; now as the one-env
// kernel's: ~2). Where the indices come from is the caller's: registers in k_pd_server_tree58_multi, LDS tables in _multi_dyn.
template <class UpIndex, class LoIndex>
__device__ __forceinline__ double tree_solve_two_sweeps(const double *F, int id_diag, double b, UpIndex up, LoIndex lo) {
    double cf[PD_NV];
#pragma unroll
    for (int K = 0; K < PD_NV; ++K) cf[K] = F[up(K)];
    const double d_own = F[id_diag];
#pragma unroll
    for (int K = PD_NV - 1; K >= 0; --K) b = fma(-cf[K], readlane_f64(b, K), b);      // L^T y = b: leaves -> root
    b *= d_own;
#pragma unroll
    for (int K = 0; K < PD_NV; ++K) cf[K] = F[lo(K)];
#pragma unroll
    for (int J = 0; J < PD_NV; ++J) b = fma(-cf[J], readlane_f64(b, J), b);           // L x = z: root -> leaves
    return b;
}

// The dynamic LDS of the two DYN kernels, in doubles from its start: the kernels address it and the host sizes it from these.
// k_pd_server_tree58<true>: the tree tables | K8 scratch per wave | per wave qpos[64] | qvel[64] | bias[64]
namespace dyn_lds {
constexpr size_t TB = (sizeof(egp_dyn::DynTables) + 7) / 8;
constexpr size_t SCR = TB, SCR_WAVE = egp_dyn::DY_ENV_DOUBLES;
constexpr size_t Q = SCR + 4 * SCR_WAVE, Q_ROW = 192;
constexpr size_t BYTES = (Q + 4 * Q_ROW) * sizeof(double);
}  // namespace dyn_lds
// k_pd_server_tree58_multi_dyn<KE>: tables | K8 scratch per wave | factor rows [4][KE][PD_NM_MAX] | state + bias rows [4][KE][192]
// | the sweeps' index tables, 2 x [PD_NV][64] shorts
namespace multi_dyn_lds {
constexpr size_t SCR = dyn_lds::TB, SCR_WAVE = egp_dyn::DY_ENV_DOUBLES;
constexpr size_t FAC = SCR + 4 * SCR_WAVE, Q_ROW = 192;
constexpr size_t q(int ke) { return FAC + (size_t)4 * ke * PD_NM_MAX; }
constexpr size_t idx(int ke) { return q(ke) + (size_t)4 * ke * Q_ROW; }
constexpr size_t bytes(int ke) { return idx(ke) * sizeof(double) + 2 * PD_NV * 64 * sizeof(short); }
}  // namespace multi_dyn_lds

// DYN (device_dynamics engines): the wave computes the inertia and the bias force itself from the (qpos, qvel) rows it reads
// (K8's wave function: FK + CRBA + RNE, egp_dynamics_dev.hpp) instead of taking qM / qfrc_bias from the host -- a backend whose
// inertia changes with every substep (MuJoCo's does) then sends 117 doubles per env-substep, not 1 085.
// With the reference's timing: compute_torque (ego_pose/envs/humanoid_v1.py:130-144) reads data.qM / data.qfrc_bias as the
// PREVIOUS mj_step left them -- evaluated at the state that step started from -- and only a reset's sim.forward()
// (envs/common/mujoco_env.py:97-101) makes them fresh. So substep k solves with the factors of M(q_{k-1}) and with C(q_{k-1}, v_{k-1})
// it already holds, stores the torque, and only THEN runs K8 + the factorisation on the row it has just read, for substep k + 1
// -- behind the host's physics step instead of in front of the torque. Across launches the env's (qM, bias) rows persist in
// HBM (qM_dev / bias_dev: written after the last substep, and by the engine's reset = sim.forward()). Needs the dynamic LDS.
template <bool DYN>
__global__ __launch_bounds__(256) void k_pd_server_tree58(DevModel m, PdLd ld, const double *qpos, const double *qvel,
                                                          const double *__restrict__ action, const double *qM, const double *C,
                                                          int n, double *torque, PdServe sv) {
    extern __shared__ double s_dynmem[];
    __shared__ short s_map[PD_NV * PD_NV];
    __shared__ double s_qM[4][PD_NM_MAX];
    __shared__ unsigned long long s_go[2];
    __shared__ int s_abort;
    if (sv.probe) { server_residency_probe(sv); return; }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long env = (long)blockIdx.x * 4 + wave;
    const bool valid = env < n;
    const int row = lane < PD_NV ? lane : PD_NV - 1;
    const int act = row >= 6 ? row - 6 : 0;
    const int slice = sv.block_slice[blockIdx.x];
    const bool live = valid && (!sv.active || sv.active[env] != 0);
    // a workgroup none of whose envs is stepped (finished slots: most of the grid in a rollout's tail) has nothing to solve, nothing
    // to hand back in the epilogue and nobody waiting for it: leave, instead of polling its slice's go word over PCIe for 15 substeps
    if (__syncthreads_or(live ? 1 : 0) == 0) return;
    const double r_a = valid ? action[env * ld.action + act] : 0.0;
    const double c_kp = row >= 6 ? m.jkp[act] : 0.0, c_kd = row >= 6 ? m.jkd[act] : 0.0;
    const double c_ref = m.a_ref[act], c_scale = m.a_scale[act], c_lim = m.torque_lim[act];
    constexpr int QM_IT = PD_NM_MAX / 64;
    {
        constexpr int MAP_IT = (PD_NV * PD_NV + 255) / 256;
        short t_map[MAP_IT];
#pragma unroll
        for (int k = 0; k < MAP_IT; ++k) {
            const int i = threadIdx.x + 256 * k;
            t_map[k] = i < PD_NV * PD_NV ? m.m_map[i] : (short)0;
        }
        double t_qM[QM_IT];
        const double *src = qM + (valid ? env : 0) * ld.qM;
#pragma unroll
        for (int k = 0; k < QM_IT; ++k) {
            const int i = lane + 64 * k;
            t_qM[k] = (valid && i < m.nM) ? src[i] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < MAP_IT; ++k) {
            const int i = threadIdx.x + 256 * k;
            if (i < PD_NV * PD_NV) s_map[i] = t_map[k];
        }
#pragma unroll
        for (int k = 0; k < QM_IT; ++k) s_qM[wave][lane + 64 * k] = t_qM[k];
    }
    // the dynamic LDS (dyn_lds) exists for DYN only: the other kernel is launched without any and forms no address in it
    egp_dyn::DynTables *tb = nullptr;
    double *s_scr = nullptr, *s_q = nullptr;
    if constexpr (DYN) {
        tb = reinterpret_cast<egp_dyn::DynTables *>(s_dynmem);
        s_scr = s_dynmem + dyn_lds::SCR + wave * dyn_lds::SCR_WAVE;                    // K8 scratch of this wave
        s_q = s_dynmem + dyn_lds::Q + wave * dyn_lds::Q_ROW;                           // qpos[64] | qvel[64] | bias[64]
    }
    if constexpr (DYN) {
        const int words = sizeof(egp_dyn::DynTables) / 4;
        const int *src = reinterpret_cast<const int *>(sv.dyn);
        int *dst = reinterpret_cast<int *>(tb);
        for (int i = threadIdx.x; i < words; i += 256) dst[i] = src[i];
    }
    if (threadIdx.x == 0) s_abort = 0;
    const double target = c_ref + r_a * c_scale;
    const bool tracer = sv.trace && blockIdx.x == 0 && threadIdx.x == 0;
    // (M + Kd dt) only changes when the owner flags a new inertia row: factor it then (and at substep 0), and run only
    // the right-hand side through the stored multipliers otherwise -- 9 us of elimination become 0.6 us per substep.
    double a[PD_NV];
    double dinv = 0.0;
    const double kd_dt = c_kd * m.sub_dt;
    double c_held = 0.0;                    // DYN: the bias entry of this lane's dof that the previous substep left behind
    double nx_q = 0.0, nx_v = 0.0;          // DYN: the next substep's state row, when it could be requested early
    bool have_next = false;
    auto factor_from_lds = [&]() {
#pragma unroll
        for (int j = 0; j < PD_NV; ++j) {
            const int id = s_map[row * PD_NV + j];
            double v = id >= 0 ? s_qM[wave][id] : 0.0;
            a[j] = v + (j == row ? kd_dt : 0.0);
        }
        tree_factor<PD_NV - 1>(a, dinv, row);
    };
    if constexpr (DYN) {
        // what the last env-step's final mj_step (or the reset's forward) left in HBM: factor it before the first go word
        __syncthreads();
        if (live && !m.action_torque) {
            c_held = C[env * ld.bias + row];
            factor_from_lds();
        }
    }
    for (int sub = 0; sub < sv.n_sub; ++sub) {
        if (server_wait_go(sv, slice, sv.base + (unsigned long long)sub, s_go[sub & 1], s_abort,
                           tracer ? sv.trace + sub * 8 : nullptr))
            return;
        const bool refresh = DYN || (s_go[sub & 1] & 1ull) != 0ull;
        if (live && m.action_torque) {          // action_type 'torque' (humanoid_v1.py:170-172): the clipped control itself
            if (lane < PD_NV && row >= 6) store_torque_clipped(torque, env * m.nu + act, target, c_lim);
        } else if (live) {
            double r_q, r_v, r_c;
            if constexpr (DYN) {
                if (have_next) {                // requested under the previous substep's factorisation (below)
                    if (lane < sv.nq) s_q[lane] = nx_q;
                    if (lane < sv.nv) s_q[64 + lane] = nx_v;
                } else {
                    if (lane < sv.nq) s_q[lane] = sys_load_f64(qpos + env * ld.qpos + lane);
                    if (lane < sv.nv) s_q[64 + lane] = sys_load_f64(qvel + env * ld.qvel + lane);
                }
                egp_dyn::wave_sync();
                r_q = s_q[7 + act]; r_v = s_q[64 + row]; r_c = c_held;
            } else if (sv.row_contig) {
                // The state row over PCIe, lane l taking doubles l, 64 + l, 128 + l: whole 64-byte lines, each once (22 for the
                // humanoid's 175 doubles). As three lane = dof segments (qpos + 7.., qvel, bias) the same row costs ~25 line reads,
                // the segments start mid-line -- tools/probes/pcie_read_probe.hip: 48 against 57 GB/s, and the full-activity
                // env-step is bound by exactly this traffic. The lanes then fetch their dof's three values with ds_bpermute.
                const double *rowp = qpos + env * ld.qpos;
                const int tot = sv.nq + 2 * sv.nv;
                const double c0 = lane < tot ? sys_load_f64(rowp + lane) : 0.0;
                const double c1 = 64 + lane < tot ? sys_load_f64(rowp + 64 + lane) : 0.0;
                const double c2 = 128 + lane < tot ? sys_load_f64(rowp + 128 + lane) : 0.0;
                auto pick = [&](int i) {
                    const double a0 = __shfl(c0, i & 63), a1 = __shfl(c1, i & 63), a2 = __shfl(c2, i & 63);
                    return i < 64 ? a0 : (i < 128 ? a1 : a2);
                };
                r_q = pick(7 + act);
                r_v = pick(sv.nq + row);
                r_c = pick(sv.nq + sv.nv + row);
            } else {
                r_q = sys_load_f64(qpos + env * ld.qpos + 7 + act);
                r_v = sys_load_f64(qvel + env * ld.qvel + row);
                r_c = sys_load_f64(C + env * ld.bias + row);
            }
            if (!DYN && refresh) refresh_inertia_row(sv.qM_host + env * ld.qM, sv.qM_dev + env * ld.qM, &s_qM[wave][0], m.nM, lane);
            if (!DYN && (sub == 0 || refresh)) factor_from_lds();      // (wave-uniform: the go word is per slice, the wave per env)
            const double eq = row >= 6 ? r_q - target : 0.0;
            double b = pd_rhs(r_c, c_kp, eq, c_kd, r_v);
            if (tracer) sv.trace[sub * 8 + 2] = b != 12345.678 ? wall_clock64() : 0;
            tree_solve<PD_NV - 1>(a, b);
            const double qacc = b * dinv;
            if (tracer) sv.trace[sub * 8 + 3] = qacc != 12345.678 ? wall_clock64() : 0;
            if (lane < PD_NV && row >= 6)
                store_torque_clipped(torque, env * m.nu + act, pd_torque(c_kp, eq, c_kd, r_v, qacc, m.sub_dt), c_lim);
            if (tracer) sv.trace[sub * 8 + 4] = wall_clock64();
            if constexpr (DYN) {
                // the torque is on its way and the host steps: now what that mj_step leaves behind for the NEXT compute_torque --
                // M and C at the state just read -- and its factors
                egp_dyn::dynamics_wave(*tb, s_scr, s_q, s_q + 64, lane, true, &s_qM[wave][0], s_q + 128, nullptr);
                egp_dyn::wave_sync();
                c_held = s_q[128 + row];
                // K8 took its 11 us: if the owner has raised the next go word meanwhile (with free physics it has; the rows were
                // written before the word, fenced), the next state row is requested NOW and crosses PCIe under the factorisation
                // instead of in front of the next solve (2.6 us of every 24.6 us substep in the rollout's tail)
                have_next = false;
                if (sub + 1 < sv.n_sub && (scalar_poll_u64(sv.go + slice * 8) >> 1) >= sv.base + (unsigned long long)sub + 1ull) {
                    nx_q = lane < sv.nq ? sys_load_f64(qpos + env * ld.qpos + lane) : 0.0;
                    nx_v = lane < sv.nv ? sys_load_f64(qvel + env * ld.qvel + lane) : 0.0;
                    have_next = true;
                }
                factor_from_lds();
                if (sub == sv.n_sub - 1) {       // ... and across launches
                    double *dst = sv.qM_dev + env * ld.qM;
#pragma unroll
                    for (int k = 0; k < QM_IT; ++k) {
                        const int i = lane + 64 * k;
                        if (i < m.nM) dst[i] = s_qM[wave][i];
                    }
                    if (lane < PD_NV) sv.bias_dev[env * ld.bias + row] = c_held;
                }
                if (tracer) sv.trace[sub * 8 + 5] = wall_clock64();
            }
        }
    }
    // epilogue: the final state to HBM once the slice's last physics step is drained
    if (server_wait_go(sv, slice, sv.base + (unsigned long long)sv.n_sub, s_go[sv.n_sub & 1], s_abort, nullptr)) return;
    if (live) server_epilogue_env(sv, ld, qpos, qvel, env, lane);
}

// KE envs per wavefront ("multi" form of the resident K1): the grid must fit the chip at once -- one 350-register workgroup per
// CU -- so beyond 4 envs per CU (1 024 slots on 256 CUs), or when fewer CUs are to be had, a wave serves its KE envs in turn in
// every substep. The wave's registers hold ONE env's factors while it eliminates; what the solves need is then kept in LDS in
// place of the env's inertia row, in the same sparse layout: entry (K, r), r an ancestor of K, holds the multiplier of pivot K in
// row r -- L[K][r] of M + Kd dt = L^T D L (the tree elimination's upper multipliers ARE Featherstone's L) -- and the diagonal
// entry 1 / D_K. A solve is two sweeps over those 852 + 58 numbers: leaves -> root through L^T, scale, root -> leaves through L
// (the one-env kernel keeps both triangles' multipliers in registers and needs one sweep: the two forms agree to rounding).
// All state rows of the wave's envs are requested before the first solve, so their PCIe round trips overlap.
template <int KE>
__global__ __launch_bounds__(256) void k_pd_server_tree58_multi(DevModel m, PdLd ld, const double *qpos, const double *qvel,
                                                                const double *__restrict__ action, const double *qM, const double *C,
                                                                int n, double *torque, PdServe sv) {
    extern __shared__ double s_fac[];                  // [4 waves][KE][PD_NM_MAX]
    __shared__ short s_map[PD_NV * PD_NV];
    __shared__ unsigned long long s_go[2];
    __shared__ int s_abort;
    if (sv.probe) { server_residency_probe(sv); return; }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = lane < PD_NV ? lane : PD_NV - 1;
    const int act = row >= 6 ? row - 6 : 0;
    const int slice = sv.block_slice[blockIdx.x];
    // the workgroup's envs [be0, be1) (at most 4 KE of them, dealt out evenly by the engine: with 4.5 envs per workgroup only every
    // second workgroup has a wave that serves two); wave w takes be0 + w, be0 + w + 4, ...
    const long be0 = sv.block_env0[blockIdx.x], be1 = sv.block_env0[blockIdx.x + 1];
    const long env0 = be0 + wave;
    bool live[KE];
    bool any = false;
#pragma unroll
    for (int e = 0; e < KE; ++e) {
        live[e] = env0 + 4 * e < be1 && env0 + 4 * e < n && (!sv.active || sv.active[env0 + 4 * e] != 0);
        any = any || live[e];
    }
    if (__syncthreads_or(any ? 1 : 0) == 0) return;
    const double c_kp = row >= 6 ? m.jkp[act] : 0.0, c_kd = row >= 6 ? m.jkd[act] : 0.0;
    const double c_ref = m.a_ref[act], c_scale = m.a_scale[act], c_lim = m.torque_lim[act];
    const double kd_dt = c_kd * m.sub_dt;
    double target[KE];
#pragma unroll
    for (int e = 0; e < KE; ++e) target[e] = c_ref + (live[e] ? action[(env0 + 4 * e) * ld.action + act] : 0.0) * c_scale;
    constexpr int QM_IT = PD_NM_MAX / 64;
    for (int i = threadIdx.x; i < PD_NV * PD_NV; i += 256) s_map[i] = m.m_map[i];
#pragma unroll
    for (int e = 0; e < KE; ++e) {
        double *F = s_fac + (size_t)(wave * KE + e) * PD_NM_MAX;
        const double *src = qM + (env0 + 4 * e) * ld.qM;
#pragma unroll
        for (int k = 0; k < QM_IT; ++k) {
            const int i = lane + 64 * k;
            F[i] = (live[e] && i < m.nM) ? src[i] : 0.0;
        }
    }
    if (threadIdx.x == 0) s_abort = 0;
    const int tot = sv.nq + 2 * sv.nv;
    const bool tracer = sv.trace && blockIdx.x == 0 && threadIdx.x == 0;
    // sparse index of entry (row, K) / (K, row) -- the same for every env -- or, where the tree has no such entry, a slot of the
    // row's padding that stays zero (nM = 910 of PD_NM_MAX = 960 doubles)
    constexpr int ZERO_SLOT = PD_NM_MAX - 1;
    short idv[PD_NV];
#pragma unroll
    for (int K = 0; K < PD_NV; ++K) {
        const short id = m.m_map[row * PD_NV + K];
        idv[K] = id >= 0 ? id : (short)ZERO_SLOT;
    }
    const int id_diag = m.m_map[row * PD_NV + row];
    auto up_index = [&](int K) { return K > row ? (int)idv[K] : ZERO_SLOT; };           // entry (K, row), K a descendant of the row
    auto lo_index = [&](int K) { return K < row ? (int)idv[K] : ZERO_SLOT; };           // entry (row, K), K an ancestor
    for (int sub = 0; sub < sv.n_sub; ++sub) {
        if (server_wait_go(sv, slice, sv.base + (unsigned long long)sub, s_go[sub & 1], s_abort,
                           tracer ? sv.trace + sub * 8 : nullptr))
            return;
        const bool refresh = (s_go[sub & 1] & 1ull) != 0ull;
        if (m.action_torque) {                  // action_type 'torque' (humanoid_v1.py:170-172): the clipped control itself
#pragma unroll
            for (int e = 0; e < KE; ++e)
                if (live[e] && lane < PD_NV && row >= 6) store_torque_clipped(torque, (env0 + 4 * e) * m.nu + act, target[e], c_lim);
            continue;
        }
        // every live env's state row first (whole 64-byte lines when the row is contiguous: see k_pd_server_tree58)
        double c0[KE], c1[KE], c2[KE];
#pragma unroll
        for (int e = 0; e < KE; ++e) {
            c0[e] = c1[e] = c2[e] = 0.0;
            if (!live[e]) continue;
            const long env = env0 + 4 * e;
            if (sv.row_contig) {
                const double *rowp = qpos + env * ld.qpos;
                if (lane < tot) c0[e] = sys_load_f64(rowp + lane);
                if (64 + lane < tot) c1[e] = sys_load_f64(rowp + 64 + lane);
                if (128 + lane < tot) c2[e] = sys_load_f64(rowp + 128 + lane);
            } else {
                c0[e] = sys_load_f64(qpos + env * ld.qpos + 7 + act);
                c1[e] = sys_load_f64(qvel + env * ld.qvel + row);
                c2[e] = sys_load_f64(C + env * ld.bias + row);
            }
        }
#pragma unroll
        for (int e = 0; e < KE; ++e) {
            if (!live[e]) continue;             // (wave-uniform)
            const long env = env0 + 4 * e;
            double *F = s_fac + (size_t)(wave * KE + e) * PD_NM_MAX;
            double r_q = c0[e], r_v = c1[e], r_c = c2[e];
            if (sv.row_contig) {
                auto pick = [&](int i) {
                    const double a0 = __shfl(c0[e], i & 63), a1 = __shfl(c1[e], i & 63), a2 = __shfl(c2[e], i & 63);
                    return i < 64 ? a0 : (i < 128 ? a1 : a2);
                };
                r_q = pick(7 + act);
                r_v = pick(sv.nq + row);
                r_c = pick(sv.nq + sv.nv + row);
            }
            if (refresh) {
                refresh_inertia_row(sv.qM_host + env * ld.qM, sv.qM_dev + env * ld.qM, F, m.nM, lane);
                egp_dyn::wave_sync();
            }
            if (sub == 0 || refresh) {
                double a[PD_NV];
                double dinv = 0.0;
#pragma unroll
                for (int j = 0; j < PD_NV; ++j) {
                    const int id = s_map[row * PD_NV + j];
                    const double v = id >= 0 ? F[id] : 0.0;
                    a[j] = v + (j == row ? kd_dt : 0.0);
                }
                tree_factor<PD_NV - 1>(a, dinv, row);
                egp_dyn::wave_sync();           // every lane has its row: the inertia entries may go
#pragma unroll
                for (int K = 0; K < PD_NV; ++K) {
                    const int id = s_map[row * PD_NV + K];
                    if (lane < PD_NV && K >= row && id >= 0) F[id] = K == row ? dinv : a[K];
                }
                egp_dyn::wave_sync();
            }
            const double eq = row >= 6 ? r_q - target[e] : 0.0;
            double b = pd_rhs(r_c, c_kp, eq, c_kd, r_v);
            if (tracer && e == 0) sv.trace[sub * 8 + 2] = b != 12345.678 ? wall_clock64() : 0;     // (stamps of block 0: its first env, then its last)
            b = tree_solve_two_sweeps(F, id_diag, b, up_index, lo_index);
            if (tracer && e == 0) sv.trace[sub * 8 + 3] = b != 12345.678 ? wall_clock64() : 0;
            if (lane < PD_NV && row >= 6)
                store_torque_clipped(torque, env * m.nu + act, pd_torque(c_kp, eq, c_kd, r_v, b, m.sub_dt), c_lim);
            if (tracer) sv.trace[sub * 8 + (e == 0 ? 4 : 5)] = wall_clock64();
        }
    }
    // epilogue: the final state of the wave's envs to HBM once the slice's last physics step is drained
    if (server_wait_go(sv, slice, sv.base + (unsigned long long)sv.n_sub, s_go[sv.n_sub & 1], s_abort, nullptr)) return;
#pragma unroll
    for (int e = 0; e < KE; ++e)
        if (live[e]) server_epilogue_env(sv, ld, qpos, qvel, env0 + 4 * e, lane);
}

// DYN form of the multi-env resident K1 (device_dynamics engines beyond one env per wave): K8 inside, as k_pd_server_tree58<true>
// has it, for KE envs per wave served in turn, as k_pd_server_tree58_multi has them. A sibling kernel rather than a template
// parameter of either: both keep the code they generate.
// Per substep: both envs' qpos | qvel rows are requested first (their PCIe round trips overlap); then every env's solve with the
// factors and the bias the PREVIOUS substep left behind (the reference's timing: see k_pd_server_tree58), its torque row stored;
// and only when ALL torques of the wave are out, env by env, K8 on the row just read + the in-place factorisation for the next
// substep -- the slice's physics thread waits for every torque of its slice, so ~22 us of K8 + factors per env sit behind the host's
// physics step, never in front of a torque.
// LDS (dynamic): the tree tables once per workgroup | one K8 scratch area per WAVE, which its envs share in time (it is dead once
// qM and the bias are written) | the factor rows [4][KE][PD_NM_MAX]: K8 writes the sparse inertia row straight into the env's row
// (the padding behind nM, the zero slot included, is never written), the factorisation replaces it in place | per env one
// qpos[64] | qvel[64] | bias[64] row: the state row just read and the bias the env's previous substep left behind | the sweeps'
// index tables, 2 x [PD_NV][64] shorts.
// For KE = 2: 9.9 + 50.7 + 61.4 + 12.3 + 14.8 kB = ~149 kB of the 160 KiB a workgroup may declare; KE = 4 would need ~223 kB and
// KE = 3 ~186 kB with float64 factors: not offered (pd_server_multi_dyn_lds_bytes).
// The early request of the next state row under the factorisation (have_next of the one-env kernel) is left out: with two envs per
// wave the second env's K8 already runs while the host steps, and a row requested before it would have to be held in registers
// across a whole K8.
template <int KE>
__global__ __launch_bounds__(256) void k_pd_server_tree58_multi_dyn(DevModel m, PdLd ld, const double *qpos, const double *qvel,
                                                                    const double *__restrict__ action, const double *qM, const double *C,
                                                                    int n, double *torque, PdServe sv) {
    extern __shared__ double s_dynmem[];
    __shared__ unsigned long long s_go[2];
    __shared__ int s_abort;
    if (sv.probe) { server_residency_probe(sv); return; }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = lane < PD_NV ? lane : PD_NV - 1;
    const int act = row >= 6 ? row - 6 : 0;
    const int slice = sv.block_slice[blockIdx.x];
    const long be0 = sv.block_env0[blockIdx.x], be1 = sv.block_env0[blockIdx.x + 1];
    const long env0 = be0 + wave;                      // wave w takes be0 + w, be0 + w + 4, ... (see k_pd_server_tree58_multi)
    bool live[KE];
    unsigned live_mask = 0u;            // (the same as bits, for the loops over the envs that are kept rolled)
#pragma unroll
    for (int e = 0; e < KE; ++e) {
        live[e] = env0 + 4 * e < be1 && env0 + 4 * e < n && (!sv.active || sv.active[env0 + 4 * e] != 0);
        live_mask |= live[e] ? 1u << e : 0u;
    }
    if (__syncthreads_or(live_mask != 0u ? 1 : 0) == 0) return;
    const double c_kp = row >= 6 ? m.jkp[act] : 0.0, c_kd = row >= 6 ? m.jkd[act] : 0.0;
    const double c_ref = m.a_ref[act], c_scale = m.a_scale[act], c_lim = m.torque_lim[act];
    const double kd_dt = c_kd * m.sub_dt;
    double target[KE];
#pragma unroll
    for (int e = 0; e < KE; ++e) target[e] = c_ref + (live[e] ? action[(env0 + 4 * e) * ld.action + act] : 0.0) * c_scale;
    constexpr int QM_IT = PD_NM_MAX / 64;
    egp_dyn::DynTables *tb = reinterpret_cast<egp_dyn::DynTables *>(s_dynmem);                         // (multi_dyn_lds)
    double *s_scr = s_dynmem + multi_dyn_lds::SCR + wave * multi_dyn_lds::SCR_WAVE;                    // K8 scratch of this wave
    double *s_fac = s_dynmem + multi_dyn_lds::FAC;                                                     // [4 waves][KE][PD_NM_MAX]
    double *s_q = s_dynmem + multi_dyn_lds::q(KE) + (size_t)wave * KE * multi_dyn_lds::Q_ROW;          // per env: qpos[64] | qvel[64] | bias[64]
    // sparse index of entry (K, lane's row) for the sweep towards the root (K a descendant: s_up) and of (row, K) for the sweep back
    // (K an ancestor: s_lo) -- the same for every env -- or, where the tree has no such entry, a slot of the row's padding that
    // stays zero (nM = 910 of PD_NM_MAX = 960 doubles). [K][lane], in the dynamic LDS on purpose: k_pd_server_tree58_multi keeps them
    // in registers, here the 116 addresses made from them would be carried across K8 and the elimination
    constexpr int ZERO_SLOT = PD_NM_MAX - 1;
    short *s_up = reinterpret_cast<short *>(s_dynmem + multi_dyn_lds::idx(KE));
    short *s_lo = s_up + PD_NV * 64;
    for (int i = threadIdx.x; i < PD_NV * 64; i += 256) {
        const int K = i >> 6, r = (i & 63) < PD_NV ? (i & 63) : PD_NV - 1;
        const short id = m.m_map[r * PD_NV + K];
        s_up[i] = (K > r && id >= 0) ? id : (short)ZERO_SLOT;
        s_lo[i] = (K < r && id >= 0) ? id : (short)ZERO_SLOT;
    }
    {
        const int words = sizeof(egp_dyn::DynTables) / 4;
        const int *src = reinterpret_cast<const int *>(sv.dyn);
        int *dst = reinterpret_cast<int *>(tb);
        for (int i = threadIdx.x; i < words; i += 256) dst[i] = src[i];
    }
    // what the env's last mj_step (the previous launch) or the reset's forward left in HBM
#pragma unroll
    for (int e = 0; e < KE; ++e) {
        double *F = s_fac + (size_t)(wave * KE + e) * PD_NM_MAX;
        const double *src = qM + (env0 + 4 * e) * ld.qM;
#pragma unroll
        for (int k = 0; k < QM_IT; ++k) {
            const int i = lane + 64 * k;
            F[i] = (live[e] && i < m.nM) ? src[i] : 0.0;
        }
    }
    if (threadIdx.x == 0) s_abort = 0;
    const bool tracer = sv.trace && blockIdx.x == 0 && threadIdx.x == 0;
    const int id_diag = m.m_map[row * PD_NV + row];
    const short *up_l = s_up + lane, *lo_l = s_lo + lane;       // (entry K of the lane: a constant offset from these)
    auto up_index = [&](int K) { return up_l[K * 64]; };
    auto lo_index = [&](int K) { return lo_l[K * 64]; };
    // the env's inertia row in F -> the factors of M + Kd dt in its place (k_pd_server_tree58_multi's layout)
    auto factor_in_place = [&](double *F) {
        double a[PD_NV];
        double dinv = 0.0;
#pragma unroll
        for (int j = 0; j < PD_NV; ++j) {       // (the row of the symmetric matrix: entry ids are below the zero slot, so min() picks the one that exists)
            const int up = up_l[j * 64], lo = lo_l[j * 64];
            const int id = j == row ? id_diag : (up < lo ? up : lo);
            a[j] = F[id] + (j == row ? kd_dt : 0.0);
        }
        tree_factor<PD_NV - 1>(a, dinv, row);
        egp_dyn::wave_sync();           // every lane has its row: the inertia entries may go
#pragma unroll
        for (int K = 0; K < PD_NV; ++K) {
            const int id = up_l[K * 64];
            if (lane < PD_NV && id != ZERO_SLOT) F[id] = a[K];
        }
        if (lane < PD_NV) F[id_diag] = dinv;
        egp_dyn::wave_sync();
    };
    __syncthreads();
    // before the first go word: the bias the env's last mj_step left behind into its held row, the factors of its inertia row.
    // (This loop and the K8 loop below stay rolled: one copy of K8 and of the elimination each, and no registers held across them.)
#pragma unroll 1
    for (int e = 0; e < KE; ++e) {
        if ((live_mask >> e & 1u) == 0u || m.action_torque) continue;       // (wave-uniform)
        if (lane < PD_NV) s_q[e * 192 + 128 + lane] = C[(env0 + 4 * e) * ld.bias + lane];
        factor_in_place(s_fac + (size_t)(wave * KE + e) * PD_NM_MAX);       // (its wave_syncs order the held row too)
    }
    for (int sub = 0; sub < sv.n_sub; ++sub) {
        if (server_wait_go(sv, slice, sv.base + (unsigned long long)sub, s_go[sub & 1], s_abort,
                           tracer ? sv.trace + sub * 8 : nullptr))
            return;
        if (m.action_torque) {                  // action_type 'torque' (humanoid_v1.py:170-172): the clipped control itself
#pragma unroll
            for (int e = 0; e < KE; ++e)
                if (live[e] && lane < PD_NV && row >= 6) store_torque_clipped(torque, (env0 + 4 * e) * m.nu + act, target[e], c_lim);
            continue;
        }
        // every live env's qpos | qvel row first, lane = index (the bias is not in the host row), into the env's LDS row
        {
            double rq[KE], rv[KE];
#pragma unroll
            for (int e = 0; e < KE; ++e) {
                rq[e] = rv[e] = 0.0;
                if (!live[e]) continue;
                const long env = env0 + 4 * e;
                if (lane < sv.nq) rq[e] = sys_load_f64(qpos + env * ld.qpos + lane);
                if (lane < sv.nv) rv[e] = sys_load_f64(qvel + env * ld.qvel + lane);
            }
#pragma unroll
            for (int e = 0; e < KE; ++e) {
                s_q[e * 192 + lane] = rq[e];
                s_q[e * 192 + 64 + lane] = rv[e];
            }
            egp_dyn::wave_sync();
        }
        // the torques of all envs of the wave ...
#pragma unroll
        for (int e = 0; e < KE; ++e) {
            if (!live[e]) continue;             // (wave-uniform)
            const long env = env0 + 4 * e;
            const double *F = s_fac + (size_t)(wave * KE + e) * PD_NM_MAX;
            const double r_q = s_q[e * 192 + 7 + act], r_v = s_q[e * 192 + 64 + row], r_c = s_q[e * 192 + 128 + row];
            const double eq = row >= 6 ? r_q - target[e] : 0.0;
            double b = pd_rhs(r_c, c_kp, eq, c_kd, r_v);
            if (tracer && e == 0) sv.trace[sub * 8 + 2] = b != 12345.678 ? wall_clock64() : 0;     // (stamps of block 0: its first env, then its last)
            b = tree_solve_two_sweeps(F, id_diag, b, up_index, lo_index);
            if (tracer && e == 0) sv.trace[sub * 8 + 3] = b != 12345.678 ? wall_clock64() : 0;
            if (lane < PD_NV && row >= 6)
                store_torque_clipped(torque, env * m.nu + act, pd_torque(c_kp, eq, c_kd, r_v, b, m.sub_dt), c_lim);
            if (tracer) sv.trace[sub * 8 + (e == 0 ? 4 : 5)] = wall_clock64();
        }
        // ... and then, while the host steps, what that mj_step leaves behind for the NEXT compute_torque of every env: M and C at
        // the state just read, and the factors
        egp_dyn::wave_sync();                   // (every lane has read its bias entries: K8 may replace them)
#pragma unroll 1
        for (int e = 0; e < KE; ++e) {
            if ((live_mask >> e & 1u) == 0u) continue;
            const long env = env0 + 4 * e;
            double *F = s_fac + (size_t)(wave * KE + e) * PD_NM_MAX;
            double *q = s_q + e * 192;
            egp_dyn::dynamics_wave(*tb, s_scr, q, q + 64, lane, true, F, q + 128, nullptr);
            egp_dyn::wave_sync();
            if (sub == sv.n_sub - 1) {          // across launches: the INERTIA row, before the factors take its place
                double *dst = sv.qM_dev + env * ld.qM;
#pragma unroll
                for (int k = 0; k < QM_IT; ++k) {
                    const int i = lane + 64 * k;
                    if (i < m.nM) dst[i] = F[i];
                }
                if (lane < PD_NV) sv.bias_dev[env * ld.bias + lane] = q[128 + lane];
            }
            factor_in_place(F);
        }
        if (tracer) sv.trace[sub * 8 + 6] = wall_clock64();
    }
    // epilogue: the final state of the wave's envs to HBM once the slice's last physics step is drained
    if (server_wait_go(sv, slice, sv.base + (unsigned long long)sv.n_sub, s_go[sv.n_sub & 1], s_abort, nullptr)) return;
#pragma unroll
    for (int e = 0; e < KE; ++e)
        if (live[e]) server_epilogue_env(sv, ld, qpos, qvel, env0 + 4 * e, lane);
}

}  // namespace egp

using namespace egp;

// the dynamic LDS of the DYN kernels: the layouts the kernels address (dyn_lds, multi_dyn_lds)
size_t egp_pd_server_dyn_lds_bytes() { return dyn_lds::BYTES; }
constexpr size_t pd_server_multi_dyn_lds_bytes(int ke) { return multi_dyn_lds::bytes(ke); }
// the static part: s_go, s_abort (rounded up). 160 KiB is what a gfx950 workgroup may declare; two envs per wave fit, three
// (~186 kB) and four (~223 kB) do not with float64 factors
constexpr size_t PD_SERVER_STATIC_LDS = 64;
static_assert(pd_server_multi_dyn_lds_bytes(2) + PD_SERVER_STATIC_LDS <= 160 * 1024, "k_pd_server_tree58_multi_dyn<2> does not fit the LDS");
static_assert(pd_server_multi_dyn_lds_bytes(3) + PD_SERVER_STATIC_LDS > 160 * 1024, "three envs per wave fit now: offer them");
size_t egp_pd_server_multi_dyn_lds_bytes(int envs_per_wave) { return pd_server_multi_dyn_lds_bytes(envs_per_wave); }

namespace {
// the resident K1's variants: (device dynamics, envs per wavefront) -> kernel, dynamic LDS
struct ServerKernel { const void *fn; size_t lds; };
ServerKernel server_kernel(bool device_dynamics, int ke) {
    const size_t multi = (size_t)4 * ke * PD_NM_MAX * sizeof(double);
    if (device_dynamics) {
        switch (ke) {
            case 1: return {reinterpret_cast<const void *>(&k_pd_server_tree58<true>), egp_pd_server_dyn_lds_bytes()};
            case 2: return {reinterpret_cast<const void *>(&k_pd_server_tree58_multi_dyn<2>), pd_server_multi_dyn_lds_bytes(2)};
            default: return {nullptr, 0};          // more envs per wave do not fit the LDS (see pd_server_multi_dyn_lds_bytes)
        }
    }
    switch (ke) {
        case 1: return {reinterpret_cast<const void *>(&k_pd_server_tree58<false>), 0};
        case 2: return {reinterpret_cast<const void *>(&k_pd_server_tree58_multi<2>), multi};
        case 4: return {reinterpret_cast<const void *>(&k_pd_server_tree58_multi<4>), multi};
        default: return {nullptr, 0};
    }
}
int server_kernel_prepare(const ServerKernel &k) {
    if (!k.fn) { set_error("no resident K1 for this (device dynamics, envs per wave) pair"); return EGP_E_INVALID; }
    if (k.lds > 0) {
        hipError_t e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds);
        if (e != hipSuccess) { (void)hipGetLastError(); set_error("hipFuncSetAttribute(resident K1, %zu B of LDS): %s", k.lds, hipGetErrorString(e)); return EGP_E_HIP; }
    }
    return EGP_OK;
}
}  // namespace

// whether the resident K1 exists in this variant at all (device dynamics: one or two envs per wave)
bool egp_pd_server_has_kernel(bool device_dynamics, int envs_per_wave) { return server_kernel(device_dynamics, envs_per_wave).fn != nullptr; }

// How many workgroups of the resident K1 (variant: device dynamics, `envs_per_wave`) the chip holds at once: the engine runs the
// resident form only when every workgroup of every group is resident at the same time -- they wait on the host, and a workgroup
// that is not resident cannot answer its slice's go word. The occupancy calculator's figure x the CUs is the data sheet's answer;
// the kernel itself, launched in probe mode (server_residency_probe), gives the one that holds on THIS device as this process
// sees it (EGP_SERVER_PROBE=0: calculator only). 0 when the kernel cannot run at all. Cached per (device, variant).
int egp_pd_server_resident_blocks(int device, bool device_dynamics, int envs_per_wave) {
    static std::mutex mu;
    static std::map<long, int> cache;
    std::lock_guard<std::mutex> lk(mu);
    const long key = ((long)device << 8) | ((long)envs_per_wave << 1) | (device_dynamics ? 1 : 0);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int result = 0;
    do {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess) { (void)hipGetLastError(); break; }
        const ServerKernel k = server_kernel(device_dynamics, envs_per_wave);
        if (!k.fn || server_kernel_prepare(k) != EGP_OK) break;
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.fn, 256, k.lds) != hipSuccess) { (void)hipGetLastError(); break; }
        result = per_cu * prop.multiProcessorCount;
        const char *pe = getenv("EGP_SERVER_PROBE");
        if (result <= 0 || (pe && atoi(pe) == 0)) break;
        unsigned *d_probe = nullptr;
        if (hipMalloc((void **)&d_probe, 4 * sizeof(unsigned)) != hipSuccess) { (void)hipGetLastError(); break; }
        unsigned h[4] = {0, 0, 0, 0};
        bool ok = hipMemset(d_probe, 0, sizeof(h)) == hipSuccess;
        if (ok) {
            PdServe sv{};
            sv.probe = d_probe;
            sv.timeout_ticks = 100000;           // 1 ms: a workgroup that is not on the chip by then is not resident
            DevModel dm{};
            PdLd ld{};
            void *args[] = {&dm, &ld, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &sv};
            const double *np = nullptr; double *npw = nullptr; int nn = 0;
            args[2] = &np; args[3] = &np; args[4] = &np; args[5] = &np; args[6] = &np; args[7] = &nn; args[8] = &npw;
            ok = hipLaunchKernel(k.fn, dim3(result), dim3(256), args, k.lds, nullptr) == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
                 hipMemcpy(h, d_probe, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess;
        }
        (void)hipFree(d_probe);
        if (!ok) { (void)hipGetLastError(); break; }
        if ((int)h[1] > 0 && (int)h[1] < result) result = (int)h[1];
    } while (false);
    cache[key] = result;
    return result;
}

// engine entry for the resident K1 (see k_pd_server_tree58); all flag arrays are device-visible addresses. `envs_per_wave` = 1: the
// one-env kernel (4 envs per workgroup); 2 / 4: k_pd_server_tree58_multi over `n_blocks` workgroups, workgroup b serving the envs
// [block_env0[b], block_env0[b + 1]) (at most 4 * envs_per_wave; block_slice has one entry per workgroup)
int egp_launch_pd_server(egp_ctx *ctx, const double *qpos, long ld_qpos, const double *qvel, long ld_qvel, const double *bias,
                         long ld_bias, const double *qM, long ld_qM, const double *qM_host, const double *action, int32_t n,
                         double *torque, hipStream_t stream, const int *block_slice, const unsigned long long *go,
                         unsigned long long base, int n_sub, int *err, double timeout_s, long long *trace, const double *ee_host,
                         double *out_qpos, double *out_prev_qpos, double *out_qvel, double *out_ee, const int *active, bool device_dynamics,
                         int envs_per_wave, const int *block_env0, int n_blocks) {
    EGP_REQUIRE(ctx && ctx->tree58 && ctx->pd_variant == 0, "the K1 server needs the humanoid tree kernel");
    EGP_REQUIRE(!device_dynamics || ctx->dyn_tables, "device dynamics needs egp_set_dynamics_model on the context");
    EGP_REQUIRE(ee_host && out_qpos && out_prev_qpos && out_qvel && out_ee, "NULL epilogue pointer");
    EGP_REQUIRE(ctx->dm.nq <= 64 && ctx->dm.nv <= 64, "the epilogue moves one state row per wavefront");
    EGP_REQUIRE(qpos && qvel && bias && qM && qM_host && action && torque && block_slice && go && err, "NULL pointer");
    EGP_REQUIRE(n > 0 && n_sub > 0, "n and n_sub must be positive");
    const ServerKernel k = server_kernel(device_dynamics, envs_per_wave);
    EGP_REQUIRE(k.fn, "no resident K1 for this (device dynamics, envs per wave) pair");
    EGP_REQUIRE(envs_per_wave == 1 || ctx->dm.nM < PD_NM_MAX, "the multi-env K1 keeps a zero slot behind the inertia row");
    {
        static std::atomic<int> prepared[2][5];          // (the LDS attribute once per variant; egp_pd_server_resident_blocks set it already)
        std::atomic<int> &pf = prepared[device_dynamics ? 1 : 0][envs_per_wave];
        if (pf.load(std::memory_order_acquire) == 0) {
            const int rc = server_kernel_prepare(k);
            if (rc != EGP_OK) return rc;
            pf.store(1, std::memory_order_release);
        }
    }
    PdLd ld{ld_qpos, ld_qvel, ctx->dm.nu, ld_qM, ld_bias};
    const int poll_sleep = 2;          // s_sleep(1) repeats between two polls of a go word
    const int nq = ctx->dm.nq, nv = ctx->dm.nv;
    // (the engine's state rows are qpos | qvel | bias back to back: read as one contiguous stream; separate arrays: three segments)
    const int row_contig = !device_dynamics && qvel == qpos + nq && bias == qvel + nv && ld_qpos == ld_qvel &&
                           ld_qvel == ld_bias && nq + 2 * nv <= 192 && ld_qpos >= nq + 2 * nv;
    PdServe sv{block_slice, go, base, n_sub, qM_host, const_cast<double *>(qM), err, (long long)(timeout_s * 100.0e6), trace,
               ee_host, out_qpos, out_prev_qpos, out_qvel, out_ee, nq, nv, poll_sleep, active, ctx->dyn_tables,
               device_dynamics ? const_cast<double *>(bias) : nullptr, nullptr, block_env0, row_contig};
    EGP_REQUIRE(envs_per_wave == 1 || (block_env0 && n_blocks > 0), "the multi-env K1 needs the workgroups' env ranges");
    const dim3 grid(envs_per_wave == 1 ? (n + 3) / 4 : n_blocks);
    int n_envs = n;
    void *args[] = {&ctx->dm, &ld, &qpos, &qvel, &action, &qM, &bias, &n_envs, &torque, &sv};       // (the kernels' common signature)
    EGP_HIP_CHECK(hipLaunchKernel(k.fn, grid, dim3(256), args, k.lds, stream));
    return after_launch("k_pd_server_tree58");
}
