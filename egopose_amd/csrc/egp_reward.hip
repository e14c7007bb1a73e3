// K2 (the imitation reward), the two small entries of the reward registry (k_reward_simple) and K7 (the pose features of a frame
// pair), with their C-ABI entry points egp_reward_* / egp_pose_features_* declared in include/egopose_hip.h. One file because the
// per-lane feature helpers (body_feature, root_velocity, coord_vec, ee_local) serve both K2 and K7.
//
// Every per-env array is env-major and row-contiguous (qpos[n][nq], ee_wpos[n][15], ...); the shared skeleton tables
// (body -> qpos map, per-body weights) are staged in LDS.
//   K2 k_reward_quat_v3   a workgroup owns a tile of envs, two phases: lane = (env, body) for the pose / angular-velocity terms,
//                         then lane = env for the root terms and lane = (env, end effector); see reward_body.
//   K7 k_pose_features    one half-wavefront per env: lane = body, lane 0 = root terms, 5 lanes = end effectors.
#include <hip/hip_runtime.h>
#include <math.h>

#include "egp_internal.hpp"
#include "egp_quat.hpp"

namespace egp {

// ============================================================================================ K2
// quat_space_reward_v3 (ego_pose/core/reward_function.py:4-60)
// (the packed expert row and its offsets ER_*: egp_internal.hpp)

template <typename T>
__device__ __forceinline__ T half_wave_sum(T v) {
    v += __shfl_xor(v, 16, 32);
    v += __shfl_xor(v, 8, 32);
    v += __shfl_xor(v, 4, 32);
    v += __shfl_xor(v, 2, 32);
    v += __shfl_xor(v, 1, 32);
    return v;
}

// ---- per-lane feature helpers shared by the reward kernel (K2) and the feature kernel (K7)
// body lane: orientation of one non-root body now and one step ago, and its finite-difference angular
// velocity rotation_from_quaternion(q_t q_{t-1}^-1)/dt  (get_angvel_fd, utils/math.py:38-44)
template <typename T>
__device__ __forceinline__ void body_feature(const T *cq, const T *pq, int s, int nd, T dt, Q4<T> *qc, V3<T> *omega) {
    const T c0 = nd > 0 ? cq[s] : T(0), c1 = nd > 1 ? cq[s + 1] : T(0), c2 = nd > 2 ? cq[s + 2] : T(0);
    const T p0 = nd > 0 ? pq[s] : T(0), p1 = nd > 1 ? pq[s + 1] : T(0), p2 = nd > 2 ? pq[s + 2] : T(0);
    *qc = q_from_euler_sxyz<T>(c0, c1, c2);
    const Q4<T> qp = q_from_euler_sxyz<T>(p0, p1, p2);   // == env.prev_bquat (humanoid_v1.py:184,188)
    const Q4<T> dv = qmul(*qc, qinv(qp));
    V3<T> ax; T ang;
    rot_axis_angle<T>(dv, &ax, &ang);
    if (sizeof(T) == 8) {          // (float64: one division instead of three, see qinv)
        const T rate = ang / dt;
        omega->x = ax.x * rate; omega->y = ax.y * rate; omega->z = ax.z * rate;
    } else {
        omega->x = ax.x * ang / dt; omega->y = ax.y * ang / dt; omega->z = ax.z * ang / dt;
    }
}

// root lane: get_qvel_fd(prev, cur, dt) root part (utils/math.py:20-35): world-frame linear velocity `v`,
// root-frame angular velocity `rv` (frame of the PREVIOUS root quaternion, angle wrapped to (-pi, pi])
template <typename T>
__device__ __forceinline__ void root_velocity(const T *cq, const T *pq, T dt, V3<T> *v, V3<T> *rv) {
    const Q4<T> rc{cq[3], cq[4], cq[5], cq[6]};
    const Q4<T> rp{pq[3], pq[4], pq[5], pq[6]};
    v->x = (cq[0] - pq[0]) / dt; v->y = (cq[1] - pq[1]) / dt; v->z = (cq[2] - pq[2]) / dt;
    const Q4<T> qrel = qmul(rc, qinv(rp));
    V3<T> ax; T ang;
    rot_axis_angle<T>(qrel, &ax, &ang);
    const T pi = T(3.14159265358979323846);
    if (ang > pi) ang -= T(2) * pi;
    else if (ang < -pi) ang += T(2) * pi;
    const V3<T> rvw{ax.x * ang / dt, ax.y * ang / dt, ax.z * ang / dt};
    *rv = rotate_T(rp, rvw);
}

// transform_vec(v, q, cfg.obs_coord) (utils/math.py:47-59): R(q)^T v in the 'root' frame, R(heading_q(q))^T v in the 'heading' frame
template <typename T>
__device__ __forceinline__ V3<T> coord_vec(const Q4<T> &q, const V3<T> &v, bool root_frame) {
    return rotate_T(root_frame ? q : heading_q(q), v);
}

// end-effector lane: world position -> root-relative, in the frame cfg.obs_coord names (get_ee_pos(transform),
// humanoid_v1.py:98-111; the reward passes cfg.obs_coord, reward_function.py:23; gen_expert.py:18-22 always 'heading')
template <typename T>
__device__ __forceinline__ V3<T> ee_local(const T *cq, const T *wp, bool root_frame) {
    const Q4<T> rc{cq[3], cq[4], cq[5], cq[6]};
    const V3<T> rel{wp[0] - cq[0], wp[1] - cq[1], wp[2] - cq[2]};
    return coord_vec(rc, rel, root_frame);
}

// Work split (round 3). A wavefront used to carry two envs, lane = body, with lane 0 doing the root terms and five lanes the end
// effectors: three divergent branches that run one after the other, the ~1 000-instruction root branch with ONE lane per env
// active (the kernel is float64-VALU bound: VALUBusy 87 %, 18.6 % of HBM peak at 65 536 envs). Now a workgroup owns a tile of
// envs and works in two phases: (1) lane = (env, body): pose and angular-velocity terms of every body into LDS; (2) lane = env
// for the root terms, lane = (env, end effector) on the other waves, then lane = env adds up the bodies' terms and combines the
// five parts. With multi-pass tiles (PASSES = 5: 60 envs for the humanoid, large batches) the root branch runs once per tile
// with nearly every lane busy instead of once per two envs; rollout-sized batches keep one-pass tiles (12 envs: the latency of
// a tick's reward is unchanged).
// Phase 1 packs as many envs into a wavefront as its 64 lanes hold bodies (three for the humanoid's 20 non-root bodies, 60 of
// 64 lanes busy instead of 40): a pass of the workgroup covers 4 * (64 / (nbody - 1)) envs, the per-body terms go to LDS and
// phase 2's env lane adds them up in body order.
__host__ __device__ inline int reward_envs_per_wave(int nbody) { return nbody > 1 ? (64 / (nbody - 1) > 0 ? 64 / (nbody - 1) : 1) : 1; }
__host__ __device__ inline int reward_tile_envs(int nbody, int passes) {
    const int t = 4 * reward_envs_per_wave(nbody) * passes, cap = passes == 1 ? 16 : 64;     // (cap = the tile arrays' capacity)
    return t < cap ? t : cap;
}
template <typename T, int PASSES>
__device__ __forceinline__ void reward_body(const DevModel &m, const RewardW &w, const T *__restrict__ expert_rows,
                                            const T *__restrict__ cur_qpos, const T *__restrict__ prev_qpos,
                                            const T *__restrict__ ee_wpos, const int *__restrict__ tcur,
                                            const int *__restrict__ frame, const int *__restrict__ endf,
                                            const int *__restrict__ active, T end_reward, int n,
                                            T *__restrict__ reward, T *__restrict__ cinfo, int block_id) {
    constexpr int ENVS = PASSES == 1 ? 16 : 64;                    // capacity of the tile arrays; the tile itself: reward_tile_envs
    __shared__ int s_start[EGP_MAX_BODY], s_ndof[EGP_MAX_BODY];
    __shared__ double s_bw[EGP_MAX_BODY];
    __shared__ T s_bp[ENVS][EGP_MAX_BODY], s_bv[ENVS][EGP_MAX_BODY];      // per-body pose / angular-velocity terms
    __shared__ T s_rp[ENVS], s_rv[ENVS], s_ee[ENVS][5];
    if (threadIdx.x < m.nbody) {
        s_start[threadIdx.x] = m.body_qpos_start[threadIdx.x];
        s_ndof[threadIdx.x] = m.body_ndof[threadIdx.x];
        s_bw[threadIdx.x] = threadIdx.x > 0 ? m.b_diffw[threadIdx.x - 1] : 0.0;
    }
    __syncthreads();
    const int per = m.nbody - 1, epw = reward_envs_per_wave(m.nbody), tile = reward_tile_envs(m.nbody, PASSES);
    const long env0 = (long)block_id * tile;
    const T dt = (T)m.dt;
    // ---- phase 1: lane = (env of the wavefront, body)
    {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        const int sub = lane / per, bl = lane - sub * per;
#pragma unroll 1
        for (int ps = 0; ps < PASSES; ++ps) {
            const int el = (ps * 4 + wv) * epw + sub;
            const long env = env0 + el;
            if (sub >= epw || el >= tile) continue;
            T pose_sq = T(0), vel_acc = T(0);
            if (env < n && (!active || active[env])) {
                const int l = 1 + bl;
                const T *cq = cur_qpos + env * m.nq;
                const T *pq = prev_qpos + env * m.nq;
                const T *er = expert_rows + (long)frame[env] * EGP_EXPERT_ROW;
                Q4<T> qc; V3<T> om;
                body_feature<T>(cq, pq, s_start[l], s_ndof[l], dt, &qc, &om);
                const T *eb = er + ER_BQ + 4 * (l - 1);
                const Q4<T> qe{eb[0], eb[1], eb[2], eb[3]};
                const T pd = half_angle<T>(qmul(qc, qinv(qe))) * (T)s_bw[l];
                pose_sq = pd * pd;
                const T *ev = er + ER_BAV + 3 * (l - 1);
                const T dx = om.x - ev[0], dy = om.y - ev[1], dz = om.z - ev[2];
                if (w.v_ord == 2.0) {
                    vel_acc = dx * dx + dy * dy + dz * dz;
                } else {
                    const T p = (T)w.v_ord;
                    vel_acc = t_pow<T>(fabs(dx), p) + t_pow<T>(fabs(dy), p) + t_pow<T>(fabs(dz), p);
                }
            }
            s_bp[el][bl] = pose_sq;
            s_bv[el][bl] = vel_acc;
        }
    }
    __syncthreads();
    // ---- phase 2: lane = env (root terms, threads [0, ENVS)), lane = (env, end effector) (threads [64, 256))
    if (threadIdx.x < tile) {
        const long env = env0 + threadIdx.x;
        T rp_r = T(0), rv_r = T(0);
        if (env < n && (!active || active[env])) {
            const T *cq = cur_qpos + env * m.nq;
            const T *pq = prev_qpos + env * m.nq;
            const T *er = expert_rows + (long)frame[env] * EGP_EXPERT_ROW;
            V3<T> v, rv;
            root_velocity<T>(cq, pq, dt, &v, &rv);
            const Q4<T> rp{pq[3], pq[4], pq[5], pq[6]};
            // learner: get_qvel_fd(prev, cur, dt, cfg.obs_coord) (reward_function.py:19): frame of the PREVIOUS root quat
            const V3<T> vl = coord_vec(rp, v, m.obs_root != 0);
            const T dl = (vl.x - er[ER_RLINV]) * (vl.x - er[ER_RLINV]) + (vl.y - er[ER_RLINV + 1]) * (vl.y - er[ER_RLINV + 1]) +
                         (vl.z - er[ER_RLINV + 2]) * (vl.z - er[ER_RLINV + 2]);
            const T da = (rv.x - er[ER_RANGV]) * (rv.x - er[ER_RANGV]) + (rv.y - er[ER_RANGV + 1]) * (rv.y - er[ER_RANGV + 1]) +
                         (rv.z - er[ER_RANGV + 2]) * (rv.z - er[ER_RANGV + 2]);
            rv_r = t_exp<T>(-(T)w.k_rl * dl - (T)w.k_ra * da);
            const Q4<T> rc{cq[3], cq[4], cq[5], cq[6]};
            const Q4<T> rq = de_heading(rc);
            const Q4<T> erq{er[ER_RQ], er[ER_RQ + 1], er[ER_RQ + 2], er[ER_RQ + 3]};
            const T dq = half_angle<T>(qmul(rq, qinv(erq)));
            const T dh = cq[2] - er[ER_Z];
            rp_r = t_exp<T>(-(T)w.k_rh * dh * dh - (T)w.k_rq * dq * dq);
        }
        s_rp[threadIdx.x] = rp_r;
        s_rv[threadIdx.x] = rv_r;
    } else if (threadIdx.x >= 64) {
        for (int i = threadIdx.x - 64; i < 5 * tile; i += 192) {
            const int el = i / 5, k = i - 5 * el;
            const long env = env0 + el;
            T ee_sq = T(0);
            if (env < n && (!active || active[env])) {
                const T *cq = cur_qpos + env * m.nq;
                const T *er = expert_rows + (long)frame[env] * EGP_EXPERT_ROW;
                const V3<T> o = ee_local<T>(cq, ee_wpos + env * 15 + 3 * k, m.obs_root != 0);
                const T *ee = er + ER_EE + 3 * k;
                ee_sq = (o.x - ee[0]) * (o.x - ee[0]) + (o.y - ee[1]) * (o.y - ee[1]) + (o.z - ee[2]) * (o.z - ee[2]);
            }
            s_ee[el][k] = ee_sq;
        }
    }
    __syncthreads();
    if (threadIdx.x < tile) {
        const long env = env0 + threadIdx.x;
        if (env >= n) return;
        T *ci = cinfo + env * 5;
        if (active && !active[env]) {
            reward[env] = T(0);
            for (int k = 0; k < 5; ++k) ci[k] = T(0);
            return;
        }
        const T ee_sq = (((s_ee[threadIdx.x][0] + s_ee[threadIdx.x][1]) + s_ee[threadIdx.x][2]) + s_ee[threadIdx.x][3]) + s_ee[threadIdx.x][4];
        T pose_sum = T(0), vel_sq = T(0);
        for (int bl = 0; bl < per; ++bl) { pose_sum += s_bp[threadIdx.x][bl]; vel_sq += s_bv[threadIdx.x][bl]; }
        const T pose_r = t_exp<T>(-(T)w.k_p * pose_sum);
        if (w.v_ord != 2.0) vel_sq = t_pow<T>(vel_sq, T(2) / (T)w.v_ord);
        const T vel_r = t_exp<T>(-(T)w.k_v * vel_sq);
        const T ee_r = t_exp<T>(-(T)w.k_e * ee_sq);
        const T rp_r = s_rp[threadIdx.x], rv_r = s_rv[threadIdx.x];
        T r = ((T)w.w_p * pose_r + (T)w.w_v * vel_r + (T)w.w_e * ee_r + (T)w.w_rp * rp_r + (T)w.w_rv * rv_r) / (T)w.w_sum;
        if (w.decay) r *= T(1) - (T)tcur[env] / (T)w.episode_len;
        if (endf[env]) r += end_reward;
        reward[env] = r;
        ci[0] = pose_r; ci[1] = vel_r; ci[2] = ee_r; ci[3] = rp_r; ci[4] = rv_r;
    }
}

// (four workgroups per CU: the multi-pass float64 form needed 132 VGPRs -- one granule past 128 -- and ran three waves per SIMD;
//  VALUBusy 63 % at 1 M envs said the fourth was missing)
template <typename T, int PASSES>
__global__ __launch_bounds__(256, 4) void k_reward_quat_v3(DevModel m, RewardW w, const T *__restrict__ expert_rows,
                                                        const T *__restrict__ cur_qpos, const T *__restrict__ prev_qpos,
                                                        const T *__restrict__ ee_wpos, const int *__restrict__ tcur,
                                                        const int *__restrict__ frame, const int *__restrict__ endf,
                                                        const int *__restrict__ active, T end_reward, int n,
                                                        T *__restrict__ reward, T *__restrict__ cinfo) {
    reward_body<T, PASSES>(m, w, expert_rows, cur_qpos, prev_qpos, ee_wpos, tcur, frame, endf, active, end_reward, n, reward, cinfo, blockIdx.x);
}

// ============================================================================================ K7
// Expert / learner pose features of one frame pair, reference formats (gen_expert.py:28-83 keys):
//   qvel[nv] = get_qvel_fd(prev, cur, dt) (world-frame root lin-vel), rlinv_local[3], rangv[3], rq_rmh[4],
//   ee_pos[15], bquat[4*nbody], bangvel[3*nbody].
// expert_convention != 0: rlinv_local uses the heading of the CURRENT root quat (gen_expert.py:53) and the heading
// frame whatever cfg.obs_coord says (gen_expert.py:18-22 builds its own config with obs_coord 'heading');
// otherwise the previous root quat and cfg.obs_coord's frame (get_qvel_fd(..., cfg.obs_coord) and
// get_ee_pos(cfg.obs_coord) as in the reward, reward_function.py:19-23).
template <typename T>
__global__ __launch_bounds__(256) void k_pose_features(DevModel m, const T *__restrict__ cur_qpos,
                                                       const T *__restrict__ prev_qpos, const T *__restrict__ ee_wpos,
                                                       int n, int expert_convention, T *__restrict__ qvel,
                                                       T *__restrict__ rlinv_local, T *__restrict__ rangv,
                                                       T *__restrict__ rq_rmh, T *__restrict__ ee_pos,
                                                       T *__restrict__ bquat, T *__restrict__ bangvel) {
    __shared__ int s_start[EGP_MAX_BODY], s_ndof[EGP_MAX_BODY];
    if (threadIdx.x < m.nbody) {
        s_start[threadIdx.x] = m.body_qpos_start[threadIdx.x];
        s_ndof[threadIdx.x] = m.body_ndof[threadIdx.x];
    }
    __syncthreads();
    const long env = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 5;
    const int l = threadIdx.x & 31;
    if (env >= n) return;
    const T *cq = cur_qpos + env * m.nq;
    const T *pq = prev_qpos + env * m.nq;
    const T dt = (T)m.dt;
    if (l >= 1 && l < m.nbody) {
        Q4<T> qc; V3<T> om;
        body_feature<T>(cq, pq, s_start[l], s_ndof[l], dt, &qc, &om);
        T *bq = bquat + env * 4 * m.nbody + 4 * l;
        bq[0] = qc.w; bq[1] = qc.x; bq[2] = qc.y; bq[3] = qc.z;
        T *bv = bangvel + env * 3 * m.nbody + 3 * l;
        bv[0] = om.x; bv[1] = om.y; bv[2] = om.z;
        // hinge velocities of this body
        for (int k = 0; k < s_ndof[l]; ++k) qvel[env * m.nv + s_start[l] - 1 + k] = (cq[s_start[l] + k] - pq[s_start[l] + k]) / dt;
    } else if (l == 0) {
        V3<T> v, rv;
        root_velocity<T>(cq, pq, dt, &v, &rv);
        const Q4<T> rc{cq[3], cq[4], cq[5], cq[6]};
        const Q4<T> rp{pq[3], pq[4], pq[5], pq[6]};
        T *qv = qvel + env * m.nv;
        qv[0] = v.x; qv[1] = v.y; qv[2] = v.z; qv[3] = rv.x; qv[4] = rv.y; qv[5] = rv.z;
        const V3<T> vl = coord_vec(expert_convention ? rc : rp, v, !expert_convention && m.obs_root != 0);
        T *o = rlinv_local + env * 3; o[0] = vl.x; o[1] = vl.y; o[2] = vl.z;
        o = rangv + env * 3; o[0] = rv.x; o[1] = rv.y; o[2] = rv.z;
        const Q4<T> rq = de_heading(rc);
        o = rq_rmh + env * 4; o[0] = rq.w; o[1] = rq.x; o[2] = rq.y; o[3] = rq.z;
        // root entries of bquat / bangvel
        o = bquat + env * 4 * m.nbody; o[0] = rc.w; o[1] = rc.x; o[2] = rc.y; o[3] = rc.z;
        const Q4<T> dv = qmul(rc, qinv(rp));
        V3<T> ax; T ang;
        rot_axis_angle<T>(dv, &ax, &ang);
        o = bangvel + env * 3 * m.nbody; o[0] = ax.x * ang / dt; o[1] = ax.y * ang / dt; o[2] = ax.z * ang / dt;
    } else if (l < m.nbody + 5) {
        const int k = l - m.nbody;
        const V3<T> e = ee_local<T>(cq, ee_wpos + env * 15 + 3 * k, !expert_convention && m.obs_root != 0);
        T *o = ee_pos + env * 15 + 3 * k; o[0] = e.x; o[1] = e.y; o[2] = e.z;
    }
}

}  // namespace egp

using namespace egp;

// The two small entries of the reward registry (ego_pose/core/reward_function.py:63-80), one thread per env:
//   EGP_REWARD_CONSTANT   reward 1.0 (the reference computes 1 + end_reward at an episode's end but returns 1.0), c_info [0]
//   EGP_REWARD_POSE_DIST  d = |expert qpos[2:] - qpos[2:]| of the step's expert frame (HumanoidEnv.get_pose_dist,
//                         humanoid_v1.py:275-280), reward 5 - 3 d (+ end_reward on the last step), c_info [d]
__global__ __launch_bounds__(256) void k_reward_simple(int kind, int nq, const double *__restrict__ qpos, const double *__restrict__ expert_qpos,
                                                       const int *__restrict__ frame, const int *__restrict__ endf, const int *__restrict__ active,
                                                       double end_reward, int n, double *__restrict__ reward, double *__restrict__ cinfo) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n || (active && !active[e])) return;
    if (kind == EGP_REWARD_CONSTANT) {
        reward[e] = 1.0;
        cinfo[e] = 0.0;
        return;
    }
    const double *q = qpos + (long)e * nq, *x = expert_qpos + (long)frame[e] * nq;
    double s = 0.0;
    for (int k = 2; k < nq; ++k) {
        const double d = x[k] - q[k];
        s += d * d;
    }
    const double dist = sqrt(s);
    reward[e] = 5.0 - 3.0 * dist + (endf[e] ? end_reward : 0.0);
    cinfo[e] = dist;
}

template <typename T>
static int launch_reward(egp_ctx *ctx, const T *expert_rows, const T *cur_qpos, const T *prev_qpos, const T *ee_wpos,
                         const int *t, const int *frame, const int *endf, const int *active, double end_reward, int n,
                         T *reward, T *cinfo, void *stream) {
    EGP_REQUIRE(ctx, "ctx is NULL");
    EGP_REQUIRE(n >= 0, "n < 0");
    if (!expert_rows) { set_error("egp_upload_experts must be called before the reward kernel"); return EGP_E_STATE; }
    if (n == 0) return EGP_OK;
    EGP_REQUIRE(cur_qpos && prev_qpos && ee_wpos && t && frame && endf && reward && cinfo, "NULL pointer");
    // multi-pass tiles (60 envs for the humanoid) once the launch fills the chip several times over, one-pass tiles for
    // rollout-sized batches
    if (n >= 16384) {
        const int tile = reward_tile_envs(ctx->dm.nbody, 5);
        k_reward_quat_v3<T, 5><<<dim3((n + tile - 1) / tile), dim3(256), 0, (hipStream_t)stream>>>(
            ctx->dm, ctx->rw, expert_rows, cur_qpos, prev_qpos, ee_wpos, t, frame, endf, active, (T)end_reward, n, reward, cinfo);
    } else {
        const int tile = reward_tile_envs(ctx->dm.nbody, 1);
        k_reward_quat_v3<T, 1><<<dim3((n + tile - 1) / tile), dim3(256), 0, (hipStream_t)stream>>>(
            ctx->dm, ctx->rw, expert_rows, cur_qpos, prev_qpos, ee_wpos, t, frame, endf, active, (T)end_reward, n, reward, cinfo);
    }
    return after_launch("k_reward_quat_v3");
}

template <typename T>
static int launch_features(egp_ctx *ctx, const T *cur, const T *prev, const T *ee_w, int n, int expert_conv, T *qvel, T *rlinv,
                           T *rangv, T *rq, T *ee, T *bq, T *bav, void *stream) {
    EGP_REQUIRE(ctx, "ctx is NULL");
    EGP_REQUIRE(n >= 0, "n < 0");
    if (n == 0) return EGP_OK;
    EGP_REQUIRE(cur && prev && ee_w && qvel && rlinv && rangv && rq && ee && bq && bav, "NULL pointer");
    const long threads = (long)n * 32;
    k_pose_features<T><<<dim3((threads + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(ctx->dm, cur, prev, ee_w, n, expert_conv,
                                                                                         qvel, rlinv, rangv, rq, ee, bq, bav);
    return after_launch("k_pose_features");
}

extern "C" {

int egp_reward_simple_f64(egp_ctx *c, int32_t kind, const double *qpos, const int32_t *frame, const int32_t *endf, const int32_t *active,
                          double end_reward, int32_t n, double *reward, double *cinfo, void *s) {
    EGP_REQUIRE(c, "ctx is NULL");
    EGP_REQUIRE(kind == EGP_REWARD_CONSTANT || kind == EGP_REWARD_POSE_DIST, "unknown reward kind");
    EGP_REQUIRE(n >= 0, "n < 0");
    if (n == 0) return EGP_OK;
    EGP_REQUIRE(reward && cinfo && (kind == EGP_REWARD_CONSTANT || (qpos && frame && endf)), "NULL pointer");
    if (kind == EGP_REWARD_POSE_DIST && !c->expert_qpos_f64) { set_error("egp_upload_experts must be called before the pose_dist reward"); return EGP_E_STATE; }
    k_reward_simple<<<dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)s>>>(kind, c->dm.nq, qpos, c->expert_qpos_f64, frame, endf, active,
                                                                              end_reward, n, reward, cinfo);
    return after_launch("k_reward_simple");
}

int egp_reward_quat_v3_f64(egp_ctx *c, const double *cq, const double *pq, const double *ee, const int32_t *t,
                           const int32_t *frame, const int32_t *endf, const int32_t *active, double end_reward, int32_t n,
                           double *reward, double *cinfo, void *s) {
    EGP_REQUIRE(c, "ctx is NULL");
    return launch_reward<double>(c, c->expert_rows_f64, cq, pq, ee, t, frame, endf, active, end_reward, n, reward, cinfo, s);
}
int egp_reward_quat_v3_f32(egp_ctx *c, const float *cq, const float *pq, const float *ee, const int32_t *t,
                           const int32_t *frame, const int32_t *endf, const int32_t *active, double end_reward, int32_t n,
                           float *reward, float *cinfo, void *s) {
    EGP_REQUIRE(c, "ctx is NULL");
    return launch_reward<float>(c, c->expert_rows_f32, cq, pq, ee, t, frame, endf, active, end_reward, n, reward, cinfo, s);
}

int egp_pose_features_f64(egp_ctx *c, const double *cur, const double *prev, const double *ee_w, int32_t n, int32_t expert_conv,
                          double *qvel, double *rlinv, double *rangv, double *rq, double *ee, double *bq, double *bav, void *s) {
    return launch_features<double>(c, cur, prev, ee_w, n, expert_conv, qvel, rlinv, rangv, rq, ee, bq, bav, s);
}
int egp_pose_features_f32(egp_ctx *c, const float *cur, const float *prev, const float *ee_w, int32_t n, int32_t expert_conv,
                          float *qvel, float *rlinv, float *rangv, float *rq, float *ee, float *bq, float *bav, void *s) {
    return launch_features<float>(c, cur, prev, ee_w, n, expert_conv, qvel, rlinv, rangv, rq, ee, bq, bav, s);
}

}  // extern "C"
