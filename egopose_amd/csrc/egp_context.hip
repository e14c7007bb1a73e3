// The library's error state and the context object of the C ABI (include/egopose_hip.h): egp_last_error / egp_version /
// egp_abi_sizeof, egp_create / egp_destroy, the reward weights, the K1 variant selection and the expert table upload.
// No kernels here. What the kernels' layouts fix for the context comes from their headers: the compiled-in dof tree and the
// lane-grid K1's gather table (egp_pd_dev.hpp, egp_pd_grid.hpp), the observation width (egp_filter_dev.hpp) and the packed
// expert row (egp_internal.hpp).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "egp_internal.hpp"
#include "egp_filter_dev.hpp"
#include "egp_pd_grid.hpp"

namespace egp {

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

}  // namespace egp

using namespace egp;

template <typename T>
static int dev_copy(egp_ctx *ctx, const T *host, size_t count, const T **out) {
    void *d = nullptr;
    EGP_HIP_CHECK(hipMalloc(&d, count * sizeof(T)));
    ctx->allocs.push_back(d);
    EGP_HIP_CHECK(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
    *out = (const T *)d;
    return EGP_OK;
}

static int fill_reward(egp_ctx *ctx, const egp_model_desc *d) {
    // Checked before anything is written: a refused set of weights leaves the context's previous ones in place. v_ord = inf
    // would be the reference's max-norm (np.linalg.norm(ord=inf)); K2's pow(pow(|d|, inf), 0) is 1 instead, and NaN fails every
    // comparison: neither may reach the kernel.
    EGP_REQUIRE(std::isfinite(d->v_ord) && d->v_ord >= 1.0, "v_ord must be finite and >= 1 (the max-norm, v_ord = inf, is not implemented)");
    EGP_REQUIRE(d->episode_len > 0, "episode_len must be positive");
    RewardW &w = ctx->rw;
    w.w_p = d->w_p; w.w_v = d->w_v; w.w_e = d->w_e; w.w_rp = d->w_rp; w.w_rv = d->w_rv;
    w.w_sum = d->w_p + d->w_v + d->w_e + d->w_rp + d->w_rv;
    w.k_p = d->k_p; w.k_v = d->k_v; w.k_e = d->k_e; w.k_rh = d->k_rh; w.k_rq = d->k_rq; w.k_rl = d->k_rl; w.k_ra = d->k_ra;
    w.v_ord = d->v_ord; w.decay = d->decay; w.episode_len = d->episode_len;
    return EGP_OK;
}

extern "C" {

const char *egp_last_error(void) { return g_err; }
const char *egp_version(void) { return "egopose_hip 0.2.0 (gfx950)"; }
int64_t egp_abi_sizeof(const char *name) {
    if (!name) return -1;
#define EGP_ABI_SIZE(T) if (!strcmp(name, #T)) return (int64_t)sizeof(T);
    EGP_ABI_SIZE(egp_model_desc) EGP_ABI_SIZE(egp_expert_table) EGP_ABI_SIZE(egp_gemm_desc)
    EGP_ABI_SIZE(egp_dynamics_desc) EGP_ABI_SIZE(egp_mlp_layer) EGP_ABI_SIZE(egp_physics_vtable)
    EGP_ABI_SIZE(egp_surrogate_desc) EGP_ABI_SIZE(egp_engine_desc) EGP_ABI_SIZE(egp_rollout_tick)
    EGP_ABI_SIZE(egp_ppo_loss_desc) EGP_ABI_SIZE(egp_adam_segment) EGP_ABI_SIZE(egp_host_probe_result)
    EGP_ABI_SIZE(egp_minibatch_plan_desc) EGP_ABI_SIZE(egp_ppo_loss_mb_desc) EGP_ABI_SIZE(egp_tcn_desc)
    EGP_ABI_SIZE(egp_policy_desc) EGP_ABI_SIZE(egp_gail_rows_desc) EGP_ABI_SIZE(egp_bce_logits_desc)
    EGP_ABI_SIZE(egp_lstm_desc) EGP_ABI_SIZE(egp_ppo_stats_desc)
#undef EGP_ABI_SIZE
    return -1;
}
int32_t egp_obs_dim(const egp_ctx *ctx) { return ctx ? ctx->dm.obs_dim : -1; }

int egp_create(const egp_model_desc *d, int device, egp_ctx **out) {
    EGP_REQUIRE(d && out, "desc/out is NULL");
    EGP_REQUIRE(d->nv > 6 && d->nv <= EGP_MAX_NV, "nv must be in (6, 64]");
    EGP_REQUIRE(d->nq == d->nv + 1 && d->nu == d->nv - 6, "expects one free root joint + hinges (nq=nv+1, nu=nv-6)");
    EGP_REQUIRE(d->nbody >= 2 && d->nbody + 5 <= EGP_MAX_BODY && 26 + 4 * (d->nbody - 1) <= 106 && 106 + 3 * (d->nbody - 1) <= EGP_EXPERT_ROW,
                "nbody must be in [2, 21] (the packed expert row holds 20 non-root bodies)");
    EGP_REQUIRE(d->nM > 0 && d->nM <= PD_NM_MAX, "nM must be in (0, 960] (the stable-PD kernels stage the sparse inertia row in LDS)");
    EGP_REQUIRE(d->body_qpos_start && d->body_ndof && d->dof_parentid && d->dof_Madr && d->ee_body, "skeleton table is NULL");
    EGP_REQUIRE(d->jkp && d->jkd && d->a_ref && d->a_scale && d->torque_lim && d->b_diffw, "gain table is NULL");
    EGP_REQUIRE(d->sub_dt > 0 && d->frame_skip > 0, "timestep/frame_skip must be positive");
    EGP_HIP_CHECK(hipSetDevice(device));
    egp_ctx *ctx = new egp_ctx();
    ctx->device = device;
    ctx->frame_skip = d->frame_skip;
    int rc = fill_reward(ctx, d);
    if (rc != EGP_OK) { delete ctx; return rc; }
    DevModel &m = ctx->dm;
    m.nq = d->nq; m.nv = d->nv; m.nu = d->nu; m.nbody = d->nbody; m.nM = d->nM;
    m.sub_dt = d->sub_dt;
    m.dt = d->sub_dt * d->frame_skip;
    m.obs_heading = d->obs_heading != 0; m.obs_keep = d->obs_keep_root_heading != 0; m.obs_root = d->obs_coord_root != 0;
    m.obs_vel = d->obs_vel;
    m.action_torque = d->action_torque != 0;
    if (m.obs_vel < 0 || m.obs_vel > 2) { delete ctx; set_error("obs_vel must be 0 (full), 1 (root) or 2 (none)"); return EGP_E_INVALID; }
    m.obs_phase = d->obs_phase != 0;
    m.episode_len = d->episode_len;
    if (m.obs_phase && d->episode_len <= 0) { delete ctx; set_error("obs_phase needs episode_len > 0"); return EGP_E_INVALID; }
    m.obs_dim = obs_width(d->nq, d->nv, m.obs_heading, m.obs_vel, m.obs_phase);
    // sparse-inertia index tables from the dof tree (what mj_fullM walks)
    std::vector<int> rows(d->nM), cols(d->nM);
    std::vector<short> mmap((size_t)d->nv * d->nv, (short)-1);
    int total = 0;
    for (int i = 0; i < d->nv; ++i) {
        int adr = d->dof_Madr[i], j = i;
        while (j >= 0) {
            if (adr < 0 || adr >= d->nM) { delete ctx; set_error("dof_Madr/dof_parentid inconsistent with nM"); return EGP_E_INVALID; }
            rows[adr] = i; cols[adr] = j;
            mmap[(size_t)i * d->nv + j] = (short)adr;
            mmap[(size_t)j * d->nv + i] = (short)adr;
            ++adr; ++total;
            j = d->dof_parentid[j];
        }
    }
    if (total != d->nM) { delete ctx; set_error("dof tree has %d inertia entries, nM says %d", total, d->nM); return EGP_E_INVALID; }
    for (int k = 0; k < 5; ++k) ctx->ee_body.push_back(d->ee_body[k]);
#define EGP_TRY(x) do { rc = (x); if (rc != EGP_OK) { egp_destroy(ctx); return rc; } } while (0)
    EGP_TRY(dev_copy<int>(ctx, d->body_qpos_start, d->nbody, &m.body_qpos_start));
    EGP_TRY(dev_copy<int>(ctx, d->body_ndof, d->nbody, &m.body_ndof));
    EGP_TRY(dev_copy<int>(ctx, rows.data(), d->nM, &m.m_row));
    EGP_TRY(dev_copy<int>(ctx, cols.data(), d->nM, &m.m_col));
    EGP_TRY(dev_copy<short>(ctx, mmap.data(), mmap.size(), &m.m_map));
    EGP_TRY(dev_copy<double>(ctx, d->jkp, d->nu, &m.jkp));
    EGP_TRY(dev_copy<double>(ctx, d->jkd, d->nu, &m.jkd));
    EGP_TRY(dev_copy<double>(ctx, d->a_ref, d->nu, &m.a_ref));
    EGP_TRY(dev_copy<double>(ctx, d->a_scale, d->nu, &m.a_scale));
    EGP_TRY(dev_copy<double>(ctx, d->torque_lim, d->nu, &m.torque_lim));
    EGP_TRY(dev_copy<double>(ctx, d->b_diffw, d->nbody - 1, &m.b_diffw));
#undef EGP_TRY
    // fast paths: 0 = tree-ordered elimination (needs the compiled-in humanoid dof tree; one substep per launch: the lane-grid
    // kernel, 3 = its lane-per-row predecessor), 2 = dense in-register Gauss-Jordan (any tree with nv == 58), 1 = generic LDS kernel
    bool tree_ok = d->nv == Tree58::NV;
    for (int i = 0; tree_ok && i < d->nv; ++i) tree_ok = d->dof_parentid[i] == Tree58::PARENT[i];
    ctx->tree58 = tree_ok;
    if (tree_ok) {          // gather table of the lane-grid K1 (k_pd_torque_grid58)
        const std::vector<unsigned short> off = grid58_offsets(mmap);
        const unsigned short *dev = nullptr;
        rc = dev_copy<unsigned short>(ctx, off.data(), off.size(), &dev);
        if (rc != EGP_OK) { egp_destroy(ctx); return rc; }
        ctx->pd_grid_off = dev;
        ctx->pd_grid = true;
    }
    ctx->pd_variant = tree_ok ? 0 : (d->nv == PD_NV ? 2 : 1);
    *out = ctx;
    return EGP_OK;
}

int egp_destroy(egp_ctx *ctx) {
    if (!ctx) return EGP_OK;
    for (void *p : ctx->allocs) (void)hipFree(p);
    delete ctx;
    return EGP_OK;
}

int egp_set_reward_weights(egp_ctx *ctx, const egp_model_desc *d) {
    EGP_REQUIRE(ctx && d, "ctx/desc is NULL");
    return fill_reward(ctx, d);
}

int egp_set_pd_variant(egp_ctx *ctx, int variant) {
    EGP_REQUIRE(ctx, "ctx is NULL");
    EGP_REQUIRE(variant == 1 || (variant == 2 && ctx->dm.nv == PD_NV) || ((variant == 0 || variant == 3) && ctx->tree58),
                "variants 0 and 3 need the humanoid_1205_v1 dof tree, variant 2 needs nv == 58");
    ctx->pd_variant = variant == 3 ? 0 : variant;
    ctx->pd_grid = variant == 0;
    return EGP_OK;
}

int egp_get_pd_variant(const egp_ctx *ctx) {
    if (!ctx) return -1;
    return ctx->pd_variant == 0 && !ctx->pd_grid ? 3 : ctx->pd_variant;
}

int egp_upload_experts(egp_ctx *ctx, const egp_expert_table *t) {
    EGP_REQUIRE(ctx && t, "ctx/table is NULL");
    EGP_REQUIRE(t->n_takes > 0 && t->n_frames > 0 && t->take_offset, "empty expert table");
    EGP_REQUIRE(t->qpos && t->rlinv_local && t->rangv && t->rq_rmh && t->ee_pos && t->bquat && t->bangvel, "expert column is NULL");
    EGP_REQUIRE(t->take_offset[t->n_takes] == t->n_frames, "take_offset[n_takes] != n_frames");
    const int nb = ctx->dm.nbody, nq = ctx->dm.nq;
    std::vector<double> rows((size_t)t->n_frames * EGP_EXPERT_ROW, 0.0);
    for (int f = 0; f < t->n_frames; ++f) {
        double *r = rows.data() + (size_t)f * EGP_EXPERT_ROW;
        r[ER_Z] = t->qpos[(size_t)f * nq + 2];
        for (int k = 0; k < 3; ++k) r[ER_RLINV + k] = t->rlinv_local[(size_t)f * 3 + k];
        for (int k = 0; k < 3; ++k) r[ER_RANGV + k] = t->rangv[(size_t)f * 3 + k];
        for (int k = 0; k < 4; ++k) r[ER_RQ + k] = t->rq_rmh[(size_t)f * 4 + k];
        for (int k = 0; k < 15; ++k) r[ER_EE + k] = t->ee_pos[(size_t)f * 15 + k];
        for (int k = 0; k < 4 * (nb - 1); ++k) r[ER_BQ + k] = t->bquat[(size_t)f * 4 * nb + 4 + k];
        for (int k = 0; k < 3 * (nb - 1); ++k) r[ER_BAV + k] = t->bangvel[(size_t)f * 3 * nb + 3 + k];
    }
    std::vector<float> rows32(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) rows32[i] = (float)rows[i];
    EGP_HIP_CHECK(hipSetDevice(ctx->device));
    if (ctx->expert_rows_f64) { (void)hipFree(ctx->expert_rows_f64); (void)hipFree(ctx->expert_rows_f32); (void)hipFree(ctx->expert_qpos_f64); }
    EGP_HIP_CHECK(hipMalloc((void **)&ctx->expert_qpos_f64, (size_t)t->n_frames * nq * sizeof(double)));
    EGP_HIP_CHECK(hipMemcpy(ctx->expert_qpos_f64, t->qpos, (size_t)t->n_frames * nq * sizeof(double), hipMemcpyHostToDevice));
    EGP_HIP_CHECK(hipMalloc((void **)&ctx->expert_rows_f64, rows.size() * sizeof(double)));
    EGP_HIP_CHECK(hipMalloc((void **)&ctx->expert_rows_f32, rows.size() * sizeof(float)));
    EGP_HIP_CHECK(hipMemcpy(ctx->expert_rows_f64, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice));
    EGP_HIP_CHECK(hipMemcpy(ctx->expert_rows_f32, rows32.data(), rows32.size() * sizeof(float), hipMemcpyHostToDevice));
    ctx->n_takes = t->n_takes;
    ctx->n_frames = t->n_frames;
    return EGP_OK;
}

}  // extern "C"
