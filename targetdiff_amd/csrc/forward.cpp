// C ABI of libtargetdiff_hip.so, part 4 of 5: the stateless entry points (graph construction, backbone, denoiser, posterior,
// likelihood terms, embeddings), the standalone EGNN refine net and the debug hooks.  td_refine_forward and td_model_forward are: checks,
// carve, (general graphs) the call's GraphPlan under a PlanGuard, compose / pack, run_blocks (plan.cpp), head / unpack.
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "td_device.h"
#include "td_internal.h"
#include "td_api.h"

using namespace tdapi;

// ------------------------------------------------------------------------------------------ entry points
extern "C" int td_graph_ptr(const int64_t *d_batch, int64_t N, int64_t B, int32_t *d_ptr, void *stream) {
    if (!d_ptr || (N > 0 && !d_batch) || N < 0 || B < 0) { td_set_error("td_graph_ptr: bad argument"); return TD_EINVAL; }
    return td_launch_graph_ptr(d_batch, N, B, d_ptr, static_cast<hipStream_t>(stream));
}

extern "C" int td_knn(const float *d_x, const int32_t *d_node_ptr, int64_t N, int64_t B, int32_t k,
                      int32_t max_graph_nodes, int32_t *d_out_nbr, void *stream) {
    if (k < 1 || k > TD_MAX_FANIN) { td_set_error("td_knn: k must be in 1..%d (got %d)", TD_MAX_FANIN, k); return TD_EINVAL; }
    if (N < 0 || B < 0 || (N > 0 && (!d_x || !d_node_ptr || !d_out_nbr))) { td_set_error("td_knn: bad argument"); return TD_EINVAL; }
    if (N == 0) return TD_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // scratch: float4 coordinates + graph ids (stream-ordered allocation keeps the call self-contained)
    AsyncScratch scratch(s);
    float4 *x4 = nullptr;
    int32_t *gid = nullptr;
    int rc;
    if ((rc = scratch.take(&x4, (size_t)N * sizeof(float4), "td_knn")) != TD_OK) return rc;
    if ((rc = scratch.take(&gid, (size_t)N * sizeof(int32_t), "td_knn")) != TD_OK) return rc;
    TD_CHECK_HIP(hipMemsetAsync(gid, 0, (size_t)N * sizeof(int32_t), s));
    // the ligand flag (.w) is irrelevant for the search: pack with an all-zero mask (gid is zero-filled scratch)
    rc = td_launch_pack_x(d_x, reinterpret_cast<const uint8_t *>(gid), N, x4, s);
    if (rc == TD_OK) rc = td_launch_node_gid(d_node_ptr, N, B, gid, s);
    TdNodes nodes{x4, d_node_ptr, nullptr, gid, N, B, max_graph_nodes};
    if (rc == TD_OK && k == TD_K) rc = td_launch_knn(nodes, d_out_nbr, TD_K, s);
    else if (rc == TD_OK) {
        // any other k: through the chunked table of the general-graph path (every node counts as "protein": one row kind)
        td_config c = {};
        c.cutoff_mode = TD_CUTOFF_KNN; c.knn = k;
        std::vector<int32_t> hp((size_t)B + 1), hl((size_t)B + 1, 0);
        hipError_t e = hipMemcpyAsync(hp.data(), d_node_ptr, (size_t)(B + 1) * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        GraphPlan p;
        if (e != hipSuccess) { td_set_error("td_knn: %s", hipGetErrorString(e)); rc = TD_EHIP; }
        else rc = plan_create(c, hp.data(), hl.data(), B, s, &p);
        if (rc == TD_OK) {
            rc = plan_layout(p, d_node_ptr, gid, s);
            nodes.pptr = p.pptr;
            if (rc == TD_OK) rc = td_launch_graph_general(TD_CUTOFF_KNN, nodes, TdRows{}, TdRows{}, k, 0.f, plan_tab(p), s);
            if (rc == TD_OK) rc = td_launch_slots_to_dense(p.cptr, p.cnbr, N, k, d_out_nbr, s);
            plan_destroy(p, s);
        }
    }
    return rc;
}

extern "C" int td_graph_build(const td_model *m, const float *d_x, const uint8_t *d_mask_ligand, const int32_t *d_node_ptr,
                              int64_t N, int64_t B, int32_t max_graph_nodes, int32_t *d_out_nbr, int32_t width, void *stream) {
    if (!m || N < 0 || B < 0 || width < 1 || (N > 0 && (!d_x || !d_mask_ligand || !d_node_ptr || !d_out_nbr))) {
        td_set_error("td_graph_build: bad argument");
        return TD_EINVAL;
    }
    if (N == 0) return TD_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    AsyncScratch scratch(s);
    float4 *x4 = nullptr;
    int32_t *gid = nullptr, *lig = nullptr;
    int rc;
    if ((rc = scratch.take(&x4, (size_t)N * sizeof(float4), "td_graph_build")) != TD_OK) return rc;
    if ((rc = scratch.take(&gid, (size_t)N * sizeof(int32_t), "td_graph_build")) != TD_OK) return rc;
    if ((rc = scratch.take(&lig, (size_t)(N + 1) * sizeof(int32_t), "td_graph_build")) != TD_OK) return rc;
    rc = td_launch_pack_x(d_x, d_mask_ligand, N, x4, s);
    if (rc == TD_OK) rc = td_launch_node_gid(d_node_ptr, N, B, gid, s);
    if (rc == TD_OK) rc = td_launch_ligand_list(d_mask_ligand, N, lig, lig + N, s);
    GraphPlan p;
    int64_t nl = 0;
    if (rc == TD_OK) rc = plan_from_mask(m->cfg, d_mask_ligand, d_node_ptr, N, B, s, &p, &nl);
    if (rc == TD_OK) {
        rc = plan_layout(p, d_node_ptr, gid, s);
        const TdNodes nodes{x4, d_node_ptr, p.pptr, gid, N, B, max_graph_nodes};
        if (rc == TD_OK) rc = td_launch_graph_general(p.mode, nodes, TdRows{p.prot_node, nullptr, p.Np}, TdRows{lig, nullptr, nl}, p.k, p.radius,
                                                      plan_tab(p), s);
        if (rc == TD_OK) rc = td_launch_slots_to_dense(p.cptr, p.cnbr, N, width, d_out_nbr, s);
        plan_destroy(p, s);
    }
    return rc;
}

extern "C" int td_refine_forward(const td_model *m, const float *d_h, const float *d_x, const uint8_t *d_mask_ligand,
                                 const int32_t *d_node_ptr, int64_t N, int64_t B, int32_t fix_x,
                                 int32_t max_graph_nodes, float *d_out_h, float *d_out_x, int32_t *d_out_nbr,
                                 float *d_out_ew, void *d_workspace, size_t workspace_bytes, void *stream) {
    if (!m || N < 0 || B < 0) { td_set_error("td_refine_forward: bad argument"); return TD_EINVAL; }
    if (N == 0) return TD_OK;
    if (!d_h || !d_x || !d_mask_ligand || !d_node_ptr || !d_out_h || !d_out_x || !d_workspace) {
        td_set_error("td_refine_forward: null pointer");
        return TD_EINVAL;
    }
    Workspace w = carve(static_cast<char *>(d_workspace), N, B, 0);
    if (w.bytes > workspace_bytes) {
        td_set_error("td_refine_forward: workspace has %zu bytes, need %zu", workspace_bytes, w.bytes);
        return TD_ENOMEM;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc;
    TD_CHECK_HIP(hipMemcpyAsync(w.node_ptr, d_node_ptr, (size_t)(B + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if ((rc = td_launch_node_gid(w.node_ptr, N, B, w.gid, s)) != TD_OK) return rc;
    if ((rc = td_launch_pack_x(d_x, d_mask_ligand, N, w.x4a, s)) != TD_OK) return rc;
    // ligand row list (h2x destinations; the x2h value pass serves the ligand rows from it); its length is needed for the
    // launch shapes -> one small D2H (this entry point mirrors the refine_net seam; the sampler path uses td_model_forward,
    // which knows N_l on the host).
    int32_t nl = 0;
    {
        if ((rc = td_launch_ligand_list(d_mask_ligand, N, w.lig_node, w.lig_node + N, s)) != TD_OK) return rc;
        TD_CHECK_HIP(hipMemcpyAsync(&nl, w.lig_node + N, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        TD_CHECK_HIP(hipStreamSynchronize(s));
    }
    if (d_out_h != d_h) TD_CHECK_HIP(hipMemcpyAsync(d_out_h, d_h, (size_t)N * TD_H * sizeof(float), hipMemcpyDeviceToDevice, s));
    PlanGuard plan{GraphPlan(), s};
    const bool general = !default_graph(m->cfg);
    int64_t nl_all = nl;
    if (general) {
        if (d_out_nbr || d_out_ew) { td_set_error("td_refine_forward: graph / gate outputs exist for the k = 32 kNN graph only (use td_graph_build)"); return TD_EINVAL; }
        if ((rc = plan_from_mask(m->cfg, d_mask_ligand, w.node_ptr, N, B, s, &plan.p, &nl_all)) != TD_OK) return rc;
        if ((rc = plan_layout(plan.p, w.node_ptr, w.gid, s)) != TD_OK) return rc;
    }
    float4 *xf = nullptr;
    if ((rc = run_blocks(m, w, general ? &plan.p : nullptr, d_out_h, N, nl_all, fix_x, max_graph_nodes, &xf, s)) != TD_OK) return rc;
    if ((rc = td_launch_unpack_x(xf, N, d_out_x, s)) != TD_OK) return rc;
    if (d_out_nbr) TD_CHECK_HIP(hipMemcpyAsync(d_out_nbr, w.nbr, (size_t)N * TD_K * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (d_out_ew) TD_CHECK_HIP(hipMemcpyAsync(d_out_ew, w.ew, (size_t)N * TD_K * sizeof(float), hipMemcpyDeviceToDevice, s));
    return TD_OK;
}

extern "C" int td_model_forward(const td_model *m, const float *d_protein_pos, const float *d_protein_v,
                                const int32_t *d_protein_ptr, int64_t N_p, const float *d_ligand_pos,
                                const int64_t *d_ligand_v, const int32_t *d_ligand_ptr, int64_t N_l, int64_t B,
                                int32_t fix_x, int32_t max_graph_nodes, float *d_pred_ligand_pos,
                                float *d_pred_ligand_v, float *d_final_ligand_h, float *d_final_h, void *d_workspace,
                                size_t workspace_bytes, const float *d_ligand_graph_bias, void *stream) {
    if (!m || N_p < 0 || N_l < 0 || B < 0) { td_set_error("td_model_forward: bad argument"); return TD_EINVAL; }
    const int64_t N = N_p + N_l;
    if (N == 0) return TD_OK;
    if (!d_protein_ptr || !d_ligand_ptr || !d_workspace || (N_p > 0 && (!d_protein_pos || !d_protein_v)) ||
        (N_l > 0 && (!d_ligand_pos || !d_ligand_v || !d_pred_ligand_pos || !d_pred_ligand_v))) {
        td_set_error("td_model_forward: null pointer");
        return TD_EINVAL;
    }
    Workspace w = carve(static_cast<char *>(d_workspace), N, B, N_l);
    if (w.bytes > workspace_bytes) {
        td_set_error("td_model_forward: workspace has %zu bytes, need %zu", workspace_bytes, w.bytes);
        return TD_ENOMEM;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc;
    float *h = d_final_h ? d_final_h : w.h;
    PlanGuard plan{GraphPlan(), s};
    const bool general = !default_graph(m->cfg);
    if (general) {
        std::vector<int32_t> hp, hl;
        if ((rc = fetch_ptrs(d_protein_ptr, d_ligand_ptr, B, hp, hl, s)) != TD_OK) return rc;
        if ((rc = plan_create(m->cfg, hp.data(), hl.data(), B, s, &plan.p)) != TD_OK) return rc;
    }
    {
        ProfScope ps(PC_COMPOSE, s);
        if ((rc = td_launch_compose(m, d_protein_pos, d_protein_v, d_protein_ptr, N_p, d_ligand_pos, d_ligand_v, d_ligand_ptr, N_l, B, h,
                                    w.x4a, w.node_ptr, w.gid, w.lig_node, plan.p.prot_node, d_ligand_graph_bias, s)) != TD_OK) return rc;
    }
    if (general && (rc = plan_layout(plan.p, w.node_ptr, w.gid, s)) != TD_OK) return rc;
    float4 *xf = nullptr;
    if ((rc = run_blocks(m, w, general ? &plan.p : nullptr, h, N, N_l, fix_x, max_graph_nodes, &xf, s)) != TD_OK) return rc;
    ProfScope ps(PC_HEAD, s);
    return td_launch_head(m->head, h, xf, w.lig_node, N_l, m->cfg.ligand_num_classes, d_pred_ligand_pos, d_pred_ligand_v,
                          d_final_ligand_h, s);
}

namespace tdapi {
int check_known_atoms(const char *who, const td_model *m, const uint8_t *d_fixed_mask, const float *d_fixed_pos,
                      const int64_t *d_fixed_v) {
    if (d_fixed_mask && (!d_fixed_pos || !d_fixed_v)) {
        td_set_error("%s: d_fixed_mask needs d_fixed_pos and d_fixed_v", who);
        return TD_EINVAL;
    }
    if (d_fixed_mask && !m->sched.abar) {
        td_set_error("%s: the model was created without alphas_cumprod (8 schedule arrays)", who);
        return TD_EINVAL;
    }
    return TD_OK;
}
}  // namespace tdapi

namespace {
// The stateless step entry points below all end here: the one place that fills a TdStepArgs from a C call.  Each passes null for the
// pointers its signature does not have; `who` names it in the error texts.  renoise: the forward-process step of a time program, which
// reads neither t, the offsets nor the network's outputs.
int step_entry(const char *who, const td_model *m, const int32_t *d_t, const float *d_prog_row, const int32_t *d_ligand_ptr, int64_t N_l,
               int64_t B, const float *d_ligand_pos, const int64_t *d_ligand_v, const float *d_pred_pos, const float *d_pred_v,
               const float *d_noise, const float *d_uniform, float *d_pos_next, int64_t *d_v_next, float *d_log_v0, float *d_log_post,
               const uint8_t *d_fixed_mask, const float *d_fixed_pos, const int64_t *d_fixed_v, const float *d_x0_shift, void *stream,
               bool renoise = false) {
    if (!m || N_l < 0 || B < 0) { td_set_error("%s: bad argument", who); return TD_EINVAL; }
    if (N_l == 0) return TD_OK;
    const bool own = renoise ? d_prog_row != nullptr : d_t && d_ligand_ptr && d_pred_pos && d_pred_v && d_uniform;
    if (!own || !d_ligand_pos || !d_ligand_v || !d_noise || !d_pos_next || !d_v_next) {
        td_set_error("%s: null pointer", who);
        return TD_EINVAL;
    }
    const int rc = check_known_atoms(who, m, d_fixed_mask, d_fixed_pos, d_fixed_v);
    if (rc != TD_OK) return rc;
    TdStepArgs a;
    a.t = d_t; a.prow = d_prog_row; a.lptr = d_ligand_ptr; a.Nl = N_l; a.pos = d_ligand_pos; a.v = d_ligand_v;
    a.pred_pos = d_pred_pos; a.pred_v = d_pred_v; a.noise = d_noise; a.uni = d_uniform;
    a.pos_next = d_pos_next; a.v_next = d_v_next; a.log_v0 = d_log_v0; a.log_post = d_log_post;
    a.fixed_mask = d_fixed_mask; a.fixed_pos = d_fixed_pos; a.fixed_v = d_fixed_v; a.x0_shift = d_x0_shift;
    a.B = (int)B; a.C = m->cfg.ligand_num_classes; a.T = m->cfg.num_timesteps; a.mean_type = m->cfg.model_mean_type;
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope ps(PC_POST, s);
    return renoise ? td_launch_renoise(a, s) : td_launch_posterior(m->sched, a, s);
}
}  // namespace

extern "C" int td_posterior_step(const td_model *m, const int32_t *d_t, const int32_t *d_ligand_ptr, int64_t N_l,
                                 int64_t B, const float *d_ligand_pos, const int64_t *d_ligand_v,
                                 const float *d_pred_pos, const float *d_pred_v, const float *d_noise,
                                 const float *d_uniform, float *d_pos_next, int64_t *d_v_next, float *d_log_v0,
                                 float *d_log_post, void *stream) {
    return step_entry("td_posterior_step", m, d_t, nullptr, d_ligand_ptr, N_l, B, d_ligand_pos, d_ligand_v, d_pred_pos, d_pred_v, d_noise,
                      d_uniform, d_pos_next, d_v_next, d_log_v0, d_log_post, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int td_posterior_step_fixed(const td_model *m, const int32_t *d_t, const int32_t *d_ligand_ptr, int64_t N_l,
                                       int64_t B, const float *d_ligand_pos, const int64_t *d_ligand_v,
                                       const float *d_pred_pos, const float *d_pred_v, const float *d_noise,
                                       const float *d_uniform, float *d_pos_next, int64_t *d_v_next, float *d_log_v0,
                                       float *d_log_post, const uint8_t *d_fixed_mask, const float *d_fixed_pos,
                                       const int64_t *d_fixed_v, void *stream) {
    return step_entry("td_posterior_step_fixed", m, d_t, nullptr, d_ligand_ptr, N_l, B, d_ligand_pos, d_ligand_v, d_pred_pos, d_pred_v,
                      d_noise, d_uniform, d_pos_next, d_v_next, d_log_v0, d_log_post, d_fixed_mask, d_fixed_pos, d_fixed_v, nullptr, stream);
}

extern "C" int td_posterior_step_program(const td_model *m, const int32_t *d_t, const float *d_prog_row, const int32_t *d_ligand_ptr,
                                         int64_t N_l, int64_t B, const float *d_ligand_pos, const int64_t *d_ligand_v,
                                         const float *d_pred_pos, const float *d_pred_v, const float *d_noise,
                                         const float *d_uniform, float *d_pos_next, int64_t *d_v_next, float *d_log_v0,
                                         float *d_log_post, const uint8_t *d_fixed_mask, const float *d_fixed_pos,
                                         const int64_t *d_fixed_v, void *stream) {
    if (!d_prog_row) { td_set_error("td_posterior_step_program: null d_prog_row"); return TD_EINVAL; }
    return step_entry("td_posterior_step_program", m, d_t, d_prog_row, d_ligand_ptr, N_l, B, d_ligand_pos, d_ligand_v, d_pred_pos, d_pred_v,
                      d_noise, d_uniform, d_pos_next, d_v_next, d_log_v0, d_log_post, d_fixed_mask, d_fixed_pos, d_fixed_v, nullptr, stream);
}

extern "C" int td_renoise_step(const td_model *m, const float *d_prog_row, int64_t N_l, const float *d_ligand_pos,
                               const int64_t *d_ligand_v, const float *d_noise, const float *d_uniform, float *d_pos_next,
                               int64_t *d_v_next, float *d_log_v0, float *d_log_q, void *stream) {
    return step_entry("td_renoise_step", m, nullptr, d_prog_row, nullptr, N_l, 0, d_ligand_pos, d_ligand_v, nullptr, nullptr, d_noise,
                      d_uniform, d_pos_next, d_v_next, d_log_v0, d_log_q, nullptr, nullptr, nullptr, nullptr, stream, true);
}

// ------------------------------------------------------------------------------------------ clash guidance
extern "C" int td_posterior_step_guided(const td_model *m, const int32_t *d_t, const float *d_prog_row, const int32_t *d_ligand_ptr,
                                        int64_t N_l, int64_t B, const float *d_ligand_pos, const int64_t *d_ligand_v,
                                        const float *d_pred_pos, const float *d_pred_v, const float *d_noise,
                                        const float *d_uniform, float *d_pos_next, int64_t *d_v_next, float *d_log_v0,
                                        float *d_log_post, const uint8_t *d_fixed_mask, const float *d_fixed_pos,
                                        const int64_t *d_fixed_v, const float *d_x0_shift, void *stream) {
    return step_entry("td_posterior_step_guided", m, d_t, d_prog_row, d_ligand_ptr, N_l, B, d_ligand_pos, d_ligand_v, d_pred_pos, d_pred_v,
                      d_noise, d_uniform, d_pos_next, d_v_next, d_log_v0, d_log_post, d_fixed_mask, d_fixed_pos, d_fixed_v, d_x0_shift,
                      stream);
}

namespace {
int clash_args(const char *who, const float *d_protein_pos, const float *d_sigma, const int32_t *d_protein_ptr,
               const int32_t *d_ligand_ptr, int64_t B, const float *d_pos, float w, float max_shift, TdClashArgs &a) {
    if (B < 0 || B > 0x7fffffff) { td_set_error("%s: bad argument", who); return TD_EINVAL; }
    if (B > 0 && (!d_protein_pos || !d_sigma || !d_protein_ptr || !d_ligand_ptr || !d_pos)) {
        td_set_error("%s: null pointer", who);
        return TD_EINVAL;
    }
    if (!(w >= 0.f)) { td_set_error("%s: the weight must be >= 0 (got %g)", who, (double)w); return TD_EINVAL; }
    if (!(max_shift >= 0.f)) { td_set_error("%s: max_shift must be >= 0 (0: no cap; got %g)", who, (double)max_shift); return TD_EINVAL; }
    a.ppos = d_protein_pos; a.sigma = d_sigma; a.pptr = d_protein_ptr; a.lptr = d_ligand_ptr; a.B = (int)B; a.eval = d_pos;
    a.w = w; a.max_shift = max_shift;
    return TD_OK;
}
}  // namespace

extern "C" int td_clash_shift(const float *d_protein_pos, const float *d_sigma, const int32_t *d_protein_ptr,
                              const int32_t *d_ligand_ptr, int64_t B, const float *d_pos, float w, float max_shift, float *d_shift,
                              void *stream) {
    TdClashArgs a;
    const int rc = clash_args("td_clash_shift", d_protein_pos, d_sigma, d_protein_ptr, d_ligand_ptr, B, d_pos, w, max_shift, a);
    if (rc != TD_OK) return rc;
    if (B > 0 && !d_shift) { td_set_error("td_clash_shift: null pointer"); return TD_EINVAL; }
    return td_launch_clash_shift(a, d_shift, static_cast<hipStream_t>(stream));
}

extern "C" int td_clash_report(const float *d_protein_pos, const float *d_sigma, const int32_t *d_protein_ptr,
                               const int32_t *d_ligand_ptr, int64_t B, const float *d_pos, int32_t *d_count, float *d_energy,
                               float *d_min_dist, void *stream) {
    TdClashArgs a;
    const int rc = clash_args("td_clash_report", d_protein_pos, d_sigma, d_protein_ptr, d_ligand_ptr, B, d_pos, 0.f, 0.f, a);
    if (rc != TD_OK) return rc;
    if (B > 0 && (!d_count || !d_energy || !d_min_dist)) { td_set_error("td_clash_report: null pointer"); return TD_EINVAL; }
    return td_launch_clash_report(a, d_count, d_energy, d_min_dist, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------ standalone EGNN refine net
struct td_egnn {
    int num_layers;
    float *blob;
    TdEgnnLayer *layers;     // host array
};

namespace tdapi {
constexpr int EGNN_EDGE_IN = 2 * TD_H + 1 + 4;      // [h_i | h_j | d^2 | one_hot(type)]  (models/egnn.py:22, num_r_gaussian = 1)
size_t egnn_layer_floats() {
    return (size_t)TD_H * EGNN_EDGE_IN + TD_H + (size_t)TD_H * TD_H + TD_H + TD_H + 1 + (size_t)TD_H * TD_H + TD_H + TD_H +
           (size_t)TD_H * 2 * TD_H + TD_H + (size_t)TD_H * TD_H + TD_H;
}
// 128 x 128 weight (row-major [out][in]) as A fragments of the 16x16x4 product: [ot][hb][lane] x 4 r
size_t pack_A16(Packer &pk, const float *W) {
    size_t off = pk.alloc((size_t)8 * 8 * 64 * 4);
    float *d = pk.data.data() + off;
    for (int ot = 0; ot < 8; ++ot)
        for (int hb = 0; hb < 8; ++hb)
            for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 4; ++r)
                    d[(((size_t)ot * 8 + hb) * 64 + lane) * 4 + r] = W[(size_t)(16 * ot + (lane & 15)) * TD_H + 16 * hb + 4 * (lane >> 4) + r];
    return off;
}
}  // namespace tdapi

extern "C" size_t td_egnn_num_weights(int32_t num_layers) { return num_layers > 0 ? (size_t)num_layers * egnn_layer_floats() : 0; }

extern "C" int td_egnn_create(int32_t num_layers, int32_t hidden_dim, int32_t edge_feat_dim, int32_t knn,
                              const float *host_weights, size_t num_weights, td_egnn **out) {
    if (!host_weights || !out || num_layers <= 0) { td_set_error("td_egnn_create: bad argument"); return TD_EINVAL; }
    if (hidden_dim != TD_H || edge_feat_dim != 4 || knn != TD_K) {
        td_set_error("td_egnn_create: unsupported configuration (need hidden 128, edge_feat_dim 4, knn 32; got %d/%d/%d)",
                     hidden_dim, edge_feat_dim, knn);
        return TD_EINVAL;
    }
    if (num_weights != td_egnn_num_weights(num_layers)) {
        td_set_error("td_egnn_create: weight blob has %zu floats, expected %zu", num_weights, td_egnn_num_weights(num_layers));
        return TD_EINVAL;
    }
    struct Off { size_t projB, projBias, W2f, Wxf, vec, nodeB, nb1, nb2; };
    std::vector<Off> off((size_t)num_layers);
    Packer pk;
    Cursor cur{host_weights, num_weights};
    for (int l = 0; l < num_layers; ++l) {
        const float *W1 = cur.take((size_t)TD_H * EGNN_EDGE_IN), *b1 = cur.take(TD_H);
        const float *W2 = cur.take((size_t)TD_H * TD_H), *b2 = cur.take(TD_H);
        const float *winf = cur.take(TD_H), *binf = cur.take(1);
        const float *Wx = cur.take((size_t)TD_H * TD_H), *bx = cur.take(TD_H), *wx2 = cur.take(TD_H);
        const float *Wn1 = cur.take((size_t)TD_H * 2 * TD_H), *bn1 = cur.take(TD_H);
        const float *Wn2 = cur.take((size_t)TD_H * TD_H), *bn2 = cur.take(TD_H);
        Off &o = off[(size_t)l];
        o.projB = pack_B128(pk, W1, EGNN_EDGE_IN, 0);          // h_i columns (dst)
        pack_B128(pk, W1, EGNN_EDGE_IN, TD_H);                 // h_j columns (src): consecutive block
        o.projBias = pk.alloc(5 * TD_H);
        memcpy(pk.data.data() + o.projBias, b1, TD_H * sizeof(float));
        o.W2f = pack_A16(pk, W2);
        o.Wxf = pack_A16(pk, Wx);
        o.vec = pk.alloc(128 + 512 + 128 + 132 + 128 + 128);
        float *v = pk.data.data() + o.vec;
        for (int n = 0; n < TD_H; ++n) {
            v[n] = W1[(size_t)n * EGNN_EDGE_IN + 2 * TD_H];                                    // d^2 column
            for (int t = 0; t < 4; ++t) v[128 + t * TD_H + n] = W1[(size_t)n * EGNN_EDGE_IN + 2 * TD_H + 1 + t];
            v[640 + n] = b2[n];
            v[768 + n] = winf[n];
            v[900 + n] = bx[n];
            v[1028 + n] = wx2[n];
        }
        v[768 + 128] = binf[0];
        o.nodeB = pack_B128(pk, Wn1, 2 * TD_H, 0);             // mi half of node_mlp.net.0  (cat([mi, h]), models/egnn.py:56)
        pack_B128(pk, Wn1, 2 * TD_H, TD_H);                    // h half
        pack_B128(pk, Wn2, TD_H, 0);
        o.nb1 = pack_vec(pk, bn1, TD_H);
        o.nb2 = pack_vec(pk, bn2, TD_H);
    }
    if (!cur.ok || cur.left != 0) { td_set_error("td_egnn_create: weight blob layout mismatch"); return TD_EINVAL; }
    td_egnn *m = new (std::nothrow) td_egnn();
    if (!m) { td_set_error("td_egnn_create: out of host memory"); return TD_ENOMEM; }
    m->num_layers = num_layers;
    m->layers = new (std::nothrow) TdEgnnLayer[(size_t)num_layers];
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&m->blob), pk.data.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(m->blob, pk.data.data(), pk.data.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess || !m->layers) {
        td_set_error("td_egnn_create: device upload failed: %s", hipGetErrorString(e));
        if (m->blob) (void)hipFree(m->blob);
        delete[] m->layers;
        delete m;
        return TD_EHIP;
    }
    const float *D = m->blob;
    for (int l = 0; l < num_layers; ++l) {
        const Off &o = off[(size_t)l];
        TdEgnnLayer &L = m->layers[l];
        L.proj = TdNodeStage{D + o.projB, D + o.projBias, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, false, false, false};
        L.W2f = D + o.W2f; L.Wxf = D + o.Wxf; L.vec = D + o.vec; L.nodeB = D + o.nodeB; L.nb1 = D + o.nb1; L.nb2 = D + o.nb2;
    }
    *out = m;
    return TD_OK;
}

extern "C" void td_egnn_destroy(td_egnn *m) {
    if (!m) return;
    if (m->blob) (void)hipFree(m->blob);
    delete[] m->layers;
    delete m;
}

namespace tdapi {
struct EgnnWs { float4 *x4a, *x4b; int32_t *gid, *nbr; float *P, *mi; size_t bytes; };
EgnnWs egnn_carve(char *base, int64_t N) {
    EgnnWs w;
    Carver c{base};
    const size_t n = (size_t)(N > 0 ? N : 1);
    w.x4a = c.take<float4>(n); w.x4b = c.take<float4>(n);
    w.gid = c.take<int32_t>(n);
    w.nbr = c.take<int32_t>(n * TD_K);
    w.P = c.take<float>(n * 4 * TD_H);
    w.mi = c.take<float>(n * TD_H);
    w.bytes = c.off;
    return w;
}
}  // namespace tdapi

extern "C" size_t td_egnn_workspace_bytes(int64_t N) { return egnn_carve(nullptr, N).bytes; }

// EGNN.forward (models/egnn.py:121-133): per layer a fresh kNN graph on the current coordinates, then one EnBaseLayer.
extern "C" int td_egnn_forward(const td_egnn *m, const float *d_h, const float *d_x, const uint8_t *d_mask_ligand,
                               const int32_t *d_node_ptr, int64_t N, int64_t B, int32_t max_graph_nodes, float *d_out_h,
                               float *d_out_x, float *d_all_h, float *d_all_x, void *d_workspace, size_t workspace_bytes,
                               void *stream) {
    if (!m || N < 0 || B < 0) { td_set_error("td_egnn_forward: bad argument"); return TD_EINVAL; }
    if (N == 0) return TD_OK;
    if (!d_h || !d_x || !d_mask_ligand || !d_node_ptr || !d_out_h || !d_out_x || !d_workspace) {
        td_set_error("td_egnn_forward: null pointer");
        return TD_EINVAL;
    }
    EgnnWs w = egnn_carve(static_cast<char *>(d_workspace), N);
    if (w.bytes > workspace_bytes) {
        td_set_error("td_egnn_forward: workspace has %zu bytes, need %zu", workspace_bytes, w.bytes);
        return TD_ENOMEM;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc;
    if ((rc = td_launch_node_gid(d_node_ptr, N, B, w.gid, s)) != TD_OK) return rc;
    if ((rc = td_launch_pack_x(d_x, d_mask_ligand, N, w.x4a, s)) != TD_OK) return rc;
    TD_CHECK_HIP(hipMemcpyAsync(w.x4b, w.x4a, (size_t)N * sizeof(float4), hipMemcpyDeviceToDevice, s));
    if (d_out_h != d_h) TD_CHECK_HIP(hipMemcpyAsync(d_out_h, d_h, (size_t)N * TD_H * sizeof(float), hipMemcpyDeviceToDevice, s));
    float4 *xc = w.x4a, *xn = w.x4b;
    for (int l = 0; l < m->num_layers; ++l) {
        const TdEgnnLayer &L = m->layers[l];
        if ((rc = td_launch_knn(TdNodes{xc, d_node_ptr, nullptr, w.gid, N, B, max_graph_nodes}, w.nbr, TD_K, s)) != TD_OK) return rc;
        if ((rc = td_launch_node_proj(L.proj, d_out_h, TdRows{nullptr, nullptr, N}, 0x03, TdRows{}, 0, w.P, w.P, s)) != TD_OK) return rc;
        if ((rc = td_launch_egnn_edge(L, xc, xn, w.nbr, w.P, w.mi, N, s)) != TD_OK) return rc;
        if ((rc = td_launch_egnn_node(L, w.mi, d_out_h, N, s)) != TD_OK) return rc;
        float4 *t = xc; xc = xn; xn = t;
        // keep the protein rows of the (now stale) buffer in sync is not needed: only ligand rows ever change and the
        // edge kernel rewrites every ligand row of its output buffer
        if (d_all_x && (rc = td_launch_unpack_x(xc, N, d_all_x + (size_t)l * N * 3, s)) != TD_OK) return rc;
        if (d_all_h) TD_CHECK_HIP(hipMemcpyAsync(d_all_h + (size_t)l * N * TD_H, d_out_h, (size_t)N * TD_H * sizeof(float),
                                                 hipMemcpyDeviceToDevice, s));
    }
    return td_launch_unpack_x(xc, N, d_out_x, s);
}

// ---- the other forward consumers: likelihood estimation (scripts/likelihood_est_diffusion.py) and return_all
extern "C" int td_perturb(const td_model *m, const int32_t *d_t, const int32_t *d_ligand_ptr, int64_t N_l, int64_t B,
                          const float *d_ligand_pos, const int64_t *d_ligand_v, const float *d_noise, const float *d_uniform,
                          float *d_pos_t, int64_t *d_v_t, void *stream) {
    if (!m || N_l < 0 || B < 0) { td_set_error("td_perturb: bad argument"); return TD_EINVAL; }
    if (!m->sched.abar) { td_set_error("td_perturb: the model was created without alphas_cumprod (8 schedule arrays)"); return TD_EINVAL; }
    if (N_l == 0) return TD_OK;
    if (!d_t || !d_ligand_ptr || !d_ligand_pos || !d_ligand_v || !d_noise || !d_uniform || !d_pos_t || !d_v_t) {
        td_set_error("td_perturb: null pointer");
        return TD_EINVAL;
    }
    return td_launch_perturb(m->sched, m->cfg.num_timesteps, d_t, d_ligand_ptr, N_l, B, m->cfg.ligand_num_classes, d_ligand_pos,
                             d_ligand_v, d_noise, d_uniform, d_pos_t, d_v_t, static_cast<hipStream_t>(stream));
}

extern "C" int td_likelihood_terms(const td_model *m, const int32_t *d_t, const int32_t *d_ligand_ptr, int64_t N_l, int64_t B,
                                   const float *d_pos_0, const float *d_pos_t, const int64_t *d_v_0, const int64_t *d_v_t,
                                   const float *d_pred_pos, const float *d_pred_v, float *d_kl_pos, float *d_kl_v,
                                   void *stream) {
    if (!m || N_l < 0 || B < 0) { td_set_error("td_likelihood_terms: bad argument"); return TD_EINVAL; }
    if (B == 0) return TD_OK;
    if (!d_t || !d_ligand_ptr || !d_kl_pos || !d_kl_v ||
        (N_l > 0 && (!d_pos_0 || !d_pos_t || !d_v_0 || !d_v_t || !d_pred_pos || !d_pred_v))) {
        td_set_error("td_likelihood_terms: null pointer");
        return TD_EINVAL;
    }
    return td_launch_likelihood_terms(m->sched, m->cfg.num_timesteps, d_t, d_ligand_ptr, B, m->cfg.ligand_num_classes, d_pos_0,
                                      d_pos_t, d_v_0, d_v_t, d_pred_pos, d_pred_v, d_kl_pos, d_kl_v,
                                      static_cast<hipStream_t>(stream));
}

extern "C" int td_likelihood_prior(const td_model *m, const int32_t *d_ligand_ptr, int64_t N_l, int64_t B,
                                   const float *d_pos_0, const int64_t *d_v_index, float *d_kl_pos, float *d_kl_v,
                                   void *stream) {
    if (!m || N_l < 0 || B < 0) { td_set_error("td_likelihood_prior: bad argument"); return TD_EINVAL; }
    if (!m->sched.abar) { td_set_error("td_likelihood_prior: the model was created without alphas_cumprod (8 schedule arrays)"); return TD_EINVAL; }
    if (B == 0) return TD_OK;
    if (!d_ligand_ptr || !d_kl_pos || !d_kl_v || (N_l > 0 && (!d_pos_0 || !d_v_index))) {
        td_set_error("td_likelihood_prior: null pointer");
        return TD_EINVAL;
    }
    return td_launch_likelihood_prior(m->sched, m->cfg.num_timesteps, d_ligand_ptr, B, m->cfg.ligand_num_classes, d_pos_0,
                                      d_v_index, d_kl_pos, d_kl_v, static_cast<hipStream_t>(stream));
}

extern "C" int td_embed_ligand(const td_model *m, const int64_t *d_ligand_v, int64_t N_l, float *d_h, void *stream) {
    if (!m || N_l < 0 || (N_l > 0 && (!d_ligand_v || !d_h))) { td_set_error("td_embed_ligand: bad argument"); return TD_EINVAL; }
    return td_launch_embed_ligand(m->emb, m->cfg.ligand_num_classes, d_ligand_v, N_l, d_h, static_cast<hipStream_t>(stream));
}

extern "C" int td_v_inference(const td_model *m, const float *d_h, int64_t n, float *d_logits, void *stream) {
    if (!m || n < 0 || (n > 0 && (!d_h || !d_logits))) { td_set_error("td_v_inference: bad argument"); return TD_EINVAL; }
    return td_launch_head(m->head, d_h, nullptr, nullptr, n, m->cfg.ligand_num_classes, nullptr, d_logits, nullptr,
                          static_cast<hipStream_t>(stream));
}

extern "C" int td_center_pos(float *d_protein_pos, const int32_t *d_protein_ptr, float *d_ligand_pos,
                             const int32_t *d_ligand_ptr, int64_t B, float *d_offset, int32_t compute_offset,
                             int32_t sign, void *stream) {
    if (B < 0 || !d_offset || !d_protein_ptr || !d_ligand_ptr || (compute_offset && !d_protein_pos)) {
        td_set_error("td_center_pos: bad argument");
        return TD_EINVAL;
    }
    return td_launch_center(d_protein_pos, d_protein_ptr, d_ligand_pos, d_ligand_ptr, B, d_offset, compute_offset,
                            sign, static_cast<hipStream_t>(stream));
}

extern "C" int td_debug_node_stage(const td_model *m, int32_t layer, int32_t stage, const float *d_h, int64_t N,
                                   float *d_P, float *d_q, void *stream) {
    if (!m || layer < 0 || layer >= m->cfg.num_layers || (stage != 0 && stage != 1) || N < 0 || (N > 0 && (!d_h || !d_P || !d_q))) {
        td_set_error("td_debug_node_stage: bad argument");
        return TD_EINVAL;
    }
    if (stage_rows(m->cfg) != 1) {       // m->layers holds stage_rows rows per reference layer: this hook addresses whole layers only
        td_set_error("td_debug_node_stage: models with several x2h / h2x stages per layer are not addressed by this hook");
        return TD_EINVAL;
    }
    const TdLayer &L = m->layers[layer];
    return td_launch_node_proj(stage == 0 ? L.nodeX2h : L.nodeH2x, d_h, TdRows{nullptr, nullptr, N}, 0x1f, TdRows{}, 0, d_P, d_q,
                               static_cast<hipStream_t>(stream));
}

extern "C" int td_debug_fail_alloc(int32_t nth) {
    g_fail_alloc.store(nth > 0 ? nth : 0);
    return TD_OK;
}

extern "C" int td_debug_wg_trace(uint64_t *d_buf, int32_t slots) {
    return td_set_wg_trace(reinterpret_cast<unsigned long long *>(d_buf), d_buf ? slots : 0);
}

extern "C" int td_debug_reductions(const float *d_in64, float *d_out6x64, void *stream) {
    return td_launch_reductions(d_in64, d_out6x64, static_cast<hipStream_t>(stream));
}
