// C ABI of libtargetdiff_hip.so, part 3 of 5: workspace carving, the launch sequence of one denoiser evaluation, each part written once
// and shared by the stateless entry points and the sampling session -- run_blocks (per block: graph + gate, layers, buffer swap),
// run_backbone (the layer loop), x2h_stage / h2x_project + h2x_attend (one stage) -- and the chunked layout of general graphs (GraphPlan).
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

// ------------------------------------------------------------------------------------------ workspace
namespace tdapi {

Workspace carve(char *base, int64_t N, int64_t B, int64_t Nl) {
    Workspace w;
    Carver c{base};
    const size_t n = (size_t)(N > 0 ? N : 1), nl = (size_t)(Nl > 0 ? Nl : n);
    w.x4a = c.take<float4>(n); w.x4b = c.take<float4>(n);
    w.gid = c.take<int32_t>(n);
    w.nbr = c.take<int32_t>(n * TD_K);
    w.lig_node = c.take<int32_t>(nl + 1);
    w.node_ptr = c.take<int32_t>((size_t)(B + 1));
    w.ew = c.take<float>(n * TD_K);
    w.P = c.take<float>(n * 4 * TD_H); w.q = c.take<float>(n * TD_H);
    w.h = c.take<float>(n * TD_H);
    w.alpha = c.take<float>(n * TD_HEADS * TD_K);
    w.Px = c.take<float>(n * 4 * TD_H); w.qx = c.take<float>(n * TD_H);
    w.bytes = c.off;
    return w;
}

// One x2h stage of layer L on the rows a.rows: the projections (unless they are in place), the stage's own gate (ew_net_type 'r' / none:
// from the layer's coordinates, every row), key pass, value pass into h, node_output (x2h_out_fc) on every row.
int x2h_stage(const TdLayer &L, const TdGraphTab &gt, const float4 *xc, float *h, int64_t N, const X2hStage &a, hipStream_t s) {
    int rc;
    const float *h_in = a.h_in ? a.h_in : h;
    if (a.project) {
        ProfScope ps(PC_NODE, s, a.scoped);
        if ((rc = td_launch_node_proj(L.nodeX2h, h_in, a.proj, 0x1f, TdRows{}, 0, a.P, a.q, s)) != TD_OK) return rc;
    }
    if (L.ew_x2h) {
        ProfScope ps(PC_GATE, s, a.scoped);
        if ((rc = td_launch_layer_gate(L.ew_x2h, L.offsets, L.coeff, xc, gt, TdRows{nullptr, nullptr, N}, s)) != TD_OK) return rc;
    }
    { ProfScope ps(PC_X2H_K, s, a.scoped); if ((rc = td_launch_edge_key16(L.hk, L, xc, gt, a.P, a.q, a.rows, a.lig, false, s)) != TD_OK) return rc; }
    if (h_in != h) TD_CHECK_HIP(hipMemcpyAsync(h, h_in, (size_t)N * TD_H * sizeof(float), hipMemcpyDeviceToDevice, s));
    // x2h_out_fc: the attention output goes to q (the queries are spent once the key pass is done) without the residual, and
    // node_output([output | h]) + h follows on every row
    float *att_out = L.nodeOut.B ? a.q : nullptr;
    { ProfScope ps(PC_X2H_V, s, a.scoped); if ((rc = td_launch_edge_value16(L.hv, L, xc, gt, a.P, a.rows, a.lig, h, att_out, s)) != TD_OK) return rc; }
    if (att_out) {
        ProfScope ps(PC_NODE, s, a.scoped);
        if ((rc = td_launch_node_output(L.nodeOut, att_out, h, N, s)) != TD_OK) return rc;
    }
    return TD_OK;
}

// h2x stage, projections in one launch: src-side (k_j, v_j) of the nodes a ligand atom can see -- `hop` (the ligand atoms and their
// neighbours, fixed for the step) when the caller has the list, every node otherwise -- plus, as a second segment, the dst-side
// projections and queries of the ligand atoms
int h2x_project(const TdLayer &L, Workspace &w, float *h, int64_t Nl, float *P, float *q, const TdRows &hop, hipStream_t s) {
    ProfScope ps(PC_NODE, s);
    return td_launch_node_proj(L.nodeH2x, h, hop, 0x0a, TdRows{w.lig_node, nullptr, Nl}, 0x15, P, q, s);
}

// attention over the ligand atoms' edges and the coordinate update xc -> xn.  Rows of several chunks (general graphs) take the
// two-launch form (keys + softmax over all chunks of a row -> alpha in memory -> xv); one 32-slot row per node: fused.
int h2x_attend(const td_model *m, const TdLayer &L, Workspace &w, const TdGraphTab &gt, int64_t Nl, float4 *xc, float4 *xn, float *P,
               float *q, hipStream_t s) {
    int rc;
    const TdRows lig{w.lig_node, nullptr, Nl};
    if (m->opt.h2x_fused && (!gt.cptr || (L.xk.use_split && L.xv.use_split))) {
        // (general graphs: the chunk-walking fused form exists for the bf16 first layer; alpha holds the logits between its two sweeps)
        ProfScope ps(PC_H2X_K, s);
        return td_launch_edge_h2x16(L.xk, L.xv, L, xc, xn, gt, P, q, lig, s);
    }
    {
        ProfScope ps(PC_H2X_K, s);
        if ((rc = td_launch_edge_key16(L.xk, L, xc, gt, P, q, lig, TdRows{}, true, s)) != TD_OK) return rc;
    }
    ProfScope ps(PC_H2X_V, s);
    return td_launch_edge_xv16(L.xv, L, xc, xn, gt, P, lig, s);
}

// A layer is NX x2h stages, one after the other on the layer's start coordinates, then NH h2x stages, each on the coordinates the previous one
// left and all on the last x2h stage's features (models/uni_transformer.py:190-206); stage i of layer l is m->layers[l * M + i].  With one
// stage of each kind (M == 1, the live architecture) projections are fused across stages -- the h2x stage of a layer and the x2h stage of
// the next project the same h: one pair launch; sync_twoup: both stages of a layer project its input features -- and a caching session's
// row lists prune the layers from the end.  Several stages per layer: every stage takes its own projections, every row.
int run_backbone(const td_model *m, Workspace &w, const TdGraphTab &gt, float *h, int64_t N, int64_t Nl, int fix_x, float4 **x_final,
                 hipStream_t s, const CachedStep &cs) {
    int rc;
    const int Lc = m->cfg.num_layers, NX = num_x2h(m->cfg), NH = num_h2x(m->cfg), M = stage_rows(m->cfg);
    const bool one = M == 1, sync = one && m->cfg.sync_twoup != 0;
    const int32_t *hop_rows = one ? cs.hop_rows : nullptr;
    // row list of receptive-field level k (1-based); every row without one
    const TdRows every{nullptr, nullptr, N}, lig{w.lig_node, nullptr, Nl};
    auto level = [&](int k) { return (hop_rows && k <= cs.hop_levels) ? TdRows{hop_rows + (size_t)(k - 1) * N, cs.hop_count + (k - 1), N} : every; };
    // Sampling session: only ligand outputs are consumed, so the layer e from the end updates receptive-field level e + 1
    // only, and its projections are needed on level e + 2 (those rows and their neighbours).
    auto att_rows = [&](int l) { return l > 0 ? level(Lc - 1 - l + 1) : every; };
    auto proj_rows = [&](int l) { return l > 0 ? level(Lc - 1 - l + 2) : every; };
    float4 *xc = w.x4a, *xn = w.x4b;
    const bool do_h2x = !fix_x && Nl > 0;
    if (do_h2x && cs.init_xn) TD_CHECK_HIP(hipMemcpyAsync(xn, xc, (size_t)N * sizeof(float4), hipMemcpyDeviceToDevice, s));
    const TdRows hop1 = level(1);
    // the projections of an h2x stage (hx) and of an x2h stage (nx, on the rows pr) from the same h: one launch
    auto project_pair = [&](const TdLayer &hx, const TdLayer &nx, const TdRows &pr) {
        ProfScope ps(PC_NODE, s);
        return td_launch_node_proj_pair(hx.nodeH2x, hop1, lig, w.Px, w.qx, nx.nodeX2h, pr, w.P, w.q, h, s);
    };
    bool proj_done = false;        // this layer's x2h-stage projections rode in the previous layer's paired launch
    for (int l = 0; l < Lc; ++l) {
        for (int i = 0; i < NX; ++i) {
            if (l == 0 && one && cs.layer0_x2h_done) continue;
            const TdLayer &L = m->layers[(size_t)l * M + i];
            X2hStage a;
            a.P = w.P; a.q = w.q; a.lig = lig;
            a.rows = att_rows(l);
            a.proj = proj_rows(l);
            const bool use_fwd = one && cs.fwd && l == 1 && !a.rows.rows;
            if (use_fwd) a.rows = cs.fwd->rows;
            // sync_twoup: the h2x stage reads the layer's input features, i.e. the h this stage's projections are taken from: both
            // stages' projections in one launch, before the value pass overwrites h
            if (sync && do_h2x && (rc = project_pair(L, L, a.proj)) != TD_OK) return rc;
            a.project = !proj_done && !(sync && do_h2x);
            proj_done = false;
            if ((rc = x2h_stage(L, gt, xc, h, N, a, s)) != TD_OK) return rc;
            if (use_fwd && (rc = td_launch_restore_rows(cs.fwd->rest, cs.fwd->hs, h, cs.fwd->nodes, cs.fwd->tabs, s)) != TD_OK) return rc;
        }
        if (!do_h2x) continue;
        for (int j = 0; j < NH; ++j) {
            const TdLayer &L = m->layers[(size_t)l * M + j];
            if (sync) {
                // (projections taken at the top of the layer)
            } else if (one && l + 1 < Lc) {
                // the h2x stage of this layer and the x2h stage of the next project the same h
                if ((rc = project_pair(L, m->layers[l + 1], proj_rows(l + 1))) != TD_OK) return rc;
                proj_done = true;
            } else if ((rc = h2x_project(L, w, h, Nl, w.Px, w.qx, hop1, s)) != TD_OK) {
                return rc;
            }
            if (L.ew_h2x) {              // the h2x stage's own gate, from the same (not yet updated) coordinates
                ProfScope ps(PC_GATE, s);
                if ((rc = td_launch_layer_gate(L.ew_h2x, L.offsets, L.coeff, xc, gt, every, s)) != TD_OK) return rc;
            }
            if ((rc = h2x_attend(m, L, w, gt, Nl, xc, xn, w.Px, w.qx, s)) != TD_OK) return rc;
            std::swap(xc, xn);
        }
    }
    *x_final = xc;
    return TD_OK;
}

// graph + edge gate of a composed batch on the default graph (32-slot rows: k-NN with k <= 32, radius with cap <= 32)
int build_default_graph(const td_model *m, const TdGraphTab &gt, const TdNodes &nodes, hipStream_t s) {
    int rc;
    {
        ProfScope ps(PC_KNN, s);
        if (m->cfg.cutoff_mode == TD_CUTOFF_RADIUS)
            rc = td_launch_radius32(nodes, m->cfg.radius, m->cfg.max_num_neighbors, gt.nbr, s);
        else
            rc = td_launch_knn(nodes, gt.nbr, m->cfg.knn, s);
        if (rc != TD_OK) return rc;
    }
    if (m->cfg.ew_net_type != 0) return TD_OK;          // 'r' / none: every stage computes its own gate (run_backbone)
    ProfScope ps(PC_GATE, s);
    return td_launch_gate(m->gate, nodes.x4, gt, table_rows(gt, nodes.N), s);
}

// td_debug_fail_alloc: the n-th stream-ordered allocation from now fails (fault injection for the error paths)
std::atomic<int> g_fail_alloc{0};
hipError_t td_malloc_async(void **p, size_t bytes, hipStream_t s) {
    int n = g_fail_alloc.load(std::memory_order_relaxed);
    while (n > 0 && !g_fail_alloc.compare_exchange_weak(n, n - 1)) {}
    if (n == 1) { *p = nullptr; return hipErrorOutOfMemory; }
    return hipMallocAsync(p, bytes, s);
}
void plan_destroy(GraphPlan &p, hipStream_t s) {
    free_async_or_sync(p.block, s);
    p.block = nullptr;
}

// host_pptr / host_lptr: [B+1] prefix offsets of the protein / ligand atoms (host copies)
int plan_create(const td_config &c, const int32_t *host_pptr, const int32_t *host_lptr, int64_t B, hipStream_t s, GraphPlan *out) {
    GraphPlan p;
    p.mode = c.cutoff_mode;
    p.k = c.cutoff_mode == TD_CUTOFF_RADIUS ? c.max_num_neighbors : c.knn;
    p.radius = c.radius;
    p.cpn_p = (p.k + TD_K - 1) / TD_K;
    p.B = B;
    p.Np = host_pptr[B]; p.Nl = host_lptr[B]; p.N = p.Np + p.Nl;
    std::vector<int32_t> meta((size_t)3 * (B + 1));
    int32_t *g_cbase = meta.data(), *g_cl = g_cbase + (B + 1), *g_lbase = g_cl + (B + 1);
    int64_t nc = 0, ncl = 0;
    for (int64_t g = 0; g < B; ++g) {
        const int np = host_pptr[g + 1] - host_pptr[g], nl = host_lptr[g + 1] - host_lptr[g];
        int cl = p.cpn_p;
        if (p.mode == TD_CUTOFF_HYBRID) { cl = (nl - 1 + p.k + TD_K - 1) / TD_K; if (cl < 1) cl = 1; }
        g_cbase[g] = (int32_t)nc; g_cl[g] = cl; g_lbase[g] = (int32_t)ncl;
        nc += (int64_t)np * p.cpn_p + (int64_t)nl * cl;
        ncl += (int64_t)nl * cl;
    }
    g_cbase[B] = (int32_t)nc; g_cl[B] = 0; g_lbase[B] = (int32_t)ncl;
    if (nc > 0x7fffffff / TD_K) { td_set_error("graph plan: %lld chunks overflow the 32-bit slot index", (long long)nc); return TD_EINVAL; }
    p.NC = nc; p.NCl = ncl;
    // one block, laid out twice: for its size, then bound (an empty buffer still takes 4 bytes)
    auto layout = [&](char *base) {
        Carver cv{base, 4};
        p.cptr = cv.take<int32_t>((size_t)(p.N + 1));
        p.chunk_node = cv.take<int32_t>((size_t)nc); p.lig_chunks = cv.take<int32_t>((size_t)ncl);
        p.cnbr = cv.take<int32_t>((size_t)nc * TD_K); p.ew = cv.take<float>((size_t)nc * TD_K);
        p.alpha = cv.take<float>((size_t)nc * TD_HEADS * TD_K);
        p.prot_node = cv.take<int32_t>((size_t)p.Np); p.pptr = cv.take<int32_t>((size_t)(B + 1));
        p.meta = cv.take<int32_t>(meta.size());
        return cv.off;
    };
    const size_t bytes = layout(nullptr);
    hipError_t e = td_malloc_async(reinterpret_cast<void **>(&p.block), bytes, s);
    if (e != hipSuccess) { td_set_error("graph plan: hipMallocAsync(%zu) failed: %s", bytes, hipGetErrorString(e)); return TD_ENOMEM; }
    layout(p.block);
    // the small per-graph tables: synchronous copies (the source vectors die with this frame)
    e = hipMemcpyAsync(p.meta, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p.pptr, host_pptr, (size_t)(B + 1) * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        td_set_error("graph plan: copying the per-graph tables failed: %s", hipGetErrorString(e));
        plan_destroy(p, s);
        return TD_EHIP;
    }
    *out = p;
    return TD_OK;
}

// cptr / chunk_node / lig_chunks from the per-graph tables (needs node_ptr and gid of the composed batch)
int plan_layout(GraphPlan &p, const int32_t *node_ptr, const int32_t *gid, hipStream_t s) {
    const int32_t *meta = p.meta;
    return td_launch_layout(node_ptr, p.pptr, gid, meta, meta + (p.B + 1), meta + 2 * (p.B + 1), p.cpn_p, p.N, p.cptr,
                            p.chunk_node, p.lig_chunks, (int32_t)p.NC, s);
}

// graph + edge gate of a composed batch on a general graph (chunked table of the plan)
int build_general_graph(const td_model *m, GraphPlan &p, Workspace &w, const TdGraphTab &gt, const TdNodes &nodes, int64_t Nl, hipStream_t s) {
    int rc;
    {
        ProfScope ps(PC_KNN, s);
        if ((rc = td_launch_graph_general(p.mode, nodes, TdRows{p.prot_node, nullptr, p.Np}, TdRows{w.lig_node, nullptr, Nl}, p.k, p.radius, gt,
                                          s)) != TD_OK) return rc;
    }
    ProfScope ps(PC_GATE, s);
    return td_launch_gate(m->gate, nodes.x4, gt, table_rows(gt, nodes.N), s);
}

// Every block of one denoiser evaluation (models/uni_transformer.py:306-323): graph + gate from the current coordinates (in w.x4a), then
// the layer stack.  A block that ends in x4b hands its coordinates to the next one by swapping the two buffers of `w` (the caller's own
// copy).  plan: the chunked table of a general graph; nullptr: the workspace's default graph.
int run_blocks(const td_model *m, Workspace &w, GraphPlan *plan, float *h, int64_t N, int64_t Nl, int fix_x, int max_graph_nodes,
               float4 **x_final, hipStream_t s) {
    int rc;
    const TdGraphTab gt = plan ? plan_tab(*plan) : default_tab(w);
    for (int blk = 0; blk < num_blocks(m->cfg); ++blk) {
        const TdNodes nodes{w.x4a, w.node_ptr, plan ? plan->pptr : nullptr, w.gid, N, plan ? plan->B : 0, max_graph_nodes};          // (x4a changes hands between blocks)
        rc = plan ? build_general_graph(m, *plan, w, gt, nodes, Nl, s) : build_default_graph(m, gt, nodes, s);
        if (rc != TD_OK) return rc;
        if ((rc = run_backbone(m, w, gt, h, N, Nl, fix_x, x_final, s)) != TD_OK) return rc;
        if (*x_final == w.x4b) std::swap(w.x4a, w.x4b);
    }
    return TD_OK;
}

// Plan of a composed batch given as (mask_ligand, node_ptr) -- the refine_net seam: per-graph protein / ligand counts and
// the protein row list are derived on the host (one round trip; compose_context order = protein rows first is required).
int plan_from_mask(const td_config &c, const uint8_t *d_mask, const int32_t *d_node_ptr, int64_t N, int64_t B, hipStream_t s,
                   GraphPlan *out, int64_t *nl_out) {
    std::vector<uint8_t> mask((size_t)N);
    std::vector<int32_t> nptr((size_t)B + 1);
    TD_CHECK_HIP(hipMemcpyAsync(mask.data(), d_mask, (size_t)N, hipMemcpyDeviceToHost, s));
    TD_CHECK_HIP(hipMemcpyAsync(nptr.data(), d_node_ptr, (size_t)(B + 1) * 4, hipMemcpyDeviceToHost, s));
    TD_CHECK_HIP(hipStreamSynchronize(s));
    std::vector<int32_t> hp((size_t)B + 1, 0), hl((size_t)B + 1, 0), prot;
    prot.reserve((size_t)N);
    for (int64_t g = 0; g < B; ++g) {
        int np = 0, nl = 0;
        for (int i = nptr[g]; i < nptr[g + 1]; ++i) {
            if (mask[(size_t)i]) ++nl;
            else {
                if (nl) { td_set_error("general graphs need compose_context order (protein rows first inside every graph)"); return TD_EINVAL; }
                ++np;
                prot.push_back(i);
            }
        }
        hp[g + 1] = hp[g] + np; hl[g + 1] = hl[g] + nl;
    }
    int rc = plan_create(c, hp.data(), hl.data(), B, s, out);
    if (rc != TD_OK) return rc;
    if (!prot.empty()) {
        hipError_t e = hipMemcpyAsync(out->prot_node, prot.data(), prot.size() * 4, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            td_set_error("graph plan: copying the protein row list failed: %s", hipGetErrorString(e));
            plan_destroy(*out, s);
            return TD_EHIP;
        }
    }
    *nl_out = hl[B];
    return TD_OK;
}

// host copies of two [B+1] device arrays (one synchronisation)
int fetch_ptrs(const int32_t *d_a, const int32_t *d_b, int64_t B, std::vector<int32_t> &a, std::vector<int32_t> &b, hipStream_t s) {
    a.resize((size_t)B + 1); b.resize((size_t)B + 1);
    TD_CHECK_HIP(hipMemcpyAsync(a.data(), d_a, (size_t)(B + 1) * 4, hipMemcpyDeviceToHost, s));
    TD_CHECK_HIP(hipMemcpyAsync(b.data(), d_b, (size_t)(B + 1) * 4, hipMemcpyDeviceToHost, s));
    TD_CHECK_HIP(hipStreamSynchronize(s));
    return TD_OK;
}
}  // namespace tdapi

extern "C" size_t td_workspace_bytes(const td_model *m, int64_t N, int64_t B, int64_t N_l) {
    (void)m;
    return carve(nullptr, N, B, N_l).bytes;
}
