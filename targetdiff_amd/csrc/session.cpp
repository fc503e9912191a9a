// C ABI of libtargetdiff_hip.so, part 5 of 5: the sampling session (one ScorePosNet3D.sample_diffusion call): static-protein caching,
// the per-step launch sequence and its hipGraph capture.
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <vector>

#include "td_device.h"
#include "td_internal.h"
#include "td_api.h"

using namespace tdapi;

// ------------------------------------------------------------------------------------------ sampling session
// State of one ScorePosNet3D.sample_diffusion call (models/molopt_score_model.py:633-703).  Everything that depends
// only on the protein is loop-invariant there (protein_pos, protein_v, batch_protein are passed unchanged to every
// forward, :652-661; protein coordinates are never updated, models/uni_transformer.py:206) and is computed once:
// embeddings, protein-only sorted neighbour lists, and -- for protein atoms that no ligand atom displaces from
// their k-NN row ("clean" rows, 80-90 % of them) -- the edge gate row and the layer-0 x2h output.
// Three kinds:
//   CACHING, default graph    k-NN with k <= 32: one 32-slot row per node (the workspace's nbr / ew / alpha)
//   CACHING, general graph    k-NN with 32 < k <= 64 and `hybrid` (protein rows are plain k-NN rows there too): the same
//                             machinery on the chunked table of a GraphPlan -- 64 static keys per protein row, cached gate
//                             chunks, chunk-aware row lists, the chunk-loop edge kernels
//   PLAIN                     radius graphs (rows in index order: no sorted lists to merge into) and graphs too large for
//                             the row-list kernel's LDS flags: every step is a stateless forward on the session's layout
struct td_session {
    const td_model *m;
    int64_t N, Np, Nl, B;
    int max_graph_nodes;
    char *block;
    hipStream_t last_stream;     // stream of the latest call: the block is freed in its order
    Workspace w;                 // per-step buffers (x4a/x4b, gid, nbr, lig_node, node_ptr, ew, P, q, h, alpha)
    int32_t *prot_node, *pptr, *lptr, *dirty_rows, *dirty_count, *hop_rows, *hop_count, *dirty_chunks;
    int hop_levels;
    TdStaticTabs tabs;           // static protein tables (skeys, snbr, h0, h1s, ews; cgraph / cbase when they are shared per pocket)
    float *h2s, *P0, *q0;
    uint8_t *flags2;
    int32_t *fwd_rows, *fwd_rest, *fwd_counts;
    bool use_fwd;
    uint8_t *clean;
    float *setup_lpos; int64_t *setup_lv; int32_t *canon_rows;          // set-up only: zero ligand atoms for the first compose, the canonical graphs' protein rows
    int graph_nodes_max;         // exact size of the largest graph -- sizes the LDS flags of td_launch_step_lists
    // Per-pocket sharing of the static tables (CACHING, default graph; model option session_share_pockets): all samples of a pocket carry the
    // same protein block (scripts/sample_diffusion.py:42 replicates one pocket n_data times), so `tabs` and h2s are kept ONCE per distinct
    // block -- `static_rows` compact rows, the canonical graphs' protein atoms back to back (TdStaticTabs::cgraph / cbase).  P0 / q0 (the
    // layer-0 projections the attention passes gather through the neighbour index) stay per node.
    int64_t static_rows = 0;
    int pocket_groups = 0;
    bool caching;                // static-protein caching + receptive-field pruning (false: PLAIN)
    bool chunked;                // general graph: the neighbour table lives in `plan`
    GraphPlan plan;
    // td_session_step: the denoiser's outputs of the step, and the step as a captured graph
    float *pred_pos, *pred_v;
    hipGraph_t graph;
    hipGraphExec_t graph_exec;
    td_step_io graph_io;         // the arguments the graph was captured with
    unsigned graph_epoch = 0;    // ... and the model's option epoch at that time
    int eager_steps;             // steps issued launch by launch so far (the first one also does the one-time kernel set-up)
    bool graph_failed, last_step_graph;
    // time program (td_session_set_program): the caller's device table, the slot kinds, and the slot the next td_session_step runs
    const float *prog_table = nullptr;
    std::vector<int32_t> prog_kinds;
    size_t prog_next = 0;
    // clash guidance (td_session_set_guidance): the centred protein + radii as float4 and the step's shift, in a block of their own
    // (allocated at the first call, kept until the session goes); guide = on
    char *guide_block = nullptr;
    float4 *guide_prot4 = nullptr;
    float *guide_shift = nullptr;
    bool guide = false;
    float guide_w = 0.f, guide_max = 0.f;
};

namespace tdapi {
constexpr int TD_STEP_LISTS_MAX_NODES = 12288;       // LDS flags of step_lists_kernel: 4 bytes per node of a graph, 48 KiB

TdGraphTab session_tab(td_session *S) {
    TdGraphTab gt = S->chunked ? plan_tab(S->plan) : default_tab(S->w);
    if (S->caching) gt.mixed = S->dirty_count;
    return gt;
}
// the session's batch as the graph launchers of a CACHING session read it (a general graph knows its largest graph exactly)
TdNodes session_nodes(const td_session *S) {
    return TdNodes{S->w.x4a, S->w.node_ptr, S->pptr, S->w.gid, S->N, S->B, S->chunked ? S->graph_nodes_max : S->max_graph_nodes};
}

// stream-ordered free with a fallback: the stream may have been destroyed by the caller in the meantime (a C-ABI user with its own
// hipStreamCreate / hipStreamDestroy) -- then synchronise the device and free synchronously instead of leaking the block
void free_async_or_sync(void *p, hipStream_t s) {
    if (!p) return;
    if (hipFreeAsync(p, s) == hipSuccess) return;
    (void)hipGetLastError();
    (void)hipDeviceSynchronize();
    (void)hipFree(p);
}

void session_drop_graph(td_session *S) {
    // the previous replay may still be in flight on the stream it was launched on (an option change between two steps lands here):
    // whether destroying an executing graph is deferred depends on the runtime version, so wait for it.  Cold path.
    if (S->graph_exec) (void)hipStreamSynchronize(S->last_stream);
    if (S->graph_exec) (void)hipGraphExecDestroy(S->graph_exec);
    if (S->graph) (void)hipGraphDestroy(S->graph);
    S->graph_exec = nullptr;
    S->graph = nullptr;
}

void session_free(td_session *S, hipStream_t s) {
    if (!S) return;
    session_drop_graph(S);
    if (S->chunked) plan_destroy(S->plan, s);
    free_async_or_sync(S->block, s);
    free_async_or_sync(S->guide_block, s);
    delete S;
}
}  // namespace tdapi

namespace {
// the session object until td_session_create hands it out: whatever it owns by then goes back on every other way out
struct SessionGuard {
    td_session *S; hipStream_t s;
    ~SessionGuard() { session_free(S, s); }
};

// Per-pocket sharing of the static tables: which graphs carry the same protein block, bit for bit?  cgraph[g] = the first graph of the
// batch with graph g's block (its canonical graph), cbase[g] = where that graph's rows start in the compact tables, canon_rows = the
// protein nodes of the canonical graphs back to back: the rows of the compact tables.
struct PocketGroups { std::vector<int32_t> cgraph, cbase, canon_rows; int groups = 0; };
int group_pockets(const td_model *m, const float *d_protein_pos, const float *d_protein_v, const int32_t *d_protein_ptr, int64_t B,
                  const std::vector<int32_t> &hp, const std::vector<int32_t> &hl, hipStream_t s, PocketGroups *out) {
    const int F = m->cfg.protein_feat_dim;
    const size_t nb = (size_t)B;
    unsigned long long *d_hash = nullptr;
    int32_t *d_cand = nullptr, *d_flag = nullptr;
    auto layout = [&](char *base) {
        Carver c{base};
        d_hash = c.take<unsigned long long>(nb);
        d_cand = c.take<int32_t>(nb); d_flag = c.take<int32_t>(nb);
        return c.off;
    };
    AsyncScratch tmp(s);
    char *block = nullptr;
    int rc;
    if ((rc = tmp.take(&block, layout(nullptr), "td_session_create")) != TD_OK) return rc;
    layout(block);
    std::vector<unsigned long long> hash(nb);
    std::vector<int32_t> flag(nb, 0);
    out->cgraph.assign(nb, 0); out->cbase.assign(nb, 0);
    if ((rc = td_launch_pocket_hash(d_protein_pos, d_protein_v, d_protein_ptr, B, F, d_hash, s)) != TD_OK) return rc;
    TD_CHECK_HIP(hipMemcpyAsync(hash.data(), d_hash, nb * 8, hipMemcpyDeviceToHost, s));
    TD_CHECK_HIP(hipStreamSynchronize(s));
    {   // candidate = the first graph of the batch with the same (atom count, hash): an ordered map, B log B for any mix of pockets
        std::map<std::pair<int32_t, unsigned long long>, int32_t> first;
        for (int64_t g = 0; g < B; ++g)
            out->cgraph[(size_t)g] = first.emplace(std::make_pair(hp[g + 1] - hp[g], hash[(size_t)g]), (int32_t)g).first->second;
    }
    TD_CHECK_HIP(hipMemcpyAsync(d_cand, out->cgraph.data(), nb * 4, hipMemcpyHostToDevice, s));
    TD_CHECK_HIP(hipMemsetAsync(d_flag, 0, nb * 4, s));
    if ((rc = td_launch_pocket_verify(d_protein_pos, d_protein_v, d_protein_ptr, B, F, d_cand, d_flag, s)) != TD_OK) return rc;
    TD_CHECK_HIP(hipMemcpyAsync(flag.data(), d_flag, nb * 4, hipMemcpyDeviceToHost, s));
    TD_CHECK_HIP(hipStreamSynchronize(s));
    for (int64_t g = 0; g < B; ++g) {
        if (flag[(size_t)g]) out->cgraph[(size_t)g] = (int32_t)g;          // same hash, different block: keeps its own tables
        const int32_t c = out->cgraph[(size_t)g];
        if (c == (int32_t)g) {
            out->cbase[(size_t)g] = (int32_t)out->canon_rows.size();
            const int32_t n0 = hp[g] + hl[g], np = hp[g + 1] - hp[g];          // the graph's nodes start at node_ptr[g]; protein atoms first
            for (int32_t a = 0; a < np; ++a) out->canon_rows.push_back(n0 + a);
            ++out->groups;
        } else {
            out->cbase[(size_t)g] = out->cbase[(size_t)c];
        }
    }
    return TD_OK;
}

// The session's device block, [workspace | session-static buffers]: with base == nullptr its size, otherwise every buffer bound.  The
// one place that knows what the block holds.  share: the static tables have S->static_rows compact rows, not one per node.
size_t session_layout(td_session *S, char *base, bool share) {
    S->w = carve(base, S->N, S->B, S->Nl);
    Carver c{base ? base + S->w.bytes : nullptr, 4};
    const size_t n = (size_t)S->N, np = (size_t)S->Np, nl = (size_t)S->Nl, nb = (size_t)S->B;
    const size_t nc = S->chunked ? (size_t)S->plan.NC : n;          // 32-slot rows of the neighbour table
    const size_t ks = S->chunked ? 64 : TD_K;                       // static keys kept per protein row
    const size_t ns = share ? (size_t)S->static_rows : n, ncs = share ? (size_t)S->static_rows : nc;          // rows of the static tables
    const size_t C = S->caching ? 1 : 0;                            // (a PLAIN session keeps none of the caching tables)
    S->prot_node = c.take<int32_t>(np);
    S->pptr = c.take<int32_t>(nb + 1); S->lptr = c.take<int32_t>(nb + 1);
    S->tabs.h0 = c.take<float>(ns * TD_H);
    S->setup_lpos = c.take<float>(nl * 3); S->setup_lv = c.take<int64_t>(nl);
    S->tabs.snbr = c.take<int32_t>(C * ncs * TD_K);
    S->tabs.skeys = c.take<unsigned long long>(C * ns * ks);
    S->tabs.ews = c.take<float>(C * ncs * TD_K);
    S->tabs.h1s = c.take<float>(C * ns * TD_H); S->h2s = c.take<float>(C * ns * TD_H);
    S->flags2 = c.take<uint8_t>(C * n);
    S->fwd_rows = c.take<int32_t>(C * n); S->fwd_rest = c.take<int32_t>(C * n); S->fwd_counts = c.take<int32_t>(64);
    S->P0 = c.take<float>(C * n * 4 * TD_H); S->q0 = c.take<float>(C * n * TD_H);
    S->clean = c.take<uint8_t>(C * n);
    S->dirty_rows = c.take<int32_t>(C * n); S->dirty_count = c.take<int32_t>(64);          // counts: [0] rows, [1] chunks (general graphs)
    S->hop_rows = c.take<int32_t>(C * n * TD_HOP_LEVELS); S->hop_count = c.take<int32_t>(64);
    S->dirty_chunks = c.take<int32_t>(S->chunked ? C * nc : 0);
    S->pred_pos = c.take<float>(nl * 3); S->pred_v = c.take<float>(nl * TD_MAXC);
    S->tabs.cgraph = c.take<int32_t>(share ? nb : 0); S->tabs.cbase = c.take<int32_t>(share ? nb : 0);
    S->canon_rows = c.take<int32_t>(share ? ns : 0);
    if (!share) S->tabs.cgraph = S->tabs.cbase = S->canon_rows = nullptr;          // (nullptr: tables indexed by node)
    return S->w.bytes + c.off;
}

// Fills a bound session block: the packed batch (ligand rows are placeholders until the first step) and, for a CACHING session, the
// protein-only graph, its gate rows, the layer-0 projections / queries and the layer-0 / layer-1 x2h outputs.  With sharing all of it runs
// on the canonical graphs' protein rows only, into full-size (node-indexed) scratch tables whose canonical rows are then compacted into
// the shared tables.
int session_build_static(td_session *S, const float *d_protein_pos, const float *d_protein_v, const int32_t *d_protein_ptr,
                         const int32_t *d_ligand_ptr, const PocketGroups &pg, hipStream_t s) {
    const td_model *m = S->m;
    const int64_t N = S->N, N_p = S->Np, N_l = S->Nl, B = S->B;
    const size_t n = (size_t)N, nb = (size_t)B;
    const bool share = S->tabs.cgraph != nullptr;
    const TdStaticTabs &T = S->tabs;
    Workspace &w = S->w;
    int rc;
    TD_CHECK_HIP(hipMemcpyAsync(S->pptr, d_protein_ptr, (nb + 1) * 4, hipMemcpyDeviceToDevice, s));
    TD_CHECK_HIP(hipMemcpyAsync(S->lptr, d_ligand_ptr, (nb + 1) * 4, hipMemcpyDeviceToDevice, s));
    TD_CHECK_HIP(hipMemsetAsync(S->setup_lpos, 0, (size_t)N_l * 12, s));
    TD_CHECK_HIP(hipMemsetAsync(S->setup_lv, 0, (size_t)N_l * 8, s));
    AsyncScratch scratch(s);          // (goes back in stream order when this function returns: after the compaction, or on an error)
    unsigned long long *skeys_f = T.skeys;
    int32_t *snbr_f = T.snbr;
    float *ews_f = T.ews, *h0_f = T.h0, *h1_f = T.h1s, *h2_f = S->h2s;
    if (share) {
        auto layout = [&](char *base) {
            Carver c{base};
            skeys_f = c.take<unsigned long long>(n * TD_K);
            snbr_f = c.take<int32_t>(n * TD_K); ews_f = c.take<float>(n * TD_K);
            h0_f = c.take<float>(n * TD_H); h1_f = c.take<float>(n * TD_H); h2_f = c.take<float>(n * TD_H);
            return c.off;
        };
        char *block = nullptr;
        if ((rc = scratch.take(&block, layout(nullptr), "td_session_create")) != TD_OK) return rc;
        layout(block);
        TD_CHECK_HIP(hipMemcpyAsync(T.cgraph, pg.cgraph.data(), nb * 4, hipMemcpyHostToDevice, s));
        TD_CHECK_HIP(hipMemcpyAsync(T.cbase, pg.cbase.data(), nb * 4, hipMemcpyHostToDevice, s));
        TD_CHECK_HIP(hipMemcpyAsync(S->canon_rows, pg.canon_rows.data(), pg.canon_rows.size() * 4, hipMemcpyHostToDevice, s));
        TD_CHECK_HIP(hipStreamSynchronize(s));          // (the host vectors go out of scope with td_session_create)
    }
    // embeddings + packed order, protein row list
    int32_t *prot_out = S->chunked ? S->plan.prot_node : S->prot_node;
    if ((rc = td_launch_compose(m, d_protein_pos, d_protein_v, S->pptr, N_p, S->setup_lpos, S->setup_lv, S->lptr, N_l, B, h0_f, w.x4a,
                                w.node_ptr, w.gid, w.lig_node, prot_out, nullptr, s)) != TD_OK) return rc;
    if (S->chunked) {
        S->prot_node = S->plan.prot_node;
        if ((rc = plan_layout(S->plan, w.node_ptr, w.gid, s)) != TD_OK) return rc;
    }
    TD_CHECK_HIP(hipMemcpyAsync(w.x4b, w.x4a, n * sizeof(float4), hipMemcpyDeviceToDevice, s));
    if (!S->caching) return TD_OK;
    // ---- protein-only graph, its gate rows, layer-0 projections / queries, layer-0 x2h output
    const TdRows set{share ? S->canon_rows : S->prot_node, nullptr, share ? S->static_rows : N_p};          // the rows of the static tables
    const int32_t *set_rows = set.rows;
    const int64_t set_count = set.count;
    const size_t nc = S->chunked ? (size_t)S->plan.NC : n;
    const TdNodes nodes = session_nodes(S);
    const TdGraphTab gt = session_tab(S);
    TdGraphTab st = gt;                            // the static table: its own nbr / ew, the step's alpha as scratch
    st.nbr = snbr_f; st.ew = ews_f;
    TD_CHECK_HIP(hipMemsetAsync(snbr_f, 0xff, nc * TD_K * 4, s));
    if (S->chunked) {
        if ((rc = td_launch_knn_general_static(nodes, set, m->cfg.knn, st, skeys_f, s)) != TD_OK) return rc;
        if ((rc = td_launch_gate(m->gate, w.x4a, st, table_rows(st, N), s)) != TD_OK) return rc;
        // the step's table: ligand rows start as all pads; hybrid: their ligand half never changes
        TD_CHECK_HIP(hipMemsetAsync(gt.nbr, 0xff, nc * TD_K * 4, s));
        TD_CHECK_HIP(hipMemsetAsync(gt.ew, 0, nc * TD_K * 4, s));
        if (m->cfg.cutoff_mode == TD_CUTOFF_HYBRID &&
            (rc = td_launch_hybrid_ligand_half(nodes, TdRows{w.lig_node, nullptr, N_l}, gt, s)) != TD_OK) return rc;
    } else {
        if ((rc = td_launch_knn_static(nodes, set, st.nbr, skeys_f, m->cfg.knn, s)) != TD_OK) return rc;
        if ((rc = td_launch_gate(m->gate, w.x4a, st, set, s)) != TD_OK) return rc;
    }
    // (no profile scopes: set-up; the rows' input features stay -- h0 / h1s are tables of their own)
    X2hStage a;
    a.P = S->P0; a.q = S->q0; a.scoped = false;
    a.proj = TdRows{nullptr, nullptr, N};
    a.rows = set;
    a.h_in = h0_f;
    if ((rc = x2h_stage(m->layers[0], st, w.x4a, h1_f, N, a, s)) != TD_OK) return rc;
    if (S->use_fwd) {      // layer-1 x2h output of the protein-only graph (valid wherever the ligand is two hops away)
        a.P = w.P; a.q = w.q; a.h_in = h1_f;
        if ((rc = x2h_stage(m->layers[1], st, w.x4a, h2_f, N, a, s)) != TD_OK) return rc;
    }
    if (share) {           // the canonical rows of the scratch tables -> the compact shared tables
        if ((rc = td_launch_compact_rows(skeys_f, set_rows, set_count, TD_K * 8, T.skeys, s)) != TD_OK) return rc;
        if ((rc = td_launch_compact_rows(snbr_f, set_rows, set_count, TD_K * 4, T.snbr, s)) != TD_OK) return rc;
        if ((rc = td_launch_compact_rows(ews_f, set_rows, set_count, TD_K * 4, T.ews, s)) != TD_OK) return rc;
        if ((rc = td_launch_compact_rows(h0_f, set_rows, set_count, TD_H * 4, T.h0, s)) != TD_OK) return rc;
        if ((rc = td_launch_compact_rows(h1_f, set_rows, set_count, TD_H * 4, T.h1s, s)) != TD_OK) return rc;
        if (S->use_fwd && (rc = td_launch_compact_rows(h2_f, set_rows, set_count, TD_H * 4, S->h2s, s)) != TD_OK) return rc;
    }
    return TD_OK;
}
}  // namespace

extern "C" int td_session_create(const td_model *m, const float *d_protein_pos, const float *d_protein_v,
                                 const int32_t *d_protein_ptr, int64_t N_p, const int32_t *d_ligand_ptr, int64_t N_l,
                                 int64_t B, int32_t max_graph_nodes, void *stream, td_session **out) {
    if (!m || !out || N_p <= 0 || N_l <= 0 || B <= 0 || !d_protein_pos || !d_protein_v || !d_protein_ptr || !d_ligand_ptr) {
        td_set_error("td_session_create: bad argument");
        return TD_EINVAL;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    td_session *S = new (std::nothrow) td_session();
    if (!S) { td_set_error("td_session_create: out of host memory"); return TD_ENOMEM; }
    SessionGuard guard{S, s};
    S->m = m; S->N = N_p + N_l; S->Np = N_p; S->Nl = N_l; S->B = B; S->max_graph_nodes = max_graph_nodes; S->last_stream = s;
    int rc;
    // per-graph atom counts: the exact size of the largest graph, and the chunk layout of a general graph
    std::vector<int32_t> hp, hl;
    if ((rc = fetch_ptrs(d_protein_ptr, d_ligand_ptr, B, hp, hl, s)) != TD_OK) return rc;
    int gmax = 0;
    for (int64_t g = 0; g < B; ++g) gmax = std::max(gmax, (hp[g + 1] - hp[g]) + (hl[g + 1] - hl[g]));
    S->graph_nodes_max = gmax;
    S->chunked = !default_graph(m->cfg);
    const bool knn_like = m->cfg.cutoff_mode == TD_CUTOFF_KNN || m->cfg.cutoff_mode == TD_CUTOFF_HYBRID;
    S->caching = knn_like && (!S->chunked || gmax <= TD_STEP_LISTS_MAX_NODES) && num_blocks(m->cfg) == 1 && m->cfg.ew_net_type == 0 &&
                 !m->cfg.x2h_out_fc && !m->cfg.sync_twoup && stage_rows(m->cfg) == 1;      // (the static-protein tables hold the global gate's rows and plain x2h outputs;
                                                                 // a cached layer 0 skips the projections sync_twoup takes at its top)
    S->use_fwd = S->caching && m->opt.session_forward_reach && m->cfg.num_layers >= 2;
    // receptive-field levels tracked per step (each prunes one more layer from the end)
    S->hop_levels = std::min(std::min(std::max(m->opt.session_hop_levels, 1), TD_HOP_LEVELS), m->cfg.num_layers);
    if (S->chunked && (rc = plan_create(m->cfg, hp.data(), hl.data(), B, s, &S->plan)) != TD_OK) return rc;
    // the three phases: pocket groups (default graph, model option session_share_pockets), the device block, its contents
    const bool share = S->caching && !S->chunked && m->opt.session_share_pockets != 0;
    PocketGroups pg;
    if (share) {
        if ((rc = group_pockets(m, d_protein_pos, d_protein_v, d_protein_ptr, B, hp, hl, s, &pg)) != TD_OK) return rc;
        S->static_rows = (int64_t)pg.canon_rows.size();
        S->pocket_groups = pg.groups;
    }
    const size_t bytes = session_layout(S, nullptr, share);
    hipError_t e = td_malloc_async(reinterpret_cast<void **>(&S->block), bytes, s);
    if (e != hipSuccess) { S->block = nullptr; td_set_error("td_session_create: hipMallocAsync(%zu) failed: %s", bytes, hipGetErrorString(e)); return TD_ENOMEM; }
    session_layout(S, S->block, share);
    if ((rc = session_build_static(S, d_protein_pos, d_protein_v, d_protein_ptr, d_ligand_ptr, pg, s)) != TD_OK) return rc;
    *out = S;
    guard.S = nullptr;
    return TD_OK;
}

extern "C" void td_session_destroy(td_session *S) {
    if (!S) return;
    session_free(S, S->last_stream);
}

extern "C" int td_session_forward(td_session *S, const float *d_ligand_pos, const int64_t *d_ligand_v,
                                  float *d_pred_ligand_pos, float *d_pred_ligand_v, float *d_final_ligand_h,
                                  const float *d_ligand_graph_bias, void *stream) {
    if (!S || !d_ligand_pos || !d_ligand_v || !d_pred_ligand_pos || !d_pred_ligand_v) {
        td_set_error("td_session_forward: null pointer");
        return TD_EINVAL;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    S->last_stream = s;
    const td_model *m = S->m;
    Workspace &w = S->w;
    const int64_t N = S->N, Nl = S->Nl;
    const TdGraphTab gt = session_tab(S);
    const TdNodes nodes = session_nodes(S);
    const TdRows prot{S->prot_node, nullptr, S->Np}, lig{w.lig_node, nullptr, Nl};
    const TdRows dirty{S->dirty_rows, S->dirty_count, N};
    uint8_t *const flags2 = S->use_fwd ? S->flags2 : nullptr;          // forward-reach flags, cleared by the step's first launches
    int rc;
    if (!S->caching) {
        {
            ProfScope ps(PC_COMPOSE, s);
            TD_CHECK_HIP(hipMemcpyAsync(w.h, S->tabs.h0, (size_t)N * TD_H * sizeof(float), hipMemcpyDeviceToDevice, s));
            if ((rc = td_launch_ligand_update(m, d_ligand_pos, d_ligand_v, lig, w.h, w.x4a, nullptr, d_ligand_graph_bias, w.gid, s)) != TD_OK) return rc;
        }
        float4 *xg = nullptr;
        Workspace wb = w;             // (the block loop swaps x4a / x4b of its workspace: the session's own stays as it is)
        if ((rc = run_blocks(m, wb, S->chunked ? &S->plan : nullptr, wb.h, N, Nl, 0, S->max_graph_nodes, &xg, s)) != TD_OK) return rc;
        ProfScope ps(PC_HEAD, s);
        return td_launch_head(m->head, w.h, xg, w.lig_node, Nl, m->cfg.ligand_num_classes, d_pred_ligand_pos, d_pred_ligand_v,
                              d_final_ligand_h, s);
    }
    {
        // first kernel of the step: also zeroes the row-list counters and the ligand rows' forward-reach flags
        ProfScope ps(PC_COMPOSE, s);
        TdStepReset rs;
        rs.c0 = S->dirty_count; rs.n0 = 2;
        rs.c1 = S->fwd_counts; rs.n1 = 2;
        rs.c2 = S->hop_count; rs.n2 = TD_HOP_LEVELS;
        rs.flags2 = flags2;
        if ((rc = td_launch_ligand_update(m, d_ligand_pos, d_ligand_v, lig, w.h, w.x4a, &rs, d_ligand_graph_bias, w.gid, s)) != TD_OK) return rc;
    }
    bool lists_done = false;
    {
        ProfScope ps(PC_KNN, s);
        const TdStepLists lists{S->dirty_rows, S->dirty_count, S->use_fwd ? S->fwd_rows : nullptr, S->fwd_rest, S->fwd_counts,
                                S->hop_rows, S->hop_count, S->hop_levels, S->chunked ? S->dirty_chunks : nullptr,
                                S->chunked ? S->dirty_count + 1 : nullptr};
        if (S->chunked) {
            if ((rc = td_launch_knn_merge_general(nodes, prot, S->tabs, gt, w.h, S->clean, flags2, m->cfg.knn, s)) != TD_OK) return rc;
            if ((rc = td_launch_ligand_rows_general(S->plan.mode, nodes, lig, S->plan.k, gt, s)) != TD_OK) return rc;
            // every row list of the step in one launch (the session is CACHING only when every graph fits its LDS flags)
            if ((rc = td_launch_step_lists(S->clean, nodes, gt, S->graph_nodes_max, lists, s)) != TD_OK) {
                if (rc == TD_EINVAL) td_set_error("td_session_forward: a graph of %d nodes does not fit the row-list kernel", S->graph_nodes_max);
                return rc;
            }
            lists_done = true;
        } else {
            // the protein rows' merge and the ligand rows' full search: independent, one launch
            if ((rc = td_launch_knn_merge(nodes, prot, lig, S->tabs, gt, w.h, S->clean, flags2, m->cfg.knn, s)) != TD_OK) return rc;
            // every row list of the step (dirty rows, forward reach, receptive-field levels) in one launch, one workgroup per graph;
            // graphs too large for its LDS flags take the separate kernels
            rc = (m->opt.session_step_lists && S->graph_nodes_max > 0) ? td_launch_step_lists(S->clean, nodes, gt, S->graph_nodes_max, lists, s) : TD_EINVAL;
            lists_done = rc == TD_OK;
            if (rc != TD_OK && rc != TD_EINVAL) return rc;
            if (!lists_done) {
                if ((rc = td_launch_compact_dirty(S->clean, w.x4a, N, S->dirty_rows, S->dirty_count, s)) != TD_OK) return rc;
                // S->clean gets its second life as the receptive-field flags below: the forward-reach compaction (its last reader)
                // clears it; without the forward reach a memset does
                if (S->use_fwd) {
                    if ((rc = td_launch_forward_reach(S->clean, w.x4a, w.nbr, N, S->flags2, S->fwd_rows, S->fwd_rest, S->fwd_counts,
                                                      S->clean, s)) != TD_OK) return rc;
                } else {
                    TD_CHECK_HIP(hipMemsetAsync(S->clean, 0, (size_t)N, s));
                }
            }
        }
    }
    {
        ProfScope ps(PC_GATE, s);
        // the gate rows of the dirty rows: their chunks on a general graph
        const TdRows gate_rows = S->chunked ? TdRows{S->dirty_chunks, S->dirty_count + 1, gt.NC} : dirty;
        if ((rc = td_launch_gate(m->gate, w.x4a, gt, gate_rows, s)) != TD_OK) return rc;
    }
    {   // layer 0, x2h: only ligand rows need new projections, only dirty rows need the attention passes
        X2hStage a;
        a.P = S->P0; a.q = S->q0; a.lig = lig;
        a.proj = lig;
        a.rows = dirty;
        if ((rc = x2h_stage(m->layers[0], gt, w.x4a, w.h, N, a, s)) != TD_OK) return rc;
    }
    // rows the last layer still has to update (S->clean is free again after the dirty-row compaction: reuse as flags)
    if (!lists_done && (rc = td_launch_hop_levels(lig, gt, N, S->clean, S->hop_rows, S->hop_count, S->hop_levels, true, s)) != TD_OK) return rc;
    float4 *xf = nullptr;
    const FwdReach fwd{TdRows{S->fwd_rows, S->fwd_counts, N}, TdRows{S->fwd_rest, S->fwd_counts + 1, N}, S->h2s, nodes, S->tabs};
    CachedStep cs;
    cs.init_xn = false; cs.layer0_x2h_done = true;
    cs.hop_rows = S->hop_rows; cs.hop_count = S->hop_count; cs.hop_levels = S->hop_levels;
    cs.fwd = S->use_fwd ? &fwd : nullptr;
    if ((rc = run_backbone(m, w, gt, w.h, N, Nl, 0, &xf, s, cs)) != TD_OK) return rc;
    ProfScope ps(PC_HEAD, s);
    return td_launch_head(m->head, w.h, xf, w.lig_node, Nl, m->cfg.ligand_num_classes, d_pred_ligand_pos,
                          d_pred_ligand_v, d_final_ligand_h, s);
}

namespace {
// the argument blocks of a step's update kernel (posterior or renoise): the state is updated in place, slot s of the trajectories filled
TdStepArgs step_args(const td_session *S, const td_step_io &io) {
    const td_model *m = S->m;
    TdStepArgs a;
    a.lptr = S->lptr; a.Nl = S->Nl; a.B = (int)S->B;
    a.C = m->cfg.ligand_num_classes; a.T = m->cfg.num_timesteps; a.mean_type = m->cfg.model_mean_type;
    a.pos = io.d_ligand_pos; a.v = io.d_ligand_v; a.pos_cur = io.d_ligand_pos; a.v_cur = io.d_ligand_v;
    a.pred_pos = S->pred_pos; a.pred_v = S->pred_v; a.noise = io.d_noise; a.uni = io.d_uniform;
    a.fixed_mask = io.d_fixed_mask; a.fixed_pos = io.d_fixed_pos; a.fixed_v = io.d_fixed_v;
    a.x0_shift = S->guide ? S->guide_shift : nullptr;
    return a;
}
TdStepSlot step_slot(const td_session *S, const td_step_io &io) {
    TdStepSlot sl;
    sl.step = io.d_step; sl.t_all = io.d_t_all; sl.num_steps = io.num_steps;
    sl.pos_traj = io.d_pos_traj; sl.v_traj = io.d_v_traj; sl.v0_traj = io.d_v0_traj; sl.vt_traj = io.d_vt_traj;
    sl.pos_only = io.pos_only; sl.prog_table = S->prog_table;
    return sl;
}
}  // namespace

namespace tdapi {
// the launches of one step, in order (eagerly or into a capturing stream)
int session_step_issue(td_session *S, const td_step_io &io, hipStream_t s) {
    const td_model *m = S->m;
    int rc = td_session_forward(S, io.d_ligand_pos, io.d_ligand_v, S->pred_pos, S->pred_v, nullptr, io.d_ligand_graph_bias, s);
    if (rc != TD_OK) return rc;
    ProfScope ps(PC_POST, s);
    if (S->guide) {
        // clash guidance: the shift of the predicted x0, one launch between the denoiser and the posterior update
        TdClashArgs a;
        a.prot4 = S->guide_prot4; a.pptr = S->pptr; a.lptr = S->lptr; a.B = (int)S->B; a.eval = S->pred_pos;
        a.w = S->guide_w; a.max_shift = S->guide_max;
        a.mean_type = m->cfg.model_mean_type; a.T = m->cfg.num_timesteps; a.num_steps = io.num_steps;
        a.xt = io.d_ligand_pos; a.rc = m->sched.rc; a.rm1 = m->sched.rm1; a.t_all = io.d_t_all; a.step = io.d_step;
        if ((rc = td_launch_clash_shift(a, S->guide_shift, s)) != TD_OK) return rc;
    }
    return td_launch_posterior_step(m->sched, step_args(S, io), step_slot(S, io), s);
}
}  // namespace tdapi

extern "C" int td_session_set_program(td_session *S, const float *d_prog_table, const int32_t *host_kinds, int32_t num_slots) {
    if (!S || (d_prog_table && (!host_kinds || num_slots < 1))) { td_set_error("td_session_set_program: bad argument"); return TD_EINVAL; }
    if (d_prog_table)
        for (int32_t k = 0; k < num_slots; ++k)
            if (host_kinds[k] != TD_PROG_DENOISE && host_kinds[k] != TD_PROG_RENOISE) {
                td_set_error("td_session_set_program: slot %d has kind %d", (int)k, (int)host_kinds[k]);
                return TD_EINVAL;
            }
    session_drop_graph(S);          // the captured step reads, or does not read, the table
    S->prog_table = d_prog_table;
    S->prog_kinds.clear();
    if (d_prog_table) S->prog_kinds.assign(host_kinds, host_kinds + num_slots);
    S->prog_next = 0;
    return TD_OK;
}

extern "C" int td_session_set_guidance(td_session *S, const float *d_sigma, float w, float max_shift) {
    if (!S) { td_set_error("td_session_set_guidance: bad argument"); return TD_EINVAL; }
    if (d_sigma && !(w >= 0.f)) { td_set_error("td_session_set_guidance: the weight must be >= 0 (got %g)", (double)w); return TD_EINVAL; }
    if (d_sigma && !(max_shift >= 0.f)) {
        td_set_error("td_session_set_guidance: max_shift must be >= 0 (0: no cap; got %g)", (double)max_shift);
        return TD_EINVAL;
    }
    session_drop_graph(S);          // the captured step holds, or does not hold, the shift kernel and the guided posterior
    S->guide = false;
    if (!d_sigma) return TD_OK;
    hipStream_t s = S->last_stream;
    if (!S->guide_block) {
        auto layout = [&](char *base) {
            Carver c{base};
            S->guide_prot4 = c.take<float4>((size_t)S->Np);
            S->guide_shift = c.take<float>((size_t)S->Nl * 3);
            return c.off;
        };
        const size_t bytes = layout(nullptr);
        hipError_t e = td_malloc_async(reinterpret_cast<void **>(&S->guide_block), bytes, s);
        if (e != hipSuccess) { S->guide_block = nullptr; td_set_error("td_session_set_guidance: hipMallocAsync(%zu) failed: %s", bytes, hipGetErrorString(e)); return TD_ENOMEM; }
        layout(S->guide_block);
    }
    // the centred protein the session holds (its rows of the packed coordinates: written at creation, never by a step) + the radii.
    // Cold path: wait, so that the caller may step on any stream and let go of nothing early.
    const int rc = td_launch_clash_pack(S->w.x4a, S->prot_node, d_sigma, S->Np, S->guide_prot4, s);
    if (rc != TD_OK) return rc;
    TD_CHECK_HIP(hipStreamSynchronize(s));
    S->guide = true;
    S->guide_w = w;
    S->guide_max = max_shift;
    return TD_OK;
}

extern "C" int td_session_step(td_session *S, const td_step_io *io, int32_t use_graph, void *stream) {
    if (!S || !io || !io->d_step || !io->d_t_all || io->num_steps < 1 || !io->d_ligand_pos || !io->d_ligand_v || !io->d_noise ||
        !io->d_uniform || !io->d_pos_traj || !io->d_v_traj) {
        td_set_error("td_session_step: bad argument");
        return TD_EINVAL;
    }
    if (const int rc = check_known_atoms("td_session_step", S->m, io->d_fixed_mask, io->d_fixed_pos, io->d_fixed_v)) return rc;
    if (S->guide && S->m->cfg.model_mean_type == 1 && (!S->m->sched.rc || !S->m->sched.rm1)) {
        td_set_error("td_session_step: guidance with model_mean_type 'noise' needs the 10 schedule arrays");
        return TD_EINVAL;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    S->last_step_graph = false;
    if (S->prog_table) {
        if ((size_t)io->num_steps != S->prog_kinds.size()) {
            td_set_error("td_session_step: num_steps = %d, the session's program has %zu slots", (int)io->num_steps, S->prog_kinds.size());
            return TD_EINVAL;
        }
        if (S->prog_next >= S->prog_kinds.size()) { td_set_error("td_session_step: the program has run to its end"); return TD_EINVAL; }
        if (S->prog_kinds[S->prog_next++] == TD_PROG_RENOISE) {
            // a forward-process step: one kernel, launched eagerly whatever use_graph says; no denoiser, no capture
            S->last_stream = s;
            ProfScope ps(PC_POST, s);
            return td_launch_renoise_step(step_args(S, *io), step_slot(S, *io), s);
        }
    }
    // measurement hooks put events / trace pointers into the launch sequence: those steps are issued launch by launch
    const bool graph_ok = use_graph && !S->graph_failed && g_prof.mask == 0 && !td_wg_trace_armed();
    if (graph_ok && S->graph_exec && (memcmp(&S->graph_io, io, sizeof(td_step_io)) != 0 || S->graph_epoch != S->m->option_epoch)) session_drop_graph(S);
    if (graph_ok && !S->graph_exec && S->eager_steps > 0) {
        // capture the launch sequence of a step (nothing executes while the stream captures), instantiate it once
        hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed);
        if (e == hipSuccess) {
            const int rc = session_step_issue(S, *io, s);
            hipGraph_t g = nullptr;
            e = hipStreamEndCapture(s, &g);
            if (rc == TD_OK && e == hipSuccess && g) {
                e = hipGraphInstantiate(&S->graph_exec, g, nullptr, nullptr, 0);
                if (e == hipSuccess) { S->graph = g; S->graph_io = *io; S->graph_epoch = S->m->option_epoch; }
                else { (void)hipGraphDestroy(g); S->graph_exec = nullptr; }
            } else if (g) {
                (void)hipGraphDestroy(g);
            }
        }
        if (!S->graph_exec) {       // not fatal: this session keeps issuing its steps launch by launch
            (void)hipGetLastError();
            S->graph_failed = true;
        }
    }
    if (graph_ok && S->graph_exec) {
        S->last_stream = s;
        TD_CHECK_HIP(hipGraphLaunch(S->graph_exec, s));
        S->last_step_graph = true;
        return TD_OK;
    }
    const int rc = session_step_issue(S, *io, s);
    if (rc == TD_OK) ++S->eager_steps;
    return rc;
}

extern "C" int td_session_step_graph(const td_session *S) { return S && S->last_step_graph ? 1 : 0; }

extern "C" int td_session_row_counts(td_session *S, int32_t *host_counts, int32_t n_counts, void *stream) {
    if (!S || !host_counts || n_counts < 2) { td_set_error("td_session_row_counts: bad argument"); return TD_EINVAL; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    host_counts[0] = (int32_t)S->N;
    if (!S->caching) {            // every layer runs on every row
        host_counts[1] = (int32_t)S->N;
        for (int k = 2; k < n_counts; ++k) host_counts[k] = -1;
        return TD_OK;
    }
    TD_CHECK_HIP(hipMemcpyAsync(host_counts + 1, S->dirty_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    for (int k = 2; k < n_counts; ++k) host_counts[k] = -1;
    const int room = n_counts - 2 < TD_HOP_LEVELS ? n_counts - 2 : TD_HOP_LEVELS;
    const int lv = S->hop_levels < room ? S->hop_levels : room;
    if (lv > 0) TD_CHECK_HIP(hipMemcpyAsync(host_counts + 2, S->hop_count, sizeof(int32_t) * (size_t)lv, hipMemcpyDeviceToHost, s));
    if (n_counts > 2 + TD_HOP_LEVELS && S->use_fwd)
        TD_CHECK_HIP(hipMemcpyAsync(host_counts + 2 + TD_HOP_LEVELS, S->fwd_counts, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    // rows of the static tables and distinct protein blocks of the batch (per-pocket sharing; -1: tables indexed by node)
    if (n_counts > 3 + TD_HOP_LEVELS) host_counts[3 + TD_HOP_LEVELS] = S->tabs.cgraph ? (int32_t)S->static_rows : -1;
    if (n_counts > 4 + TD_HOP_LEVELS) host_counts[4 + TD_HOP_LEVELS] = S->tabs.cgraph ? (int32_t)S->pocket_groups : -1;
    TD_CHECK_HIP(hipStreamSynchronize(s));
    return TD_OK;
}

