// Internal declarations shared by the five translation units of the C ABI (entry.cpp, pack.cpp, plan.cpp, forward.cpp, session.cpp).
// Not part of the interface: include/targetdiff_hip.h is.
#pragma once

#include <atomic>
#include <mutex>
#include <vector>

#include "td_internal.h"

void td_set_error(const char *fmt, ...);

namespace tdapi {

// ---- per-class kernel timers (entry.cpp): HIP events on the launch stream around the selected classes
enum { PC_KNN = 0, PC_GATE, PC_NODE, PC_X2H_K, PC_X2H_V, PC_H2X_K, PC_H2X_V, PC_COMPOSE, PC_HEAD, PC_POST, PC_COUNT };
struct Profiler {
    std::atomic<unsigned> mask{0};
    std::mutex mu;                            // the event lists: launches may come from several host threads (one stream each)
    std::vector<hipEvent_t> ev[PC_COUNT];     // start/stop pairs
    std::vector<hipEvent_t> pool;
    hipEvent_t get() {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
};
extern Profiler g_prof;
struct ProfScope {
    int cls; hipStream_t s; bool on; hipEvent_t e0 = nullptr;
    // wanted = false: a launch site that takes no scope (the set-up of a session's static tables)
    ProfScope(int c, hipStream_t st, bool wanted = true) : cls(c), s(st), on(wanted && ((g_prof.mask.load(std::memory_order_relaxed) >> c) & 1u)) {
        if (on) { e0 = g_prof.get(); (void)hipEventRecord(e0, s); }
    }
    ~ProfScope() {
        if (on) {
            hipEvent_t e1 = g_prof.get();
            (void)hipEventRecord(e1, s);
            std::lock_guard<std::mutex> lk(g_prof.mu);       // the pair enters the list together, whatever other threads record meanwhile
            g_prof.ev[cls].push_back(e0);
            g_prof.ev[cls].push_back(e1);
        }
    }
};

// ---- the weight blob (pack.cpp)
struct MlpSrc {          // one reference MLP (models/common.py:60-80) inside the flat blob
    const float *w0, *b0, *g, *b, *w3, *b3;
};

struct Cursor {
    const float *p;
    size_t left;
    bool ok = true;
    const float *take(size_t n) {
        if (n > left) { ok = false; return p; }
        const float *r = p;
        p += n; left -= n;
        return r;
    }
    MlpSrc mlp(int in, int hid, int out) {
        MlpSrc m;
        m.w0 = take((size_t)hid * in); m.b0 = take(hid); m.g = take(hid); m.b = take(hid);
        m.w3 = take((size_t)out * hid); m.b3 = take(out);
        return m;
    }
};

inline size_t mlp_floats(int in, int hid, int out) { return (size_t)hid * in + 3 * (size_t)hid + (size_t)out * hid + out; }

// stages per layer (0 in the config = 1): m->layers has stage_rows(c) rows per reference layer
inline int num_x2h(const td_config &c) { return c.num_x2h > 0 ? c.num_x2h : 1; }
inline int num_h2x(const td_config &c) { return c.num_h2x > 0 ? c.num_h2x : 1; }
inline int stage_rows(const td_config &c) { return num_x2h(c) > num_h2x(c) ? num_x2h(c) : num_h2x(c); }

inline int kv_in(const td_config &c) { return 2 * c.hidden_dim + c.edge_feat_dim + 4 * c.num_r_gaussian; }

inline bool config_supported(const td_config &c) {
    const bool graph_ok = (c.cutoff_mode == TD_CUTOFF_KNN && c.knn >= 1 && c.knn <= TD_MAX_FANIN) ||
                          (c.cutoff_mode == TD_CUTOFF_HYBRID && c.knn >= 1 && c.knn <= TD_MAX_FANIN) ||
                          (c.cutoff_mode == TD_CUTOFF_RADIUS && c.radius > 0.f && c.max_num_neighbors >= 1 &&
                           c.max_num_neighbors <= TD_MAX_FANIN);
    return c.hidden_dim == TD_H && c.n_heads == TD_HEADS && graph_ok && c.num_r_gaussian == TD_NG &&
           c.edge_feat_dim == 4 && c.num_layers >= 1 && c.protein_feat_dim >= 1 && c.protein_feat_dim <= 32 &&
           c.ligand_num_classes >= 1 && c.ligand_num_classes <= TD_MAXC && c.num_timesteps >= 1;
}

// the graph every kernel's fast path is specialised for: exactly 32 in-edges per node, one MFMA tile per dst row
// (a k-NN graph with k < 32 is the 32-NN graph with the slots >= k masked, so it shares that path; so does a radius graph
// whose fan-out cap is <= 32).  The caching session additionally needs the k-NN structure (sorted lists to merge into).
inline bool caching_graph(const td_config &c) { return c.cutoff_mode == TD_CUTOFF_KNN && c.knn <= TD_K; }
inline bool default_graph(const td_config &c) {
    return caching_graph(c) || (c.cutoff_mode == TD_CUTOFF_RADIUS && c.max_num_neighbors <= TD_K);
}


// Packed-buffer builder: collects tensors into one host vector; pointers are fixed up after the upload.
struct Packer {
    std::vector<float> data;
    size_t alloc(size_t n) {
        size_t off = (data.size() + 63) & ~size_t(63);          // 256-byte alignment
        data.resize(off + n, 0.f);
        return off;
    }
};

size_t pack_B128(Packer &pk, const float *W, int ld, int col0);
size_t pack_B128_split(Packer &pk, const float *W, int ld, int col0);
size_t pack_vec(Packer &pk, const float *v, size_t n, size_t padded = 0);
float gaussian_coeff(const float *off);
inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// One device block cut into 256-byte-aligned buffers, each named once: on the line that sizes it and binds it.  A layout function
// runs twice over the same lines -- with base == nullptr for the size (`off`; every pointer comes back null), then bound to the block.
// empty_bytes: what a buffer of no elements still takes (the layout's zero-size rule).
struct Carver {
    char *base;
    size_t empty_bytes = 0, off = 0;
    template <class T>
    T *take(size_t count) {
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += align_up(count ? count * sizeof(T) : empty_bytes);
        return p;
    }
};

// ---- workspace, graph tables, the layer sequence (plan.cpp)
struct Workspace {
    float4 *x4a, *x4b;
    int32_t *gid, *nbr, *lig_node, *node_ptr;
    float *ew, *P, *q, *h, *alpha;
    float *Px, *qx;          // h2x-stage projections / queries (separate from P / q: both stages project in one launch)
    size_t bytes;
};

// Sampling session, layer 1: rows outside the ligand's one-hop forward reach keep the protein-only graph's layer-1
// output (`hs`), so the attention passes run on `rows` only and `rest` is restored from the cache afterwards.
struct FwdReach {
    TdRows rows, rest;                       // device lists with device counts
    const float *hs;
    TdNodes nodes;                           // the batch, and the session's static tables: hs is indexed like them (compact per pocket, or by node)
    TdStaticTabs tabs;
};

// What only a caching session's step sets on the layer sequence; default-constructed: the stateless call.
struct CachedStep {
    bool init_xn = true;                     // x4b is not yet a copy of x4a
    bool layer0_x2h_done = false;            // the session ran layer 0's x2h stage itself (dirty rows only)
    // hop_rows: hop_levels lists of N entries each, level k = the ligand atoms and their neighbours up to k hops -- the only rows whose
    // h2x-stage projections (level 1) and last layers' features are ever read when just the ligand outputs are consumed
    const int32_t *hop_rows = nullptr, *hop_count = nullptr;
    int hop_levels = 0;
    const FwdReach *fwd = nullptr;
};

// One x2h stage (x2h_stage, plan.cpp): where its projections live and which rows it works on.
struct X2hStage {
    float *P, *q;                            // the projection buffer pair
    TdRows rows;                             // rows of the attention passes
    bool project = true;                     // false: the projections are in place (a pair launch took them, or the session's cache)
    TdRows proj;                             // rows to project
    const float *h_in = nullptr;             // features the projections are taken from when they are not h itself: h then starts as a
                                             // copy of them, made between the two passes (a session's static tables keep every layer's h)
    TdRows lig;                              // the ligand rows of the batch, all of them among `rows` (empty: a protein-only graph)
    bool scoped = true;                      // take the profile scopes
};

// ------------------------------------------------------------------------------------------ general graphs
// Layout of the chunked neighbour table of one batch (graph.hip "general graphs") plus the chunk-indexed buffers.  The
// layout depends only on the per-graph atom counts, so a sampling session builds it once; a stateless call builds and
// frees one per call (one host round trip for the counts -- these are the non-default graph modes).
struct GraphPlan {
    int mode = 0, k = 0, cpn_p = 1;
    float radius = 0.f;
    int64_t N = 0, Np = 0, Nl = 0, B = 0, NC = 0, NCl = 0;
    char *block = nullptr;
    int32_t *cptr = nullptr, *chunk_node = nullptr, *lig_chunks = nullptr, *cnbr = nullptr, *prot_node = nullptr, *pptr = nullptr, *meta = nullptr;
    float *ew = nullptr, *alpha = nullptr;
};

Workspace carve(char *base, int64_t N, int64_t B, int64_t Nl);
inline TdGraphTab default_tab(Workspace &w) { return TdGraphTab{nullptr, w.nbr, w.ew, w.alpha, 1, 0, nullptr, nullptr, 0}; }
inline TdGraphTab plan_tab(const GraphPlan &p) { return TdGraphTab{p.cptr, p.cnbr, p.ew, p.alpha, p.cpn_p, p.NCl, nullptr, p.chunk_node, p.NC}; }
// every row of the table gt, for a launch over slots (the edge gates): its chunks on a general graph, the N nodes on the default graph
inline TdRows table_rows(const TdGraphTab &gt, int64_t N) { return TdRows{nullptr, nullptr, gt.cptr ? gt.NC : N}; }
inline int num_blocks(const td_config &c) { return c.num_blocks > 1 ? c.num_blocks : 1; }
int x2h_stage(const TdLayer &L, const TdGraphTab &gt, const float4 *xc, float *h, int64_t N, const X2hStage &a, hipStream_t s);
int h2x_project(const TdLayer &L, Workspace &w, float *h, int64_t Nl, float *P, float *q, const TdRows &hop, hipStream_t s);
int h2x_attend(const td_model *m, const TdLayer &L, Workspace &w, const TdGraphTab &gt, int64_t Nl, float4 *xc, float4 *xn, float *P,
               float *q, hipStream_t s);
// num_layers x (x2h stages, h2x stages) on a composed batch whose graph (gt.nbr) and edge gate (gt.ew) are in place.  h is updated in
// place; returns the buffer holding the final coordinates through *x_final.
int run_backbone(const td_model *m, Workspace &w, const TdGraphTab &gt, float *h, int64_t N, int64_t Nl, int fix_x, float4 **x_final,
                 hipStream_t s, const CachedStep &cs = CachedStep());
// num_blocks x (graph + gate from w.x4a, run_backbone, buffer swap); plan == nullptr: the default graph
int run_blocks(const td_model *m, Workspace &w, GraphPlan *plan, float *h, int64_t N, int64_t Nl, int fix_x, int max_graph_nodes,
               float4 **x_final, hipStream_t s);
// known atoms of a posterior step (scaffold-constrained sampling): a mask needs both arrays and a model with alphas_cumprod; `who`
// prefixes the error (forward.cpp)
int check_known_atoms(const char *who, const td_model *m, const uint8_t *d_fixed_mask, const float *d_fixed_pos, const int64_t *d_fixed_v);
// stream-ordered memory: td_debug_fail_alloc makes the n-th allocation from now fail (fault injection for the error paths)
extern std::atomic<int> g_fail_alloc;
hipError_t td_malloc_async(void **p, size_t bytes, hipStream_t s);
void free_async_or_sync(void *p, hipStream_t s);          // (session.cpp)
void plan_destroy(GraphPlan &p, hipStream_t s);
int plan_create(const td_config &c, const int32_t *host_pptr, const int32_t *host_lptr, int64_t B, hipStream_t s, GraphPlan *out);
int plan_layout(GraphPlan &p, const int32_t *node_ptr, const int32_t *gid, hipStream_t s);
int plan_from_mask(const td_config &c, const uint8_t *d_mask, const int32_t *d_node_ptr, int64_t N, int64_t B, hipStream_t s,
                   GraphPlan *out, int64_t *nl_out);
// the GraphPlan of a stateless call: freed in stream order on every way out
struct PlanGuard {
    GraphPlan p;
    hipStream_t s;
    ~PlanGuard() { plan_destroy(p, s); }
};
int fetch_ptrs(const int32_t *d_a, const int32_t *d_b, int64_t B, std::vector<int32_t> &a, std::vector<int32_t> &b, hipStream_t s);
// stream-ordered scratch of one call: every block taken so far is given back on every exit path (a failing second or third
// allocation used to leak the earlier ones)
struct AsyncScratch {
    hipStream_t s;
    std::vector<void *> blocks;
    explicit AsyncScratch(hipStream_t st) : s(st) {}
    AsyncScratch(const AsyncScratch &) = delete;
    AsyncScratch &operator=(const AsyncScratch &) = delete;
    ~AsyncScratch() { for (void *b : blocks) free_async_or_sync(b, s); }
    template <class T>
    int take(T **out, size_t bytes, const char *who) {
        void *p = nullptr;
        hipError_t e = td_malloc_async(&p, bytes ? bytes : 4, s);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            td_set_error("%s: hipMallocAsync(%zu) failed: %s", who, bytes, hipGetErrorString(e));
            return TD_ENOMEM;
        }
        blocks.push_back(p);
        *out = static_cast<T *>(p);
        return TD_OK;
    }
};

}  // namespace tdapi
