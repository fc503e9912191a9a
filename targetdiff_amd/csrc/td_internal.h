// Internal declarations shared by the translation units of libtargetdiff_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "../../include/targetdiff_hip.h"

// ---- compile-time shape of the live configuration (configs/training.yml:9-42) ----------------------
constexpr int TD_H = 128;        // hidden_dim
constexpr int TD_HEADS = 16;     // n_heads
constexpr int TD_DH = 8;         // head dim
constexpr int TD_K = 32;         // knn fan-in: one node's in-edges = one 32-row MFMA tile
constexpr int TD_NG = 20;        // num_r_gaussian
constexpr int TD_SLOTK = 24;     // K columns per source-class slot of the first-layer edge GEMM: 20 g + 1 + 3 pad
constexpr int TD_SLOT_STEPS = TD_SLOTK / 2;   // 12 MFMA k-steps per slot
constexpr int TD_KSTEPS = TD_H / 2;           // 64 k-steps (32x32x2) for a 128-deep contraction
constexpr int TD_MAXC = 16;      // ligand classes padded
constexpr int TD_SMALL_BATCH_ROWS = 16384;   // below this many rows a launch is shaped for latency (more, smaller workgroups)

void td_set_error(const char *fmt, ...);
#define TD_CHECK_HIP(expr)                                                                       \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            td_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return TD_EHIP;                                                                      \
        }                                                                                        \
    } while (0)

// Dynamic-LDS opt-in of a kernel, once per device (not per process: a second GPU used from the same process needs its
// own hipFuncSetAttribute) and safe against concurrent first launches.
struct TdLdsOnce {
    std::atomic<unsigned long long> mask{0};
};
inline int td_set_lds(TdLdsOnce &once, const void *fn, size_t bytes) {
    int dev = 0;
    TD_CHECK_HIP(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (once.mask.load(std::memory_order_acquire) & bit) return TD_OK;
    TD_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    once.mask.fetch_or(bit, std::memory_order_release);
    return TD_OK;
}
// Launch of a kernel that takes dynamic LDS beyond the default limit: the kernel is the template argument, so every kernel has its
// own TdLdsOnce here and a launch site names it once.
template <auto Kernel, class... Args>
int td_launch(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, const Args &...args) {
    static TdLdsOnce once;
    const int rc = td_set_lds(once, reinterpret_cast<const void *>(Kernel), lds_bytes);
    if (rc != TD_OK) return rc;
    Kernel<<<grid, block, lds_bytes, s>>>(args...);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

// ---- packed weights (device pointers) ---------------------------------------------------------------
// One edge MLP (hk/hv/xk/xv: Linear(340,128) -> LN -> ReLU -> Linear(128,out)), re-packed:
//  * the 340-wide first Linear is split into node-side projections (proj_*), a per-(dst class, src class)
//    radial/type table R and a bias;  * the second Linear is stored as per-wave MFMA B fragments.
struct TdEdgeMlp {
    const float *R;        // [2 dst class][2 slot][12 kstep][64 lane][4 ntile]  first-layer radial+type B fragments
    // (every table below comes from the MLP with its LayerNorm folded into the two Linears: FoldedMlp, pack.cpp)
    const float *gamma;    // [128] |LayerNorm weight| x the folded scale M (0 for a dead unit): already inside the second Linear's columns; not read by the kernels
    const float *beta;     // [128] LayerNorm bias / (|LayerNorm weight| M): z'' = clamp_[0,1](centred pre-activation / (sigma M) + beta)
    const float *W2;       // out=128: [64 kstep][64 lane][4 ntile];  out=16 (xv): [64 kstep][64 lane] (cols >= 16 zero)
    const float *b2;       // [128] or [16]
    const float *R16;      // [2 dst class][2 slot][6 kstep][64 lane][8 hidden block]  radial/type table for 16x16x4 tiles
    const float *Walt16;   // key MLPs: Wq16[hb][r][jq][lane][4] = W2[8 lo + 4jq + jj][16hb + 4g + r]
    const float *Walt;     // key MLPs: Wq[t][r][jq][hi][c<16][4] = W2[8c+4jq+jj][32t+erow(r,hi)];  hv: Wt[d][k/4][head][4] = W2v[8 head + d][k]
    const float *R16q;     // the radial/type table as exact bf16 piece triples, K-packed for four v_mfma_f32_16x16x32_bf16 per tile
                           // (pack_pk4_table, pack.cpp): [2 dst class][2 slot] x {QA, QB, H7, QC}[8 hidden block][64 lanes]
    const float *R16h;     // attention MLPs (hk, hv, xk, xv): the same table as f16 piece pairs for two v_mfma_f32_16x16x32_f16 per tile (pack_h2_table); the MLP's whole
                           // first layer, node projections included, is in units of 2^FoldedMlp::first_scale_exp
    float ln_c1, ln_c2;    // folded LayerNorm (FoldedMlp, pack.cpp): 1 / (sigma M) = rsqrt(sum_n c_n^2 * ln_c1 + ln_c2); z'' = clamp_[0,1](c_n / (sigma M) + beta_n)
    float w2_bound;        // key MLPs: 8 max |W2'| (folded second Linear): |U_i[n][head]| = |sum_d W2'[8 head + d][n] q_i[8 head + d]| <= w2_bound max |q_i|
                           // (the f16 logits product scales the query by a power of two from this bound, edge16.hip)
    bool l2_f16;           // x2h passes: logits (rows of one chunk) / alpha^T z (every graph) on v_mfma_f32_16x16x32_f16 with f16 piece pairs (model option "edge_second_layer_f16")
    bool l1_f16;           // attention kernels (x2h passes, h2x stage): the radial / type first layer on f16 piece pairs (R16h; model option "edge_first_layer_f16"); false: exact bf16 piece triples
    bool z_plain;          // f16 second layer: the folded scale M is at most TD_Z_PLAIN_MAX_M, take the f16 pieces of z'' itself (edge16.hip, td_ln_relu16_pairs_*)
    bool use_split;        // run the first layer on the piece triples where a kernel has that variant (model option "edge_key_split")
    int deal_rows;         // x2h passes: rows dealt round-robin inside an XCD's range (model option "edge_row_dealing": 0 contiguous
                           // shares, 1 dealt, 2 dealt + the workgroup's rows handed to its waves through an LDS counter)
    bool f16_safe;         // pack time: the f16 piece pairs keep this MLP's precision (folded scale M <= TD_F16_MAX_M, first_scale_exp
                           // not clipped; pack.cpp); false: l1_f16 and l2_f16 stay off whatever the model options say
};

// Node-side weights of one stage (x2h or h2x): 4 projections (k_i,k_j,v_i,v_j) + the query MLP.
struct TdNodeStage {
    const float *projB;    // [5 mat][64 kstep][64 lane][4 ntile]   mats: k_i, k_j, v_i, v_j, q.net.0
    const float *projBias; // [5][128]  (k_i: b0 of k MLP, k_j: 0, v_i: b0 of v MLP, v_j: 0, q: b0)
    const float *qGamma, *qBeta;   // [128]
    const float *q3B;      // [64 kstep][64 lane][4 ntile]  q.net.3
    const float *q3Bias;   // [128]
    const float *projB3;   // optional: the same 5 matrices as bf16 piece triples [mat][8 kstep][3 piece][64 lane][4 ntile] x 8 bf16
    const float *q3B3;     // optional: q.net.3 likewise (nullptr: the fp32 path is the only one)
    bool use_split;        // run the GEMMs on the exact 3-way bf16 operand split (model option "node_proj_split")
    bool bpipe;            // split kernel: B fragments of the next k-step read ahead of the current k-step's MFMAs ("node_proj_bpipe")
    bool async_copy;         // split kernel: B chunks by inline-asm global_load_lds + explicit wait (model option "node_proj_async", default)
};

// node_output MLP of an x2h stage with out_fc (models/uni_transformer.py:39-40): Linear(256, 128) -> LayerNorm -> ReLU -> Linear(128, 128)
struct TdNodeOut {
    const float *B;        // 3 x B fragments (pack_B128): net.0[:, 0:128] (attention output), net.0[:, 128:256] (h), net.3
    const float *b1, *gamma, *beta, *b2;
};

struct TdLayer {
    TdNodeStage nodeX2h, nodeH2x;
    TdEdgeMlp hk, hv, xk, xv;
    const float *ew_x2h, *ew_h2x;   // ew_net_type 'r' / 'm' / none: [4 types][20] + bias of the stage's gate (nullptr: the global gate; 'm' and none:
                                    // zero weights and a bias of 40, i.e. e_w = 1 -- 'm' gates in the value pass instead)
    const float *gate_m;            // ew_net_type 'm': [128] folded W2v^T w_m, then w_m . b2v + b_m (nullptr: off)
    TdNodeOut nodeOut;              // x2h_out_fc (B == nullptr: off)
    const float *offsets;  // [20] Gaussian centres of this layer (models/common.py:15)
    float coeff;           // -0.5 / (offset[1]-offset[0])^2
};

struct TdGate {            // edge_pred_layer MLP(20 -> 128 -> 1) (models/uni_transformer.py:236-237,312-316)
    const float *R;        // [12 kstep][64 lane][4 ntile]
    const float *b0, *gamma, *beta, *w3;   // [128] each, LayerNorm folded like the edge MLPs' (FoldedMlp): beta = bias / (|weight| M), w3 carries |weight| M
    float b3;
    const float *offsets;  // [20]
    float coeff;
    const float *R16q;     // the 20 x 128 first layer as exact bf16 piece triples, K-packed (pack_pk4_table, pack.cpp)
    float ln_c1, ln_c2;    // as in TdEdgeMlp
    bool use_split;        // model option "edge_key_split"
};

struct TdEmbed {
    const float *WpT;      // [protein_feat_dim][128]  (column 127 zero)
    const float *bp;       // [128] (entry 127 = 0: node indicator of protein atoms)
    const float *WlT;      // [classes][128]
    const float *bl;       // [128] (entry 127 = 1: node indicator of ligand atoms)
};

struct TdHead {            // v_inference (models/molopt_score_model.py:307-311)
    const float *W0T;      // [128 in][128 out]
    const float *b0;       // [128]
    const float *W2T;      // [128 in][16 out] (classes padded)
    const float *b2;       // [16]
};

// One EnBaseLayer of the standalone EGNN refine net (models/egnn.py:10-35), packed by td_egnn_create
struct TdEgnnLayer {
    TdNodeStage proj;      // node_proj_kernel, mask 0x03: mat 0 = edge_mlp.net.0[:, 0:128] (+ bias), mat 1 = [:, 128:256]
    const float *W2f;      // edge_mlp.net.2 as 16x16x4 A fragments [ot][hb][lane] x 4 r
    const float *Wxf;      // x_mlp.0, same layout
    const float *vec;      // [w_d 128 | W_t 4 x 128 | b2 128 | w_inf 128, b_inf, pad 3 | b_x 128 | w_x2 128]
    const float *nodeB;    // 3 x B fragments (pack_B128): node_mlp.net.0[:, 0:128] (mi), [:, 128:256] (h), node_mlp.net.2
    const float *nb1, *nb2;
};

// One EnBaseLayer of the binding-affinity encoder (models/property_pred/prop_egnn.py:8-45), packed by td_prop_create
constexpr int TD_PROP_H = 256;         // hidden width the prop kernels are built for
constexpr int TD_PROP_G = 64;          // Gaussians of the edge feature
constexpr int TD_PROP_ACT_NONE = 0, TD_PROP_ACT_RELU = 1, TD_PROP_ACT_SSP = 2;   // prop_linear_kernel epilogues
constexpr int TD_PROP_EPI_NONE = 0, TD_PROP_EPI_RELU_MASK = 1, TD_PROP_EPI_SSP_DERIV = 2;   // prop_bgemm_kernel epilogues
constexpr int TD_PROP_XTY_CHUNKS = 64; // most split-K chunks of a weight-gradient reduction (prop_bwd.hip)
struct TdPropLayer {
    const float *projW, *projB;   // [512][256] = [edge_mlp.net.0[:, 64:320]; [:, 320:576]], bias [b1 | 0]
    const float *W1f;             // edge_mlp.net.0[:, 0:64] as 16x16x4 A fragments [ot 16][kb 4][lane] x 4 r
    const float *W2f;             // edge_mlp.net.2 as A fragments [ot 16][hb 16][lane] x 4 r
    const float *b2, *winf, *binf;
    const float *offset;          // GaussianSmearing offsets [64]
    const float *n1W, *n1b, *n2W, *n2b;   // node_mlp.net.0 [256][512], node_mlp.net.2 [256][256] (row-major, as PyTorch stores them)
};

struct TdSchedules {       // [T] each
    const float *c0, *ct, *logvar, *log_a, *log_1ma, *log_ca, *log_1mca;
    const float *abar;     // alphas_cumprod of the position schedule; nullptr when the model was created without it
    const float *rc, *rm1; // sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod (model_mean_type 'noise'); nullptr without them
};

// Per-model switches (td_model_set_option; defaults = the shipped configuration).  They live in the model, i.e. per device
// and per handle -- nothing is read from the environment.
struct TdOptions {
    int h2x_fused = 1;             // one launch for the h2x stage's key + value halves (0: two launches, alpha through memory)
    int node_proj_split = 1;       // node-side GEMMs on exact bf16 x 3 operand pieces with fp32 accumulation (0: fp32 MFMA)
    int edge_key_split = 1;        // attention passes: radial/type first layer on exact bf16 x 3 pieces (0: fp32 MFMA)
    int edge_first_layer_f16 = 1;  // x2h passes and h2x stage: the 21-wide radial / type first layer on f16 piece pairs (two products per tile; 0: the exact bf16 piece triples, four)
    int edge_second_layer_f16 = 1; // x2h passes: logits / alpha^T z on f16 piece pairs (0: fp32 MFMA products; the chunk-walking key pass takes the f16 logits only beside the f16 first layer)
    int session_hop_levels = 4;    // receptive-field levels a sampling session tracks (1 .. 4)
    int session_forward_reach = 1; // layer 1 of a session runs on the ligand's one-hop forward reach only
    int edge_row_dealing = 2;      // x2h key / value passes: units of rows dealt round-robin to an XCD's workgroups (0: one
                                   // contiguous share per workgroup; 1: a fixed row sequence per wave; 2: the workgroup's rows
                                   // handed to its waves one at a time through an LDS counter; the value pass's protein rows on a
                                   // general graph with one chunk per protein row always take 2: the 12-wave kernel has no other form)
    int node_proj_bpipe = 0;       // split node GEMMs: register double-buffering of the B fragments (LDS reads ahead of the MFMAs; measured
                                   // slower at C2: 0.848 vs 0.817 ms per step, profiles/r03b_*; kept as a switch)
    int node_proj_async = 1;    // split node GEMMs: B chunks by inline-asm global_load_lds + an explicit wait per round (0: the builtin, which the compiler serialises)
    int session_share_pockets = 1; // a session's static tables (protein-only k-NN keys / lists, cached gate rows, embeddings, layer-0 / layer-1 outputs of the
                                   // protein-only graph) once per distinct pocket of the batch instead of once per graph (default graph; 0: per graph)
    int session_step_lists = 1;    // a step's row lists from one launch (a workgroup per graph; 0: the separate kernels, which
                                   // graphs too large for its LDS flags use anyway)
};

struct td_model {
    td_config cfg;
    TdOptions opt;
    float *blob;           // one device allocation holding every packed tensor
    size_t blob_floats;
    TdEmbed emb;
    TdGate gate;
    TdLayer *layers;       // host array [num_layers]
    TdHead head;
    TdSchedules sched;
    unsigned option_epoch = 0;   // bumped by td_model_set_option: sessions drop a step graph captured under older options
    int fold_dead_units = 0;     // LayerNorm units the fold replaced by their constant, over every folded MLP (read-only option "fold_dead_units")
    int fold_fp32_mlps = 0;      // attention MLPs kept off the f16 piece pairs by TdEdgeMlp::f16_safe (read-only option "fold_fp32_mlps")
};

// ---- argument blocks of the graph, gate, projection and attention launchers ---------------------------
// Read on the host only: a launcher fills its kernel's own argument list from them.  Every member is value-initialised ({}: null, 0).
// The rows a launch works on.
struct TdRows {
    const int32_t *rows{};              // row ids; null: every row 0 .. count - 1
    const int32_t *count_ptr{};         // device-side length of `rows` (at most `count`); null: exactly `count` rows
    int64_t count{};                    // 0: an empty selection, nothing is launched for it
};
// Neighbour table and per-slot buffers of one batch, 32 slots per row (-1 padded).  Default graph: one row per node.  General graphs: the
// chunk-indexed buffers of a GraphPlan.
struct TdGraphTab {
    const int32_t *cptr{};              // general graphs: the in-edges of dst node i are the chunks cptr[i] .. cptr[i+1]-1 of nbr / ew / alpha;
                                        // null: the default graph (chunk == node)
    int32_t *nbr{};                     // [rows,32] src node of every slot
    float *ew{}, *alpha{};              // [rows,32] edge gate, [rows,16 heads,32] attention weights
    int cpn_p{};                        // chunks per protein row (default graph: 1).  A general graph with 1 (`hybrid`) runs the x2h passes of its
                                        // protein rows as on the default graph and those of its ligand rows in a second, chunk-walking launch
    int64_t NCl{};                      // chunks of all ligand rows together (default graph: 0)
    const int32_t *mixed{};             // device count of the rows that see both source classes (a session's dirty rows); null: none known
    const int32_t *chunk_node{};        // general graphs: dst node of every chunk; null: row == node
    int64_t NC{};                       // general graphs: chunks of the table (default graph: 0, the table has one row per node)
};
// The composed batch every graph builder reads.
struct TdNodes {
    const float4 *x4{};                 // [N] (x, y, z, ligand flag)
    const int32_t *node_ptr{};          // [B + 1] nodes of every graph, protein rows first
    const int32_t *pptr{};              // [B + 1] protein atoms of every graph; null where the launch makes no protein / ligand difference
    const int32_t *gid{};               // [N] graph of every node
    int64_t N{};
    int64_t B{};                        // graphs (read by the row-list launch of a session step; a stateless call on the default graph leaves 0)
    int max_graph_nodes{};              // upper bound on the nodes of one graph (selects the candidates-per-lane kernel form); 0: unknown
};
// Static protein tables of a caching session (session.cpp), read by the step's merge and restore launches.
struct TdStaticTabs {
    unsigned long long *skeys{};        // sorted keys of the protein-only k-NN rows: [rows,32], general graphs [N,64]
    int32_t *snbr{};                    // the protein-only neighbour rows
    float *h0{}, *h1s{}, *ews{};        // embeddings, layer-0 x2h outputs and gate rows of the protein-only graph
    // A session that shares its tables between the replicas of a pocket: graph g's protein block is a bitwise copy of graph cgraph[g]'s (the first
    // such graph of the batch: cgraph[g] <= g), whose rows sit at cbase[g] .. in the COMPACT tables above; row i of graph g reads compact row
    // cbase[g] + (i - node_ptr[g]) and shifts the node indices it finds there (they are the canonical graph's) by node_ptr[g] - node_ptr[cgraph[g]].
    int32_t *cgraph{}, *cbase{};        // null: the tables are indexed by node
};

// ---- kernel launchers (each defined next to its kernels) --------------------------------------------
// graph.hip
int td_launch_graph_ptr(const int64_t *batch, int64_t N, int64_t B, int32_t *ptr, hipStream_t s);
int td_launch_node_gid(const int32_t *node_ptr, int64_t N, int64_t B, int32_t *gid, hipStream_t s);
int td_launch_pack_x(const float *x3, const uint8_t *mask, int64_t N, float4 *x4, hipStream_t s);
int td_launch_unpack_x(const float4 *x4, int64_t N, float *x3, hipStream_t s);
// k <= TD_K neighbours per 32-slot row (slots >= k are -1): every fan-in up to 32 runs on the 32-slot fast path.  _rows: the listed query
// rows only; _static: protein-only lists of the listed (protein) rows and their sorted keys
int td_launch_knn(const TdNodes &nd, int32_t *nbr, int k, hipStream_t s);
int td_launch_knn_rows(const TdNodes &nd, const TdRows &rows, int32_t *nbr, int k, hipStream_t s);
int td_launch_knn_static(const TdNodes &nd, const TdRows &rows, int32_t *nbr, unsigned long long *skeys, int k, hipStream_t s);
// gbias: optional [B,128] per-graph bias of the ligand embeddings (null: none)
int td_launch_compose(const td_model *m, const float *ppos, const float *pv, const int32_t *pptr, int64_t Np,
                      const float *lpos, const int64_t *lv, const int32_t *lptr, int64_t Nl, int64_t B,
                      float *h, float4 *x4, int32_t *node_ptr, int32_t *gid, int32_t *lig_node, int32_t *prot_node,
                      const float *gbias, hipStream_t s);
// a session step's neighbour search: the protein rows `prot` merge the graph's ligand atoms into their static lists and take h / gt.ew from
// the tables where the row stays clean; `lig` (default graph; empty: none) are searched in full by the same launch.  flags2 null: not cleared
int td_launch_knn_merge(const TdNodes &nd, const TdRows &prot, const TdRows &lig, const TdStaticTabs &tabs, const TdGraphTab &gt, float *h,
                        uint8_t *clean, uint8_t *flags2, int k, hipStream_t s);
// per-pocket sharing of a session's static tables (graph.hip, session.cpp)
int td_launch_pocket_hash(const float *ppos, const float *pv, const int32_t *pptr, int64_t B, int F, unsigned long long *out, hipStream_t s);
int td_launch_pocket_verify(const float *ppos, const float *pv, const int32_t *pptr, int64_t B, int F, const int32_t *cand, int32_t *flags,
                            hipStream_t s);
int td_launch_compact_rows(const void *src, const int32_t *rows, int64_t n_rows, int row_bytes, void *dst, hipStream_t s);
int td_launch_compact_dirty(const uint8_t *clean, const float4 *x4, int64_t N, int32_t *rows, int32_t *count,
                            hipStream_t s);
int td_launch_forward_reach(const uint8_t *clean, const float4 *x4, const int32_t *nbr, int64_t N, uint8_t *flags2,
                            int32_t *rows_on, int32_t *rows_off, int32_t *counts2, uint8_t *clean_to_zero, hipStream_t s);
// h[i] = hs[i] for the listed rows (a device-side count), hs indexed like the tables of `tabs`
int td_launch_restore_rows(const TdRows &rows, const float *hs, float *h, const TdNodes &nd, const TdStaticTabs &tabs, hipStream_t s);
constexpr int TD_HOP_LEVELS = 4;
// rows: [levels][N] row lists, counts: [levels] device-side lengths; zeroed: flags and counts were cleared earlier in the step
int td_launch_hop_levels(const TdRows &lig, const TdGraphTab &gt, int64_t N, uint8_t *flags, int32_t *rows, int32_t *counts, int levels,
                         bool zeroed, hipStream_t s);
// edge gate on 16 x 16 tiles with the bf16 first layer (edge16.hip); td_launch_gate (gate.hip) dispatches to it
int td_launch_gate16(const TdGate &g, const float4 *x4, const TdGraphTab &gt, const TdRows &rows, hipStream_t s);
// all row lists of a sampling step in one launch (graph.hip); TD_EINVAL when a graph does not fit the LDS flag arrays
struct TdStepLists {
    int32_t *dirty_rows, *dirty_count;
    int32_t *reach_rows, *rest_rows, *reach_counts;
    int32_t *level_rows, *level_counts;
    int levels;
    int32_t *dirty_chunks = nullptr, *dirty_chunk_count = nullptr;     // general graphs: the chunks of the dirty rows
};
// max_nodes: the exact size of the largest graph (it sizes the LDS flag arrays; nd.max_graph_nodes is not read)
int td_launch_step_lists(const uint8_t *clean, const TdNodes &nd, const TdGraphTab &gt, int max_nodes, const TdStepLists &out, hipStream_t s);
// bookkeeping a session step resets in its first kernel: up to three counter arrays and the ligand rows' forward-reach flags
struct TdStepReset {
    int32_t *c0 = nullptr, *c1 = nullptr, *c2 = nullptr;
    int n0 = 0, n1 = 0, n2 = 0;
    uint8_t *flags2 = nullptr;
};
// reset: null: nothing to reset; gbias / gid: as td_launch_compose, gid read only with gbias
int td_launch_ligand_update(const td_model *m, const float *lpos, const int64_t *lv, const TdRows &lig, float *h, float4 *x4,
                            const TdStepReset *reset, const float *gbias, const int32_t *gid, hipStream_t s);
int td_launch_ligand_list(const uint8_t *mask, int64_t N, int32_t *lig_node, int32_t *count, hipStream_t s);
// node.hip
// mat_mask bits 0..3 = [k_i, k_j, v_i, v_j] projections, bit 4 = query MLP, on `rows`; rows2 / mask2: a second segment of the same stage
// (empty: none)
int td_launch_node_proj(const TdNodeStage &st, const float *h, const TdRows &rows, unsigned mat_mask, const TdRows &rows2, unsigned mask2,
                        float *P, float *q, hipStream_t s);
// stage hx: src-side units on `hop`, dst-side units + queries on `lig`, into Px / qx; stage nx: all units on `rows`, into P / q
int td_launch_node_proj_pair(const TdNodeStage &hx, const TdRows &hop, const TdRows &lig, float *Px, float *qx, const TdNodeStage &nx,
                             const TdRows &rows, float *P, float *q, const float *h, hipStream_t s);
int td_launch_node_output(const TdNodeOut &no, const float *out, float *h, int64_t N, hipStream_t s);
// gate.hip -- rows: rows of gt.nbr / gt.ew (chunks on a general graph), all of them or a list
int td_launch_layer_gate(const float *w, const float *offsets, float coeff, const float4 *x4, const TdGraphTab &gt, const TdRows &rows,
                         hipStream_t s);
int td_launch_gate(const TdGate &g, const float4 *x4, const TdGraphTab &gt, const TdRows &rows, hipStream_t s);
// edge16.hip.  lig (x2h passes): the ligand rows of the batch, all of them among `rows` (every row list of a forward pass or sampling step
// holds the ligand atoms); empty: a list without ligand rows.  h2x_stage: the unfused h2x key pass.  out: null: the value pass adds into h
int td_launch_edge_key16(const TdEdgeMlp &mlp, const TdLayer &L, const float4 *x4, const TdGraphTab &gt, const float *P, const float *q,
                         const TdRows &rows, const TdRows &lig, bool h2x_stage, hipStream_t s);
int td_launch_edge_value16(const TdEdgeMlp &mlp, const TdLayer &L, const float4 *x4, const TdGraphTab &gt, const float *P, const TdRows &rows,
                           const TdRows &lig, float *h, float *out, hipStream_t s);
int td_launch_edge_xv16(const TdEdgeMlp &mlp, const TdLayer &L, const float4 *x4_in, float4 *x4_out, const TdGraphTab &gt, const float *P,
                        const TdRows &rows, hipStream_t s);
int td_launch_edge_h2x16(const TdEdgeMlp &mlp_k, const TdEdgeMlp &mlp_v, const TdLayer &L, const float4 *x4_in, float4 *x4_out,
                         const TdGraphTab &gt, const float *P, const float *q, const TdRows &rows, hipStream_t s);
int td_set_wg_trace(unsigned long long *buf, int slots);
bool td_wg_trace_armed();
// graph.hip, general graphs
int td_launch_layout(const int32_t *node_ptr, const int32_t *pptr, const int32_t *gid, const int32_t *g_cbase,
                     const int32_t *g_cl, const int32_t *g_lbase, int cpn_p, int64_t N, int32_t *cptr, int32_t *chunk_node,
                     int32_t *lig_chunks, int32_t total_chunks, hipStream_t s);
// prot / lig: the protein / ligand rows of the batch (lists of exactly `count` rows); gt: the chunked table whose nbr is written (cptr, NC)
int td_launch_graph_general(int mode, const TdNodes &nd, const TdRows &prot, const TdRows &lig, int k, float radius, const TdGraphTab &gt,
                            hipStream_t s);
int td_launch_knn_general_static(const TdNodes &nd, const TdRows &prot, int k, const TdGraphTab &gt, unsigned long long *skeys, hipStream_t s);
int td_launch_ligand_rows_general(int mode, const TdNodes &nd, const TdRows &lig, int k, const TdGraphTab &gt, hipStream_t s);
int td_launch_hybrid_ligand_half(const TdNodes &nd, const TdRows &lig, const TdGraphTab &gt, hipStream_t s);
// the protein rows' merge of td_launch_knn_merge on the chunked table (the ligand rows: td_launch_ligand_rows_general)
int td_launch_knn_merge_general(const TdNodes &nd, const TdRows &prot, const TdStaticTabs &tabs, const TdGraphTab &gt, float *h,
                                uint8_t *clean, uint8_t *flags2, int k, hipStream_t s);
int td_launch_radius32(const TdNodes &nd, float radius, int cap, int32_t *nbr, hipStream_t s);
int td_launch_slots_to_dense(const int32_t *cptr, const int32_t *cnbr, int64_t N, int width, int32_t *out, hipStream_t s);
// misc.hip
int td_launch_head(const TdHead &hd, const float *h, const float4 *x4, const int32_t *lig_node, int64_t Nl,
                   int classes, float *pred_pos, float *pred_v, float *lig_h, hipStream_t s);
// The per-atom update that ends a sampling step -- the posterior draw or the renoise step of a time program (misc.hip; DESIGN.md
// section 3) -- reads and writes what this block names, over N_l ligand atoms.  pos / v may alias pos_next / v_next and pos_cur / v_cur
// (the in-place form of td_session_step): none of the pointers is __restrict__.  Every member is value-initialised ({}: null, 0, false).
struct TdStepArgs {
    const int32_t *lptr{};              // [B + 1] ligand atoms of every graph (the renoise step does not read it)
    int64_t Nl{};                       // ligand atoms: 0 launches nothing
    int B{}, C{}, T{};                  // graphs, ligand classes, diffusion levels
    int mean_type{};                    // 0: pred_pos is x0 (model_mean_type 'C0'); 1: it is x_t + eps ('noise')
    const int32_t *t{};                 // [B] time step of every graph; null only where a session slot fills it in
    const float *pos{};                 // [N_l,3] x_t, never null
    const int64_t *v{};                 // [N_l] v_t, never null
    const float *pred_pos{};            // [N_l,3] the network's output, never null for the posterior (renoise: not read)
    const float *pred_v{};              // [N_l,C] logits, likewise
    const float *noise{};               // [N_l,3] Gaussian draws, never null
    const float *uni{};                 // [N_l,C] uniform draws; null (renoise only): the types are not touched
    float *pos_next{};                  // [N_l,3] x_{t-1}; null only where a session slot fills it in
    int64_t *v_next{};                  // [N_l] v_{t-1}, likewise
    float *log_v0{};                    // [N_l,C] log-probabilities of the predicted v0; null: not written
    float *log_post{};                  // [N_l,C] log-probabilities the draw was taken from; null: not written
    float *pos_cur{};                   // second copy of x_{t-1} (a session's current state); null: none
    int64_t *v_cur{};                   // second copy of v_{t-1}; null: none
    bool v_frozen{};                    // pos_only: v_next = the input type
    const uint8_t *fixed_mask{};        // [N_l] known atoms (scaffold-constrained sampling); null: the kernels without the feature
    const float *fixed_pos{};           // [N_l,3] their centred positions; read only with fixed_mask
    const int64_t *fixed_v{};           // [N_l] their types; read only with fixed_mask
    const float *prow{};                // TD_PROG_ROW floats, a time program's slot; null: the per-t schedule tables (renoise: never null)
    const float *x0_shift{};            // [N_l,3] clash-guidance shift of the predicted x0; null: the kernels without the feature
};
// What the session-step form adds: the step's own arguments are in device memory, slot s = step[0] of each array (td_step_io)
struct TdStepSlot {
    int32_t *step{};                    // [2] step index and workgroup ticket, advanced by the launch; never null
    const int32_t *t_all{};             // [num_steps,B] time steps; row s becomes TdStepArgs::t
    int num_steps{};                    // s is clamped to num_steps - 1
    float *pos_traj{};                  // [num_steps,N_l,3]; slot s becomes pos_next, never null
    int64_t *v_traj{};                  // [num_steps,N_l]; slot s becomes v_next, never null
    float *v0_traj{};                   // [num_steps,N_l,C]; slot s becomes log_v0; null: not written
    float *vt_traj{};                   // [num_steps,N_l,C]; slot s becomes log_post; null: not written
    int pos_only{};                     // != 0: the types stay (v_frozen, no v_cur, renoise without uniform draws)
    const float *prog_table{};          // [num_steps,TD_PROG_ROW] a time program; row s becomes prow; null: no program
};
// Three runtime switches as template arguments: f(std::bool_constant<a>, std::bool_constant<b>, std::bool_constant<c>)
template <class F>
void td_dispatch3(bool a, bool b, bool c, F &&f) {
    const auto pick = [](bool on, auto &&g) { on ? g(std::true_type{}) : g(std::false_type{}); };
    pick(a, [&](auto A) { pick(b, [&](auto B) { pick(c, [&](auto C) { f(A, B, C); }); }); });
}
// a null fixed_mask / prow (prog_table) / x0_shift selects the kernel variant without that feature
int td_launch_posterior(const TdSchedules &sc, const TdStepArgs &a, hipStream_t s);
int td_launch_posterior_step(const TdSchedules &sc, const TdStepArgs &a, const TdStepSlot &sl, hipStream_t s);
// time programs: the renoise step of a slot (reads prow, Nl, C, pos, v, noise, uni and the outputs)
int td_launch_renoise(const TdStepArgs &a, hipStream_t s);
int td_launch_renoise_step(const TdStepArgs &a, const TdStepSlot &sl, hipStream_t s);
// guidance.hip (clash guidance): the arguments of one launch over B graphs.  Protein atoms either as ppos [N_p,3] +
// sigma [N_p] or as prot4 [N_p] (x, y, z, sigma) (a session's packed copy).  eval [N_l,3]: the positions the energy is taken at; with
// mean_type 1 (a session step of a model_mean_type 'noise' model) it is the network's output and x0 is formed from it, xt and the
// schedule entries of the graph's time step t_all[step[0] * B + g], as the posterior kernel forms it.
constexpr int TD_CLASH_TILE = 1024;
struct TdClashArgs {
    const float *ppos = nullptr, *sigma = nullptr;
    const float4 *prot4 = nullptr;
    const int32_t *pptr = nullptr, *lptr = nullptr;
    int B = 0;
    const float *eval = nullptr;
    float w = 0.f, max_shift = 0.f;
    int mean_type = 0, T = 0, num_steps = 0;
    const float *xt = nullptr, *rc = nullptr, *rm1 = nullptr;
    const int32_t *t_all = nullptr, *step = nullptr;
};
int td_launch_clash_shift(const TdClashArgs &a, float *shift, hipStream_t s);
int td_launch_clash_report(const TdClashArgs &a, int32_t *count, float *energy, float *min_dist, hipStream_t s);
int td_launch_clash_pack(const float4 *x4, const int32_t *prot_node, const float *sigma, int64_t Np, float4 *prot4, hipStream_t s);
// quality.hip (sample quality): the arguments of one launch over S frames x B molecules.  elem: class -> element
// index 0..7 (H C N O F P S Cl), filled by the entry point from the caller's atomic numbers; a profile's pe1 / pe2 are element indices
// too, -1 for "any".  The launcher zeroes hist and counts on the stream before the kernel adds to them.
constexpr int TD_QUALITY_MAX_CLASSES = 64, TD_QUALITY_MAX_PROFILES = 4, TD_QUALITY_BINS = 128;
struct TdQualityArgs {
    const float *pos = nullptr;              // [S,N_l,3]
    const int64_t *v = nullptr;              // [S,N_l]
    const int32_t *lptr = nullptr;           // [B+1]
    const uint8_t *include = nullptr;        // [S,B] or null: every molecule enters the histograms and counts
    int64_t Nl = 0;
    int S = 0, B = 0, K = 0, P = 0;
    int8_t elem[TD_QUALITY_MAX_CLASSES] = {};
    int pe1[TD_QUALITY_MAX_PROFILES] = {}, pe2[TD_QUALITY_MAX_PROFILES] = {}, n_edges[TD_QUALITY_MAX_PROFILES] = {};
    double cutoff[TD_QUALITY_MAX_PROFILES] = {};
    const double *edges[TD_QUALITY_MAX_PROFILES] = {};
    int32_t *nr_bonds = nullptr;             // [S,N_l] or null
    int32_t *stable_atoms = nullptr;         // [S,B]
    uint8_t *mol_stable = nullptr;           // [S,B]
    unsigned long long *hist = nullptr;      // [S,P,TD_QUALITY_BINS]
    unsigned long long *counts = nullptr;    // [S,8]
};
int td_launch_quality(const TdQualityArgs &a, hipStream_t s);
int td_element_index(int z);                 // quality_api.cpp: 0..7 (H C N O F P S Cl) of an atomic number, -1 for any other
int td_profile_element(int z);              // quality_api.cpp: of a profile's atomic number: -1 for 0 (any), -2 outside the table
// quality_api.cpp: the checks every entry point over a pack makes of its sizes and its class table (td_set_error under `who`); fills elem
int td_check_pack(const char *who, int64_t S, int64_t N_l, int64_t B, const int32_t *class_atomic_number, int32_t K, int8_t *elem);
// bonds.hip, rings.hip, fingerprint.hip (bond graph): the arguments of td_bond_graph / td_bond_list / td_ring_report / td_fingerprint over S
// frames x B molecules.  elem and a profile's pe1 / pe2 as in TdQualityArgs; aromatic: bit c set when class c is aromatic; pcat: 0 = any category.  The launcher zeroes
// hist on the stream before the kernels add to it.  Molecules of up to TD_BOND_SMALL_ATOMS atoms run in 128-lane workgroups, larger
// ones (up to TD_BOND_MAX_ATOMS) in 512-lane workgroups: both grids cover every molecule and each workgroup takes only its own kind.
constexpr int TD_BOND_MAX_ATOMS = 512, TD_BOND_SMALL_ATOMS = 128, TD_BOND_MAX_PROFILES = 16, TD_BOND_BINS = 128;
struct TdBondArgs {
    const float *pos = nullptr;              // [S,N_l,3]
    const int64_t *v = nullptr;              // [S,N_l]
    const int32_t *lptr = nullptr;           // [B+1]
    const uint8_t *include = nullptr;        // [S,B] or null: every molecule enters the histograms
    int64_t Nl = 0;
    int S = 0, B = 0, K = 0, P = 0;
    unsigned long long aromatic = 0ull;
    int8_t elem[TD_QUALITY_MAX_CLASSES] = {};
    int8_t pe1[TD_BOND_MAX_PROFILES] = {}, pe2[TD_BOND_MAX_PROFILES] = {}, pcat[TD_BOND_MAX_PROFILES] = {};
    int16_t n_edges[TD_BOND_MAX_PROFILES] = {};
    const double *edges[TD_BOND_MAX_PROFILES] = {};
    int32_t *n_bonds = nullptr, *n_fragments = nullptr, *largest = nullptr;      // [S,B]
    int32_t *fragment = nullptr;             // [S,N_l] or null
    unsigned long long *hist = nullptr;      // [S,P,TD_BOND_BINS]
    int64_t *bond_ptr = nullptr;             // [S*B+1] or null (td_bond_graph: written; td_bond_list: read)
    int64_t capacity = 0;                    // td_bond_list: entries the four outputs below hold
    int32_t *bond_atoms = nullptr;           // [capacity,2]
    uint8_t *bond_order = nullptr, *bond_category = nullptr;
    double *bond_length = nullptr;
    // rings.hip (td_ring_report, DESIGN.md section 3, "Rings"): bond_ptr is read and may be null; capacity bounds bond_ring and
    // bond_category (here the ring-aware category), each of which may be null.  The launcher zeroes ring_hist on the stream.
    uint32_t *ring_mask = nullptr;           // [S,B]
    int32_t *n_ring_bonds = nullptr, *n_ring_atoms = nullptr;                    // [S,B]
    int32_t *atom_ring = nullptr;            // [S,N_l] or null
    unsigned long long *ring_hist = nullptr; // [S,TD_RING_BITS]
    uint16_t *bond_ring = nullptr;           // [capacity] or null
    // fingerprint.hip (td_fingerprint, DESIGN.md section 3, "Fingerprints and diversity"): bits of the rounds 0 .. fp_radius, the key
    // after fp_rounds >= fp_radius rounds
    int fp_radius = 0, fp_rounds = 0;
    unsigned long long *fp_words = nullptr;  // [S,B,TD_FP_WORDS]
    int32_t *fp_bits = nullptr;              // [S,B]
    unsigned long long *fp_key = nullptr;    // [S,B]
    unsigned long long *atom_key = nullptr;  // [S,N_l] or null
};
constexpr int TD_RING_BITS = 32;
constexpr int TD_FP_BITS = 2048, TD_FP_WORDS = TD_FP_BITS / 64, TD_FP_MAX_RADIUS = 4, TD_FP_MAX_ROUNDS = 16;
// fingerprint.hip (td_fingerprint_similarity): the molecules of every frame against each other and against Q query fingerprints
struct TdSimArgs {
    const unsigned long long *words = nullptr;   // [S,B,TD_FP_WORDS]
    const int32_t *bits = nullptr;               // [S,B]
    const unsigned long long *key = nullptr;     // [S,B]
    const uint8_t *include = nullptr;            // [S,B] or null: every molecule with a fingerprint
    const unsigned long long *q_words = nullptr; // [Q,TD_FP_WORDS] or null
    int S = 0, B = 0, Q = 0;
    double *sim_sum = nullptr, *sim_max = nullptr;   // [S,B]
    int32_t *first_equal = nullptr;              // [S,B]
    int32_t *common = nullptr;                   // [S,B,B] or null
    int32_t *query_common = nullptr;             // [S,B,Q] or null
};
int td_launch_bond_graph(const TdBondArgs &a, hipStream_t s);
int td_launch_bond_list(const TdBondArgs &a, hipStream_t s);
int td_launch_ring_report(const TdBondArgs &a, hipStream_t s);
int td_launch_fingerprint(const TdBondArgs &a, hipStream_t s);
int td_launch_fingerprint_similarity(const TdSimArgs &a, hipStream_t s);
// geometry.hip (td_geometry_report, DESIGN.md section 3, "Local geometry"): the pack and the include bytes in `b`; of b's bond outputs
// only bond_ptr / capacity / bond_ring are used, and read (the ring filter of a torsion profile).  z: element index per position, -1 =
// any; kind 1 = angle, 2 = torsion; ring 0 = any, 1 = central bond in no ring, 2 = in a ring.  The launcher zeroes hist on the stream.
constexpr int TD_GEOM_MAX_DEGREE = 8, TD_GEOM_MAX_PROFILES = 16, TD_GEOM_BINS = 128;
struct TdGeomArgs {
    TdBondArgs b;
    int P = 0;
    int8_t kind[TD_GEOM_MAX_PROFILES] = {}, z[TD_GEOM_MAX_PROFILES][4] = {}, cat[TD_GEOM_MAX_PROFILES] = {}, ring[TD_GEOM_MAX_PROFILES] = {};
    int16_t n_edges[TD_GEOM_MAX_PROFILES] = {};
    const double *edges[TD_GEOM_MAX_PROFILES] = {};
    bool clash = false;                      // clash_thr holds the table
    double clash_thr[64] = {};
    int32_t *n_angles = nullptr, *n_torsions = nullptr, *n_degenerate = nullptr, *n_crowded = nullptr;   // [S,B]
    int32_t *n_clashes = nullptr;            // [S,B], written when clash
    int32_t *atom_clash = nullptr;           // [S,N_l] or null
    unsigned long long *hist = nullptr;      // [S,P,TD_GEOM_BINS]
};
int td_launch_geometry_report(const TdGeomArgs &a, hipStream_t s);
// pocket.hip (td_pocket_report, DESIGN.md section 3, "Pocket contacts"): the pack and the include bytes in `b` (none of b's outputs is
// used); one pocket of Np atoms for every molecule.  pelem: index over H C N O S Se, pkind in [0, n_kinds); an atom with either outside
// its range takes part nowhere.  clash_thr[e_l * 6 + e_p], e_l over H C N O F P S Cl.  reject2: a pair whose squared distance is not
// below it is below neither limit (the launcher forms it; +inf: no pair is rejected).  One plane of contact bits.
// The launcher zeroes kind_hist and pocket_freq on the stream.
constexpr int TD_POCKET_MAX_KINDS = 64, TD_POCKET_ELEMENTS = 6, TD_POCKET_THREADS = 256;
// The protein side of a pocket report, said once for the contacts and the interactions: the pocket, and the outputs that are indexed by
// protein atom or by kind.  T is the report's number of bit planes (contacts 1, interactions 3).
struct TdProteinSide {
    const float *ppos = nullptr;             // [Np,3]
    const int32_t *pelem = nullptr, *pkind = nullptr;                            // [Np]
    int Np = 0, W = 0, n_kinds = 0;          // W = ceil(Np / 64)
    const unsigned long long *ref_bits = nullptr;                                // [T,W] or null
    unsigned long long *bits = nullptr;      // [S,B,T,W] or null
    unsigned long long *kind_hist = nullptr; // [S,rows,n_kinds]: rows = 8 ligand elements (contacts), T (interactions)
    int32_t *pocket_freq = nullptr;          // [S,T,Np]
};
struct TdPocketArgs {
    TdBondArgs b;
    TdProteinSide p;
    double cutoff = 0.0, reject2 = 0.0;
    bool clash = false;                      // clash_thr holds the table
    double clash_thr[8 * TD_POCKET_ELEMENTS] = {};
    int32_t *n_contacts = nullptr, *n_contact_atoms = nullptr, *n_pocket_atoms = nullptr;   // [S,B]
    int32_t *n_clashes = nullptr, *n_clash_atoms = nullptr;                      // [S,B], written when clash
    double *min_dist = nullptr;              // [S,B]
    int32_t *n_ref_common = nullptr;         // [S,B], written when ref_bits
    int32_t *atom_contacts = nullptr, *atom_clash = nullptr;                     // [S,N_l] or null
};
int td_launch_pocket_report(const TdPocketArgs &a, hipStream_t s);
// interactions.hip (td_interaction_report, DESIGN.md section 3, "Pocket interactions"): the pack and the include bytes in `b`; the pocket
// as TdProteinSide holds it, and prole: the donor / acceptor bits of the host's table or a negative number.  A protein atom takes part
// when its element and its kind are in range and its role is >= 0; role_out is then its role with the hydrophobic bit resolved on the
// device (-1 for an atom that takes no part), and the pair kernel reads role_out alone.  reject2 as TdPocketArgs.  Three planes (ligand
// donates, ligand accepts, hydrophobic) of W = ceil(Np / 64) words.  The launcher zeroes kind_hist and pocket_freq on the stream.
constexpr int TD_ROLE_DONOR = 1, TD_ROLE_ACCEPTOR = 2, TD_ROLE_HYDROPHOBIC = 4, TD_INTERACTION_TYPES = 3;
struct TdInteractionArgs {
    TdBondArgs b;
    TdProteinSide p;
    const int32_t *prole = nullptr;          // [Np]
    double hbond_cutoff = 0.0, hydrophobic_cutoff = 0.0, hetero_cutoff = 0.0, reject2 = 0.0;
    int32_t *role_out = nullptr;             // [Np]
    int32_t *n_donated = nullptr, *n_accepted = nullptr, *n_hbonds = nullptr, *n_hydrophobic = nullptr;      // [S,B] pairs
    int32_t *n_hb_atoms = nullptr, *n_donors = nullptr, *n_acceptors = nullptr, *n_hydrophobic_atoms = nullptr;   // [S,B] ligand atoms
    int32_t *n_ref_common = nullptr;         // [S,B,3], written when ref_bits
    int32_t *atom_role = nullptr, *atom_hbonds = nullptr, *atom_hydrophobic = nullptr;      // [S,N_l] or null
};
int td_launch_interaction_report(const TdInteractionArgs &a, hipStream_t s);
// the protein roles alone (protein_role_kernel: reads p, prole and hetero_cutoff, writes role_out); score.hip resolves them with it
int td_launch_protein_roles(const TdInteractionArgs &a, hipStream_t s);
// score.hip (td_score_report, DESIGN.md section 3, "Docking-style score"): the pack in `b` (its include bytes are not used; bond_ptr /
// capacity / bond_ring are read by the rotor kernel, all null: no rotor kernel); of the pocket ppos, pelem, pkind, Np and n_kinds; role:
// the resolved protein roles (role_out of td_launch_protein_roles).  rsum[e_l * 6 + e_p] = R_l + R_p, e_l over H C N O F P S Cl.
// reject2 as TdPocketArgs, of the cutoff.  terms: per molecule the five unweighted term sums in units of 2^-TD_SCORE_FRAC_BITS.
constexpr int TD_SCORE_TERMS = 5, TD_SCORE_FRAC_BITS = 24;
struct TdScoreArgs {
    TdBondArgs b;
    TdProteinSide p;
    const int32_t *role = nullptr;           // [Np]
    double cutoff = 0.0, reject2 = 0.0;
    double rsum[8 * TD_POCKET_ELEMENTS] = {};
    long long *terms = nullptr;              // [S,B,TD_SCORE_TERMS]
    int32_t *n_pairs = nullptr;              // [S,B]
    int32_t *n_rot = nullptr;                // [S,B], written when bond_ptr
};
int td_launch_score_report(const TdScoreArgs &a, hipStream_t s);
int td_launch_rotors(const TdScoreArgs &a, hipStream_t s);      // the rotor kernel alone; nothing without bond_ptr
// relax.hip (td_score_minimize, DESIGN.md section 3, "Pose relaxation"): `sc` as td_launch_score_report takes it, of which terms and
// n_pairs are not used (n_rot is written by the rotor kernel when bond_ptr).  list_capacity: the entries of the LDS list of protein
// atoms, 0 .. TD_RELAX_LIST_CAPACITY; a molecule with more candidates walks the pocket in global memory, with the same integers.  The
// launcher copies the positions to pos_out on the stream first; the kernel writes the molecules that moved.
constexpr int TD_RELAX_LIST_CAPACITY = 4096, TD_RELAX_TRIALS = 10, TD_RELAX_DOF = 6;
constexpr double TD_RELAX_ARMIJO = 1e-4;
struct TdRelaxArgs {
    TdScoreArgs sc;
    double w[TD_SCORE_TERMS] = {};
    int max_steps = 0, max_evals = 0, list_capacity = TD_RELAX_LIST_CAPACITY;
    double max_shift = 0.0;
    float *pos_out = nullptr;                // [S,N_l,3]
    long long *terms_in = nullptr, *terms_out = nullptr;                         // [S,B,TD_SCORE_TERMS]
    int32_t *n_pairs_out = nullptr, *n_steps = nullptr, *n_evals = nullptr, *status = nullptr;   // [S,B]
    double *transform = nullptr;             // [S,B,7]: q (w, x, y, z), c - c0
    long long *grad_in = nullptr;            // [S,B,TD_RELAX_DOF]
};
int td_launch_score_minimize(const TdRelaxArgs &a, hipStream_t s);
// bonds_api.cpp also exports td_internal_score_minimize_capacity: td_score_minimize with list_capacity as a last argument, for the tests
// that hold the two walks to identical bytes.  It is not declared in include/targetdiff_hip.h and is no part of the public ABI.
// relax.hip (td_score_dock, DESIGN.md section 3, "Docking search"): `rx` as td_launch_score_minimize takes it, its outputs being the
// winning chain's (n_steps and n_evals summed over the chains).  One workgroup per (frame, molecule, chain), then one per (frame,
// molecule) that selects.  chain_aux is scratch of the caller's, on the stream: per chain the pairs and the status of its best and its
// steps.  td_internal_score_dock_capacity is to td_score_dock what td_internal_score_minimize_capacity is to td_score_minimize.
constexpr int TD_DOCK_MAX_CHAINS = 64, TD_DOCK_MAX_ROUNDS = 256, TD_DOCK_DRAWS = 7;
struct TdDockArgs {
    TdRelaxArgs rx;
    int n_chains = 1, n_rounds = 0;
    double amplitude = 0.0, temperature = 0.0;
    const double *draws = nullptr;           // [S,B,n_chains,n_rounds+1,TD_DOCK_DRAWS] in [0, 1): six for the mutation, one for Metropolis
    int32_t *best_chain = nullptr;           // [S,B]
    long long *chain_terms = nullptr;        // [S,B,n_chains,TD_SCORE_TERMS]
    double *chain_transform = nullptr;       // [S,B,n_chains,7]
    int32_t *chain_accepts = nullptr, *chain_evals = nullptr;                    // [S,B,n_chains]
    int32_t *chain_aux = nullptr;            // [S,B,n_chains,3]
};
int td_launch_score_dock(const TdDockArgs &a, hipStream_t s);
// sasa.hip (td_sasa_report, DESIGN.md section 3, "Solvent-accessible surface"): the pack and the include bytes in `b` (none of b's
// outputs is used); the pocket as TdProteinSide holds it, without kinds, in fields of its own (its kernels keep the argument block they
// were measured with: EXPERIMENTS.md "Pocket reports").  lig_R over H C N O F P S Cl and prot_R over H C N O S Se: the
// reach (van der Waals radius + probe) per element; dirs: P unit directions.  A candidate occluder is dropped only when its centre is
// farther than (R_a + R_b) (1 + TD_SASA_CULL_REL) + TD_SASA_CULL_ABS: sasa.hip says why that changes no result.  W = ceil(Np / 64).
// The launcher zeroes buried_sum and bits on the stream.
constexpr int TD_SASA_THREADS = 256, TD_SASA_MAX_POINTS = 256, TD_SASA_CHUNK = 512;
constexpr double TD_SASA_CULL_REL = 1e-4, TD_SASA_CULL_ABS = 1e-4;
struct TdSasaArgs {
    TdBondArgs b;
    const float *ppos = nullptr;             // [Np,3]
    const int32_t *pelem = nullptr;          // [Np]
    const double *dirs = nullptr;            // [P,3]
    int Np = 0, W = 0, P = 0;
    double lig_R[8] = {}, prot_R[TD_POCKET_ELEMENTS] = {};
    int32_t *n_free = nullptr, *n_bound = nullptr;                               // [S,B,8]
    int32_t *pocket_buried = nullptr;        // [S,B,6]
    int32_t *atom_free = nullptr, *atom_bound = nullptr;                         // [S,N_l] or null
    unsigned long long *bits = nullptr;      // [S,B,W] or null
    int32_t *pocket_free = nullptr;          // [Np]
    unsigned long long *pocket_mask = nullptr;                                   // [Np,4]
    unsigned long long *buried_sum = nullptr;                                    // [S,Np]
};
int td_launch_sasa_report(const TdSasaArgs &a, hipStream_t s);
// egnn.hip / node.hip
int td_launch_egnn_edge(const TdEgnnLayer &L, const float4 *x4, float4 *x4_out, const int32_t *nbr, const float *P, float *mi,
                        int64_t N, hipStream_t s);
int td_launch_egnn_node(const TdEgnnLayer &L, const float *mi, float *h, int64_t N, hipStream_t s);
// prop.hip
int td_launch_prop_linear(const float *X1, int K1, const float *X2, int K2, const float *W, const float *bias, const float *R, float *Y,
                          int64_t N, int O, int act, hipStream_t s);
int td_launch_prop_compose(const float *hp, const float *hl, const float *pp, const float *pl, const int32_t *protein_ptr,
                           const int32_t *ligand_ptr, float *h, float *x, int32_t *node_ptr, int64_t B, hipStream_t s);
int td_launch_prop_edge(const TdPropLayer &L, const float *x, const int32_t *nbr, int k, const float *P, float *mi, int64_t N,
                        float coeff, hipStream_t s);
int td_launch_prop_segment_sum(const float *h, const int32_t *node_ptr, const float *enc_graph, int Eg, float *pre_out, int64_t B,
                               hipStream_t s);
int td_launch_prop_select(const float *y, const int64_t *kind, int O, float *out, int64_t B, hipStream_t s);
// prop_bwd.hip
int td_launch_prop_bgemm(const float *X1, int ldx1, int K1, const float *X2, int ldx2, int K2, const float *W, int ldw, int trans,
                         const float *M, int ldm, int epi, const float *R1, int ldr1, const float *R2, int ldr2, float *Y, int ldy,
                         int64_t N, int O, hipStream_t s);
int td_prop_xty_chunks(int64_t N);
int td_launch_prop_xty(const float *A, int lda, int O, const float *B1, int ldb1, int K1, const float *B2, int ldb2, int K2, int64_t N,
                       float *part, float *G, int ldg, int col0, hipStream_t s);
int td_launch_prop_edge_bwd(const TdPropLayer &L, const float *W2Tf, const float *x, const int32_t *nbr, int k, const float *P,
                            const float *dmi, int64_t N, float coeff, float *Ae, float *DZ2, float *DZ1, float *RBF, float *Q, float *S,
                            float *DWP, hipStream_t s);
int td_launch_prop_radj(const int32_t *nbr, int64_t N, int k, int32_t *cnt, int32_t *ptr, int32_t *idx, hipStream_t s);
int td_launch_prop_gather(const float *X, const int32_t *ptr, const int32_t *idx, float *out, int64_t N, hipStream_t s);
int td_launch_prop_select_bwd(const float *gout, const int64_t *kind, int O, float *dy, int64_t B, hipStream_t s);
int td_launch_prop_broadcast(const float *dpre, const int32_t *node_ptr, float *dh, int64_t B, hipStream_t s);
int td_launch_prop_uncompose(const float *dh, const int32_t *protein_ptr, const int32_t *ligand_ptr, float *dhp, float *dhl, int64_t B,
                             hipStream_t s);
int td_launch_prop_pack_afrag(const float *W, int ld, int col0, int kb_count, int trans, float *out, hipStream_t s);
// likelihood.hip
int td_launch_perturb(const TdSchedules &sc, int T, const int32_t *t, const int32_t *lptr, int64_t Nl, int64_t B, int classes,
                      const float *pos, const int64_t *v, const float *noise, const float *uni, float *pos_t, int64_t *v_t,
                      hipStream_t s);
int td_launch_likelihood_terms(const TdSchedules &sc, int T, const int32_t *t, const int32_t *lptr, int64_t B, int classes,
                               const float *x0, const float *xt, const int64_t *v0, const int64_t *vt, const float *pred_pos,
                               const float *pred_v, float *kl_pos, float *kl_v, hipStream_t s);
int td_launch_likelihood_prior(const TdSchedules &sc, int T, const int32_t *lptr, int64_t B, int classes, const float *x0,
                               const int64_t *vidx, float *kl_pos, float *kl_v, hipStream_t s);
int td_launch_embed_ligand(const TdEmbed &emb, int classes, const int64_t *lv, int64_t Nl, float *h, hipStream_t s);
int td_launch_center(float *ppos, const int32_t *pptr, float *lpos, const int32_t *lptr, int64_t B, float *offset,
                     int compute, int sign, hipStream_t s);
int td_launch_reductions(const float *in, float *out, hipStream_t s);
