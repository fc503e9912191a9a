/*
 * targetdiff_hip.h -- C ABI of libtargetdiff_hip.so: the MI355X-native (gfx950) implementation of the
 * TargetDiff denoising hot path.
 *
 * The reference (guanjq/targetdiff) is pure Python: it has no FFI / plugin interface, its seams are
 * Python call signatures.  Each entry point below replaces one of those seams and
 * cites it.  All pointers named d_* are DEVICE pointers (HIP), caller-owned; outputs are
 * caller-allocated; `stream` is a hipStream_t passed as void*.  Every function returns TD_OK (0) or a
 * negative TD_E* code; td_last_error() gives the message for the calling thread.  No exceptions cross
 * the ABI.  Process-wide state: the per-thread error string, the td_profile_* timers (measurement only) and a per-kernel,
 * per-device "dynamic LDS size configured" bit; every switch lives in the td_model handle (td_model_set_option), nothing is
 * read from the environment.  A td_model may be shared by streams/threads of its device; a workspace or a session must
 * not be shared by concurrent calls.
 *
 * Packed-graph convention (what compose_context produces, models/common.py:120-137): the batch holds B
 * graphs stored contiguously; inside a graph the protein atoms come first, then the ligand atoms.
 * node_ptr[b]..node_ptr[b+1] is graph b's node range.
 */
#ifndef TARGETDIFF_HIP_H
#define TARGETDIFF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: the entry points declared below are its whole dynamic symbol table. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define TD_OK 0
#define TD_EINVAL (-1)      /* bad argument / unsupported configuration */
#define TD_ENOMEM (-2)      /* workspace too small or allocation failure */
#define TD_EHIP (-3)        /* HIP runtime error (message in td_last_error) */

#define TD_ABI_VERSION 5

typedef struct td_model td_model;

/* Model hyper-parameters (configs/training.yml:9-42, read from the checkpoint's config at
 * scripts/sample_diffusion.py:158-162).  The HIP kernels are specialised for the live architecture (hidden 128, 16 heads,
 * 20 Gaussians, 4 edge types, uni_o2, global edge gate); td_model_create returns TD_EINVAL for anything else.  The graph
 * construction of models/uni_transformer.py:276-286 is a run-time choice:
 *   TD_CUTOFF_KNN     knn_graph(x, k = knn), any 1 <= knn <= 64; knn <= 32 (32 = the live configuration) takes the fast path in
 *                     which one dst row is one 32-row MFMA tile (slots >= knn masked: the knn nearest are the first knn of
 *                     the 32 nearest) and the sampling session caches the static protein;
 *   TD_CUTOFF_HYBRID  batch_hybrid_edge_connection(add_p_index=True) (models/common.py:165-212): a ligand atom sees every
 *                     other ligand atom of its graph and its knn nearest protein atoms, a protein atom its knn nearest nodes;
 *   TD_CUTOFF_RADIUS  radius graph with a fan-out cap: the first max_num_neighbors nodes j != i of the graph (index order)
 *                     with |x_i - x_j|^2 < radius^2.  The reference's own radius mode is dead code (:278 reads an attribute
 *                     that is never assigned); the rule is this project's (oracle/shims.py).
 * Rows wider or narrower than 32 run as chunks of 32 slots through ragged (CSR-segment) variants of the edge kernels. */
#define TD_CUTOFF_KNN 0
#define TD_CUTOFF_HYBRID 1
#define TD_CUTOFF_RADIUS 2
#define TD_MAX_FANIN 64         /* largest knn / max_num_neighbors */

typedef struct td_config {
    int32_t hidden_dim;          /* 128 */
    int32_t n_heads;             /* 16 */
    int32_t knn;                 /* 32 (1 .. 64) */
    int32_t num_layers;          /* 9 (any >= 1) */
    int32_t num_r_gaussian;      /* 20 */
    int32_t edge_feat_dim;       /* 4 */
    int32_t protein_feat_dim;    /* 27 (<= 32) */
    int32_t ligand_num_classes;  /* 13 (<= 16) */
    int32_t num_timesteps;       /* 1000 */
    int32_t cutoff_mode;         /* TD_CUTOFF_* (0 = knn) */
    float radius;                /* TD_CUTOFF_RADIUS: cut-off in Angstrom */
    int32_t max_num_neighbors;   /* TD_CUTOFF_RADIUS: fan-out cap (1 .. 64) */
    int32_t model_mean_type;     /* 0 = 'C0' (the network predicts x0; configs/training.yml), 1 = 'noise' (it predicts x_t + eps:
                                    x0 = sqrt_recip_alphas_cumprod[t] x_t - sqrt_recipm1_alphas_cumprod[t] (pred - x_t),
                                    models/molopt_score_model.py:412-416, 663-666; sampling only, as in the reference) */
    int32_t num_blocks;          /* 0 or 1 (configs/training.yml) .. 8: the layer stack is applied num_blocks times, the graph and the
                                    edge gate rebuilt from the current coordinates before every pass, same weights
                                    (models/uni_transformer.py:306-323).  > 1: sampling sessions do not cache (their static-protein
                                    tables describe the first pass only) */
    int32_t ew_net_type;         /* 0 = 'global' (configs/training.yml: one gate MLP on the step-start distances), 1 = 'r' (every x2h / h2x
                                    stage has its own Linear(4 x 20 -> 1) + sigmoid on the layer's radial features,
                                    models/uni_transformer.py:34-35, 60-61, 102-103, 124-125), 2 = none (any other value of the
                                    reference's option: e_w = 1), 3 = 'm' (x2h: sigmoid(Linear(128 -> 1)) of the edge's value vector,
                                    :36-37, 62-63; h2x: e_w = 1, :126-127).  Other than 'global': default graph only, sessions do not cache */
    int32_t x2h_out_fc;          /* 1: h += node_output([attention output | h]) after every x2h stage (models/uni_transformer.py:39-40,
                                    81-84; the reference class's default, False in configs/training.yml); sessions do not cache */
    int32_t sync_twoup;          /* 1: the h2x stage of a layer reads the layer's INPUT features instead of its x2h output
                                    (models/uni_transformer.py:198); 0 in configs/training.yml and in the class */
    int32_t num_x2h, num_h2x;    /* stages per layer, 1 .. 4 (0 = 1, as in configs/training.yml): a layer runs num_x2h x2h stages on its
                                    start coordinates, then num_h2x h2x stages (models/uni_transformer.py:190-206), each stage with its
                                    own weights.  != 1: sessions do not cache, nothing is fused across stages */
    int32_t reserved[1];         /* zero */
} td_config;                     /* (ABI 5: the struct grew by 16 bytes; ew_net_type / x2h_out_fc took the place of ABI 4's reserved[2]) */

/* ---- library ------------------------------------------------------------------------------------ */
int td_abi_version(void);
const char *td_last_error(void);
/* 12 hex digits naming the SOURCES this binary was built from (SHA-256 over csrc/, this header and the compiler flags, set by
 * targetdiff_amd/build.py): bench lines and committed PMC profiles carry it, so a profile can be matched to the build it describes. */
const char *td_build_tag(void);

/* ---- model (replaces: ScorePosNet3D.__init__ + load_state_dict, models/molopt_score_model.py:194-311,
 *      scripts/sample_diffusion.py:158-163).  `host_weights` is the flat fp32 blob of the reference
 *      state_dict tensors in the order documented in targetdiff_amd/capi.py::flatten_state_dict
 *      (row-major [out, in] exactly as PyTorch stores them); the library re-packs them for its kernels
 *      (node-side projection split of the 340-wide first Linear, MFMA fragment order) and uploads them.
 *      `host_schedules` = 7 arrays of num_timesteps fp32 each, in this order: posterior_mean_c0_coef,
 *      posterior_mean_ct_coef, posterior_logvar, log_alphas_v, log_one_minus_alphas_v,
 *      log_alphas_cumprod_v, log_one_minus_alphas_cumprod_v (models/molopt_score_model.py:248-267); optionally an 8th,
 *      alphas_cumprod (td_perturb / td_likelihood_prior), and a 9th and 10th, sqrt_recip_alphas_cumprod and
 *      sqrt_recipm1_alphas_cumprod (:228-229; required by model_mean_type = 1). */
int td_model_create(const td_config *cfg, const float *host_weights, size_t num_weights,
                    const float *host_schedules, size_t num_schedule_floats, td_model **out);
void td_model_destroy(td_model *m);
size_t td_model_num_weights(const td_config *cfg);      /* expected length of the flat blob */
/* Per-model switches (stored in the handle: per device, nothing is read from the environment).  Set them before the model
 * is used; not to be changed while a call is in flight.
 *   "node_proj_split"        1 (default): the node-side 128 x 128 GEMMs run on v_mfma_f32_32x32x16_bf16 with both operands
 *                            split exactly into three bf16 pieces (an fp32 significand = 3 x 8 bits; 6 of the 9 piece products,
 *                            fp32 accumulation): fp32-equivalent results, 0 = plain fp32 MFMA
 *   "edge_key_split"         1 (default): the 21-wide radial / edge-type first layer of the attention passes on 32-slot rows
 *                            (x2h key and value passes, the h2x stage), of the chunked key pass and of the edge gate on v_mfma_f32_16x16x32_bf16
 *                            with the same exact three-piece split of both operands; 0 = fp32 MFMA (v_mfma_f32_16x16x4_f32)
 *   "edge_first_layer_f16"   1 (default): the 21-wide radial / type first layer of the attention kernels (x2h key / value passes, h2x stage) on v_mfma_f32_16x16x32_f16, weights
 *                            and inputs as pairs of f16 pieces (22 significant bits each; the MLP's first layer -- node projections included --
 *                            is packed in units of a power of two so that no piece meets the f16 subnormal floor): two products and two
 *                            16-byte table reads per tile; 0 = the exact bf16 x 3 piece triples (four products, three reads).  Needs
 *                            "edge_key_split"; the edge gate uses the bf16 form under either setting
 *   "edge_second_layer_f16"  1 (default): the per-edge 128-deep products of the x2h key / value passes (logits = z . U_i, alpha^T z) on
 *                            v_mfma_f32_16x16x32_f16, both operands as pairs of f16 pieces (22 significant bits each, scaled by exact
 *                            powers of two; three piece products, fp32 accumulation): within one to two fp32 roundings of the fp32
 *                            products; 0 = v_mfma_f32_16x16x4_f32 on the fp32 values.  Applies to the value pass
 *                            on every graph and to the key pass on rows of one 32-slot chunk (the default k = 32 graph; the protein rows
 *                            of `hybrid`, k < 32 and capped-radius graphs); the key pass of rows that span several chunks (k > 32, the
 *                            ligand rows of `hybrid`) follows it only while "edge_first_layer_f16" is on (fp32 logits otherwise).
 *                            Both f16 options apply per attention MLP only where the f16 pieces keep its precision: an MLP whose folded
 *                            LayerNorm scale M (csrc/pack.cpp FoldedMlp) exceeds 2^16, or whose first layer could not take its full power-of-two
 *                            scale, runs both layers in fp32 whatever these options say ("fold_fp32_mlps")
 *   "edge_row_dealing"       0 .. 2 (default 2; other values are clamped): x2h key / value passes: units of rows dealt round-robin to an
 *                            XCD's workgroups (0: one contiguous share per workgroup; 1: a fixed row sequence per wave; 2: the workgroup's
 *                            rows handed to its waves one at a time through an LDS counter; the value pass's protein rows on a general graph
 *                            with one chunk per protein row always take 2: the 12-wave kernel has no other form)
 *   "node_proj_bpipe"        0 (default): split node GEMMs: register double-buffering of the B fragments (LDS reads ahead of the MFMAs;
 *                            measured slower, kept as a switch)
 *   "node_proj_async"        1 (default): split node GEMMs: B chunks by inline-asm global_load_lds + an explicit wait per round
 *                            (0: the builtin, which the compiler serialises)
 *   "h2x_fused"              1 (default): key + value halves of the h2x stage in one launch; 0 = two launches
 *   "session_hop_levels"     1 .. 4 (default 4): receptive-field levels a sampling session prunes the last layers with
 *   "session_forward_reach"  1 (default): layer 1 of a session runs on the ligand's one-hop forward reach only
 *   "session_share_pockets"  1 (default): a sampling session on the default graph keeps its static tables (protein-only sorted k-NN keys and lists,
 *                            cached gate rows, embeddings, layer-0 / layer-1 outputs of the protein-only graph) once per DISTINCT protein block
 *                            of the batch -- all samples of a pocket carry the same block (scripts/sample_diffusion.py:42) -- found by a hash +
 *                            bitwise comparison at td_session_create; same results bit for bit; 0 = once per graph
 *   "session_step_lists"     1 (default): the row lists of a session step come from one launch (a workgroup per graph);
 *                            0 = the separate list kernels (also used when a graph exceeds 12288 nodes)
 * Read-only (td_model_get_option; td_model_set_option returns TD_EINVAL): decisions of the LayerNorm fold at td_model_create --
 *   "fold_dead_units"        LayerNorm units, over every folded MLP (attention MLPs and the edge gate), replaced by their constant relu(beta):
 *                            those whose largest possible term sqrt(hidden) |weight| max |second-Linear column| is at most 2^-30 of the MLP's
 *                            largest unit's
 *   "fold_fp32_mlps"         attention MLPs (hk, hv, xk, xv of every layer) that run both layers in fp32 because the f16 pieces would lose
 *                            precision there (0 for the seeded and trained-like weight sets of the tests and the benchmark) */
int td_model_set_option(td_model *m, const char *name, int32_t value);
int td_model_get_option(const td_model *m, const char *name, int32_t *value);

/* ---- workspace ---------------------------------------------------------------------------------- */
/* Bytes of scratch td_refine_forward / td_model_forward need for a batch of N nodes (N_l of them ligand)
 * in B graphs.  Graph modes other than the 32-slot default (k > 32, hybrid, radius cap > 32), td_knn and td_graph_build
 * additionally take ONE stream-ordered block (hipMallocAsync on `stream`, freed in stream order before the call returns) for
 * the chunked neighbour table, whose size depends on the per-graph atom counts and is not known from (N, B, N_l) alone. */
size_t td_workspace_bytes(const td_model *m, int64_t N, int64_t B, int64_t N_l);

/* ---- graph bookkeeping ---------------------------------------------------------------------------
 * batch [N] int64, sorted ascending (torch_geometric `batch` vector) -> ptr [B+1] int32. */
int td_graph_ptr(const int64_t *d_batch, int64_t N, int64_t B, int32_t *d_ptr, void *stream);

/* ---- kNN graph (replaces: torch_geometric.nn.knn_graph(x, k, batch, flow='source_to_target') at
 *      models/uni_transformer.py:280).  out_nbr [N, k] int32: row i = the k nearest same-graph nodes of
 *      node i, ascending by (d2, index), d2 = (dx*dx + dy*dy) + dz*dz in fp32 without FMA contraction;
 *      -1 padded when the graph has fewer than k+1 nodes.  1 <= k <= 64.  `max_graph_nodes` is a performance hint
 *      (0 = unknown). */
int td_knn(const float *d_x /*[N,3]*/, const int32_t *d_node_ptr /*[B+1]*/, int64_t N, int64_t B, int32_t k,
           int32_t max_graph_nodes, int32_t *d_out_nbr, void *stream);

/* ---- the model's graph on a composed batch (replaces: UniTransformerO2TwoUpdateGeneral._connect_edge,
 *      models/uni_transformer.py:276-286, for the model's cutoff_mode).  d_out_nbr [N, width] int32, -1 padded: the
 *      in-neighbours (edge sources) of node i.  kNN: ascending (d2, index).  hybrid ligand rows: the other ligand atoms
 *      (ascending index), then the knn nearest protein atoms (ascending (d2, index)).  radius: ascending index.  Entries
 *      beyond `width` are dropped.  Needs compose_context order (protein rows first in every graph). */
int td_graph_build(const td_model *m, const float *d_x, const uint8_t *d_mask_ligand, const int32_t *d_node_ptr, int64_t N,
                   int64_t B, int32_t max_graph_nodes, int32_t *d_out_nbr, int32_t width, void *stream);

/* ---- backbone (replaces: refine_net(h, x, mask_ligand, batch, return_all=False, fix_x) ->
 *      {'x','h'}, UniTransformerO2TwoUpdateGeneral.forward, models/uni_transformer.py:301-328).
 *      d_h [N,128] f32, d_x [N,3] f32, d_mask_ligand [N] uint8, d_node_ptr [B+1] int32.
 *      d_out_nbr ([N,32] int32) and d_out_ew ([N,32] f32, the global edge gate of :312-316) may be NULL; they exist for
 *      the default k = 32 kNN graph only (other graphs: td_graph_build). */
int td_refine_forward(const td_model *m, const float *d_h, const float *d_x, const uint8_t *d_mask_ligand,
                      const int32_t *d_node_ptr, int64_t N, int64_t B, int32_t fix_x, int32_t max_graph_nodes,
                      float *d_out_h, float *d_out_x, int32_t *d_out_nbr, float *d_out_ew,
                      void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- one denoiser evaluation (replaces: ScorePosNet3D.forward, models/molopt_score_model.py:313-368).
 *      Protein / ligand atoms are given un-composed, each sorted by graph:
 *      d_protein_ptr / d_ligand_ptr are [B+1] int32 prefix offsets.  Outputs: pred_ligand_pos [N_l,3],
 *      pred_ligand_v [N_l,C], final_ligand_h [N_l,128]; d_final_h [N,128] may be NULL.
 *      d_ligand_graph_bias (NULL when time_emb_dim == 0, the live configuration): [B][128] fp32, row g is added to the embedding
 *      of every ligand atom of graph g before the bias -- the time-embedding columns of ligand_atom_emb applied to the graph's
 *      time feature (:319-329: `simple` = (t / T) * W[:, C], `sin` = W[:, C:] time_emb(t)); column 127 (the node indicator) is 0.
 *      The caller evaluates that small per-graph term (the mirror does it with torch). */
int td_model_forward(const td_model *m, const float *d_protein_pos, const float *d_protein_v,
                     const int32_t *d_protein_ptr, int64_t N_p, const float *d_ligand_pos,
                     const int64_t *d_ligand_v, const int32_t *d_ligand_ptr, int64_t N_l, int64_t B,
                     int32_t fix_x, int32_t max_graph_nodes, float *d_pred_ligand_pos, float *d_pred_ligand_v,
                     float *d_final_ligand_h, float *d_final_h, void *d_workspace, size_t workspace_bytes,
                     const float *d_ligand_graph_bias, void *stream);

/* ---- posterior update of one reverse-diffusion step (replaces the loop body
 *      models/molopt_score_model.py:673-685: q_pos_posterior :424, extract :706, q_v_posterior :401,
 *      q_v_pred :383, q_v_pred_one_timestep :371, log_add_exp :173, index_to_log_onehot :124,
 *      log_sample_categorical :160).  d_t [B] int32 per-graph timestep; d_noise [N_l,3] ~ N(0,1) and
 *      d_uniform [N_l,C] ~ U[0,1) are supplied by the caller (torch.randn_like / rand_like in the
 *      reference).  d_log_v0 / d_log_post ([N_l,C]) may be NULL. */
int td_posterior_step(const td_model *m, const int32_t *d_t, const int32_t *d_ligand_ptr, int64_t N_l,
                      int64_t B, const float *d_ligand_pos, const int64_t *d_ligand_v,
                      const float *d_pred_pos, const float *d_pred_v, const float *d_noise,
                      const float *d_uniform, float *d_pos_next, int64_t *d_v_next, float *d_log_v0,
                      float *d_log_post, void *stream);
/* ---- the same step with known ("fixed") ligand atoms: scaffold-constrained sampling by replacement conditioning (DESIGN.md,
 *      "Scaffold-constrained sampling"; no seam in the reference, which has no such mode -- the pieces are its q_v_sample
 *      :394-398 and the forward-process sample of :577-588).  d_fixed_mask [N_l] bytes (0 / non-0; a torch bool tensor),
 *      d_fixed_pos [N_l,3] the known positions in the centred frame of d_ligand_pos, d_fixed_v [N_l] the known types; rows with
 *      mask 0 are not read.  A flagged atom of a graph at time step t takes, instead of the posterior draw,
 *        t > 0:  x' = sqrt(abar[t-1]) x0 + sqrt(1 - abar[t-1]) d_noise[atom]        (each product and the sum rounded on its own)
 *                v' = argmax_c(gumbel(d_uniform[atom][c]) + log q(v_{t-1} = c | v0)), first maximum
 *        t == 0: x' = x0, v' = v0
 *      d_log_post receives that log q (t == 0: log(clamp(onehot(v0), 1e-30))), d_log_v0 the model's log-softmax as for every
 *      atom.  No draw is added or skipped.  d_fixed_mask == NULL is td_posterior_step.  Needs a model created with
 *      alphas_cumprod (8 or 10 schedule arrays): TD_EINVAL otherwise. */
int td_posterior_step_fixed(const td_model *m, const int32_t *d_t, const int32_t *d_ligand_ptr, int64_t N_l,
                            int64_t B, const float *d_ligand_pos, const int64_t *d_ligand_v,
                            const float *d_pred_pos, const float *d_pred_v, const float *d_noise,
                            const float *d_uniform, float *d_pos_next, int64_t *d_v_next, float *d_log_v0,
                            float *d_log_post, const uint8_t *d_fixed_mask, const float *d_fixed_pos,
                            const int64_t *d_fixed_v, void *stream);

/* ---- time programs ("Time programs"; no seam in the reference, whose sampler walks T-1, T-2, ... one level per
 *      denoiser call, models/molopt_score_model.py:649).  A program is a list of slots, each a DENOISE step t -> s (s < t, any
 *      distance; s = -1 is clean data) or a RENOISE step s -> t (t > s, the forward process).  A slot's coefficients are one row of
 *      TD_PROG_ROW floats, computed on the host in float64 and rounded once (targetdiff_amd/schedule.py, TimeProgram.tables;
 *      abar = alphas_cumprod, Lc = log_alphas_cumprod_v, abar(-1) = 1, Lc(-1) = 0, log1m(a) = log(1 - exp(a) + 1e-40)):
 *        DENOISE  C0 = (1 - abar_t/abar_s) sqrt(abar_s) / (1 - abar_t), CT = (1 - abar_s) sqrt(abar_t/abar_s) / (1 - abar_t),
 *                 LOGVAR = log var (not read when LAST), LOG_A = Lc_t - Lc_s, LOG_1MA = log1m(LOG_A), LOG_CA = Lc_s,
 *                 LOG_1MCA = log1m(Lc_s), ABAR_TO = abar_s (the level known atoms are diffused to), LAST = 1 when s = -1 (no noise,
 *                 known atoms take their known state); a unit step holds the model's own table entries, which makes it
 *                 td_posterior_step bit for bit
 *        RENOISE  RHO = abar_t / abar_s, LOG_R = Lc_t - Lc_s, LOG_1MR = log1m(LOG_R)
 *      td_posterior_step_program = td_posterior_step_fixed with the step's coefficients read from d_prog_row (device memory, one
 *      row); d_t is still the time the denoiser ran at (model_mean_type 'noise' reads its entries).  d_fixed_mask may be NULL.
 *      td_renoise_step: x' = sqrt(RHO) x + sqrt(1 - RHO) d_noise (roots in fp32, each product and the sum rounded on its own);
 *      log q_c = log_add_exp(log(clamp(onehot(v), 1e-30))_c + LOG_R, LOG_1MR - ln C), v' = argmax_c(gumbel(d_uniform_c) + log q_c),
 *      first maximum; every atom alike.  d_uniform == NULL (pos_only): d_v_next = d_ligand_v.  d_log_v0 / d_log_q ([N_l,C], may be
 *      NULL) receive the clamped log one-hot of the incoming type and log q.  Outputs may alias inputs. */
enum { TD_PROG_C0 = 0, TD_PROG_CT, TD_PROG_LOGVAR, TD_PROG_LOG_A, TD_PROG_LOG_1MA, TD_PROG_LOG_CA, TD_PROG_LOG_1MCA, TD_PROG_ABAR_TO,
       TD_PROG_LAST, TD_PROG_RHO, TD_PROG_LOG_R, TD_PROG_LOG_1MR, TD_PROG_ROW };
enum { TD_PROG_DENOISE = 0, TD_PROG_RENOISE = 1 };
int td_posterior_step_program(const td_model *m, const int32_t *d_t, const float *d_prog_row, const int32_t *d_ligand_ptr,
                              int64_t N_l, int64_t B, const float *d_ligand_pos, const int64_t *d_ligand_v,
                              const float *d_pred_pos, const float *d_pred_v, const float *d_noise, const float *d_uniform,
                              float *d_pos_next, int64_t *d_v_next, float *d_log_v0, float *d_log_post,
                              const uint8_t *d_fixed_mask, const float *d_fixed_pos, const int64_t *d_fixed_v, void *stream);
int td_renoise_step(const td_model *m, const float *d_prog_row, int64_t N_l, const float *d_ligand_pos, const int64_t *d_ligand_v,
                    const float *d_noise, const float *d_uniform, float *d_pos_next, int64_t *d_v_next, float *d_log_v0,
                    float *d_log_q, void *stream);

/* ---- clash guidance ("Clash guidance"; the reference has no such mode).  All coordinates in one frame (the
 *      sampler's: centred).  Graph g has protein atoms p_j with contact radii sigma_j > 0 (Angstrom) and ligand points x_i:
 *        E_g = 1/2 sum_i sum_j max(0, sigma_j - d_ij)^2,  d_ij = |x_i - p_j|
 *        D_i = -w grad_{x_i} E_g = w sum_j max(0, sigma_j - d_ij) (x_i - p_j) / d_ij      (pairs with d_ij < 1e-6 add nothing)
 *      and D_i is scaled to length max_shift when max_shift > 0 and |D_i| exceeds it (max_shift == 0: no cap).
 *      td_clash_shift writes D [N_l,3] for the points d_pos [N_l,3]; td_clash_report writes per graph the number of pairs with
 *      d_ij < sigma_j (coincident pairs included), E_g and min d_ij (+inf for a graph without pairs).  d_protein_ptr / d_ligand_ptr:
 *      [B+1] int32 prefix offsets.  A graph's result depends on that graph alone, and the same inputs give the same bits every time
 *      (fixed-order reductions, no atomics).  TD_EINVAL for w < 0 or max_shift < 0; the radii are not read on the host: a binding
 *      checks sigma > 0.
 *      td_posterior_step_guided = td_posterior_step_program whose x0 -- d_pred_pos for model_mean_type 'C0', rc[t] x_t - rm1[t]
 *      (d_pred_pos - x_t) for 'noise' -- is replaced by fl32(x0 + d_x0_shift[atom]) (one rounded add), on every step, the last
 *      included; atoms flagged in d_fixed_mask ignore the shift.  d_prog_row == NULL: the model's own tables (td_posterior_step_fixed);
 *      d_x0_shift == NULL: exactly the kernels of the unguided entry points.
 *      (These entry points are additions: no existing signature or struct changes, and TD_ABI_VERSION stays 5.) */
int td_clash_shift(const float *d_protein_pos, const float *d_sigma, const int32_t *d_protein_ptr, const int32_t *d_ligand_ptr,
                   int64_t B, const float *d_pos, float w, float max_shift, float *d_shift, void *stream);
int td_clash_report(const float *d_protein_pos, const float *d_sigma, const int32_t *d_protein_ptr, const int32_t *d_ligand_ptr,
                    int64_t B, const float *d_pos, int32_t *d_count, float *d_energy, float *d_min_dist, void *stream);
int td_posterior_step_guided(const td_model *m, const int32_t *d_t, const float *d_prog_row, const int32_t *d_ligand_ptr,
                             int64_t N_l, int64_t B, const float *d_ligand_pos, const int64_t *d_ligand_v,
                             const float *d_pred_pos, const float *d_pred_v, const float *d_noise, const float *d_uniform,
                             float *d_pos_next, int64_t *d_v_next, float *d_log_v0, float *d_log_post,
                             const uint8_t *d_fixed_mask, const float *d_fixed_pos, const int64_t *d_fixed_v,
                             const float *d_x0_shift, void *stream);

/* ---- sample quality of ligand frames ("Sample quality"; replaces the chemistry-free half of
 *      scripts/evaluate_diffusion.py:75-87: utils/evaluation/analyze.py check_stability with hs=False, the counts behind
 *      utils/evaluation/eval_bond_length.py get_pair_length_profile and the element Counter).  No model handle.
 *      Input: S frames of the same B molecules: d_pos [S,N_l,3] fp32, d_v [S,N_l] int64 class indices, d_ligand_ptr [B+1] int32
 *      prefix offsets shared by all frames.  class_atomic_number [K] (HOST memory, 1 <= K <= 64): the atomic number of every
 *      class; TD_EINVAL when one is not H C N O F P S Cl.  An atom whose class is outside [0, K) has no element: it bonds with
 *      nothing, is never stable and is counted nowhere (a binding refuses it).
 *      Per pair i < j of one molecule: d = sqrt((dx dx + dy dy) + dz dz) in float64 on the widened coordinates, every product and
 *      sum rounded once; with D = 100 d and b1, b2, b3 the single / double / triple bond length of the element pair in pm (-1:
 *      none), the order is 0 if D >= b1 + 10, else 1 if D >= b2 + 5, else 2 if D >= b3 + 3, else 3.  nr_bonds of an atom is the
 *      sum of its pairs' orders; an atom is stable when 0 < nr_bonds <= the bonds its element may hold (1 4 3 2 1 5 4 1); a
 *      molecule is stable when all its atoms are (0 atoms: stable; 1 atom: not).
 *      Output: d_nr_bonds [S,N_l] int32 (may be NULL), d_stable_atoms [S,B] int32, d_mol_stable [S,B] uint8, and per frame, over
 *      the molecules whose d_include [S,B] byte is non-zero (NULL: all): d_hist [S,P,128] int64 pair-distance histograms and
 *      d_counts [S,8] int64 atoms per element (H C N O F P S Cl).  Both are zeroed by the call.  Profile p (HOST array, P <= 4)
 *      takes the pairs whose unordered elements are (z1, z2) (0: any) and whose d < cutoff, into bin numpy.searchsorted(edges, d,
 *      'left'), found by a search of d_edges [n_edges] (DEVICE memory, float64, ascending, 1 <= n_edges <= 127; not read on the
 *      host: a binding checks the order).  All outputs are integers summed in integer arithmetic: they do not depend on the grid
 *      or on the order of arrival.  (An addition: TD_ABI_VERSION stays 5.) */
typedef struct td_pair_profile {
    int32_t z1, z2;
    double cutoff;
    int32_t n_edges, reserved;
    const double *d_edges;
} td_pair_profile;
int td_quality_report(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                      const int32_t *class_atomic_number, int32_t K, const uint8_t *d_include, const td_pair_profile *profiles,
                      int32_t P, int32_t *d_nr_bonds, int32_t *d_stable_atoms, uint8_t *d_mol_stable, int64_t *d_hist,
                      int64_t *d_counts, void *stream);

/* ---- bond graph of ligand frames ("Bond graph"): the bonds the rule above implies, kept instead of summed.
 *      No model handle.  The pack (d_pos, d_v, d_ligand_ptr, S, N_l, B, class_atomic_number, K, d_include) is td_quality_report's.
 *      class_aromatic [K] (HOST bytes, NULL: no class is aromatic) flags the aromatic classes.
 *      Bond: a pair i < j of one molecule whose order, by exactly the rule of td_quality_report, is > 0; an atom whose class is
 *      outside [0, K) bonds with nothing.  Category of a bond: its order, except 4 (aromatic) when both atoms' classes are aromatic
 *      and the order is 1 or 2.  Fragment: a connected component of the bond graph; an atom's label is the smallest molecule-local
 *      atom index of its component.  A molecule of more than 512 atoms (TD_BOND_MAX_ATOMS), or one whose offsets leave [0, N_l], gets
 *      n_bonds = n_fragments = largest_fragment = -1, counts 0 bonds in d_bond_ptr and contributes nothing else (a binding refuses it).
 *      td_bond_graph output: d_n_bonds, d_n_fragments (0 for an empty molecule), d_largest_fragment (atoms of the largest component)
 *      [S,B] int32; d_fragment [S,N_l] int32 labels (may be NULL); d_bond_hist [S,P,128] int64, zeroed by the call: over the molecules
 *      whose d_include byte is non-zero (NULL: all), profile p (HOST array, P <= 16) takes the bonds whose unordered elements are
 *      (z1, z2) (0: any) and whose category is `category` (1 .. 4, 0: any) into bin numpy.searchsorted(edges, d, 'left') of d_edges
 *      [n_edges] (DEVICE float64, ascending, 1 <= n_edges <= 127; the last bin takes everything beyond the last edge: no cutoff);
 *      d_bond_ptr [S*B+1] int64 (may be NULL): the exclusive prefix of n_bonds in (frame, molecule) order, summed in a fixed order.
 *      td_bond_list writes the n_bonds = d_bond_ptr[S*B] bonds (the caller reads that entry: the one host synchronisation of the
 *      path) in ascending (frame, molecule, i, j) order: d_bond_atoms [n_bonds,2] int32 indices along the pack's atom axis,
 *      d_bond_order / d_bond_category [n_bonds] uint8 and d_bond_length [n_bonds] float64 (the d of the rule).  Nothing is written
 *      at or beyond entry n_bonds, whatever d_bond_ptr holds.  All outputs are integers or float64 values formed by one lane: they
 *      do not depend on the grid or on the order of arrival.  (Additions: TD_ABI_VERSION stays 5.) */
typedef struct td_bond_profile {
    int32_t z1, z2, category, n_edges;
    const double *d_edges;
} td_bond_profile;
int td_bond_graph(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                  const int32_t *class_atomic_number, int32_t K, const uint8_t *d_include, const uint8_t *class_aromatic,
                  const td_bond_profile *profiles, int32_t P, int32_t *d_n_bonds, int32_t *d_n_fragments, int32_t *d_largest_fragment,
                  int32_t *d_fragment, int64_t *d_bond_hist, int64_t *d_bond_ptr, void *stream);
int td_bond_list(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                 const int32_t *class_atomic_number, int32_t K, const uint8_t *class_aromatic, const int64_t *d_bond_ptr, int64_t n_bonds,
                 int32_t *d_bond_atoms, uint8_t *d_bond_order, uint8_t *d_bond_category, double *d_bond_length, void *stream);

/* ---- rings of ligand frames ("Rings"): per (frame, molecule), on the bond graph exactly as td_bond_graph
 *      defines it (the same pack, class table, aromatic flags and d_include bytes; an atom whose class is outside [0, K) bonds with
 *      nothing).  Ring size of a bond (i, j): the number of atoms of the shortest cycle through it = 1 + the shortest path from i to
 *      j in the graph without the edge (i, j); 0 when there is none (a bridge); a unique integer in {0, 3 .. n}.  Ring size of an
 *      atom: the minimum of the non-zero ring sizes of its bonds, 0 when it has none: the smallest ring that contains the atom.  Ring
 *      mask of a molecule: bit min(k, 31) is set when some bond has ring size k; "has a ring of size k" means that bit.  This is not a
 *      smallest set of smallest rings: a basis ring all of whose bonds also lie in smaller rings is not seen.  Ring-aware category
 *      of a bond: td_bond_list's, except that 4 (aromatic) also needs a ring size of 5 or 6; otherwise the category is the order.
 *      Output: d_ring_mask [S,B] uint32; d_n_ring_bonds / d_n_ring_atoms [S,B] int32, the bonds / atoms with a non-zero ring size;
 *      d_atom_ring [S,N_l] int32 (may be NULL); d_ring_hist [S,32] int64, zeroed by the call: entry k > 0 counts the molecules whose
 *      d_include byte is non-zero (NULL: all) and whose mask has bit k, entry 0 those whose mask is 0 (no ring at all).  Per bond, in
 *      td_bond_list's order and at its offsets (d_bond_ptr [S*B+1] of td_bond_graph on the same pack; n_bonds = d_bond_ptr[S*B]):
 *      d_bond_ring [n_bonds] uint16 and d_bond_category [n_bonds] uint8, the ring-aware category; either may be NULL, d_bond_ptr may
 *      be NULL when both are, and TD_EINVAL when one is asked for without it.  Nothing is written at or beyond entry n_bonds,
 *      whatever d_bond_ptr holds.  A molecule of more than 512 atoms, or one whose offsets leave [0, N_l], gets n_ring_bonds =
 *      n_ring_atoms = -1 and mask 0 and contributes nothing else (a binding refuses it).  All outputs are integers: they do not
 *      depend on the grid or on the order of arrival.  (An addition: TD_ABI_VERSION stays 5.) */
int td_ring_report(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                   const int32_t *class_atomic_number, int32_t K, const uint8_t *d_include, const uint8_t *class_aromatic,
                   const int64_t *d_bond_ptr, int64_t n_bonds, uint32_t *d_ring_mask, int32_t *d_n_ring_bonds, int32_t *d_n_ring_atoms,
                   int32_t *d_atom_ring, int64_t *d_ring_hist, uint16_t *d_bond_ring, uint8_t *d_bond_category, void *stream);

/* ---- fingerprints of ligand frames ("Fingerprints and diversity"): per (frame, molecule), on the bond graph
 *      exactly as td_bond_graph defines it (the same pack, class table and aromatic flags).  This is not RDKit's RDKFingerprint: it
 *      is a circular, Morgan-style fingerprint over this project's bond graph, whose orders come from the bond-length table; its
 *      similarities are comparable between runs of this library, not with published tables.  All arithmetic on uint64, wrapping.
 *      mix(x), the splitmix64 finaliser: x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) *
 *      0x94D049BB133111EB; x ^= x >> 31.  An atom whose class is in [0, K): id_0 = mix(Z | aromatic << 8 | degree << 16 | valence <<
 *      24) with Z its atomic number, aromatic its class flag, degree its number of bonds and valence the sum of their orders; an atom
 *      of no class takes no part anywhere.  Round r = 1, 2, ...: id_r[i] = mix(mix(id_{r-1}[i] ^ r) + sum over the bonded j of
 *      mix(id_{r-1}[j] ^ mix(category_ij))), the category that of td_bond_list (1, 2, 3, 4 = aromatic); the sum is commutative: the
 *      order the atoms are stored in does not matter.  Fingerprint: TD_FP_BITS = 2048 bits, bit id_r[i] mod 2048 set for every such
 *      atom and every r = 0 .. radius (0 <= radius <= 4).  Key, after key_rounds rounds (radius <= key_rounds <= 16): mix((sum over
 *      the atoms of mix(id[i])) ^ mix(n_valid << 32 | n_bonds)).  Equal keys: not told apart by Weisfeiler-Lehman colour refinement
 *      with these invariants after that many rounds.  This is not a canonical form: graphs that refinement cannot separate (the
 *      skeletons of decalin and bicyclopentyl) have equal keys.
 *      Output: d_fp_words [S,B,32] int64, word w bit k = fingerprint bit 64 w + k; d_n_bits [S,B] int32, the number of set bits;
 *      d_key [S,B] int64; d_atom_key [S,N_l] int64 (may be NULL), the atom's id after key_rounds rounds, 0 for an atom of no class.
 *      A molecule of more than 512 atoms, or one whose offsets leave [0, N_l], gets n_bits = -1, words and key 0 and its atoms'
 *      d_atom_key entries are not written (a binding refuses it).
 *      td_fingerprint_similarity compares the molecules of each frame.  Included: d_include byte non-zero (NULL: all) and n_bits >= 0.
 *      T(a, b) = (double)c / (double)(n_a + n_b - c), c = popcount(fp_a & fp_b); 0 when the union is empty.  d_sim_sum [S,B] float64:
 *      the sum of T(a, b) over the included b != a, added in ascending b with one add per term (it does not depend on the grid), 0
 *      for an a that is not included; d_sim_max [S,B] float64: the largest such T, 0 without a partner; d_first_equal [S,B] int32:
 *      the smallest included b with key_b == key_a (a itself when none is earlier), -1 for an a that is not included; d_common
 *      [S,B,B] int32 (may be NULL): c of every pair of the frame, whatever d_include says; with Q > 0 query fingerprints d_q_words
 *      [Q,32] (made elsewhere by td_fingerprint), d_query_common [S,B,Q] int32: popcount(fp_a & q).  (Additions: TD_ABI_VERSION
 *      stays 5.) */
int td_fingerprint(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                   const int32_t *class_atomic_number, int32_t K, const uint8_t *class_aromatic, int32_t radius, int32_t key_rounds,
                   int64_t *d_fp_words, int32_t *d_n_bits, int64_t *d_key, int64_t *d_atom_key, void *stream);
int td_fingerprint_similarity(const int64_t *d_fp_words, const int32_t *d_n_bits, const int64_t *d_key, int64_t S, int64_t B,
                              const uint8_t *d_include, const int64_t *d_q_words, int64_t Q, double *d_sim_sum, double *d_sim_max,
                              int32_t *d_first_equal, int32_t *d_common, int32_t *d_query_common, void *stream);

/* ---- local geometry of ligand frames ("Local geometry"): per (frame, molecule), on the bond graph exactly as
 *      td_bond_graph defines it (the same pack, class table, aromatic flags and d_include bytes; an atom whose class is outside
 *      [0, K) bonds with nothing and takes part nowhere).  Coordinates are the fp32 inputs widened to float64; every product, sum and
 *      difference is rounded on its own, division and square root are IEEE.  Degree of an atom: the number of its bonds; an atom of
 *      degree > 8 (TD_GEOM_MAX_DEGREE) is crowded: it is the centre of no angle, a bond with a crowded end is central to no torsion,
 *      and a crowded atom may still be an end atom.
 *      Bond angle (i, j, k), j the centre, i < k both bonded to j: u = p_i - p_j, w = p_k - p_j, uu = (u_x u_x + u_y u_y) + u_z u_z, ww
 *      and uw likewise; degenerate when uu ww == 0, else c = uw / sqrt(uu ww).  Torsion (i, j, k, l): the central bond j < k, i bonded
 *      to j with i != k, l bonded to k with l != j and l != i (no three-rings), each such quadruple once: b1 = p_j - p_i, b2 = p_k -
 *      p_j, b3 = p_l - p_k, n1 = b1 x b2, n2 = b2 x b3 with every component formed as (a b) - (c d); degenerate when (n1.n1)(n2.n2)
 *      == 0, else c = (n1.n2) / sqrt((n1.n1)(n2.n2)): the cosine of the unsigned torsion 0 .. 180 degrees (mirror images alike).  No
 *      acos or atan2 runs on the device: angles are binned by their cosine.  Profile p (HOST array, P <= 16): kind 1 = angle, 2 =
 *      torsion; z[4] atomic numbers (0: any) -- an angle matches with z[1] the centre and z[0], z[2] the ends in either order (z[3]
 *      must be 0), a torsion with its four elements as given or reversed; category (0: any, else the central bond's category as
 *      td_bond_list gives it, 1 .. 4) and ring (0: any, 1: the central bond is in no ring, 2: it is in one) filter torsions and must be
 *      0 for an angle; the value enters bin numpy.searchsorted(edges, c, 'left') of d_edges [n_edges] (DEVICE float64 cosines,
 *      ascending, 1 <= n_edges <= 127).  The ring filter reads d_bond_ring [n_bonds] of td_ring_report at the offsets d_bond_ptr
 *      [S*B+1] of td_bond_graph on the same pack (both may be NULL otherwise; TD_EINVAL when a profile asks for the filter without
 *      them; an offset outside [0, n_bonds) matches neither 1 nor 2 and nothing out of bounds is read).
 *      Internal clash: a pair i < j of one molecule, both with a class, more than 3 bonds apart in the graph (pairs in different
 *      fragments included), with d < clash_threshold[e_i * 8 + e_j]; d is the distance of the bond rule, bit for bit, e the element
 *      index over H C N O F P S Cl; clash_threshold is a HOST float64 [64] table, NULL: no clash pass (d_n_clashes and d_atom_clash
 *      are then not written and may be NULL).
 *      Output: d_n_angles, d_n_torsions [S,B] int32, every non-degenerate angle / torsion whatever the profiles; d_n_degenerate [S,B]
 *      the degenerate angles and torsions, which are counted nowhere else; d_n_crowded [S,B] the crowded atoms; d_n_clashes [S,B];
 *      d_atom_clash [S,N_l] int32 (may be NULL), the clashes an atom takes part in; d_hist [S,P,128] int64, zeroed by the call, over
 *      the molecules whose d_include byte is non-zero (NULL: all).  A molecule of more than 512 atoms, or one whose offsets leave
 *      [0, N_l], gets -1 in the five per-molecule outputs and contributes nothing else (a binding refuses it).  All outputs are
 *      integers: they do not depend on the grid or on the order of arrival.  (An addition: TD_ABI_VERSION stays 5.) */
typedef struct td_geometry_profile {
    int32_t kind;
    int32_t z[4];
    int32_t category, ring, n_edges;
    const double *d_edges;
} td_geometry_profile;
int td_geometry_report(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                       const int32_t *class_atomic_number, int32_t K, const uint8_t *d_include, const uint8_t *class_aromatic,
                       const td_geometry_profile *profiles, int32_t P, const int64_t *d_bond_ptr, int64_t n_bonds,
                       const uint16_t *d_bond_ring, const double *clash_threshold, int32_t *d_n_angles, int32_t *d_n_torsions,
                       int32_t *d_n_degenerate, int32_t *d_n_crowded, int32_t *d_n_clashes, int32_t *d_atom_clash, int64_t *d_hist,
                       void *stream);

/* ---- pocket contacts of ligand frames ("Pocket contacts"): one pocket and one pack per call; every molecule of
 *      the pack is in that pocket.  The pack, the class table and d_include as td_geometry_report takes them.  d_protein_pos [N_p,3]
 *      fp32 in the frame of d_pos; d_protein_elem [N_p] int32, an index over H C N O S Se, or -1; d_protein_kind [N_p] int32 in
 *      [0, n_kinds) or -1, 1 <= n_kinds <= 64.  A protein atom whose element or kind is outside its range takes part nowhere.
 *      Distance: the distance of the bond rule, bit for bit: fp32 inputs widened to float64, d = sqrt((dx dx + dy dy) + dz dz) with
 *      every product and sum rounded on its own and an IEEE square root.  Pair: a ligand atom with a class inside [0, K) and a protein
 *      atom that takes part.  Contact: a pair with d < contact_cutoff (a finite double > 0), strictly.  Clash: a pair with d <
 *      clash_threshold[e_l * 6 + e_p], strictly; clash_threshold is a HOST float64 [8 * 6] table, ligand element over H C N O F P S Cl
 *      by protein element; NULL: no clash pass (d_n_clashes, d_n_clash_atoms and d_atom_clash are then not written and may be NULL).
 *      d_ref_bits [W] uint64, W = ceil(N_p / 64), may be NULL: bit j & 63 of word j >> 6 marks protein atom j.
 *      Output per (frame, molecule), [S,B]: d_n_contacts int32, the contact pairs; d_n_contact_atoms, the ligand atoms with at least
 *      one contact; d_n_pocket_atoms, the protein atoms with at least one contact; d_n_clashes, the clash pairs; d_n_clash_atoms, the
 *      ligand atoms in at least one clash; d_min_dist float64, the smallest d over the molecule's pairs, +inf without pairs;
 *      d_n_ref_common, the contacted protein atoms that d_ref_bits marks (written only with d_ref_bits).  May be NULL: d_atom_contacts
 *      and d_atom_clash [S,N_l] int32, the pairs each ligand atom takes part in; d_bits [S,B,W] uint64, the contacted protein atoms
 *      in the layout of d_ref_bits.  Over the molecules whose d_include byte is non-zero (NULL: all), zeroed by the call:
 *      d_kind_hist [S,8,n_kinds] int64, the contact pairs by ligand element and protein kind; d_pocket_freq [S,N_p] int32, the number
 *      of such molecules of the frame that contact protein atom j.  A molecule of more than 512 atoms, or one whose offsets leave
 *      [0, N_l], gets -1 in the integer per-molecule outputs, +inf in d_min_dist and zero words in d_bits, its per-atom outputs are not
 *      written, and it contributes nothing else (a binding refuses it).  512 N_p and S N_p must fit 31 bits.  S, B and N_p may be 0.
 *      All outputs but d_min_dist are integers and d_min_dist is a minimum: nothing depends on the grid or on the order of arrival.
 *      (An addition: TD_ABI_VERSION stays 5.) */
int td_pocket_report(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                     const int32_t *class_atomic_number, int32_t K, const uint8_t *d_include, const float *d_protein_pos,
                     const int32_t *d_protein_elem, const int32_t *d_protein_kind, int64_t N_p, int32_t n_kinds, double contact_cutoff,
                     const double *clash_threshold, const uint64_t *d_ref_bits, int32_t *d_n_contacts, int32_t *d_n_contact_atoms,
                     int32_t *d_n_pocket_atoms, int32_t *d_n_clashes, int32_t *d_n_clash_atoms, double *d_min_dist,
                     int32_t *d_n_ref_common, int32_t *d_atom_contacts, int32_t *d_atom_clash, uint64_t *d_bits, int64_t *d_kind_hist,
                     int32_t *d_pocket_freq, void *stream);

/* ---- typed pocket interactions of ligand frames ("Pocket interactions"): hydrogen bonds and hydrophobic
 *      contacts, counted; no energy, no score, no float output.  The pack, the class table, d_include, d_protein_pos, d_protein_elem,
 *      d_protein_kind, N_p and n_kinds as td_pocket_report takes them, and the distance d is the same: the bond rule's, bit for bit.
 *      Role bits: DONOR = 1, ACCEPTOR = 2, HYDROPHOBIC = 4.  All comparisons are strict; the three cutoffs are finite doubles > 0.
 *      Protein roles: d_protein_role [N_p] int32, the donor / acceptor bits of the caller's table (bits above 2 are ignored) or a
 *      negative number.  A protein atom takes part when its element and kind are in range and its role is >= 0; any other takes part
 *      nowhere.  A carbon that takes part is HYDROPHOBIC when no N or O that takes part lies at d < hetero_cutoff.
 *      d_protein_role_out [N_p] int32: the role with that bit resolved, -1 for an atom that takes no part.
 *      Ligand roles, per frame and molecule on the bond graph of td_bond_graph (the same pack, class table and distance; orders 1 / 2 /
 *      3; an atom whose class is outside [0, K) bonds with nothing and has no role): val = the sum of the orders of the atom's bonds,
 *      n_h = its bonded H, hetero = its bonded N and O, h = n_h + max(0, V - val) with V = 3 for N and 2 for O.  DONOR: N or O with
 *      h >= 1.  ACCEPTOR: O; N with h = 0 and val <= 3.  HYDROPHOBIC: C with hetero = 0; F; Cl.  H, P, S: none.  The donors are a
 *      valence-deficit heuristic (the sampler places no hydrogens), not perceived chemistry.
 *      Interactions of a ligand atom that has a role with a protein atom that takes part: type 0, the ligand donates (DONOR to
 *      ACCEPTOR, d < hbond_cutoff); type 1, the ligand accepts (ACCEPTOR to DONOR, d < hbond_cutoff); type 2, hydrophobic (both
 *      HYDROPHOBIC, d < hydrophobic_cutoff).  A pair of type 0 and type 1 at once is one hydrogen bond.
 *      d_ref_bits [3,W] uint64, W = ceil(N_p / 64), may be NULL: per type, bit j & 63 of word j >> 6 marks protein atom j.
 *      Output per (frame, molecule), [S,B] int32: d_n_donated, d_n_accepted, d_n_hbonds, d_n_hydrophobic, the pairs of type 0, of
 *      type 1, of type 0 or 1, of type 2; d_n_hb_atoms, the ligand atoms in at least one hydrogen bond; d_n_donors, d_n_acceptors,
 *      d_n_hydrophobic_atoms, the ligand atoms that hold each role; d_n_ref_common [S,B,3], per type the protein atoms hit that
 *      d_ref_bits marks (written only with d_ref_bits).  May be NULL: d_atom_role [S,N_l] int32, the role bits; d_atom_hbonds and
 *      d_atom_hydrophobic [S,N_l] int32, the hydrogen bonds and the hydrophobic pairs each ligand atom takes part in; d_bits
 *      [S,B,3,W] uint64, the protein atoms hit per type in the layout of d_ref_bits.  Over the molecules whose d_include byte is
 *      non-zero (NULL: all), zeroed by the call: d_kind_hist [S,3,n_kinds] int64, the pairs by type and protein kind; d_pocket_freq
 *      [S,3,N_p] int32, the number of such molecules of the frame that hit protein atom j with that type.  A molecule of more than
 *      512 atoms, or one whose offsets leave [0, N_l], gets -1 in every per-molecule output and zero words in d_bits, its per-atom
 *      outputs are not written, and it contributes nothing else (a binding refuses it).  512 N_p and 3 S N_p must fit 31 bits.
 *      S, B and N_p may be 0.  Every output is an integer: nothing depends on the grid or on the order of arrival.
 *      (An addition: TD_ABI_VERSION stays 5.) */
int td_interaction_report(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                          const int32_t *class_atomic_number, int32_t K, const uint8_t *d_include, const float *d_protein_pos,
                          const int32_t *d_protein_elem, const int32_t *d_protein_kind, const int32_t *d_protein_role, int64_t N_p,
                          int32_t n_kinds, double hbond_cutoff, double hydrophobic_cutoff, double hetero_cutoff,
                          const uint64_t *d_ref_bits, int32_t *d_protein_role_out, int32_t *d_n_donated, int32_t *d_n_accepted,
                          int32_t *d_n_hbonds, int32_t *d_n_hydrophobic, int32_t *d_n_hb_atoms, int32_t *d_n_donors,
                          int32_t *d_n_acceptors, int32_t *d_n_hydrophobic_atoms, int32_t *d_n_ref_common, int32_t *d_atom_role,
                          int32_t *d_atom_hbonds, int32_t *d_atom_hydrophobic, uint64_t *d_bits, int64_t *d_kind_hist,
                          int32_t *d_pocket_freq, void *stream);

/* ---- docking-style score of ligand frames ("Docking-style score"): per molecule the five unweighted term sums
 *      of a Vina-style pair energy with one pocket, as integers, and the rotatable bonds.  No energy is formed here: the weights and
 *      the rotor normalisation are the caller's.  It is a score on this project's heuristic typing -- no hydrogens are placed, the
 *      roles come from valence deficits, there is no intramolecular term -- and NOT AutoDock Vina's number: comparable between runs of
 *      this library, not with published tables.  The pack, the class table, d_protein_pos, d_protein_elem, d_protein_kind,
 *      d_protein_role, N_p, n_kinds and hetero_cutoff as td_interaction_report takes them; there is no d_include (nothing is summed
 *      over molecules).  class_aromatic as td_bond_graph's, read by the rotor kernel's bond graph only.
 *      Who takes part: a ligand atom whose class is in [0, K) and whose element is not H; a protein atom that takes part in
 *      td_interaction_report (element and kind in range, role >= 0) and whose element is not H.  Roles: the ligand's and the
 *      protein's resolved roles of td_interaction_report, bit for bit; d_protein_role_out [N_p] int32 is written as there.
 *      Distance: r, the bond rule's float64 distance (td_pocket_report's d).  A pair counts when r < cutoff, strictly (finite, > 0;
 *      8.0 by convention).  Surface distance d = r - rsum[e_l * 6 + e_p], one rounding; rsum: HOST float64 [8 * 6], ligand element
 *      over H C N O F P S Cl by protein element over H C N O S Se, R_l + R_p formed by the caller, every entry in (0, 6] (else
 *      TD_EINVAL; the H entries are never read).
 *      Terms of a pair, float64 with every product, sum and difference rounded on its own (no FMA contraction):
 *        0 gauss1      exp(-(d 2)^2)                                             every pair
 *        1 gauss2      exp(-((d - 3) / 2)^2)                                     every pair
 *        2 repulsion   d d if d < 0, else 0                                      every pair
 *        3 hydrophobic 1 if d < 0.5; 1.5 - d if d < 1.5; else 0                  both atoms HYDROPHOBIC
 *        4 hbond       1 if d < -0.7; (-d) / 0.7 if d < 0; else 0                ligand DONOR with protein ACCEPTOR, or ligand
 *                                                                                ACCEPTOR with protein DONOR; once per pair
 *      Each value becomes llrint(ldexp(value, 24)) (nearest, ties to even) and is added as int64: d_terms [S,B,5] int64 in units of
 *      2^-24, exact whatever the order of arrival; d_n_pairs [S,B] int32, the pairs with r < cutoff.  Only exp can differ from a
 *      float64 restatement: terms 2, 3, 4 are exact, terms 0 and 1 differ by at most one unit per pair.  A value is at most 36, 512
 *      N_p must fit 31 bits, so a molecule's sum stays below 2^61.
 *      Rotatable bonds, d_n_rot [S,B] int32, on the bond graph of td_bond_graph (the same pack, class table and aromatic flags): a
 *      bond i < j whose order is 1, whose ring size is 0 -- d_bond_ring [n_bonds] of td_ring_report at the bond's index in
 *      td_bond_list's order, d_bond_ptr [S * B + 1] of td_bond_graph; an index outside [0, n_bonds) reads nothing and the bond counts
 *      as not rotatable -- and whose two ends each have at least two bonded heavy atoms (a class in the table, an element other than
 *      H; the other end counts).  Amide bonds and single bonds next to a triple bond are NOT excluded: a convention.  d_bond_ptr,
 *      n_bonds and d_bond_ring may all be NULL / 0: no rotor kernel runs and d_n_rot is not written; only some of them: TD_EINVAL
 *      (d_bond_ring may be NULL when n_bonds is 0).
 *      A molecule of more than 512 atoms, or one whose offsets leave [0, N_l], gets -1 in d_n_pairs and d_n_rot and INT64_MIN in its
 *      five terms, and contributes nothing else (a binding refuses it).  S, B and N_p may be 0; with N_p = 0 every term and
 *      d_n_pairs are 0.  Every output is an integer: two runs give identical bytes, and there is no floating-point atomic.
 *      (An addition: TD_ABI_VERSION stays 5.) */
int td_score_report(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                    const int32_t *class_atomic_number, int32_t K, const uint8_t *class_aromatic, const float *d_protein_pos,
                    const int32_t *d_protein_elem, const int32_t *d_protein_kind, const int32_t *d_protein_role, int64_t N_p,
                    int32_t n_kinds, double cutoff, double hetero_cutoff, const double *rsum, const int64_t *d_bond_ptr,
                    int64_t n_bonds, const uint16_t *d_bond_ring, int32_t *d_protein_role_out, int64_t *d_terms, int32_t *d_n_pairs,
                    int32_t *d_n_rot, void *stream);

/* ---- rigid-body relaxation of ligand frames under the docking-style score ("Pose relaxation"): per (frame,
 *      molecule) the pose after a local optimisation of inter = weights . terms, the five term sums of td_score_report, over rigid
 *      motions of the molecule.  It is a local optimisation under this project's heuristic score, NOT AutoDock Vina's `minimize`, and
 *      it is rigid-body only: three translations and three rotations, no torsions.  No global search, no intramolecular term, no
 *      hydrogens.  Inputs as td_score_report takes them (the rotor inputs too: d_n_rot is the INPUT pose's; the caller forms
 *      score = inter / (1 + w_rot n_rot)), plus weights: HOST float64 [5], finite; max_steps >= 0 accepted steps (64 by convention),
 *      max_evals >= 1 evaluations, max_shift finite and > 0 (3.0 by convention), else TD_EINVAL.
 *      Typing: the ligand roles are those of the INPUT pose and are held fixed.  Pairs, r, d and the term values as td_score_report,
 *      with the same rounding of each value to units of 2^-24.
 *      State: c0, the centroid of the scored atoms (class in [0, K), not H) in float64, summed in index order; x0 = x - c0 for ALL
 *      atoms of the molecule (hydrogens and atoms outside the table ride along); a unit quaternion q = (w, x, y, z) and a shift t, the
 *      centre being c = c0 + t.  A pose is fp32(R(q) x0 + c): row k as ((R_k0 x0 + R_k1 y0) + R_k2 z0) + c_k with R_00 =
 *      1 - 2 (yy + zz), R_01 = 2 (xy - wz), R_02 = 2 (xz + wy), R_10 = 2 (xy + wz), R_11 = 1 - 2 (xx + zz), R_12 = 2 (yz - wx),
 *      R_20 = 2 (xz - wy), R_21 = 2 (yz + wx), R_22 = 1 - 2 (xx + yy), every product and sum rounded on its own.  Energies and
 *      gradients are always taken at the fp32-rounded pose: the final terms are exactly the score of the coordinates written.
 *      Gradient: per counted pair f = dE/dd = (((w0 (-4 t e1) + w1 (-u e2)) + w2 [d < 0] 2 d) + w3 [0.5 <= d < 1.5] (-1)) +
 *      w4 [-0.7 <= d < 0] (-1 / 0.7), with t = 2 d, e1 = exp(-t t), u = (d - 3) / 2, e2 = exp(-u u) and the role conditions of terms
 *      3 and 4: zero on the flat pieces, at a breakpoint the piece that the term value takes, no derivative of the cutoff.
 *      g = f (x_l - x_p) / r; the six components are sum g and sum (x_l - c) x g; each component of each pair is rounded to units of
 *      2^-24 and added as int64, so the sums are exact whatever the order of arrival.  There is no floating-point atomic.
 *      Step: BFGS on the 6-vector with an Armijo backtracking line search (f1 - f0 < 1e-4 alpha g.p; alpha = 1, halved, at most 10
 *      trials); H0 is the identity on translation and 1 / mean |x0|^2 (over the scored atoms) on rotation; H is reset to H0 when -H g
 *      is no descent direction and updated only when s.y > 0.  The rotation increment of omega is the normalised quaternion
 *      (1, omega / 2), composed on the left and renormalised.  A trial with |t| > max_shift fails without an evaluation.  The kernel
 *      stops when a line search fails, after max_steps accepted steps or after max_evals evaluations.
 *      Outputs: d_pos_out [S,N_l,3] fp32 (may not be d_pos; an atom of no molecule and a molecule that took no step keep the input's
 *      bytes); d_terms_in / d_terms_out [S,B,5] int64, the term sums at the input and at the written pose; d_n_pairs_out [S,B] int32
 *      at the written pose; d_n_steps, d_n_evals [S,B] int32; d_status [S,B] int32: bit 1 a line search ended (converged), 2 out of
 *      steps or evaluations, 4 some trial hit max_shift; d_transform [S,B,7] float64: q, then t = c - c0; d_grad_in [S,B,6] int64:
 *      the gradient at the input pose in units of 2^-24.  d_protein_role_out and d_n_rot as td_score_report.
 *      A molecule of more than 512 atoms, or one whose offsets leave [0, N_l]: positions copied through, INT64_MIN in both terms,
 *      -1 in d_n_pairs_out and d_status (and d_n_rot), zero steps.  No scored atom, or N_p = 0: positions copied through, zero steps.
 *      max_steps = 0: one evaluation, d_terms_out == d_terms_in.  Two runs give identical bytes.  (An addition: TD_ABI_VERSION
 *      stays 5.) */
int td_score_minimize(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                      const int32_t *class_atomic_number, int32_t K, const uint8_t *class_aromatic, const float *d_protein_pos,
                      const int32_t *d_protein_elem, const int32_t *d_protein_kind, const int32_t *d_protein_role, int64_t N_p,
                      int32_t n_kinds, double cutoff, double hetero_cutoff, const double *rsum, const int64_t *d_bond_ptr,
                      int64_t n_bonds, const uint16_t *d_bond_ring, const double *weights, int32_t max_steps, int32_t max_evals,
                      double max_shift, int32_t *d_protein_role_out, int32_t *d_n_rot, float *d_pos_out, int64_t *d_terms_in,
                      int64_t *d_terms_out, int32_t *d_n_pairs_out, int32_t *d_n_steps, int32_t *d_n_evals, int32_t *d_status,
                      double *d_transform, int64_t *d_grad_in, void *stream);

/* ---- docking search of ligand frames under the docking-style score ("Docking search"): per (frame, molecule) the
 *      best pose that n_chains independent Monte-Carlo chains of n_rounds + 1 mutate-and-relax rounds find.  It is a rigid-body global
 *      search under this project's heuristic score, NOT AutoDock Vina's `dock`: three translations and three rotations, no torsions.
 *      No intramolecular term, no hydrogens; the search box is the ball of max_shift around the input centroid.  Inputs as
 *      td_score_minimize takes them (max_steps and max_evals are the budget of ONE round), plus n_chains in 1 .. 64, n_rounds in
 *      0 .. 256, amplitude and temperature finite and > 0 (2.0 Angstrom and 1.2 by convention), else TD_EINVAL, and d_draws
 *      [S,B,n_chains,n_rounds+1,7] float64 in [0, 1), the caller's uniforms: there is no random number generator on the device.
 *      Typing, state, pose, evaluation and the local optimisation (one "descent") are td_score_minimize's, from the same code.
 *      A chain keeps a current state (q, t), at first the identity.  Round r of chain c with u = d_draws[s, b, c, r, :]:
 *      Chain 0, round 0: no mutation; the descent starts at the input pose: exactly td_score_minimize.
 *      Every other (chain, round) mutates the current state first, every operation rounded on its own: s_k = 2 u_k - 1 (k < 6);
 *      t_k += amplitude s_k; h_k = 0.5 ((amplitude s_{3+k}) sqrt(hr)), hr = 1 / mean |x0|^2 over the scored atoms (1 without any);
 *      the increment d = (1, h) / sqrt(1 + ((hx hx + hy hy) + hz hz)) composed on the left, w = ((dw qw - dx qx) - dy qy) - dz qz,
 *      x = ((dw qx + dx qw) + dy qz) - dz qy, y = ((dw qy - dx qz) + dy qw) + dz qx, z = ((dw qz + dx qy) - dy qx) + dz qw, divided by
 *      sqrt(((ww + xx) + yy) + zz).  Then, where |t| = sqrt((tx tx + ty ty) + tz tz) > max_shift, t_k *= (max_shift / |t|)
 *      (1 - 2^-40), and status bit 4 is set.  No sin or cos runs on the device.  The descent starts there with a fresh H0.
 *      Metropolis on e = inter of the descent's end: a chain's first round is accepted; a later one when e < e_cur or
 *      u_6 < exp((e_cur - e) / temperature); an accepted round's end state becomes the current state.  The chain remembers the round
 *      with the lowest e (the first of equals): its state, terms, pairs and status.
 *      Selection, in a second launch: the chain with the lowest inter = (((w0 T0 + w1 T1) + w2 T2) + w3 T3) + w4 T4 of its integer
 *      terms; on a tie the lowest chain index.  Its pose is rebuilt from its transform as td_score_minimize builds a pose; the
 *      identity keeps the input's bytes.
 *      Outputs: those of td_score_minimize for the winning pose (d_status the winning round's; d_terms_in and d_grad_in of the input
 *      pose; d_n_steps and d_n_evals summed over the chains), plus d_best_chain [S,B] int32, d_chain_terms [S,B,n_chains,5] int64 and
 *      d_chain_transform [S,B,n_chains,7] float64 (each chain's best), d_chain_accepts and d_chain_evals [S,B,n_chains] int32.
 *      With n_chains = 1 and n_rounds = 0 every shared output is td_score_minimize's.  An oversize molecule, an empty one and N_p = 0
 *      answer as td_score_minimize does (INT64_MIN in d_chain_terms, identities in d_chain_transform for the first).  Every loop is
 *      bounded by (n_rounds + 1) max_evals; no floating-point atomic, no spin, no grid-wide synchronisation.  Two runs give identical
 *      bytes.  (An addition: TD_ABI_VERSION stays 5.) */
int td_score_dock(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                  const int32_t *class_atomic_number, int32_t K, const uint8_t *class_aromatic, const float *d_protein_pos,
                  const int32_t *d_protein_elem, const int32_t *d_protein_kind, const int32_t *d_protein_role, int64_t N_p,
                  int32_t n_kinds, double cutoff, double hetero_cutoff, const double *rsum, const int64_t *d_bond_ptr, int64_t n_bonds,
                  const uint16_t *d_bond_ring, const double *weights, int32_t max_steps, int32_t max_evals, double max_shift,
                  int32_t n_chains, int32_t n_rounds, double amplitude, double temperature, const double *d_draws,
                  int32_t *d_protein_role_out, int32_t *d_n_rot, float *d_pos_out, int64_t *d_terms_in, int64_t *d_terms_out,
                  int32_t *d_n_pairs_out, int32_t *d_n_steps, int32_t *d_n_evals, int32_t *d_status, double *d_transform,
                  int64_t *d_grad_in, int32_t *d_best_chain, int64_t *d_chain_terms, double *d_chain_transform,
                  int32_t *d_chain_accepts, int32_t *d_chain_evals, void *stream);

/* ---- solvent-accessible surface of ligand frames by Shrake-Rupley point counting ("Solvent-accessible
 *      surface"): every output is a count of sphere points; areas are formed by the caller.  One pocket and one pack per call; the
 *      pack, the class table and d_include as td_pocket_report takes them.  d_protein_pos [N_p,3] fp32; d_protein_elem [N_p] int32, an
 *      index over H C N O S Se, or -1: an atom outside 0 .. 5 takes part nowhere.  N_p may be 0 and the two pointers then NULL.  A
 *      ligand atom takes part when its class is in [0, K).  ligand_reach [8] over H C N O F P S Cl and protein_reach [6] over H C N O S
 *      Se: HOST float64, the expanded radius R = van der Waals radius + probe, each finite and > 0 (else TD_EINVAL).  d_dirs [P,3]
 *      DEVICE float64, unit directions, 1 <= P <= 256; they are not read on the host (a binding checks that they are finite and of
 *      unit length to 1e-6, and that no coordinate exceeds 1e5 in magnitude).
 *      Arithmetic: float64, every product, sum and difference rounded on its own, centres the fp32 inputs widened.  Test point k of an
 *      atom with centre c and reach R: x = c + R u_k, per coordinate one product and one add.  R2 = R R.  D2(x, c') = ((x0 - c'0)^2 +
 *      (x1 - c'1)^2) + (x2 - c'2)^2.  Atom j occludes the point iff D2(x, c_j) < R2_j, strictly.
 *      Free: a point of ligand atom i is exposed iff no other atom j != i of the same frame and molecule that takes part occludes it.
 *      Bound: it is free-exposed and no protein atom that takes part occludes it.  Apo: a point of a protein atom that takes part is
 *      exposed iff no other protein atom that takes part occludes it.  Buried pocket point: an apo-exposed point of protein atom j that
 *      some atom of the molecule that takes part occludes.
 *      Output per (frame, molecule): d_free and d_bound [S,B,8] int32, the exposed points by ligand element; d_pocket_buried [S,B,6]
 *      int32, the buried pocket points by protein element.  May be NULL: d_atom_free and d_atom_bound [S,N_l] int32, the exposed
 *      points of every ligand atom; d_bits [S,B,W] uint64, W = ceil(N_p / 64), the protein atoms with at least one point buried by
 *      the molecule, in td_pocket_report's bit layout.  Per pocket, whatever S and B: d_pocket_free [N_p] int32, the apo-exposed
 *      points, 0 for an atom that takes no part; d_pocket_mask [N_p,4] uint64, bit k & 63 of word k >> 6 set when point k is
 *      apo-exposed.  Per frame, zeroed by the call: d_pocket_buried_sum [S,N_p] int64, the buried points of protein atom j summed over
 *      the molecules whose d_include byte is non-zero (NULL: all).  A molecule of more than 512 atoms, or one whose offsets leave
 *      [0, N_l], gets -1 in d_free, d_bound and d_pocket_buried and zero words in d_bits, its per-atom outputs are not written, and it
 *      contributes nothing else (a binding refuses it).  512 N_p, S N_p and 8 S B must fit 31 bits.  S, B and N_p may be 0.  Every
 *      output is an integer: nothing depends on the grid or on the order of arrival, and there is no floating-point atomic.
 *      (An addition: TD_ABI_VERSION stays 5.) */
int td_sasa_report(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                   const int32_t *class_atomic_number, int32_t K, const uint8_t *d_include, const float *d_protein_pos,
                   const int32_t *d_protein_elem, int64_t N_p, const double *ligand_reach, const double *protein_reach,
                   const double *d_dirs, int32_t P, int32_t *d_free, int32_t *d_bound, int32_t *d_pocket_buried, int32_t *d_atom_free,
                   int32_t *d_atom_bound, uint64_t *d_bits, int32_t *d_pocket_free, uint64_t *d_pocket_mask,
                   int64_t *d_pocket_buried_sum, void *stream);

/* ---- standalone EGNN refine net (replaces: models/egnn.py EGNN / EnBaseLayer as get_refine_net('egnn', config) builds
 *      it, models/molopt_score_model.py:34-42: num_r_gaussian = 1, kNN rebuilt per layer, SiLU, no LayerNorm, hidden 128,
 *      4 edge types, k = 32).  `host_weights`: per layer, in this order and as PyTorch stores them: edge_mlp.net.0.{weight
 *      [128,261], bias}, edge_mlp.net.2.{weight, bias}, edge_inf.0.{weight [1,128], bias [1]}, x_mlp.0.{weight, bias},
 *      x_mlp.2.weight [1,128], node_mlp.net.0.{weight [128,256], bias}, node_mlp.net.2.{weight, bias}.
 *      td_egnn_forward = EGNN.forward(h, x, mask_ligand, batch, return_all) (models/egnn.py:121-133): d_all_h [L][N][128] /
 *      d_all_x [L][N][3] (optional) receive the state after every layer (all_h[1:], all_x[1:]). */
typedef struct td_egnn td_egnn;
size_t td_egnn_num_weights(int32_t num_layers);
int td_egnn_create(int32_t num_layers, int32_t hidden_dim, int32_t edge_feat_dim, int32_t knn, const float *host_weights,
                   size_t num_weights, td_egnn **out);
void td_egnn_destroy(td_egnn *m);
size_t td_egnn_workspace_bytes(int64_t N);
int td_egnn_forward(const td_egnn *m, const float *d_h, const float *d_x, const uint8_t *d_mask_ligand,
                    const int32_t *d_node_ptr, int64_t N, int64_t B, int32_t max_graph_nodes, float *d_out_h, float *d_out_x,
                    float *d_all_h, float *d_all_x, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- binding-affinity predictor (replaces: models/property_pred/prop_model.py PropPredNet.forward / PropPredNetEnc.forward with
 *      the EnEquiEncoder of prop_egnn.py, as utils/misc_prop.py get_model builds them; configs/prop/ (the .yml files)).  Built for hidden 256,
 *      64 Gaussians, ReLU, no LayerNorm, no coordinate update, edge_dim 0, any 1 <= knn <= 64 and any layer count.
 *      `host_weights`, as PyTorch stores them: protein_atom_emb.{weight [256,Fp], bias}, ligand_atom_emb.{weight [256,Fl+El], bias},
 *      encoder.distance_expansion.offset [64]; per layer edge_mlp.net.0.{weight [256,576], bias}, edge_mlp.net.2.{weight, bias},
 *      edge_inf.0.{weight [1,256], bias [1]}, node_mlp.net.0.{weight [256,512], bias}, node_mlp.net.2.{weight, bias};
 *      when enc_node_dim > 0 enc_node_layer.0.{weight [256,256+En], bias}, enc_node_layer.2.{weight, bias}; then
 *      out_block.0.{weight [256,256+Eg], bias}, out_block.2.{weight [O,256], bias [O]}.
 *      td_prop_forward: protein / ligand atoms un-composed, each sorted by complex (d_*_ptr [B+1] int32 prefix offsets); the
 *      composed order is the project's rule: per complex its protein atoms, then its ligand atoms, each in input order.
 *      d_enc_ligand [N_l,El] (needed when El > 0), d_enc_node [N,En] in composed order (optional: NULL skips enc_node_layer, as the
 *      reference does for enc_node_feature=None), d_enc_graph [B,Eg] (needed when Eg > 0).  d_output_kind [B] int64 (1 = Ki,
 *      2 = Kd, 3 = IC50) or NULL: d_out is [B,1] or [B,O].  Optional outputs (NULL = not wanted): d_h_layers [L][N][256] (h after
 *      every layer), d_final_h [N][256] (h after enc_node_layer), d_out_nbr [N][knn] (the graph: row i = its neighbours, ascending
 *      (d2, index), -1 padded).  No atomics: reruns are bit-identical. */
typedef struct td_prop td_prop;
typedef struct td_prop_config {
    int32_t hidden_dim, num_layers, knn, num_r_gaussian;
    float cutoff;                      /* GaussianSmearing stop; the offsets themselves come with the weights */
    int32_t protein_feat_dim, ligand_feat_dim;
    int32_t enc_ligand_dim, enc_node_dim, enc_graph_dim;
    int32_t output_dim;
} td_prop_config;
size_t td_prop_num_weights(const td_prop_config *cfg);
int td_prop_create(const td_prop_config *cfg, const float *host_weights, size_t num_weights, td_prop **out);
void td_prop_destroy(td_prop *m);
size_t td_prop_workspace_bytes(const td_prop *m, int64_t N_p, int64_t N_l, int64_t B);
int td_prop_forward(const td_prop *m, const float *d_protein_pos, const float *d_protein_feat, const int32_t *d_protein_ptr,
                    int64_t N_p, const float *d_ligand_pos, const float *d_ligand_feat, const int32_t *d_ligand_ptr, int64_t N_l,
                    int64_t B, const float *d_enc_ligand, const float *d_enc_node, const float *d_enc_graph,
                    const int64_t *d_output_kind, int32_t max_graph_nodes, float *d_out, float *d_h_layers, float *d_final_h,
                    int32_t *d_out_nbr, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- training the binding-affinity predictor (prop_model.py get_loss, then loss.backward()): gradients with respect to every
 *      parameter; positions and input features are constants.
 *      td_prop_train_workspace_bytes: one device buffer that holds td_prop_forward's workspace, the tape td_prop_backward reads
 *      (per layer the input h, mi and t = ReLU(node_mlp.net.0 pre-activation): 3 x 1 KB per node and layer) and the backward's
 *      scratch, which materialises per-edge tensors (a, dz2, dz1 [N*knn][256], rbf [N*knn][64], q [N*knn]): about 156 KB per node
 *      at knn 48.
 *      td_prop_forward_train: td_prop_forward's inputs (no optional outputs) plus that workspace; d_out equals td_prop_forward's bit
 *      for bit.  Fills *tape, a host-side record; the tape's data stay in the workspace until the next forward on it.
 *      td_prop_backward: d_grad_out shaped like d_out; overwrites d_grad_weights [td_prop_num_weights] in host_weights order (the
 *      distance_expansion.offset slot, a buffer, is written as zeros).  Refuses a tape recorded by another handle, at another
 *      (N_p, N_l, B), or before a later td_prop_set_weights.  No float atomics: reruns are bit-identical.
 *      td_prop_set_weights: d_weights [td_prop_num_weights] in host_weights order, on the device; re-packs on the device, ordered on
 *      `stream`.  The offsets are copied; the Gaussian coefficient stays the one td_prop_create derived from them. */
typedef struct td_prop_tape {
    const td_prop *model;
    uint64_t weights_version;
    int64_t N_p, N_l, B;
    int32_t has_output_kind, has_enc_node;
    void *d_workspace;
    size_t workspace_bytes;
} td_prop_tape;
size_t td_prop_train_workspace_bytes(const td_prop *m, int64_t N_p, int64_t N_l, int64_t B);
int td_prop_forward_train(const td_prop *m, const float *d_protein_pos, const float *d_protein_feat, const int32_t *d_protein_ptr,
                          int64_t N_p, const float *d_ligand_pos, const float *d_ligand_feat, const int32_t *d_ligand_ptr,
                          int64_t N_l, int64_t B, const float *d_enc_ligand, const float *d_enc_node, const float *d_enc_graph,
                          const int64_t *d_output_kind, int32_t max_graph_nodes, float *d_out, void *d_workspace,
                          size_t workspace_bytes, td_prop_tape *tape, void *stream);
int td_prop_backward(const td_prop *m, const td_prop_tape *tape, int64_t N_p, int64_t N_l, int64_t B, const float *d_grad_out,
                     float *d_grad_weights, size_t num_weights, void *stream);
int td_prop_set_weights(td_prop *m, const float *d_weights, size_t num_weights, void *stream);

/* ---- other consumers of the denoiser (scripts/likelihood_est_diffusion.py; ScorePosNet3D.forward(return_all=True)).
 * They need the 8th schedule array (alphas_cumprod of the position schedule) at td_model_create.
 *
 * td_perturb: the forward-process sample inside ScorePosNet3D.likelihood_estimation (models/molopt_score_model.py:577-588;
 *   q_v_sample :394-398): pos_t = sqrt(abar_t) pos_0 + sqrt(1 - abar_t) noise; v_t = argmax(gumbel(uniform) + log q(v_t|v_0)).
 * td_likelihood_terms: per-graph kl_pos, kl_v of the same function (:594-613 = q_pos_posterior :424-428, q_v_posterior
 *   :401-409, compute_pos_Lt :463-474, compute_v_Lt :476-483): posterior KL for t > 0, decoder NLL for t == 0, mean over
 *   the graph's ligand atoms.  kl_*: [B].
 * td_likelihood_prior: the time_step == T branch (:569-576 = kl_pos_prior :430-438, kl_v_prior :410-416).  v_index is
 *   what the reference feeds index_to_log_onehot there (it passes batch_ligand, :574).
 * td_embed_ligand / td_v_inference: ligand_atom_emb (+ node indicator, :317,334,338) and v_inference (:307-311) on
 *   free-standing rows -- the block-input entries of layer_pred_ligand_v (:360-367). */
int td_perturb(const td_model *m, const int32_t *d_t, const int32_t *d_ligand_ptr, int64_t N_l, int64_t B,
               const float *d_ligand_pos, const int64_t *d_ligand_v, const float *d_noise, const float *d_uniform,
               float *d_pos_t, int64_t *d_v_t, void *stream);
int td_likelihood_terms(const td_model *m, const int32_t *d_t, const int32_t *d_ligand_ptr, int64_t N_l, int64_t B,
                        const float *d_pos_0, const float *d_pos_t, const int64_t *d_v_0, const int64_t *d_v_t,
                        const float *d_pred_pos, const float *d_pred_v, float *d_kl_pos, float *d_kl_v, void *stream);
int td_likelihood_prior(const td_model *m, const int32_t *d_ligand_ptr, int64_t N_l, int64_t B, const float *d_pos_0,
                        const int64_t *d_v_index, float *d_kl_pos, float *d_kl_v, void *stream);
int td_embed_ligand(const td_model *m, const int64_t *d_ligand_v, int64_t N_l, float *d_h, void *stream);
int td_v_inference(const td_model *m, const float *d_h, int64_t n, float *d_logits, void *stream);

/* ---- diffusion loss and validation, forward only (replaces: the arithmetic of ScorePosNet3D.get_diffusion_loss after the network
 *      call, models/molopt_score_model.py:521-563, and get_auroc of scripts/train_diffusion.py:22-36).  No gradient is formed.
 *      td_diffusion_loss: a ragged pack of B graphs, one wave per graph.  d_t [B] int32 (clamped to [0, T - 1] as td_likelihood_terms
 *      does), d_ligand_ptr [B+1], d_pos_0 the centred x0, d_pos_t / d_v_t the perturbed state (td_perturb), d_noise the draw x_t was
 *      made from (may be NULL for model_mean_type 'C0', where it is not read), d_pred_pos [N_l,3] / d_pred_v [N_l,C] the network's
 *      outputs.  Per atom: d_pred_pos_noise [N_l,3] = pred_pos - pos_t (:522), d_v_recon [N_l,C] = softmax(pred_v) (:562).  Per
 *      graph: d_loss_pos_graph [B] = mean over the graph's atoms of sum_d (pred - target)^2 (:536-542; 'C0': pred_pos against
 *      pos_0, 'noise': pred_pos_noise against d_noise), d_loss_v_graph [B] = compute_v_Lt (:476-483): posterior KL for t > 0,
 *      decoder NLL at t == 0 -- bit for bit td_likelihood_terms' d_kl_v of the same inputs (one body serves both kernels: the
 *      macro TD_TYPE_TERM of csrc/td_type_term.h, a macro so that td_likelihood_terms' own compiled code did not change).  An
 *      empty graph counts as one atom in the mean and gives 0.  d_scalars [3] = mean_g loss_pos_graph, mean_g loss_v_graph,
 *      loss_pos + loss_v_weight * loss_v (product and sum rounded one by one, :552), taken by a second stage of one workgroup in
 *      a fixed order over g: no float atomics, nothing depends on the grid or on the order of arrival.  B == 0: the scalars are
 *      NaN (the mean of nothing).  TD_EINVAL: more than TD_MAXC = 16 classes, d_noise NULL with model_mean_type 'noise', a model
 *      created without alphas_cumprod (8 or 10 schedule arrays, what td_perturb needs), negative sizes.
 *      td_auroc: d_scores [N,C] fp32, d_labels [N] int64, no model handle.  Per class c: d_n_pos[c] = #{i: label_i = c} and
 *      d_pairs2[c] = 2 #{(i, j): label_i = c, label_j != c, s_ic > s_jc} + #{(i, j): ..., s_ic == s_jc}, both [C] int64, so that
 *      the one-vs-rest AUROC of class c is pairs2 / (2 n_pos (N - n_pos)).  fp32 values are compared as they are (a NaN compares
 *      false both ways: a binding refuses it); a label outside [0, C) is in no class (a binding refuses it too).  Integer sums:
 *      exact and independent of the order.  TD_EINVAL for N < 0, N > 2^20 (pairs2 stays below 2^41), C < 1 or C > 16.
 *      (Additions: TD_ABI_VERSION stays 5.) */
int td_diffusion_loss(const td_model *m, const int32_t *d_t, const int32_t *d_ligand_ptr, int64_t N_l, int64_t B,
                      const float *d_pos_0, const float *d_pos_t, const float *d_noise, const int64_t *d_v_0, const int64_t *d_v_t,
                      const float *d_pred_pos, const float *d_pred_v, float loss_v_weight, float *d_pred_pos_noise,
                      float *d_v_recon, float *d_loss_pos_graph, float *d_loss_v_graph, float *d_scalars, void *stream);
int td_auroc(const float *d_scores, const int64_t *d_labels, int64_t N, int32_t C, int64_t *d_n_pos, int64_t *d_pairs2,
             void *stream);

/* ---- centring (replaces: center_pos(mode='protein'), models/molopt_score_model.py:110-120).
 *      offset [B,3] = per-graph protein centroid; positions are shifted in place by -offset (sign = -1)
 *      or +offset (sign = +1, models/molopt_score_model.py:691,695).  d_protein_pos may be NULL to
 *      shift only the ligand with an offset computed earlier (compute_offset = 0). */
int td_center_pos(float *d_protein_pos, const int32_t *d_protein_ptr, float *d_ligand_pos,
                  const int32_t *d_ligand_ptr, int64_t B, float *d_offset, int32_t compute_offset,
                  int32_t sign, void *stream);

/* ---- sampling session (replaces the loop-invariant part of ScorePosNet3D.sample_diffusion,
 *      models/molopt_score_model.py:633-661: protein_pos / protein_v / batch_protein are the same tensors in every
 *      one of the ~1000 forward calls and protein coordinates never move, models/uni_transformer.py:206).
 *      td_session_create takes the CENTRED protein once and precomputes embeddings, protein-only sorted neighbour
 *      lists and -- for protein atoms whose 32-NN row no ligand atom enters -- the edge-gate row and the layer-0 x2h
 *      output.  td_session_forward = ScorePosNet3D.forward for the current ligand state; its results equal
 *      td_model_forward's (same kernels, same per-row arithmetic; neighbour rows bit-identical).  The session owns its
 *      device memory; one forward at a time per session.  The memory is stream-ordered (hipMallocAsync / hipFreeAsync): the
 *      stream of the session's latest call must still exist when td_session_destroy runs (if it does not, the free falls back
 *      to a device synchronisation + hipFree). */
typedef struct td_session td_session;
int td_session_create(const td_model *m, const float *d_protein_pos, const float *d_protein_v,
                      const int32_t *d_protein_ptr, int64_t N_p, const int32_t *d_ligand_ptr, int64_t N_l, int64_t B,
                      int32_t max_graph_nodes, void *stream, td_session **out);
void td_session_destroy(td_session *s);
int td_session_forward(td_session *s, const float *d_ligand_pos, const int64_t *d_ligand_v, float *d_pred_ligand_pos,
                       float *d_pred_ligand_v, float *d_final_ligand_h, const float *d_ligand_graph_bias, void *stream);
/* ---- one reverse-diffusion step as a single replayable unit (replaces the loop body of ScorePosNet3D.sample_diffusion,
 *      models/molopt_score_model.py:650-693: forward, posterior mean / variance + noise :673-679, categorical posterior +
 *      Gumbel-max draw :682-685, trajectory appends :687-693).  = td_session_forward on the current ligand state followed by
 *      td_posterior_step, with everything that differs from step to step held in DEVICE memory, so that the ~50 launches of a
 *      step form one hipGraph that is captured once (second call) and replayed:
 *        d_step[0]   index s of the step to run; incremented on the device when the step's last kernel finishes
 *                    (d_step[1] is scratch of that hand-over and must start as 0).  The caller zeroes both once.
 *        d_t_all     [num_steps][B] the time step of every graph at step s (:649, :652)
 *        d_ligand_pos / d_ligand_v   the CURRENT state x_t / v_t: read by the step, then overwritten with x_{t-1} / v_{t-1}
 *                    (pos_only, :681: the types are left alone)
 *        d_noise [N_l][3], d_uniform [N_l][C]   this step's draws (:677, :161), refilled by the caller before every call
 *        d_pos_traj [num_steps][N_l][3], d_v_traj [num_steps][N_l], d_v0_traj / d_vt_traj [num_steps][N_l][C] (or NULL):
 *                    slot s receives x_{t-1}, v_{t-1}, log v0 (:683) and the log posterior (:684)
 *      use_graph = 0 issues the launches one by one (also the behaviour while the kernel timers or the workgroup trace are
 *      armed, and after a failed capture): the same kernels with the same arguments either way, so the results are the same
 *      bits.  The captured graph belongs to the session and is re-captured if `io` changes.  td_session_step_graph reports
 *      whether the last td_session_step replayed a graph (1) or launched eagerly (0). */
typedef struct td_step_io {
    int32_t *d_step;
    const int32_t *d_t_all;
    int32_t num_steps;
    int32_t pos_only;
    float *d_ligand_pos;
    int64_t *d_ligand_v;
    const float *d_noise;
    const float *d_uniform;
    float *d_pos_traj;
    int64_t *d_v_traj;
    float *d_v0_traj;
    float *d_vt_traj;
    const float *d_ligand_graph_bias;   /* [B][128] or NULL: this step's time-embedding term (see td_model_forward) */
    const uint8_t *d_fixed_mask;        /* [N_l] or NULL: known atoms (td_posterior_step_fixed); with pos_only only their positions */
    const float *d_fixed_pos;           /* [N_l][3] centred known positions (read where the mask is set) */
    const int64_t *d_fixed_v;           /* [N_l] known types (read where the mask is set) */
} td_step_io;
int td_session_step(td_session *s, const td_step_io *io, int32_t use_graph, void *stream);
size_t td_step_io_size(void);           /* sizeof(td_step_io) of the library: lets a binding check its own layout */
int td_session_step_graph(const td_session *s);
/* ---- a time program on a session: d_prog_table [num_slots][TD_PROG_ROW] (device memory, kept alive by the caller), host_kinds
 *      [num_slots] (TD_PROG_DENOISE / TD_PROG_RENOISE, copied).  From then on call k (counted from this call on) of td_session_step
 *      runs slot k, which must also be the value of d_step[0]: a DENOISE slot is the step as before with row k of the table (the
 *      captured graph reads the row through d_step, so one graph serves every denoise slot); a RENOISE slot launches only the
 *      renoise kernel, eagerly -- never inside the captured graph, never the denoiser -- fills slot k of the trajectories
 *      (d_vt_traj: log q, d_v0_traj: the clamped log one-hot of the incoming type) and advances d_step[0] like any step; the
 *      captured graph stays valid across it.  io->num_steps must equal num_slots; d_t_all holds the denoiser's time per slot.
 *      The program is an argument of its own and not a field of td_step_io: that block's layout stays as it is.
 *      d_prog_table == NULL removes the program (today's behaviour).  Either way a captured graph is dropped. */
int td_session_set_program(td_session *s, const float *d_prog_table, const int32_t *host_kinds, int32_t num_slots);
/* ---- clash guidance on a session: d_sigma [N_p] contact radii of the session's protein atoms (device memory; read during this call,
 *      which packs them beside the centred protein the session holds and waits for that).  From then on every denoise step of
 *      td_session_step runs denoiser -> td_clash_shift of the predicted x0 -> td_posterior_step_guided as one replayable unit;
 *      renoise slots of a program are not guided.  d_sigma == NULL removes guidance (today's step).  Either way a captured graph is
 *      dropped.  TD_EINVAL for w < 0 or max_shift < 0. */
int td_session_set_guidance(td_session *s, const float *d_sigma, float w, float max_shift);
/* rows processed by the last td_session_forward: counts[0] = N, counts[1] = rows recomputed at layer 0 (ligand +
 * displaced protein rows), counts[2 + k] = size of receptive-field level k + 1 of the ligand outputs (level 1 = ligand
 * atoms + their neighbours, level k + 1 = level k + its neighbours; the layer e from the end updates level e + 1 only),
 * -1 for levels the session does not track (k < 4); counts[6] = rows of layer 1 inside the ligand's one-hop forward reach
 * (the others keep the protein-only graph's cached layer-1 output), -1 when off; counts[7] = rows of the session's static tables and
 * counts[8] = distinct protein blocks of the batch when the tables are shared per pocket ("session_share_pockets"), -1 otherwise; synchronises */
int td_session_row_counts(td_session *s, int32_t *host_counts, int32_t n_counts, void *stream);

/* ---- kernel timers (measurement only; process-global: one set of timers for all models and streams of the process.  Launches from
 *      several host threads may record concurrently -- every start / stop pair enters the lists under a lock -- but begin / end
 *      themselves are meant for one controlling thread).  td_profile_begin arms HIP-event
 *      timers around the kernel classes selected by `class_mask` (bit c = class c) on the launch stream;
 *      td_profile_end synchronises the device and returns per-class summed milliseconds and launch counts.
 *      Classes: 0 knn, 1 edge gate, 2 node projections, 3 x2h key pass, 4 x2h value pass, 5 h2x key pass,
 *      6 h2x value pass, 7 compose, 8 head, 9 posterior. */
#define TD_PROFILE_CLASSES 10
int td_profile_begin(uint32_t class_mask);
int td_profile_end(float *ms_out, int32_t *count_out, int32_t num_classes);

/* ---- test hook (not a reference seam): node-side GEMMs of one attention stage of layer `layer`
 *      (stage 0 = x2h: hk/hv/hq, stage 1 = h2x: xk/xv/xq).  d_P [N,512] = [k_i | k_j | v_i | v_j] node
 *      projections of the 340-wide first Linear (h_i part incl. bias) in the form the kernels consume them -- each block centred
 *      over its 128 hidden units and multiplied by the sign of the MLP's LayerNorm weight (the LayerNorm is folded into the two
 *      Linears at pack time) --, d_q [N,128] = MLP_q(h). */
int td_debug_node_stage(const td_model *m, int32_t layer, int32_t stage, const float *d_h, int64_t N, float *d_P,
                        float *d_q, void *stream);

/* ---- test hook: one wave evaluates the cross-lane reduction helpers on 64 inputs; out[6][64] =
 *      {sum over groups of 8, sum over half-waves, sum over the wave, lo+hi half sum, lo/hi half max, other half}. */
int td_debug_reductions(const float *d_in64, float *d_out6x64, void *stream);

/* ---- test hook (fault injection): the nth stream-ordered device allocation the library makes from now on fails with
 *      TD_ENOMEM (0 = off).  Used to check that no entry point leaks the blocks it took before the failing one. */
int td_debug_fail_alloc(int32_t nth);

/* ---- profiling hook: wall clock of every workgroup of the x2h key / x2h value / fused h2x launches.  d_buf [slots][3 passes]
 *      [256 workgroups][8] uint64 in s_memrealtime ticks (the 100 MHz reference clock: comparable across CUs): 0 = the row loop
 *      starts (tables staged), 1 = end, 2 = end of the workgroup's first finished wave, 3 = sum of its waves' ends, 4 = kernel entry;
 *      launch n of a pass writes slot n % slots (pass 0 = key, 1 = value, 2 = h2x).  The caller fills entries 2 with all-ones and
 *      the rest with zero before the step (atomic min / add).  d_buf == NULL switches it off (the default; one scalar test per
 *      kernel). */
int td_debug_wg_trace(uint64_t *d_buf, int32_t slots);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* TARGETDIFF_HIP_H */
