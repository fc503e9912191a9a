// C ABI of libtargetdiff_hip.so: the binding-affinity predictor (models/property_pred/prop_model.py PropPredNet / PropPredNetEnc).
// See include/targetdiff_hip.h for the contract and prop.hip for the kernels.
#include <cmath>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "td_device.h"
#include "td_internal.h"
#include "td_api.h"

using namespace tdapi;

struct td_prop {
    td_prop_config cfg;
    float *blob;
    std::vector<TdPropLayer> layers;
    const float *pW, *pb, *lW, *lb;             // protein_atom_emb, ligand_atom_emb (row-major)
    const float *e1W, *e1b, *e2W, *e2b;         // enc_node_layer.0 / .2 (enc_node_dim > 0)
    const float *o1W, *o1b, *o2W, *o2b;         // out_block.0 / .2
    float coeff;                                // GaussianSmearing coeff, models/common.py:18
    float *bwd;                                 // what only the backward reads: per layer edge_mlp.net.2 transposed, A fragments
    std::vector<const float *> W2Tf;
    uint64_t weights_version;                   // bumped by td_prop_set_weights; a tape records it
};

namespace {
constexpr int H = TD_PROP_H, G = TD_PROP_G;

bool prop_config_ok(const td_prop_config &c) {
    return c.hidden_dim == H && c.num_layers >= 1 && c.knn >= 1 && c.knn <= TD_MAX_FANIN && c.num_r_gaussian == G &&
           c.protein_feat_dim >= 1 && c.ligand_feat_dim >= 1 && c.enc_ligand_dim >= 0 && c.enc_node_dim >= 0 && c.enc_graph_dim >= 0 &&
           c.output_dim >= 1;
}

size_t layer_floats() { return (size_t)H * (G + 2 * H) + H + (size_t)H * H + H + H + 1 + (size_t)H * 2 * H + H + (size_t)H * H + H; }

// W [rows][ld] row-major, columns col0 .. col0 + 16 kb_count - 1 -> 16x16x4 A fragments [ot][kb][lane] x 4 r
size_t pack_A_frag(Packer &pk, const float *W, int ld, int col0, int kb_count) {
    size_t off = pk.alloc((size_t)(H / 16) * kb_count * 64 * 4);
    float *d = pk.data.data() + off;
    for (int ot = 0; ot < H / 16; ++ot)
        for (int kb = 0; kb < kb_count; ++kb)
            for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 4; ++r)
                    d[(((size_t)ot * kb_count + kb) * 64 + lane) * 4 + r] =
                        W[(size_t)(16 * ot + (lane & 15)) * ld + col0 + 16 * kb + 4 * (lane >> 4) + r];
    return off;
}

size_t pack_copy(Packer &pk, const float *src, size_t n) {
    size_t off = pk.alloc(n);
    memcpy(pk.data.data() + off, src, n * sizeof(float));
    return off;
}

struct PropWs { float *hp, *hl, *h, *x, *P, *mi, *t, *pre, *y1, *y; int32_t *node_ptr, *nbr; size_t bytes; };
PropWs prop_carve(const td_prop_config &c, char *base, int64_t Np, int64_t Nl, int64_t B) {
    PropWs w;
    size_t off = 0;
    auto take = [&](size_t n) { char *p = base ? base + off : nullptr; off += align_up(n ? n : 1); return p; };
    const size_t N = (size_t)(Np + Nl), b = (size_t)B;
    w.hp = reinterpret_cast<float *>(take((size_t)Np * H * 4));
    w.hl = reinterpret_cast<float *>(take((size_t)Nl * H * 4));
    w.h = reinterpret_cast<float *>(take(N * H * 4));
    w.x = reinterpret_cast<float *>(take(N * 3 * 4));
    w.P = reinterpret_cast<float *>(take(N * 2 * H * 4));
    w.mi = reinterpret_cast<float *>(take(N * H * 4));
    w.t = reinterpret_cast<float *>(take(N * H * 4));
    w.pre = reinterpret_cast<float *>(take(b * (H + c.enc_graph_dim) * 4));
    w.y1 = reinterpret_cast<float *>(take(b * H * 4));
    w.y = reinterpret_cast<float *>(take(b * c.output_dim * 4));
    w.node_ptr = reinterpret_cast<int32_t *>(take((b + 1) * 4));
    w.nbr = reinterpret_cast<int32_t *>(take(N * c.knn * 4));
    w.bytes = off;
    return w;
}
}  // namespace

extern "C" size_t td_prop_num_weights(const td_prop_config *c) {
    if (!c || !prop_config_ok(*c)) return 0;
    size_t n = (size_t)H * c->protein_feat_dim + H + (size_t)H * (c->ligand_feat_dim + c->enc_ligand_dim) + H + G;
    n += (size_t)c->num_layers * layer_floats();
    if (c->enc_node_dim > 0) n += (size_t)H * (H + c->enc_node_dim) + H + (size_t)H * H + H;
    n += (size_t)H * (H + c->enc_graph_dim) + H + (size_t)c->output_dim * H + c->output_dim;
    return n;
}

extern "C" int td_prop_create(const td_prop_config *c, const float *host_weights, size_t num_weights, td_prop **out) {
    if (!c || !host_weights || !out) { td_set_error("td_prop_create: bad argument"); return TD_EINVAL; }
    if (!prop_config_ok(*c)) {
        td_set_error("td_prop_create: unsupported configuration (need hidden 256, num_r_gaussian 64, 1 <= knn <= %d, num_layers >= 1, "
                     "feature widths >= 1, enc_* widths >= 0, output_dim >= 1; got hidden %d, gaussians %d, knn %d, layers %d, "
                     "protein %d, ligand %d, enc %d/%d/%d, output %d)", TD_MAX_FANIN, c->hidden_dim, c->num_r_gaussian, c->knn,
                     c->num_layers, c->protein_feat_dim, c->ligand_feat_dim, c->enc_ligand_dim, c->enc_node_dim, c->enc_graph_dim,
                     c->output_dim);
        return TD_EINVAL;
    }
    if (num_weights != td_prop_num_weights(c)) {
        td_set_error("td_prop_create: weight blob has %zu floats, expected %zu", num_weights, td_prop_num_weights(c));
        return TD_EINVAL;
    }
    const int Fl = c->ligand_feat_dim + c->enc_ligand_dim;
    Cursor cur{host_weights, num_weights};
    Packer pk;
    const float *pW = cur.take((size_t)H * c->protein_feat_dim), *pb = cur.take(H);
    const float *lW = cur.take((size_t)H * Fl), *lb = cur.take(H);
    const float *offset = cur.take(G);
    struct Off { size_t projW, projB, W1f, W2f, b2, winf, binf, offset, n1W, n1b, n2W, n2b; };
    std::vector<Off> lo((size_t)c->num_layers);
    Packer pkb;                                 // td_prop::bwd
    std::vector<size_t> o_w2t((size_t)c->num_layers);
    std::vector<float> w2t((size_t)H * H);
    size_t o_pW = pack_copy(pk, pW, (size_t)H * c->protein_feat_dim), o_pb = pack_copy(pk, pb, H);
    size_t o_lW = pack_copy(pk, lW, (size_t)H * Fl), o_lb = pack_copy(pk, lb, H);
    size_t o_off = pack_copy(pk, offset, G);
    const int E = G + 2 * H;                    // edge_mlp.net.0 input: [rbf 64 | h_i 256 | h_j 256]   (prop_egnn.py:33)
    for (int l = 0; l < c->num_layers; ++l) {
        const float *W1 = cur.take((size_t)H * E), *b1 = cur.take(H);
        const float *W2 = cur.take((size_t)H * H), *b2 = cur.take(H);
        const float *winf = cur.take(H), *binf = cur.take(1);
        const float *n1W = cur.take((size_t)H * 2 * H), *n1b = cur.take(H);
        const float *n2W = cur.take((size_t)H * H), *n2b = cur.take(H);
        if (!cur.ok) break;
        Off &o = lo[(size_t)l];
        o.projW = pk.alloc((size_t)2 * H * H);
        o.projB = pk.alloc((size_t)2 * H);
        for (int r = 0; r < H; ++r)
            for (int k = 0; k < H; ++k) {
                pk.data[o.projW + (size_t)r * H + k] = W1[(size_t)r * E + G + k];
                pk.data[o.projW + (size_t)(H + r) * H + k] = W1[(size_t)r * E + G + H + k];
            }
        memcpy(pk.data.data() + o.projB, b1, H * sizeof(float));
        o.W1f = pack_A_frag(pk, W1, E, 0, G / 16);
        o.W2f = pack_A_frag(pk, W2, H, 0, H / 16);
        for (int r = 0; r < H; ++r)
            for (int k = 0; k < H; ++k) w2t[(size_t)r * H + k] = W2[(size_t)k * H + r];
        o_w2t[(size_t)l] = pack_A_frag(pkb, w2t.data(), H, 0, H / 16);
        o.b2 = pack_copy(pk, b2, H);
        o.winf = pack_copy(pk, winf, H);
        o.binf = pack_copy(pk, binf, 1);
        o.offset = o_off;
        o.n1W = pack_copy(pk, n1W, (size_t)H * 2 * H);
        o.n1b = pack_copy(pk, n1b, H);
        o.n2W = pack_copy(pk, n2W, (size_t)H * H);
        o.n2b = pack_copy(pk, n2b, H);
    }
    size_t o_e1W = 0, o_e1b = 0, o_e2W = 0, o_e2b = 0;
    if (c->enc_node_dim > 0) {
        const float *e1W = cur.take((size_t)H * (H + c->enc_node_dim)), *e1b = cur.take(H);
        const float *e2W = cur.take((size_t)H * H), *e2b = cur.take(H);
        if (cur.ok) {
            o_e1W = pack_copy(pk, e1W, (size_t)H * (H + c->enc_node_dim)); o_e1b = pack_copy(pk, e1b, H);
            o_e2W = pack_copy(pk, e2W, (size_t)H * H); o_e2b = pack_copy(pk, e2b, H);
        }
    }
    const float *o1W = cur.take((size_t)H * (H + c->enc_graph_dim)), *o1b = cur.take(H);
    const float *o2W = cur.take((size_t)c->output_dim * H), *o2b = cur.take(c->output_dim);
    if (!cur.ok || cur.left != 0) { td_set_error("td_prop_create: weight blob layout mismatch"); return TD_EINVAL; }
    size_t o_o1W = pack_copy(pk, o1W, (size_t)H * (H + c->enc_graph_dim)), o_o1b = pack_copy(pk, o1b, H);
    size_t o_o2W = pack_copy(pk, o2W, (size_t)c->output_dim * H), o_o2b = pack_copy(pk, o2b, c->output_dim);

    td_prop *m = new (std::nothrow) td_prop();
    if (!m) { td_set_error("td_prop_create: out of host memory"); return TD_ENOMEM; }
    m->cfg = *c;
    m->blob = nullptr;
    m->bwd = nullptr;
    m->weights_version = 0;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&m->blob), pk.data.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(m->blob, pk.data.data(), pk.data.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&m->bwd), pkb.data.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(m->bwd, pkb.data.data(), pkb.data.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        td_set_error("td_prop_create: device upload failed: %s", hipGetErrorString(e));
        if (m->blob) (void)hipFree(m->blob);
        if (m->bwd) (void)hipFree(m->bwd);
        delete m;
        return TD_EHIP;
    }
    for (int l = 0; l < c->num_layers; ++l) m->W2Tf.push_back(m->bwd + o_w2t[(size_t)l]);
    const float *D = m->blob;
    m->pW = D + o_pW; m->pb = D + o_pb; m->lW = D + o_lW; m->lb = D + o_lb;
    m->e1W = D + o_e1W; m->e1b = D + o_e1b; m->e2W = D + o_e2W; m->e2b = D + o_e2b;
    m->o1W = D + o_o1W; m->o1b = D + o_o1b; m->o2W = D + o_o2W; m->o2b = D + o_o2b;
    m->layers.resize((size_t)c->num_layers);
    for (int l = 0; l < c->num_layers; ++l) {
        const Off &o = lo[(size_t)l];
        m->layers[(size_t)l] = TdPropLayer{D + o.projW, D + o.projB, D + o.W1f, D + o.W2f, D + o.b2, D + o.winf, D + o.binf,
                                           D + o.offset, D + o.n1W, D + o.n1b, D + o.n2W, D + o.n2b};
    }
    const double step = (double)offset[1] - (double)offset[0];      // -0.5 / (offset[1] - offset[0]).item() ** 2, in double
    m->coeff = (float)(-0.5 / (step * step));
    *out = m;
    return TD_OK;
}

extern "C" void td_prop_destroy(td_prop *m) {
    if (!m) return;
    if (m->blob) (void)hipFree(m->blob);
    if (m->bwd) (void)hipFree(m->bwd);
    delete m;
}

extern "C" size_t td_prop_workspace_bytes(const td_prop *m, int64_t N_p, int64_t N_l, int64_t B) {
    if (!m || N_p < 0 || N_l < 0 || B < 0) return 0;
    return prop_carve(m->cfg, nullptr, N_p, N_l, B).bytes;
}

extern "C" int td_prop_forward(const td_prop *m, const float *d_protein_pos, const float *d_protein_feat, const int32_t *d_protein_ptr,
                               int64_t N_p, const float *d_ligand_pos, const float *d_ligand_feat, const int32_t *d_ligand_ptr,
                               int64_t N_l, int64_t B, const float *d_enc_ligand, const float *d_enc_node, const float *d_enc_graph,
                               const int64_t *d_output_kind, int32_t max_graph_nodes, float *d_out, float *d_h_layers,
                               float *d_final_h, int32_t *d_out_nbr, void *d_workspace, size_t workspace_bytes, void *stream) {
    if (!m || N_p < 0 || N_l < 0 || B < 0) { td_set_error("td_prop_forward: bad argument"); return TD_EINVAL; }
    const td_prop_config &c = m->cfg;
    if (B == 0) return TD_OK;
    if (!d_protein_ptr || !d_ligand_ptr || !d_out || !d_workspace || (N_p > 0 && (!d_protein_pos || !d_protein_feat)) ||
        (N_l > 0 && (!d_ligand_pos || !d_ligand_feat))) {
        td_set_error("td_prop_forward: null pointer");
        return TD_EINVAL;
    }
    if (c.enc_ligand_dim > 0 && N_l > 0 && !d_enc_ligand) {
        td_set_error("td_prop_forward: enc_ligand_dim is %d but no enc_ligand_feature was given", c.enc_ligand_dim);
        return TD_EINVAL;
    }
    if (c.enc_graph_dim > 0 && !d_enc_graph) {
        td_set_error("td_prop_forward: enc_graph_dim is %d but no enc_graph_feature was given", c.enc_graph_dim);
        return TD_EINVAL;
    }
    if (d_enc_node && c.enc_node_dim == 0) {
        td_set_error("td_prop_forward: an enc_node_feature was given to a model with enc_node_dim 0");
        return TD_EINVAL;
    }
    PropWs w = prop_carve(c, static_cast<char *>(d_workspace), N_p, N_l, B);
    if (w.bytes > workspace_bytes) {
        td_set_error("td_prop_forward: workspace has %zu bytes, need %zu", workspace_bytes, w.bytes);
        return TD_ENOMEM;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t N = N_p + N_l;
    int rc;
    // ---- embeddings and compose (prop_model.py:124-139, models/common.py:140-153)
    if ((rc = td_launch_prop_linear(d_protein_feat, c.protein_feat_dim, nullptr, 0, m->pW, m->pb, nullptr, w.hp, N_p, H, TD_PROP_ACT_NONE, s)) != TD_OK) return rc;
    if ((rc = td_launch_prop_linear(d_ligand_feat, c.ligand_feat_dim, d_enc_ligand, c.enc_ligand_dim, m->lW, m->lb, nullptr, w.hl, N_l, H,
                                    TD_PROP_ACT_NONE, s)) != TD_OK) return rc;
    if ((rc = td_launch_prop_compose(w.hp, w.hl, d_protein_pos, d_ligand_pos, d_protein_ptr, d_ligand_ptr, w.h, w.x, w.node_ptr, B, s)) != TD_OK)
        return rc;
    // ---- graph: each node's knn nearest same-complex nodes (prop_egnn.py:76, flow='target_to_source': dst = the query row)
    int32_t *nbr = d_out_nbr ? d_out_nbr : w.nbr;
    if (N > 0 && (rc = td_knn(w.x, w.node_ptr, N, B, c.knn, max_graph_nodes, nbr, stream)) != TD_OK) return rc;
    // ---- encoder layers: h = h + EnBaseLayer(h)
    for (int l = 0; l < c.num_layers; ++l) {
        const TdPropLayer &L = m->layers[(size_t)l];
        if ((rc = td_launch_prop_linear(w.h, H, nullptr, 0, L.projW, L.projB, nullptr, w.P, N, 2 * H, TD_PROP_ACT_NONE, s)) != TD_OK) return rc;
        if ((rc = td_launch_prop_edge(L, w.x, nbr, c.knn, w.P, w.mi, N, m->coeff, s)) != TD_OK) return rc;
        if ((rc = td_launch_prop_linear(w.mi, H, w.h, H, L.n1W, L.n1b, nullptr, w.t, N, H, TD_PROP_ACT_RELU, s)) != TD_OK) return rc;
        if ((rc = td_launch_prop_linear(w.t, H, nullptr, 0, L.n2W, L.n2b, w.h, w.h, N, H, TD_PROP_ACT_NONE, s)) != TD_OK) return rc;
        if (d_h_layers) TD_CHECK_HIP(hipMemcpyAsync(d_h_layers + (size_t)l * N * H, w.h, (size_t)N * H * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    // ---- enc_node_layer on [h | enc_node_feature] (prop_model.py:147-149)
    if (d_enc_node) {
        if ((rc = td_launch_prop_linear(w.h, H, d_enc_node, c.enc_node_dim, m->e1W, m->e1b, nullptr, w.t, N, H, TD_PROP_ACT_RELU, s)) != TD_OK) return rc;
        if ((rc = td_launch_prop_linear(w.t, H, nullptr, 0, m->e2W, m->e2b, nullptr, w.h, N, H, TD_PROP_ACT_NONE, s)) != TD_OK) return rc;
    }
    if (d_final_h) TD_CHECK_HIP(hipMemcpyAsync(d_final_h, w.h, (size_t)N * H * sizeof(float), hipMemcpyDeviceToDevice, s));
    // ---- readout: scatter_sum per complex, [| enc_graph_feature], out_block, output_kind (prop_model.py:152-160)
    if ((rc = td_launch_prop_segment_sum(w.h, w.node_ptr, d_enc_graph, c.enc_graph_dim, w.pre, B, s)) != TD_OK) return rc;
    if ((rc = td_launch_prop_linear(w.pre, H + c.enc_graph_dim, nullptr, 0, m->o1W, m->o1b, nullptr, w.y1, B, H, TD_PROP_ACT_SSP, s)) != TD_OK) return rc;
    float *y = d_output_kind ? w.y : d_out;
    if ((rc = td_launch_prop_linear(w.y1, H, nullptr, 0, m->o2W, m->o2b, nullptr, y, B, c.output_dim, TD_PROP_ACT_NONE, s)) != TD_OK) return rc;
    if (d_output_kind) return td_launch_prop_select(w.y, d_output_kind, c.output_dim, d_out, B, s);
    return TD_OK;
}

// ================================================================================================ training (td_prop_forward_train,
// td_prop_backward, td_prop_set_weights; kernels in prop_bwd.hip)
namespace {
// offsets of every tensor in the flat weight order of td_prop_create (= the order of d_grad_weights)
struct PropFlatLayer { size_t W1, b1, W2, b2, winf, binf, n1W, n1b, n2W, n2b; };
struct PropFlat {
    size_t pW, pb, lW, lb, offset, e1W, e1b, e2W, e2b, o1W, o1b, o2W, o2b, total;
    std::vector<PropFlatLayer> layers;
};
PropFlat prop_flat(const td_prop_config &c) {
    PropFlat f;
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o += n; return r; };
    const int Fl = c.ligand_feat_dim + c.enc_ligand_dim;
    f.pW = take((size_t)H * c.protein_feat_dim); f.pb = take(H);
    f.lW = take((size_t)H * Fl); f.lb = take(H);
    f.offset = take(G);
    for (int l = 0; l < c.num_layers; ++l) {
        PropFlatLayer L;
        L.W1 = take((size_t)H * (G + 2 * H)); L.b1 = take(H);
        L.W2 = take((size_t)H * H); L.b2 = take(H);
        L.winf = take(H); L.binf = take(1);
        L.n1W = take((size_t)H * 2 * H); L.n1b = take(H);
        L.n2W = take((size_t)H * H); L.n2b = take(H);
        f.layers.push_back(L);
    }
    f.e1W = f.e1b = f.e2W = f.e2b = 0;
    if (c.enc_node_dim > 0) {
        f.e1W = take((size_t)H * (H + c.enc_node_dim)); f.e1b = take(H);
        f.e2W = take((size_t)H * H); f.e2b = take(H);
    }
    f.o1W = take((size_t)H * (H + c.enc_graph_dim)); f.o1b = take(H);
    f.o2W = take((size_t)c.output_dim * H); f.o2b = take(c.output_dim);
    f.total = o;
    return f;
}

// One device buffer: the forward's workspace, the tape and the backward's scratch.  Tape (node level only, per layer the input h,
// mi and t = ReLU(node_mlp.net.0 pre-activation)); per-edge tensors exist only inside the backward (a, dz2, dz1, rbf, q).
struct PropTrainWs {
    PropWs fw;
    float *hin, *mi, *t, *te, *zo1;                    // hin [L+1][N][256], mi / t [L][N][256], te [N][256], zo1 [B][256]
    int32_t *pptr, *lptr;                             // [B+1]
    float *pfeat, *lfeat, *elig, *enode;              // copies of the inputs the weight gradients need
    int64_t *kind;
    float *dy, *dy1, *dpre, *dh, *dh2, *dt, *dmi, *dhu, *S, *R, *DWP, *dhp, *dhl;
    float *Ae, *DZ2, *DZ1, *RBF, *Q, *part;
    int32_t *cnt, *rptr, *ridx;
    size_t bytes;
};
int prop_kmax(const td_prop_config &c) {
    int k = 2 * H;
    const int cand[] = {H + c.enc_node_dim, H + c.enc_graph_dim, c.protein_feat_dim, c.ligand_feat_dim + c.enc_ligand_dim};
    for (int v : cand) k = v > k ? v : k;
    return k;
}
PropTrainWs prop_train_carve(const td_prop_config &c, char *base, int64_t Np, int64_t Nl, int64_t B) {
    PropTrainWs w;
    w.fw = prop_carve(c, base, Np, Nl, B);
    size_t off = w.fw.bytes;
    auto take = [&](size_t n) { char *p = base ? base + off : nullptr; off += align_up(n ? n : 1); return p; };
    auto f = [&](size_t n) { return reinterpret_cast<float *>(take(n * 4)); };
    auto i32 = [&](size_t n) { return reinterpret_cast<int32_t *>(take(n * 4)); };
    const size_t N = (size_t)(Np + Nl), b = (size_t)B, L = (size_t)c.num_layers, E = N * (size_t)c.knn;
    w.hin = f((L + 1) * N * H); w.mi = f(L * N * H); w.t = f(L * N * H);
    w.te = f(c.enc_node_dim > 0 ? N * H : 0); w.zo1 = f(b * H);
    w.pptr = i32(b + 1); w.lptr = i32(b + 1);
    w.pfeat = f((size_t)Np * c.protein_feat_dim); w.lfeat = f((size_t)Nl * c.ligand_feat_dim);
    w.elig = f((size_t)Nl * c.enc_ligand_dim); w.enode = f(N * c.enc_node_dim);
    w.kind = reinterpret_cast<int64_t *>(take(b * 8));
    w.dy = f(b * c.output_dim); w.dy1 = f(b * H); w.dpre = f(b * H);
    w.dh = f(N * H); w.dh2 = f(N * H); w.dt = f(N * H); w.dmi = f(N * H); w.dhu = f(N * H);
    w.S = f(N * H); w.R = f(N * H); w.DWP = f(N * H);
    w.dhp = f((size_t)Np * H); w.dhl = f((size_t)Nl * H);
    w.Ae = f(E * H); w.DZ2 = f(E * H); w.DZ1 = f(E * H); w.RBF = f(E * G); w.Q = f(E);
    const size_t omax = c.output_dim > H ? (size_t)c.output_dim : (size_t)H;
    w.part = f((size_t)TD_PROP_XTY_CHUNKS * omax * prop_kmax(c));
    w.cnt = i32(N); w.rptr = i32(N + 1); w.ridx = i32(E ? E : 1);
    w.bytes = off;
    return w;
}
}  // namespace

extern "C" size_t td_prop_train_workspace_bytes(const td_prop *m, int64_t N_p, int64_t N_l, int64_t B) {
    if (!m || N_p < 0 || N_l < 0 || B < 0) return 0;
    return prop_train_carve(m->cfg, nullptr, N_p, N_l, B).bytes;
}

extern "C" int td_prop_forward_train(const td_prop *m, const float *d_protein_pos, const float *d_protein_feat,
                                     const int32_t *d_protein_ptr, int64_t N_p, const float *d_ligand_pos, const float *d_ligand_feat,
                                     const int32_t *d_ligand_ptr, int64_t N_l, int64_t B, const float *d_enc_ligand,
                                     const float *d_enc_node, const float *d_enc_graph, const int64_t *d_output_kind,
                                     int32_t max_graph_nodes, float *d_out, void *d_workspace, size_t workspace_bytes, td_prop_tape *tape,
                                     void *stream) {
    if (!m || !tape || N_p < 0 || N_l < 0 || B < 1) { td_set_error("td_prop_forward_train: bad argument"); return TD_EINVAL; }
    const td_prop_config &c = m->cfg;
    if (!d_protein_ptr || !d_ligand_ptr || !d_out || !d_workspace || (N_p > 0 && (!d_protein_pos || !d_protein_feat)) ||
        (N_l > 0 && (!d_ligand_pos || !d_ligand_feat))) {
        td_set_error("td_prop_forward_train: null pointer");
        return TD_EINVAL;
    }
    if (c.enc_ligand_dim > 0 && N_l > 0 && !d_enc_ligand) {
        td_set_error("td_prop_forward_train: enc_ligand_dim is %d but no enc_ligand_feature was given", c.enc_ligand_dim);
        return TD_EINVAL;
    }
    if (c.enc_graph_dim > 0 && !d_enc_graph) {
        td_set_error("td_prop_forward_train: enc_graph_dim is %d but no enc_graph_feature was given", c.enc_graph_dim);
        return TD_EINVAL;
    }
    if (d_enc_node && c.enc_node_dim == 0) {
        td_set_error("td_prop_forward_train: an enc_node_feature was given to a model with enc_node_dim 0");
        return TD_EINVAL;
    }
    PropTrainWs w = prop_train_carve(c, static_cast<char *>(d_workspace), N_p, N_l, B);
    if (w.bytes > workspace_bytes) {
        td_set_error("td_prop_forward_train: workspace has %zu bytes, need %zu (td_prop_train_workspace_bytes)", workspace_bytes, w.bytes);
        return TD_ENOMEM;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t N = N_p + N_l;
    const size_t NH = (size_t)N * H;
    int rc;
    // the launches of td_prop_forward, in its order and on the same inputs; the layers' h, mi and t land in the tape
    if ((rc = td_launch_prop_linear(d_protein_feat, c.protein_feat_dim, nullptr, 0, m->pW, m->pb, nullptr, w.fw.hp, N_p, H, TD_PROP_ACT_NONE, s)) != TD_OK) return rc;
    if ((rc = td_launch_prop_linear(d_ligand_feat, c.ligand_feat_dim, d_enc_ligand, c.enc_ligand_dim, m->lW, m->lb, nullptr, w.fw.hl, N_l, H,
                                    TD_PROP_ACT_NONE, s)) != TD_OK) return rc;
    if ((rc = td_launch_prop_compose(w.fw.hp, w.fw.hl, d_protein_pos, d_ligand_pos, d_protein_ptr, d_ligand_ptr, w.hin, w.fw.x, w.fw.node_ptr, B, s)) != TD_OK)
        return rc;
    if (N > 0 && (rc = td_knn(w.fw.x, w.fw.node_ptr, N, B, c.knn, max_graph_nodes, w.fw.nbr, stream)) != TD_OK) return rc;
    for (int l = 0; l < c.num_layers; ++l) {
        const TdPropLayer &L = m->layers[(size_t)l];
        float *h = w.hin + (size_t)l * NH, *mi = w.mi + (size_t)l * NH, *t = w.t + (size_t)l * NH;
        if ((rc = td_launch_prop_linear(h, H, nullptr, 0, L.projW, L.projB, nullptr, w.fw.P, N, 2 * H, TD_PROP_ACT_NONE, s)) != TD_OK) return rc;
        if ((rc = td_launch_prop_edge(L, w.fw.x, w.fw.nbr, c.knn, w.fw.P, mi, N, m->coeff, s)) != TD_OK) return rc;
        if ((rc = td_launch_prop_linear(mi, H, h, H, L.n1W, L.n1b, nullptr, t, N, H, TD_PROP_ACT_RELU, s)) != TD_OK) return rc;
        if ((rc = td_launch_prop_linear(t, H, nullptr, 0, L.n2W, L.n2b, h, h + NH, N, H, TD_PROP_ACT_NONE, s)) != TD_OK) return rc;
    }
    const float *hf = w.hin + (size_t)c.num_layers * NH;
    if (d_enc_node) {
        if ((rc = td_launch_prop_linear(hf, H, d_enc_node, c.enc_node_dim, m->e1W, m->e1b, nullptr, w.te, N, H, TD_PROP_ACT_RELU, s)) != TD_OK) return rc;
        if ((rc = td_launch_prop_linear(w.te, H, nullptr, 0, m->e2W, m->e2b, nullptr, w.fw.h, N, H, TD_PROP_ACT_NONE, s)) != TD_OK) return rc;
        hf = w.fw.h;
    }
    if ((rc = td_launch_prop_segment_sum(hf, w.fw.node_ptr, d_enc_graph, c.enc_graph_dim, w.fw.pre, B, s)) != TD_OK) return rc;
    if ((rc = td_launch_prop_linear(w.fw.pre, H + c.enc_graph_dim, nullptr, 0, m->o1W, m->o1b, nullptr, w.fw.y1, B, H, TD_PROP_ACT_SSP, s)) != TD_OK) return rc;
    if ((rc = td_launch_prop_linear(w.fw.pre, H + c.enc_graph_dim, nullptr, 0, m->o1W, m->o1b, nullptr, w.zo1, B, H, TD_PROP_ACT_NONE, s)) != TD_OK) return rc;
    float *y = d_output_kind ? w.fw.y : d_out;
    if ((rc = td_launch_prop_linear(w.fw.y1, H, nullptr, 0, m->o2W, m->o2b, nullptr, y, B, c.output_dim, TD_PROP_ACT_NONE, s)) != TD_OK) return rc;
    if (d_output_kind && (rc = td_launch_prop_select(w.fw.y, d_output_kind, c.output_dim, d_out, B, s)) != TD_OK) return rc;
    // ---- the rest of the tape: the inputs the weight gradients read
    auto copy = [&](void *dst, const void *src, size_t bytes) -> hipError_t {
        return bytes && src ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) : hipSuccess;
    };
    TD_CHECK_HIP(copy(w.pptr, d_protein_ptr, (size_t)(B + 1) * 4));
    TD_CHECK_HIP(copy(w.lptr, d_ligand_ptr, (size_t)(B + 1) * 4));
    TD_CHECK_HIP(copy(w.pfeat, d_protein_feat, (size_t)N_p * c.protein_feat_dim * 4));
    TD_CHECK_HIP(copy(w.lfeat, d_ligand_feat, (size_t)N_l * c.ligand_feat_dim * 4));
    if (c.enc_ligand_dim > 0) {
        if (d_enc_ligand) TD_CHECK_HIP(copy(w.elig, d_enc_ligand, (size_t)N_l * c.enc_ligand_dim * 4));
        else TD_CHECK_HIP(hipMemsetAsync(w.elig, 0, (size_t)N_l * c.enc_ligand_dim * 4, s));
    }
    if (d_enc_node) TD_CHECK_HIP(copy(w.enode, d_enc_node, NH / H * c.enc_node_dim * 4));
    if (d_output_kind) TD_CHECK_HIP(copy(w.kind, d_output_kind, (size_t)B * 8));
    tape->model = m;
    tape->weights_version = m->weights_version;
    tape->N_p = N_p; tape->N_l = N_l; tape->B = B;
    tape->has_output_kind = d_output_kind != nullptr;
    tape->has_enc_node = d_enc_node != nullptr;
    tape->d_workspace = d_workspace;
    tape->workspace_bytes = workspace_bytes;
    return TD_OK;
}

extern "C" int td_prop_backward(const td_prop *m, const td_prop_tape *tape, int64_t N_p, int64_t N_l, int64_t B, const float *d_grad_out,
                                float *d_grad_weights, size_t num_weights, void *stream) {
    if (!m || !tape || !d_grad_out || !d_grad_weights) { td_set_error("td_prop_backward: bad argument"); return TD_EINVAL; }
    const td_prop_config &c = m->cfg;
    if (tape->model != m) { td_set_error("td_prop_backward: the tape was recorded by another td_prop handle"); return TD_EINVAL; }
    if (tape->N_p != N_p || tape->N_l != N_l || tape->B != B) {
        td_set_error("td_prop_backward: the tape was recorded at N_p %lld, N_l %lld, B %lld, not N_p %lld, N_l %lld, B %lld",
                     (long long)tape->N_p, (long long)tape->N_l, (long long)tape->B, (long long)N_p, (long long)N_l, (long long)B);
        return TD_EINVAL;
    }
    if (tape->weights_version != m->weights_version) {
        td_set_error("td_prop_backward: the weights changed (td_prop_set_weights) after the tape was recorded");
        return TD_EINVAL;
    }
    if (num_weights != td_prop_num_weights(&c)) {
        td_set_error("td_prop_backward: gradient buffer has %zu floats, expected %zu", num_weights, td_prop_num_weights(&c));
        return TD_EINVAL;
    }
    PropTrainWs w = prop_train_carve(c, static_cast<char *>(tape->d_workspace), N_p, N_l, B);
    if (!tape->d_workspace || w.bytes > tape->workspace_bytes) {
        td_set_error("td_prop_backward: the tape's workspace has %zu bytes, need %zu", tape->workspace_bytes, w.bytes);
        return TD_ENOMEM;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t N = N_p + N_l, E = N * c.knn;
    const size_t NH = (size_t)N * H;
    const int O = c.output_dim, Eg = c.enc_graph_dim, En = c.enc_node_dim, K1 = G + 2 * H;
    const PropFlat F = prop_flat(c);
    float *Gw = d_grad_weights;
    constexpr int T = 1, RELU = TD_PROP_EPI_RELU_MASK;
    int rc;
#define PB_TRY(call) do { if ((rc = (call)) != TD_OK) return rc; } while (0)
    // ---- readout: output_kind select, out_block (prop_model.py:152-160), segment sum
    PB_TRY(td_launch_prop_select_bwd(d_grad_out, tape->has_output_kind ? w.kind : nullptr, O, w.dy, B, s));
    PB_TRY(td_launch_prop_xty(w.dy, O, O, w.fw.y1, H, H, nullptr, 0, 0, B, w.part, Gw + F.o2W, H, 0, s));
    PB_TRY(td_launch_prop_xty(w.dy, O, O, nullptr, 0, 0, nullptr, 0, 0, B, w.part, Gw + F.o2b, 1, 0, s));
    PB_TRY(td_launch_prop_bgemm(w.dy, O, O, nullptr, 0, 0, m->o2W, H, T, w.zo1, H, TD_PROP_EPI_SSP_DERIV, nullptr, 0, nullptr, 0, w.dy1, H, B, H, s));
    PB_TRY(td_launch_prop_xty(w.dy1, H, H, w.fw.pre, H + Eg, H + Eg, nullptr, 0, 0, B, w.part, Gw + F.o1W, H + Eg, 0, s));
    PB_TRY(td_launch_prop_xty(w.dy1, H, H, nullptr, 0, 0, nullptr, 0, 0, B, w.part, Gw + F.o1b, 1, 0, s));
    PB_TRY(td_launch_prop_bgemm(w.dy1, H, H, nullptr, 0, 0, m->o1W, H + Eg, T, nullptr, 0, 0, nullptr, 0, nullptr, 0, w.dpre, H, B, H, s));
    PB_TRY(td_launch_prop_broadcast(w.dpre, w.fw.node_ptr, w.dh, B, s));
    const float *hL = w.hin + (size_t)c.num_layers * NH;
    // ---- enc_node_layer (prop_model.py:147-149)
    if (tape->has_enc_node) {
        PB_TRY(td_launch_prop_xty(w.dh, H, H, w.te, H, H, nullptr, 0, 0, N, w.part, Gw + F.e2W, H, 0, s));
        PB_TRY(td_launch_prop_xty(w.dh, H, H, nullptr, 0, 0, nullptr, 0, 0, N, w.part, Gw + F.e2b, 1, 0, s));
        PB_TRY(td_launch_prop_bgemm(w.dh, H, H, nullptr, 0, 0, m->e2W, H, T, w.te, H, RELU, nullptr, 0, nullptr, 0, w.dt, H, N, H, s));
        PB_TRY(td_launch_prop_xty(w.dt, H, H, hL, H, H, w.enode, En, En, N, w.part, Gw + F.e1W, H + En, 0, s));
        PB_TRY(td_launch_prop_xty(w.dt, H, H, nullptr, 0, 0, nullptr, 0, 0, N, w.part, Gw + F.e1b, 1, 0, s));
        PB_TRY(td_launch_prop_bgemm(w.dt, H, H, nullptr, 0, 0, m->e1W, H + En, T, nullptr, 0, 0, nullptr, 0, nullptr, 0, w.dh2, H, N, H, s));
        std::swap(w.dh, w.dh2);
    } else if (En > 0) {                      // a model with enc_node_layer, run without enc_node_feature: the layer gets no gradient
        TD_CHECK_HIP(hipMemsetAsync(Gw + F.e1W, 0, (F.o1W - F.e1W) * sizeof(float), s));
    }
    // ---- encoder layers, last to first
    PB_TRY(td_launch_prop_radj(w.fw.nbr, N, c.knn, w.cnt, w.rptr, w.ridx, s));
    for (int l = c.num_layers - 1; l >= 0; --l) {
        const TdPropLayer &L = m->layers[(size_t)l];
        const PropFlatLayer &FL = F.layers[(size_t)l];
        const float *h = w.hin + (size_t)l * NH, *mi = w.mi + (size_t)l * NH, *t = w.t + (size_t)l * NH;
        // node_mlp: h' = h + N2 t + c2, t = ReLU(N1 [mi | h] + c1)
        PB_TRY(td_launch_prop_xty(w.dh, H, H, t, H, H, nullptr, 0, 0, N, w.part, Gw + FL.n2W, H, 0, s));
        PB_TRY(td_launch_prop_xty(w.dh, H, H, nullptr, 0, 0, nullptr, 0, 0, N, w.part, Gw + FL.n2b, 1, 0, s));
        PB_TRY(td_launch_prop_bgemm(w.dh, H, H, nullptr, 0, 0, L.n2W, H, T, t, H, RELU, nullptr, 0, nullptr, 0, w.dt, H, N, H, s));
        PB_TRY(td_launch_prop_xty(w.dt, H, H, mi, H, H, h, H, H, N, w.part, Gw + FL.n1W, 2 * H, 0, s));
        PB_TRY(td_launch_prop_xty(w.dt, H, H, nullptr, 0, 0, nullptr, 0, 0, N, w.part, Gw + FL.n1b, 1, 0, s));
        PB_TRY(td_launch_prop_bgemm(w.dt, H, H, nullptr, 0, 0, L.n1W, 2 * H, T, nullptr, 0, 0, nullptr, 0, nullptr, 0, w.dmi, H, N, H, s));
        PB_TRY(td_launch_prop_bgemm(w.dt, H, H, nullptr, 0, 0, L.n1W + H, 2 * H, T, nullptr, 0, 0, nullptr, 0, nullptr, 0, w.dhu, H, N, H, s));
        // edges: recompute P, then the per-edge backward
        PB_TRY(td_launch_prop_linear(h, H, nullptr, 0, L.projW, L.projB, nullptr, w.fw.P, N, 2 * H, TD_PROP_ACT_NONE, s));
        PB_TRY(td_launch_prop_edge_bwd(L, m->W2Tf[(size_t)l], w.fw.x, w.fw.nbr, c.knn, w.fw.P, w.dmi, N, m->coeff, w.Ae, w.DZ2, w.DZ1,
                                       w.RBF, w.Q, w.S, w.DWP, s));
        PB_TRY(td_launch_prop_gather(w.DZ1, w.rptr, w.ridx, w.R, N, s));
        PB_TRY(td_launch_prop_xty(w.DZ2, H, H, w.Ae, H, H, nullptr, 0, 0, E, w.part, Gw + FL.W2, H, 0, s));
        PB_TRY(td_launch_prop_xty(w.DZ2, H, H, nullptr, 0, 0, nullptr, 0, 0, E, w.part, Gw + FL.b2, 1, 0, s));
        PB_TRY(td_launch_prop_xty(w.DZ1, H, H, w.RBF, G, G, nullptr, 0, 0, E, w.part, Gw + FL.W1, K1, 0, s));
        PB_TRY(td_launch_prop_xty(w.S, H, H, h, H, H, nullptr, 0, 0, N, w.part, Gw + FL.W1, K1, G, s));
        PB_TRY(td_launch_prop_xty(w.R, H, H, h, H, H, nullptr, 0, 0, N, w.part, Gw + FL.W1, K1, G + H, s));
        PB_TRY(td_launch_prop_xty(w.S, H, H, nullptr, 0, 0, nullptr, 0, 0, N, w.part, Gw + FL.b1, 1, 0, s));
        PB_TRY(td_launch_prop_xty(w.DWP, H, H, nullptr, 0, 0, nullptr, 0, 0, N, w.part, Gw + FL.winf, 1, 0, s));
        PB_TRY(td_launch_prop_xty(w.Q, 1, 1, nullptr, 0, 0, nullptr, 0, 0, E, w.part, Gw + FL.binf, 1, 0, s));
        // dh = W1i^T S + W1j^T R + dh' + (node_mlp's h half)
        PB_TRY(td_launch_prop_bgemm(w.S, H, H, w.R, H, H, L.projW, H, T, nullptr, 0, 0, w.dh, H, w.dhu, H, w.dh2, H, N, H, s));
        std::swap(w.dh, w.dh2);
    }
    // ---- compose and the embeddings (weight gradients only)
    PB_TRY(td_launch_prop_uncompose(w.dh, w.pptr, w.lptr, w.dhp, w.dhl, B, s));
    const int Fp = c.protein_feat_dim, Fl = c.ligand_feat_dim, El = c.enc_ligand_dim;
    PB_TRY(td_launch_prop_xty(w.dhp, H, H, w.pfeat, Fp, Fp, nullptr, 0, 0, N_p, w.part, Gw + F.pW, Fp, 0, s));
    PB_TRY(td_launch_prop_xty(w.dhp, H, H, nullptr, 0, 0, nullptr, 0, 0, N_p, w.part, Gw + F.pb, 1, 0, s));
    PB_TRY(td_launch_prop_xty(w.dhl, H, H, w.lfeat, Fl, Fl, w.elig, El, El, N_l, w.part, Gw + F.lW, Fl + El, 0, s));
    PB_TRY(td_launch_prop_xty(w.dhl, H, H, nullptr, 0, 0, nullptr, 0, 0, N_l, w.part, Gw + F.lb, 1, 0, s));
    TD_CHECK_HIP(hipMemsetAsync(Gw + F.offset, 0, G * sizeof(float), s));           // a buffer, not a parameter
#undef PB_TRY
    return TD_OK;
}

extern "C" int td_prop_set_weights(td_prop *m, const float *d_weights, size_t num_weights, void *stream) {
    if (!m || !d_weights) { td_set_error("td_prop_set_weights: bad argument"); return TD_EINVAL; }
    const td_prop_config &c = m->cfg;
    if (num_weights != td_prop_num_weights(&c)) {
        td_set_error("td_prop_set_weights: weight blob has %zu floats, expected %zu", num_weights, td_prop_num_weights(&c));
        return TD_EINVAL;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const PropFlat F = prop_flat(c);
    const float *src = d_weights;
    auto cp = [&](const float *dst, size_t off, size_t n) {
        return hipMemcpyAsync(const_cast<float *>(dst), src + off, n * sizeof(float), hipMemcpyDeviceToDevice, s);
    };
    const int Fl = c.ligand_feat_dim + c.enc_ligand_dim, E = G + 2 * H;
    TD_CHECK_HIP(cp(m->pW, F.pW, (size_t)H * c.protein_feat_dim));
    TD_CHECK_HIP(cp(m->pb, F.pb, H));
    TD_CHECK_HIP(cp(m->lW, F.lW, (size_t)H * Fl));
    TD_CHECK_HIP(cp(m->lb, F.lb, H));
    if (c.num_layers > 0) TD_CHECK_HIP(cp(m->layers[0].offset, F.offset, G));
    for (int l = 0; l < c.num_layers; ++l) {
        const TdPropLayer &L = m->layers[(size_t)l];
        const PropFlatLayer &FL = F.layers[(size_t)l];
        // projW = [W1[:, 64:320]; W1[:, 320:576]], projB = [b1 | 0]; W1f / W2f / W2Tf: the A fragments of td_prop_create
        TD_CHECK_HIP(hipMemcpy2DAsync(const_cast<float *>(L.projW), H * sizeof(float), src + FL.W1 + G, E * sizeof(float),
                                      H * sizeof(float), H, hipMemcpyDeviceToDevice, s));
        TD_CHECK_HIP(hipMemcpy2DAsync(const_cast<float *>(L.projW) + (size_t)H * H, H * sizeof(float), src + FL.W1 + G + H,
                                      E * sizeof(float), H * sizeof(float), H, hipMemcpyDeviceToDevice, s));
        TD_CHECK_HIP(cp(L.projB, FL.b1, H));
        int rc;
        if ((rc = td_launch_prop_pack_afrag(src + FL.W1, E, 0, G / 16, 0, const_cast<float *>(L.W1f), s)) != TD_OK) return rc;
        if ((rc = td_launch_prop_pack_afrag(src + FL.W2, H, 0, H / 16, 0, const_cast<float *>(L.W2f), s)) != TD_OK) return rc;
        if ((rc = td_launch_prop_pack_afrag(src + FL.W2, H, 0, H / 16, 1, const_cast<float *>(m->W2Tf[(size_t)l]), s)) != TD_OK) return rc;
        TD_CHECK_HIP(cp(L.b2, FL.b2, H));
        TD_CHECK_HIP(cp(L.winf, FL.winf, H));
        TD_CHECK_HIP(cp(L.binf, FL.binf, 1));
        TD_CHECK_HIP(cp(L.n1W, FL.n1W, (size_t)H * 2 * H));
        TD_CHECK_HIP(cp(L.n1b, FL.n1b, H));
        TD_CHECK_HIP(cp(L.n2W, FL.n2W, (size_t)H * H));
        TD_CHECK_HIP(cp(L.n2b, FL.n2b, H));
    }
    if (c.enc_node_dim > 0) {
        TD_CHECK_HIP(cp(m->e1W, F.e1W, (size_t)H * (H + c.enc_node_dim)));
        TD_CHECK_HIP(cp(m->e1b, F.e1b, H));
        TD_CHECK_HIP(cp(m->e2W, F.e2W, (size_t)H * H));
        TD_CHECK_HIP(cp(m->e2b, F.e2b, H));
    }
    TD_CHECK_HIP(cp(m->o1W, F.o1W, (size_t)H * (H + c.enc_graph_dim)));
    TD_CHECK_HIP(cp(m->o1b, F.o1b, H));
    TD_CHECK_HIP(cp(m->o2W, F.o2W, (size_t)c.output_dim * H));
    TD_CHECK_HIP(cp(m->o2b, F.o2b, c.output_dim));
    ++m->weights_version;
    return TD_OK;
}
