// C ABI of libtargetdiff_hip.so: the binding-affinity predictor (models/property_pred/prop_model.py PropPredNet / PropPredNetEnc).
// See include/targetdiff_hip.h for the contract and prop.hip for the kernels.
#include <cmath>
#include <cstring>
#include <new>
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
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&m->blob), pk.data.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(m->blob, pk.data.data(), pk.data.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        td_set_error("td_prop_create: device upload failed: %s", hipGetErrorString(e));
        if (m->blob) (void)hipFree(m->blob);
        delete m;
        return TD_EHIP;
    }
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
