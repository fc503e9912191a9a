// Binding-affinity predictor (models/property_pred/prop_model.py PropPredNet / PropPredNetEnc, prop_egnn.py EnEquiEncoder) for gfx950.
// One forward (td_prop_forward, prop_api.cpp) =
//     prop_linear_kernel x2        embeddings: protein_atom_emb, ligand_atom_emb on [ligand feature | enc_ligand_feature]
//     prop_compose_kernel          compose_context_prop: per complex its protein rows, then its ligand rows (the project's order rule)
//     td_knn (k <= 64)             knn_graph(pos, k, batch, flow='target_to_source'): row i = the k nearest same-complex nodes of i
//     per layer (h = h + EnBaseLayer(h), prop_egnn.py:28-45, 80-82):
//       prop_linear_kernel         P_i = W1[:, 64:320] h_i + b1,  P_j = W1[:, 320:576] h_j            (first edge Linear, node side)
//       prop_edge_kernel           m_ij = ReLU(W2 ReLU(W1[:, 0:64] rbf(|x_i - x_j|) + P_i + P_j) + b2);  e_ij = sigmoid(w . m_ij + b);
//                                  mi = sum_j e_ij m_ij                                                    (registers, no atomics)
//       prop_linear_kernel x2      h += W2n ReLU(W1n [mi | h] + b1n) + b2n
//     prop_linear_kernel x2        enc_node_layer on [h | enc_node_feature] (when given)
//     prop_segment_sum_kernel      pre_out = scatter_sum(h, batch): one workgroup per complex, rows in index order (deterministic)
//     prop_linear_kernel x2        out_block on [pre_out | enc_graph_feature]: Linear, ShiftedSoftplus, Linear
//     prop_select_kernel           output_kind (1 = Ki, 2 = Kd, 3 = IC50) -> [B, 1]
//
// Arithmetic: fp32 throughout, every matrix product on v_mfma_f32_16x16x4_f32.  The project's bf16x3 splits and the f16 piece pairs
// of the diffusion path's edge kernels were not used: the former would triple the MFMA count of an edge kernel that is already
// MFMA-bound (~164 kFLOP per edge), the latter is the judgement call of VERDICT.md and a new model should not reopen it.  Plain fp32
// MFMA keeps the results within a few fp32 ulps of the reference's own fp32 run and needs no error analysis of its own.
//
// Operand layout of the 16x16x4 product (as in egnn.hip): A[m][k] = lane (m + 16k), B[k][n] = lane (n + 16k), D[m][n] = lane n + 16 (m / 4),
// register m % 4.  In the edge kernel the weight is the A operand (m = output unit), the activations of 16 edges the B operand
// (n = edge); k-step (b, r) pairs lane group g with hidden unit 16b + 4g + r on both sides, so an accumulator's registers are the next
// product's B operand as they are.  The second Linear's weight (256 x 256 fp32 = 256 KB) does not fit in LDS (160 KB): its A
// fragments are read from global memory, coalesced (one float4 per lane per 16 x 16 tile), and stay resident in L2 across waves.
#include "td_device.h"
#include "td_internal.h"

typedef float floatx4_t __attribute__((ext_vector_type(4)));

namespace {

constexpr int PH = TD_PROP_H;          // 256
constexpr int POT = PH / 16;           // 16 output tiles

__device__ __forceinline__ floatx4_t pp_mfma16(float a, float b, floatx4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float pp_sum16(float v) {          // over the 16 lanes of a DPP row
    v += td_dpp<DPP_QUAD_XOR1>(v);
    v += td_dpp<DPP_QUAD_XOR2>(v);
    v += td_dpp<DPP_ROW_HALF_MIRROR>(v);
    v += td_dpp<DPP_ROW_MIRROR>(v);
    return v;
}
__device__ __forceinline__ float pp_sum_groups(float v) { return td_sum_halves(td_sum_rows16(v)); }   // over the 4 lane groups

__device__ __forceinline__ float pp_act(float v, int act) {
    if (act == TD_PROP_ACT_RELU) return v > 0.f ? v : 0.f;
    if (act == TD_PROP_ACT_SSP) {                               // ShiftedSoftplus: softplus (beta 1, threshold 20) - log 2
        const float sp = v > 20.f ? v : log1pf(expf(v));
        return sp - 0.693147180559945309f;
    }
    return v;
}

// Y[n][o] = act(sum_k [X1 | X2][n][k] W[o][k] + bias[o]) + R[n][o]   (X1: K1 columns, X2: K2 columns; W row-major, ldw = K1 + K2).
// A workgroup = 4 waves = 16 rows x 256 outputs; a wave = 16 rows x 64 outputs (4 tiles).  R may alias Y (each element is read and
// written by the same lane).
__global__ __launch_bounds__(256) void prop_linear_kernel(const float *__restrict__ X1, int K1, const float *__restrict__ X2, int K2,
                                                          const float *__restrict__ W, const float *__restrict__ bias,
                                                          const float *R, float *Y, int64_t N, int O, int act) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int lo = lane & 15, g = lane >> 4;
    const int64_t n0 = (int64_t)blockIdx.x * 16;
    const int o0 = blockIdx.y * 256 + wid * 64;
    if (o0 >= O) return;
    const int K = K1 + K2;
    const int64_t node = n0 + lo;
    const bool nok = node < N;
    floatx4_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = floatx4_t{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + g;
        float b = 0.f;
        if (nok && k < K) b = k < K1 ? X1[node * K1 + k] : X2[node * K2 + (k - K1)];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int o = o0 + 16 * t + lo;
            const float a = (o < O && k < K) ? W[(size_t)o * K + k] : 0.f;
            acc[t] = pp_mfma16(a, b, acc[t]);
        }
    }
    if (!nok) return;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = o0 + 16 * t + 4 * g + r;
            if (o >= O) continue;
            float v = pp_act(acc[t][r] + (bias ? bias[o] : 0.f), act);
            if (R) v += R[node * O + o];
            Y[node * O + o] = v;
        }
}

// compose_context_prop: composed row r of complex b = its protein rows, then its ligand rows; node_ptr[b] = protein_ptr[b] + ligand_ptr[b].
__global__ void prop_compose_kernel(const float *__restrict__ hp, const float *__restrict__ hl, const float *__restrict__ pp,
                                    const float *__restrict__ pl, const int32_t *__restrict__ protein_ptr,
                                    const int32_t *__restrict__ ligand_ptr, float *__restrict__ h, float *__restrict__ x,
                                    int32_t *__restrict__ node_ptr, int64_t B) {
    const int64_t b = blockIdx.x;
    const int32_t p0 = protein_ptr[b], p1 = protein_ptr[b + 1], l0 = ligand_ptr[b], l1 = ligand_ptr[b + 1];
    const int64_t base = (int64_t)p0 + l0, np = p1 - p0, n = np + (l1 - l0);
    if (threadIdx.x == 0) {
        node_ptr[b] = (int32_t)base;
        if (b == B - 1) node_ptr[B] = p1 + l1;
    }
    for (int64_t u = threadIdx.x; u < n * PH; u += blockDim.x) {
        const int64_t r = u / PH, c = u % PH;
        h[(base + r) * PH + c] = r < np ? hp[(p0 + r) * PH + c] : hl[(l0 + r - np) * PH + c];
    }
    for (int64_t u = threadIdx.x; u < n * 3; u += blockDim.x) {
        const int64_t r = u / 3, c = u % 3;
        x[(base + r) * 3 + c] = r < np ? pp[(p0 + r) * 3 + c] : pl[(l0 + r - np) * 3 + c];
    }
}

// One wave per destination row i (a workgroup = 4 consecutive rows); its k <= 64 edges in blocks of 16 (one edge per lane column).
// P: [N][512] = [P_i | P_j].  The first Linear's activations of a 16-edge block go through the wave's slice of LDS ([edge][256],
// row stride 260 floats against bank conflicts): written as the accumulator tiles come out, read back one k-step at a time as the
// second product's B operand, so that only that product's 16 accumulator tiles and the mi partial sums are live across the loop.
constexpr int PE_STRIDE = PH + 4;

__global__ __launch_bounds__(256) void prop_edge_kernel(TdPropLayer L, const float *__restrict__ x, const int32_t *__restrict__ nbr,
                                                        int k, const float *__restrict__ P, float *__restrict__ mi, int64_t N,
                                                        float coeff) {
    __shared__ __attribute__((aligned(16))) float lds[4 * 16 * PE_STRIDE];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int lo = lane & 15, g = lane >> 4;
    float *act = lds + wid * 16 * PE_STRIDE;
    const float4 *W1f = reinterpret_cast<const float4 *>(L.W1f);        // [ot 16][kb 4][lane] float4
    const float4 *W2f = reinterpret_cast<const float4 *>(L.W2f);        // [ot 16][hb 16][lane] float4
    const int nblk = (k + 15) / 16;
    const float binf = L.binf[0];
    // every wave of a workgroup runs the same number of iterations (the barriers below); a wave past the end recomputes row N - 1
    // and writes nothing
    for (int64_t base = (int64_t)blockIdx.x * 4; base < N; base += (int64_t)gridDim.x * 4) {
        const bool live = base + wid < N;
        const int64_t i = live ? base + wid : N - 1;
        const float xi0 = x[i * 3], xi1 = x[i * 3 + 1], xi2 = x[i * 3 + 2];
        floatx4_t accm[POT];
#pragma unroll
        for (int ot = 0; ot < POT; ++ot) accm[ot] = floatx4_t{0.f, 0.f, 0.f, 0.f};
        for (int eb = 0; eb < nblk; ++eb) {
            const int slot = 16 * eb + lo;
            const int j = slot < k ? nbr[i * k + slot] : -1;
            const bool valid = j >= 0;
            const int64_t jj = valid ? j : i;
            const float dx = xi0 - x[jj * 3], dy = xi1 - x[jj * 3 + 1], dz = xi2 - x[jj * 3 + 2];
            const float d = sqrtf((dx * dx + dy * dy) + dz * dz);          // prop_egnn.py:78 (torch.norm)
            // GaussianSmearing(0, cutoff, 64, fixed_offset=False): exp(coeff (d - offset)^2), models/common.py:24-26
            float rbf[4][4];
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float t = d - L.offset[16 * kb + 4 * g + r];
                    rbf[kb][r] = expf(coeff * (t * t));
                }
            // ---- first Linear: W1[:, 0:64] rbf (K = 64 on MFMA) + P_i + P_j (b1 is in P_i), ReLU -> LDS ----------------------
#pragma unroll 4
            for (int ot = 0; ot < POT; ++ot) {
                floatx4_t a = floatx4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kb = 0; kb < 4; ++kb) {
                    const float4 w = W1f[(ot * 4 + kb) * 64 + lane];
                    a = pp_mfma16(w.x, rbf[kb][0], a);
                    a = pp_mfma16(w.y, rbf[kb][1], a);
                    a = pp_mfma16(w.z, rbf[kb][2], a);
                    a = pp_mfma16(w.w, rbf[kb][3], a);
                }
                const float4 pi = *reinterpret_cast<const float4 *>(P + (size_t)i * (2 * PH) + 16 * ot + 4 * g);
                const float4 pj = *reinterpret_cast<const float4 *>(P + (size_t)jj * (2 * PH) + PH + 16 * ot + 4 * g);
                float4 v;
                v.x = fmaxf(a[0] + (pi.x + pj.x), 0.f);
                v.y = fmaxf(a[1] + (pi.y + pj.y), 0.f);
                v.z = fmaxf(a[2] + (pi.z + pj.z), 0.f);
                v.w = fmaxf(a[3] + (pi.w + pj.w), 0.f);
                *reinterpret_cast<float4 *>(act + lo * PE_STRIDE + 16 * ot + 4 * g) = v;
            }
            __syncthreads();
            // ---- second Linear (256 x 256 on MFMA) + ReLU (act_last): m_ij ------------------------------------------------------
            floatx4_t m[POT];
#pragma unroll
            for (int ot = 0; ot < POT; ++ot) m[ot] = floatx4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
            for (int hb = 0; hb < POT; ++hb) {
                const float4 av = *reinterpret_cast<const float4 *>(act + lo * PE_STRIDE + 16 * hb + 4 * g);
#pragma unroll
                for (int ot = 0; ot < POT; ++ot) {
                    const float4 w = W2f[(ot * POT + hb) * 64 + lane];
                    m[ot] = pp_mfma16(w.x, av.x, m[ot]);
                    m[ot] = pp_mfma16(w.y, av.y, m[ot]);
                    m[ot] = pp_mfma16(w.z, av.z, m[ot]);
                    m[ot] = pp_mfma16(w.w, av.w, m[ot]);
                }
            }
            __syncthreads();                                                  // act is rewritten by the next block
            float part = 0.f;
#pragma unroll
            for (int ot = 0; ot < POT; ++ot) {
                const float4 bv = *reinterpret_cast<const float4 *>(L.b2 + 16 * ot + 4 * g);
                const float4 wv = *reinterpret_cast<const float4 *>(L.winf + 16 * ot + 4 * g);
                m[ot][0] = fmaxf(m[ot][0] + bv.x, 0.f);
                m[ot][1] = fmaxf(m[ot][1] + bv.y, 0.f);
                m[ot][2] = fmaxf(m[ot][2] + bv.z, 0.f);
                m[ot][3] = fmaxf(m[ot][3] + bv.w, 0.f);
                part = fmaf(wv.x, m[ot][0], part);
                part = fmaf(wv.y, m[ot][1], part);
                part = fmaf(wv.z, m[ot][2], part);
                part = fmaf(wv.w, m[ot][3], part);
            }
            // ---- e_ij = sigmoid(edge_inf(m_ij)); this lane's share of mi = sum_j e_ij m_ij ------------------------------------
            const float s = pp_sum_groups(part) + binf;
            const float e = valid ? 1.0f / (1.0f + expf(-s)) : 0.f;
#pragma unroll
            for (int ot = 0; ot < POT; ++ot) {
                accm[ot][0] = fmaf(e, m[ot][0], accm[ot][0]);
                accm[ot][1] = fmaf(e, m[ot][1], accm[ot][1]);
                accm[ot][2] = fmaf(e, m[ot][2], accm[ot][2]);
                accm[ot][3] = fmaf(e, m[ot][3], accm[ot][3]);
            }
        }
#pragma unroll
        for (int ot = 0; ot < POT; ++ot) {
            float4 o;
            o.x = pp_sum16(accm[ot][0]);
            o.y = pp_sum16(accm[ot][1]);
            o.z = pp_sum16(accm[ot][2]);
            o.w = pp_sum16(accm[ot][3]);
            if (live && lo == 0) *reinterpret_cast<float4 *>(mi + (size_t)i * PH + 16 * ot + 4 * g) = o;
        }
    }
}

// pre_out[b][c] = sum over complex b's composed rows (ascending) of h[r][c]; columns C .. C + Eg of a row = enc_graph_feature[b].
__global__ void prop_segment_sum_kernel(const float *__restrict__ h, const int32_t *__restrict__ node_ptr,
                                        const float *__restrict__ enc_graph, int Eg, float *__restrict__ pre_out) {
    const int64_t b = blockIdx.x;
    const int W = PH + Eg;
    const int32_t r0 = node_ptr[b], r1 = node_ptr[b + 1];
    for (int c = threadIdx.x; c < W; c += blockDim.x) {
        float s = 0.f;
        if (c < PH)
            for (int32_t r = r0; r < r1; ++r) s += h[(size_t)r * PH + c];
        else
            s = enc_graph[b * Eg + (c - PH)];
        pre_out[b * W + c] = s;
    }
}

// out[b] = y[b][kind[b] - 1]  (sum(output * one_hot(kind - 1)), prop_model.py:72-74); a kind outside 1..O gives NaN
__global__ void prop_select_kernel(const float *__restrict__ y, const int64_t *__restrict__ kind, int O, float *__restrict__ out,
                                   int64_t B) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int64_t c = kind[b] - 1;
    out[b] = (c >= 0 && c < O) ? y[b * O + c] : __builtin_nanf("");
}

}  // namespace

int td_launch_prop_linear(const float *X1, int K1, const float *X2, int K2, const float *W, const float *bias, const float *R, float *Y,
                          int64_t N, int O, int act, hipStream_t s) {
    if (N == 0 || O == 0) return TD_OK;
    const dim3 grid((unsigned)((N + 15) / 16), (unsigned)((O + 255) / 256));
    prop_linear_kernel<<<grid, dim3(256), 0, s>>>(X1, K1, X2, K2, W, bias, R, Y, N, O, act);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

int td_launch_prop_compose(const float *hp, const float *hl, const float *pp, const float *pl, const int32_t *protein_ptr,
                           const int32_t *ligand_ptr, float *h, float *x, int32_t *node_ptr, int64_t B, hipStream_t s) {
    if (B == 0) return TD_OK;
    prop_compose_kernel<<<dim3((unsigned)B), dim3(256), 0, s>>>(hp, hl, pp, pl, protein_ptr, ligand_ptr, h, x, node_ptr, B);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

int td_launch_prop_edge(const TdPropLayer &L, const float *x, const int32_t *nbr, int k, const float *P, float *mi, int64_t N,
                        float coeff, hipStream_t s) {
    if (N == 0) return TD_OK;
    int64_t g = (N + 3) / 4;
    if (g > 4096) g = 4096;
    prop_edge_kernel<<<dim3((unsigned)g), dim3(256), 0, s>>>(L, x, nbr, k, P, mi, N, coeff);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

int td_launch_prop_segment_sum(const float *h, const int32_t *node_ptr, const float *enc_graph, int Eg, float *pre_out, int64_t B,
                               hipStream_t s) {
    if (B == 0) return TD_OK;
    prop_segment_sum_kernel<<<dim3((unsigned)B), dim3(256), 0, s>>>(h, node_ptr, enc_graph, Eg, pre_out);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

int td_launch_prop_select(const float *y, const int64_t *kind, int O, float *out, int64_t B, hipStream_t s) {
    if (B == 0) return TD_OK;
    prop_select_kernel<<<dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s>>>(y, kind, O, out, B);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}
