// Backward pass of the binding-affinity predictor (td_prop_backward, prop_api.cpp): gradients of PropPredNet / PropPredNetEnc with
// respect to every parameter, given the gradient of the output and the tape td_prop_forward_train recorded.
//
// Per encoder layer (edge e = (i <- j), z1 = W1r rbf_e + W1i h_i + W1j h_j + b1, a = ReLU(z1), z2 = W2 a + b2, m = ReLU(z2),
// g = sigmoid(w . m + b), mi_i = sum_e g m, t = ReLU(N1 [mi | h] + c1), h' = h + N2 t + c2), in launch order:
//     prop_bgemm_kernel x2       dt = (dh' N2) * [t > 0],  du = dt N1   (dmi = du[:, 0:256], du[:, 256:512] joins dh)
//     prop_linear_kernel         P = [W1i; W1j] h + [b1 | 0]   (recomputed exactly as the forward computes it)
//     prop_edge_bwd_kernel       per edge, recomputed: rbf, a, m, g; then q = (dmi_i . m) g (1 - g), dz2 = (g dmi_i + q w) * [m > 0],
//                                dz1 = (W2^T dz2) * [a > 0] on MFMA; writes a, dz2, dz1, rbf and q per edge, S_i = sum_e dz1 and
//                                sum_e q m per destination row (registers, no atomics)
//     prop_gather_kernel         R_j = sum over the edges out of j of dz1, through the reverse adjacency (ascending edge index)
//     prop_bgemm_kernel          dh = [S | R] [W1i; W1j] + dh' + du[:, 256:512]
//     prop_xty_kernel + reduce   dN2, dN1, dW2, dW1r, dW1i, dW1j, every bias: fixed-order split-K partial sums, then a fixed-order pass
//
// Determinism: no float atomics.  Every sum runs in an order fixed by the shapes alone (split-K chunk count from the row count, chunks
// summed in ascending order), and the reverse adjacency is put in ascending edge order by a per-node insertion sort after an integer
// counting pass, so two runs give bit-identical gradients.
//
// Arithmetic: fp32, every matrix product on v_mfma_f32_16x16x4_f32 with the operand layout of prop.hip.
#include "td_device.h"
#include "td_internal.h"

typedef float floatx4_t __attribute__((ext_vector_type(4)));

namespace {

constexpr int PH = TD_PROP_H;          // 256
constexpr int POT = PH / 16;           // 16 output tiles
constexpr int PE_STRIDE = PH + 4;

__device__ __forceinline__ floatx4_t pb_mfma16(float a, float b, floatx4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float pb_sum16(float v) {
    v += td_dpp<DPP_QUAD_XOR1>(v);
    v += td_dpp<DPP_QUAD_XOR2>(v);
    v += td_dpp<DPP_ROW_HALF_MIRROR>(v);
    v += td_dpp<DPP_ROW_MIRROR>(v);
    return v;
}
__device__ __forceinline__ float pb_sum_groups(float v) { return td_sum_halves(td_sum_rows16(v)); }

// Y[n][o] = epi(sum_k [X1 | X2][n][k] Wt(o, k)) + R1[n][o] + R2[n][o], Wt(o, k) = trans ? W[k * ldw + o] : W[o * ldw + k].
// epi: NONE; RELU_MASK multiplies by [M[n][o] > 0]; SSP_DERIV multiplies by ShiftedSoftplus'(M[n][o]) = sigmoid(M), 1 above 20
// (torch's softplus threshold).  Tiling as prop_linear_kernel: a workgroup = 16 rows x 256 outputs.
__global__ __launch_bounds__(256) void prop_bgemm_kernel(const float *__restrict__ X1, int ldx1, int K1, const float *__restrict__ X2,
                                                         int ldx2, int K2, const float *__restrict__ W, int ldw, int trans,
                                                         const float *__restrict__ M, int ldm, int epi, const float *__restrict__ R1,
                                                         int ldr1, const float *__restrict__ R2, int ldr2, float *__restrict__ Y,
                                                         int ldy, int64_t N, int O) {
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
        if (nok && k < K) b = k < K1 ? X1[node * ldx1 + k] : X2[node * ldx2 + (k - K1)];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int o = o0 + 16 * t + lo;
            float a = 0.f;
            if (o < O && k < K) a = trans ? W[(size_t)k * ldw + o] : W[(size_t)o * ldw + k];
            acc[t] = pb_mfma16(a, b, acc[t]);
        }
    }
    if (!nok) return;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = o0 + 16 * t + 4 * g + r;
            if (o >= O) continue;
            float v = acc[t][r];
            if (epi == TD_PROP_EPI_RELU_MASK) {
                v = M[node * ldm + o] > 0.f ? v : 0.f;
            } else if (epi == TD_PROP_EPI_SSP_DERIV) {
                const float z = M[node * ldm + o];
                v *= z > 20.f ? 1.f : 1.0f / (1.0f + expf(-z));
            }
            if (R1) v += R1[node * ldr1 + o];
            if (R2) v += R2[node * ldr2 + o];
            Y[node * ldy + o] = v;
        }
}

// Split-K partial of G[o][k] = sum_n A[n][o] [B1 | B2][n][k] over the rows of chunk blockIdx.y; part[chunk][o][k].
// A workgroup = 64 o x 64 k; a wave = 16 o x 64 k (4 tiles).  B1 == nullptr: B is a single column of ones (column sums of A).
__global__ __launch_bounds__(256) void prop_xty_kernel(const float *__restrict__ A, int lda, int O, const float *__restrict__ B1,
                                                       int ldb1, int K1, const float *__restrict__ B2, int ldb2, int K2, int64_t N,
                                                       int64_t rows_per_chunk, float *__restrict__ part) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int lo = lane & 15, g = lane >> 4;
    const int K = B1 ? K1 + K2 : 1;
    const int ktiles = (K + 63) / 64;
    const int ob = blockIdx.x / ktiles, kb = blockIdx.x % ktiles;
    const int o = ob * 64 + wid * 16 + lo;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
    const int64_t r1 = r0 + rows_per_chunk < N ? r0 + rows_per_chunk : N;
    floatx4_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = floatx4_t{0.f, 0.f, 0.f, 0.f};
    for (int64_t n = r0; n < r1; n += 4) {
        const int64_t row = n + g;
        const bool rok = row < r1;
        const float a = (rok && o < O) ? A[row * lda + o] : 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k = kb * 64 + 16 * t + lo;
            float b = 0.f;
            if (rok && k < K) b = !B1 ? 1.f : k < K1 ? B1[row * ldb1 + k] : B2[row * ldb2 + (k - K1)];
            acc[t] = pb_mfma16(a, b, acc[t]);
        }
    }
    float *P = part + (size_t)blockIdx.y * O * K;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int oo = ob * 64 + wid * 16 + 4 * g + r;
            const int k = kb * 64 + 16 * t + lo;
            if (oo < O && k < K) P[(size_t)oo * K + k] = acc[t][r];
        }
}

// G[o * ldg + col0 + k] = sum over chunks c (ascending) of part[c][o][k]
__global__ void prop_reduce_kernel(const float *__restrict__ part, int chunks, int O, int K, float *__restrict__ G, int ldg, int col0) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= (int64_t)O * K) return;
    const size_t OK = (size_t)O * K;
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += part[c * OK + u];
    G[(u / K) * ldg + col0 + u % K] = s;
}

// Per-edge backward of one encoder layer; one wave per destination row i, its k edges in blocks of 16 (edge slot = lane column), as
// prop_edge_kernel.  Edge e = i * k + slot.  A padded slot (nbr = -1) of a live row writes zeros to dz2, dz1, rbf and q and adds
// nothing to S or sum q m; what it writes to a is ReLU(z1) evaluated with j = i, finite and never used: a enters only dW2 = dz2^T a,
// and dz2 is zero there.  Slots 16 * nblk > slot >= k of the last block and waves past the last row write nothing.
__global__ __launch_bounds__(256) void prop_edge_bwd_kernel(TdPropLayer L, const float *__restrict__ W2Tf, const float *__restrict__ x,
                                                            const int32_t *__restrict__ nbr, int k, const float *__restrict__ P,
                                                            const float *__restrict__ dmi, int64_t N, float coeff,
                                                            float *__restrict__ Ae, float *__restrict__ DZ2, float *__restrict__ DZ1,
                                                            float *__restrict__ RBF, float *__restrict__ Q, float *__restrict__ S,
                                                            float *__restrict__ DWP) {
    __shared__ __attribute__((aligned(16))) float lds[4 * 16 * PE_STRIDE];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int lo = lane & 15, g = lane >> 4;
    float *act = lds + wid * 16 * PE_STRIDE;
    const float4 *W1f = reinterpret_cast<const float4 *>(L.W1f);
    const float4 *W2f = reinterpret_cast<const float4 *>(L.W2f);
    const float4 *WTf = reinterpret_cast<const float4 *>(W2Tf);          // edge_mlp.net.2 transposed, same fragment layout
    const int nblk = (k + 15) / 16;
    const float binf = L.binf[0];
    for (int64_t base = (int64_t)blockIdx.x * 4; base < N; base += (int64_t)gridDim.x * 4) {
        const bool live = base + wid < N;
        const int64_t i = live ? base + wid : N - 1;
        const float xi0 = x[i * 3], xi1 = x[i * 3 + 1], xi2 = x[i * 3 + 2];
        floatx4_t accs[POT], accw[POT];
#pragma unroll
        for (int ot = 0; ot < POT; ++ot) accs[ot] = accw[ot] = floatx4_t{0.f, 0.f, 0.f, 0.f};
        for (int eb = 0; eb < nblk; ++eb) {
            const int slot = 16 * eb + lo;
            const int j = slot < k ? nbr[i * k + slot] : -1;
            const bool valid = j >= 0;
            const bool store = live && slot < k;
            const int64_t e = i * k + slot;
            const int64_t jj = valid ? j : i;
            const float dx = xi0 - x[jj * 3], dy = xi1 - x[jj * 3 + 1], dz = xi2 - x[jj * 3 + 2];
            const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
            float rbf[4][4];
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float t = d - L.offset[16 * kb + 4 * g + r];
                    rbf[kb][r] = expf(coeff * (t * t));
                }
                if (store) {
                    const float4 v = valid ? float4{rbf[kb][0], rbf[kb][1], rbf[kb][2], rbf[kb][3]} : float4{0.f, 0.f, 0.f, 0.f};
                    *reinterpret_cast<float4 *>(RBF + e * TD_PROP_G + 16 * kb + 4 * g) = v;
                }
            }
            // ---- recompute a = ReLU(z1) (as prop_edge_kernel) -> LDS and Ae --------------------------------------------------
#pragma unroll 4
            for (int ot = 0; ot < POT; ++ot) {
                floatx4_t a = floatx4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kb = 0; kb < 4; ++kb) {
                    const float4 w = W1f[(ot * 4 + kb) * 64 + lane];
                    a = pb_mfma16(w.x, rbf[kb][0], a);
                    a = pb_mfma16(w.y, rbf[kb][1], a);
                    a = pb_mfma16(w.z, rbf[kb][2], a);
                    a = pb_mfma16(w.w, rbf[kb][3], a);
                }
                const float4 pi = *reinterpret_cast<const float4 *>(P + (size_t)i * (2 * PH) + 16 * ot + 4 * g);
                const float4 pj = *reinterpret_cast<const float4 *>(P + (size_t)jj * (2 * PH) + PH + 16 * ot + 4 * g);
                float4 v;
                v.x = fmaxf(a[0] + (pi.x + pj.x), 0.f);
                v.y = fmaxf(a[1] + (pi.y + pj.y), 0.f);
                v.z = fmaxf(a[2] + (pi.z + pj.z), 0.f);
                v.w = fmaxf(a[3] + (pi.w + pj.w), 0.f);
                *reinterpret_cast<float4 *>(act + lo * PE_STRIDE + 16 * ot + 4 * g) = v;
                if (store) *reinterpret_cast<float4 *>(Ae + e * PH + 16 * ot + 4 * g) = v;
            }
            __syncthreads();
            // ---- recompute m = ReLU(W2 a + b2) -------------------------------------------------------------------------------
            floatx4_t m[POT];
#pragma unroll
            for (int ot = 0; ot < POT; ++ot) m[ot] = floatx4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
            for (int hb = 0; hb < POT; ++hb) {
                const float4 av = *reinterpret_cast<const float4 *>(act + lo * PE_STRIDE + 16 * hb + 4 * g);
#pragma unroll
                for (int ot = 0; ot < POT; ++ot) {
                    const float4 w = W2f[(ot * POT + hb) * 64 + lane];
                    m[ot] = pb_mfma16(w.x, av.x, m[ot]);
                    m[ot] = pb_mfma16(w.y, av.y, m[ot]);
                    m[ot] = pb_mfma16(w.z, av.z, m[ot]);
                    m[ot] = pb_mfma16(w.w, av.w, m[ot]);
                }
            }
            __syncthreads();                                                  // act is rewritten with dz2 below
            float part = 0.f, qpart = 0.f;
#pragma unroll
            for (int ot = 0; ot < POT; ++ot) {
                const float4 bv = *reinterpret_cast<const float4 *>(L.b2 + 16 * ot + 4 * g);
                const float4 wv = *reinterpret_cast<const float4 *>(L.winf + 16 * ot + 4 * g);
                const float4 dv = *reinterpret_cast<const float4 *>(dmi + (size_t)i * PH + 16 * ot + 4 * g);
                m[ot][0] = fmaxf(m[ot][0] + bv.x, 0.f);
                m[ot][1] = fmaxf(m[ot][1] + bv.y, 0.f);
                m[ot][2] = fmaxf(m[ot][2] + bv.z, 0.f);
                m[ot][3] = fmaxf(m[ot][3] + bv.w, 0.f);
                part = fmaf(wv.x, m[ot][0], part);
                part = fmaf(wv.y, m[ot][1], part);
                part = fmaf(wv.z, m[ot][2], part);
                part = fmaf(wv.w, m[ot][3], part);
                qpart = fmaf(dv.x, m[ot][0], qpart);
                qpart = fmaf(dv.y, m[ot][1], qpart);
                qpart = fmaf(dv.z, m[ot][2], qpart);
                qpart = fmaf(dv.w, m[ot][3], qpart);
            }
            const float s = pb_sum_groups(part) + binf;
            const float ge = valid ? 1.0f / (1.0f + expf(-s)) : 0.f;
            const float q = valid ? pb_sum_groups(qpart) * (ge * (1.0f - ge)) : 0.f;
            if (store && g == 0) Q[e] = q;
            // ---- dz2 = (g dmi + q w) * [m > 0] -> LDS and DZ2; sum_e q m --------------------------------------------------------
#pragma unroll
            for (int ot = 0; ot < POT; ++ot) {
                const float4 wv = *reinterpret_cast<const float4 *>(L.winf + 16 * ot + 4 * g);
                const float4 dv = *reinterpret_cast<const float4 *>(dmi + (size_t)i * PH + 16 * ot + 4 * g);
                float4 v;
                v.x = (valid && m[ot][0] > 0.f) ? fmaf(ge, dv.x, q * wv.x) : 0.f;
                v.y = (valid && m[ot][1] > 0.f) ? fmaf(ge, dv.y, q * wv.y) : 0.f;
                v.z = (valid && m[ot][2] > 0.f) ? fmaf(ge, dv.z, q * wv.z) : 0.f;
                v.w = (valid && m[ot][3] > 0.f) ? fmaf(ge, dv.w, q * wv.w) : 0.f;
                accw[ot][0] = fmaf(q, m[ot][0], accw[ot][0]);
                accw[ot][1] = fmaf(q, m[ot][1], accw[ot][1]);
                accw[ot][2] = fmaf(q, m[ot][2], accw[ot][2]);
                accw[ot][3] = fmaf(q, m[ot][3], accw[ot][3]);
                *reinterpret_cast<float4 *>(act + lo * PE_STRIDE + 16 * ot + 4 * g) = v;
                if (store) *reinterpret_cast<float4 *>(DZ2 + e * PH + 16 * ot + 4 * g) = v;
            }
            __syncthreads();
            // ---- da = W2^T dz2 (MFMA); dz1 = da * [a > 0] -----------------------------------------------------------------------
#pragma unroll
            for (int ot = 0; ot < POT; ++ot) m[ot] = floatx4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
            for (int hb = 0; hb < POT; ++hb) {
                const float4 av = *reinterpret_cast<const float4 *>(act + lo * PE_STRIDE + 16 * hb + 4 * g);
#pragma unroll
                for (int ot = 0; ot < POT; ++ot) {
                    const float4 w = WTf[(ot * POT + hb) * 64 + lane];
                    m[ot] = pb_mfma16(w.x, av.x, m[ot]);
                    m[ot] = pb_mfma16(w.y, av.y, m[ot]);
                    m[ot] = pb_mfma16(w.z, av.z, m[ot]);
                    m[ot] = pb_mfma16(w.w, av.w, m[ot]);
                }
            }
            __syncthreads();                                                  // act is rewritten by the next block
#pragma unroll
            for (int ot = 0; ot < POT; ++ot) {
                // a > 0 exactly where z1 > 0; this lane wrote these four values of Ae itself above
                float4 av = float4{0.f, 0.f, 0.f, 0.f};
                if (store) av = *reinterpret_cast<const float4 *>(Ae + e * PH + 16 * ot + 4 * g);
                float4 v;
                v.x = (valid && av.x > 0.f) ? m[ot][0] : 0.f;
                v.y = (valid && av.y > 0.f) ? m[ot][1] : 0.f;
                v.z = (valid && av.z > 0.f) ? m[ot][2] : 0.f;
                v.w = (valid && av.w > 0.f) ? m[ot][3] : 0.f;
                accs[ot][0] += v.x;
                accs[ot][1] += v.y;
                accs[ot][2] += v.z;
                accs[ot][3] += v.w;
                if (store) *reinterpret_cast<float4 *>(DZ1 + e * PH + 16 * ot + 4 * g) = v;
            }
        }
#pragma unroll
        for (int ot = 0; ot < POT; ++ot) {
            float4 o, w;
            o.x = pb_sum16(accs[ot][0]);
            o.y = pb_sum16(accs[ot][1]);
            o.z = pb_sum16(accs[ot][2]);
            o.w = pb_sum16(accs[ot][3]);
            w.x = pb_sum16(accw[ot][0]);
            w.y = pb_sum16(accw[ot][1]);
            w.z = pb_sum16(accw[ot][2]);
            w.w = pb_sum16(accw[ot][3]);
            if (live && lo == 0) {
                *reinterpret_cast<float4 *>(S + (size_t)i * PH + 16 * ot + 4 * g) = o;
                *reinterpret_cast<float4 *>(DWP + (size_t)i * PH + 16 * ot + 4 * g) = w;
            }
        }
    }
}

// ---- reverse adjacency: for every source node j, the edges e = i * k + slot with nbr[i][slot] == j, ascending e
__global__ void prop_radj_count_kernel(const int32_t *__restrict__ nbr, int64_t E, int32_t *__restrict__ cnt) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int32_t j = nbr[e];
    if (j >= 0) atomicAdd(cnt + j, 1);                         // integer: the counts do not depend on the order
}

// exclusive prefix sum of cnt[0..N) -> ptr[0..N], one workgroup of 1024 threads, each over a contiguous run; cnt is reset to 0
__global__ __launch_bounds__(1024) void prop_radj_scan_kernel(int32_t *__restrict__ cnt, int64_t N, int32_t *__restrict__ ptr) {
    __shared__ int32_t tot[1024];
    const int t = threadIdx.x;
    const int64_t per = (N + 1023) / 1024;
    const int64_t a = t * per, b = a + per < N ? a + per : N;
    int32_t s = 0;
    for (int64_t n = a; n < b; ++n) s += cnt[n];
    tot[t] = s;
    __syncthreads();
    if (t == 0) {
        int32_t run = 0;
        for (int u = 0; u < 1024; ++u) { const int32_t v = tot[u]; tot[u] = run; run += v; }
        ptr[N] = run;
    }
    __syncthreads();
    int32_t run = tot[t];
    for (int64_t n = a; n < b; ++n) { ptr[n] = run; run += cnt[n]; cnt[n] = 0; }
}

__global__ void prop_radj_fill_kernel(const int32_t *__restrict__ nbr, int64_t E, const int32_t *__restrict__ ptr,
                                      int32_t *__restrict__ fill, int32_t *__restrict__ idx) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int32_t j = nbr[e];
    if (j >= 0) idx[ptr[j] + atomicAdd(fill + j, 1)] = (int32_t)e;
}

// the fill order above depends on timing: sort every node's list by edge index (insertion sort, one thread per node)
__global__ void prop_radj_sort_kernel(const int32_t *__restrict__ ptr, int64_t N, int32_t *__restrict__ idx) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const int32_t a = ptr[j], b = ptr[j + 1];
    for (int32_t u = a + 1; u < b; ++u) {
        const int32_t v = idx[u];
        int32_t w = u - 1;
        while (w >= a && idx[w] > v) { idx[w + 1] = idx[w]; --w; }
        idx[w + 1] = v;
    }
}

// out[j][c] = sum over u in ptr[j] .. ptr[j+1] (ascending) of X[idx[u]][c]; a workgroup of 256 threads per node
__global__ void prop_gather_kernel(const float *__restrict__ X, const int32_t *__restrict__ ptr, const int32_t *__restrict__ idx,
                                   float *__restrict__ out) {
    const int64_t j = blockIdx.x;
    const int c = threadIdx.x;
    float s = 0.f;
    for (int32_t u = ptr[j]; u < ptr[j + 1]; ++u) s += X[(size_t)idx[u] * PH + c];
    out[j * PH + c] = s;
}

// dy[b][c] = gout[b] if c == kind[b] - 1 else 0 (the one-hot select), or dy = gout when kind is null
__global__ void prop_select_bwd_kernel(const float *__restrict__ gout, const int64_t *__restrict__ kind, int O, float *__restrict__ dy,
                                       int64_t B) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= B * O) return;
    const int64_t b = u / O, c = u % O;
    dy[u] = kind ? (c == kind[b] - 1 ? gout[b] : 0.f) : gout[u];
}

// segment sum backward: dh[r] = dpre[b] (first 256 columns of a row of width ldp) for every composed row r of complex b
__global__ void prop_broadcast_kernel(const float *__restrict__ dpre, const int32_t *__restrict__ node_ptr, float *__restrict__ dh) {
    const int64_t b = blockIdx.x;
    const int32_t r0 = node_ptr[b], r1 = node_ptr[b + 1];
    for (int64_t u = threadIdx.x; u < (int64_t)(r1 - r0) * PH; u += blockDim.x)
        dh[(r0 + u / PH) * PH + u % PH] = dpre[b * PH + u % PH];
}

// compose backward: composed row r of complex b -> its protein row or its ligand row
__global__ void prop_uncompose_kernel(const float *__restrict__ dh, const int32_t *__restrict__ protein_ptr,
                                      const int32_t *__restrict__ ligand_ptr, float *__restrict__ dhp, float *__restrict__ dhl) {
    const int64_t b = blockIdx.x;
    const int32_t p0 = protein_ptr[b], p1 = protein_ptr[b + 1], l0 = ligand_ptr[b], l1 = ligand_ptr[b + 1];
    const int64_t base = (int64_t)p0 + l0, np = p1 - p0, n = np + (l1 - l0);
    for (int64_t u = threadIdx.x; u < n * PH; u += blockDim.x) {
        const int64_t r = u / PH, c = u % PH;
        const float v = dh[(base + r) * PH + c];
        if (r < np) dhp[(p0 + r) * PH + c] = v;
        else dhl[(l0 + r - np) * PH + c] = v;
    }
}

// W [rows][ld] (or its transpose when trans) -> 16x16x4 A fragments [ot][kb][lane] x 4 r, as pack_A_frag of prop_api.cpp
__global__ void prop_pack_afrag_kernel(const float *__restrict__ W, int ld, int col0, int kb_count, int trans, float *__restrict__ out) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)POT * kb_count * 64 * 4;
    if (u >= total) return;
    const int r = (int)(u % 4), lane = (int)((u / 4) % 64), kb = (int)((u / 256) % kb_count), ot = (int)(u / (256 * kb_count));
    const int row = 16 * ot + (lane & 15), col = col0 + 16 * kb + 4 * (lane >> 4) + r;
    out[u] = trans ? W[(size_t)col * ld + row] : W[(size_t)row * ld + col];
}

}  // namespace

int td_launch_prop_bgemm(const float *X1, int ldx1, int K1, const float *X2, int ldx2, int K2, const float *W, int ldw, int trans,
                         const float *M, int ldm, int epi, const float *R1, int ldr1, const float *R2, int ldr2, float *Y, int ldy,
                         int64_t N, int O, hipStream_t s) {
    if (N == 0 || O == 0) return TD_OK;
    const dim3 grid((unsigned)((N + 15) / 16), (unsigned)((O + 255) / 256));
    prop_bgemm_kernel<<<grid, dim3(256), 0, s>>>(X1, ldx1, K1, X2, ldx2, K2, W, ldw, trans, M, ldm, epi, R1, ldr1, R2, ldr2, Y, ldy, N, O);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

int td_prop_xty_chunks(int64_t N) {
    const int64_t c = (N + 1023) / 1024;
    return c < 1 ? 1 : c > TD_PROP_XTY_CHUNKS ? TD_PROP_XTY_CHUNKS : (int)c;
}

int td_launch_prop_xty(const float *A, int lda, int O, const float *B1, int ldb1, int K1, const float *B2, int ldb2, int K2, int64_t N,
                       float *part, float *G, int ldg, int col0, hipStream_t s) {
    const int K = B1 ? K1 + K2 : 1;
    if (O == 0 || K == 0) return TD_OK;
    const int chunks = td_prop_xty_chunks(N);
    int64_t per = (N + chunks - 1) / chunks;
    per = (per + 3) / 4 * 4;
    const dim3 grid((unsigned)(((O + 63) / 64) * ((K + 63) / 64)), (unsigned)chunks);
    prop_xty_kernel<<<grid, dim3(256), 0, s>>>(A, lda, O, B1, ldb1, K1, B2, ldb2, K2, N, per, part);
    TD_CHECK_HIP(hipGetLastError());
    const int64_t total = (int64_t)O * K;
    prop_reduce_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(part, chunks, O, K, G, ldg, col0);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

int td_launch_prop_edge_bwd(const TdPropLayer &L, const float *W2Tf, const float *x, const int32_t *nbr, int k, const float *P,
                            const float *dmi, int64_t N, float coeff, float *Ae, float *DZ2, float *DZ1, float *RBF, float *Q, float *S,
                            float *DWP, hipStream_t s) {
    if (N == 0) return TD_OK;
    int64_t g = (N + 3) / 4;
    if (g > 4096) g = 4096;
    prop_edge_bwd_kernel<<<dim3((unsigned)g), dim3(256), 0, s>>>(L, W2Tf, x, nbr, k, P, dmi, N, coeff, Ae, DZ2, DZ1, RBF, Q, S, DWP);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

int td_launch_prop_radj(const int32_t *nbr, int64_t N, int k, int32_t *cnt, int32_t *ptr, int32_t *idx, hipStream_t s) {
    if (N == 0) return TD_OK;
    const int64_t E = N * k;
    TD_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)N * sizeof(int32_t), s));
    prop_radj_count_kernel<<<dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s>>>(nbr, E, cnt);
    TD_CHECK_HIP(hipGetLastError());
    prop_radj_scan_kernel<<<dim3(1), dim3(1024), 0, s>>>(cnt, N, ptr);
    TD_CHECK_HIP(hipGetLastError());
    prop_radj_fill_kernel<<<dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s>>>(nbr, E, ptr, cnt, idx);
    TD_CHECK_HIP(hipGetLastError());
    prop_radj_sort_kernel<<<dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s>>>(ptr, N, idx);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

int td_launch_prop_gather(const float *X, const int32_t *ptr, const int32_t *idx, float *out, int64_t N, hipStream_t s) {
    if (N == 0) return TD_OK;
    prop_gather_kernel<<<dim3((unsigned)N), dim3(PH), 0, s>>>(X, ptr, idx, out);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

int td_launch_prop_select_bwd(const float *gout, const int64_t *kind, int O, float *dy, int64_t B, hipStream_t s) {
    if (B == 0) return TD_OK;
    prop_select_bwd_kernel<<<dim3((unsigned)((B * O + 255) / 256)), dim3(256), 0, s>>>(gout, kind, O, dy, B);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

int td_launch_prop_broadcast(const float *dpre, const int32_t *node_ptr, float *dh, int64_t B, hipStream_t s) {
    if (B == 0) return TD_OK;
    prop_broadcast_kernel<<<dim3((unsigned)B), dim3(256), 0, s>>>(dpre, node_ptr, dh);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

int td_launch_prop_uncompose(const float *dh, const int32_t *protein_ptr, const int32_t *ligand_ptr, float *dhp, float *dhl, int64_t B,
                             hipStream_t s) {
    if (B == 0) return TD_OK;
    prop_uncompose_kernel<<<dim3((unsigned)B), dim3(256), 0, s>>>(dh, protein_ptr, ligand_ptr, dhp, dhl);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

int td_launch_prop_pack_afrag(const float *W, int ld, int col0, int kb_count, int trans, float *out, hipStream_t s) {
    const int64_t total = (int64_t)POT * kb_count * 64 * 4;
    prop_pack_afrag_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(W, ld, col0, kb_count, trans, out);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}
