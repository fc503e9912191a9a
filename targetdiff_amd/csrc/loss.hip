// The diffusion loss of a ragged pack and the atom-type AUROC of a validation run (gfx950), forward only:
//   * diffusion_loss_kernel    the arithmetic of get_diffusion_loss after the network call  (models/molopt_score_model.py:521-563:
//                              pred_pos_noise :522, scatter_mean of the squared error :536-542, compute_v_Lt :546-550 = :476-483,
//                              softmax :562), one wave per graph like likelihood_terms_kernel, whose type term it shares (td_type_term.h)
//   * loss_mean_kernel         the means over the graphs and loss = loss_pos + loss_v_weight loss_v (:543, :551-552): one workgroup, a
//                              fixed tree over g -- no float atomics, the same bits whatever the grid of the first stage
//   * auroc_pairs_kernel       get_auroc (scripts/train_diffusion.py:22-36) as exact integers: per class the positives and twice the
//                              Mann-Whitney count of (positive, negative) pairs, ties counted once
#include "td_device.h"
#include "td_internal.h"
#include "td_type_term.h"

namespace {

constexpr int LOSS_MEAN_THREADS = 256;
constexpr int AUROC_TILE = 256;                 // atoms per workgroup on the positive side, rows per LDS tile on the other
constexpr int AUROC_STRIDE = TD_MAXC + 1;       // most fp32 per LDS row; a row holds C + 1 (see auroc_pairs_kernel for what the pad does and does not buy)
constexpr int64_t AUROC_MAX_N = 1 << 20;        // pairs2 < 2 N^2 = 2^41

__global__ __launch_bounds__(64) void diffusion_loss_kernel(TdSchedules sc, int T, int mean_type, const int32_t *__restrict__ tg,
                                                            const int32_t *__restrict__ lptr, int C, const float *__restrict__ x0,
                                                            const float *__restrict__ xt, const float *__restrict__ noise,
                                                            const int64_t *__restrict__ v0, const int64_t *__restrict__ vt,
                                                            const float *__restrict__ pred_pos, const float *__restrict__ pred_v,
                                                            float *__restrict__ pred_pos_noise, float *__restrict__ v_recon,
                                                            float *__restrict__ loss_pos_g, float *__restrict__ loss_v_g) {
    const int g = blockIdx.x, lane = threadIdx.x;
    int t = tg[g];
    t = t < 0 ? 0 : (t >= T ? T - 1 : t);
    const bool decoder = t == 0;
    const int b = lptr[g], e = lptr[g + 1];
    float acc_pos = 0.f, acc_v = 0.f;
    const float LOG_EPS = logf(1e-30f);
    for (int at = b + lane; at < e; at += 64) {
        // ---- positions: ((pred - target)^2).sum(-1); 'C0': x0 against the prediction, 'noise': the drawn against the predicted noise
        float sq = 0.f;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float pp = pred_pos[(int64_t)at * 3 + d];
            const float eps = td_add_rn(pp, -xt[(int64_t)at * 3 + d]);                  // pred_pos_noise (:522)
            pred_pos_noise[(int64_t)at * 3 + d] = eps;
            const float df = mean_type == 1 ? eps - noise[(int64_t)at * 3 + d] : pp - x0[(int64_t)at * 3 + d];
            sq += df * df;
        }
        acc_pos += sq;
        // ---- types: the term of likelihood_terms_kernel; softmax(pred_v) (:562) from the exponentials and the sum it has formed
        TD_TYPE_TERM(acc_v, sc, t, C, decoder, LOG_EPS, pred_v, v0, vt, at);
#pragma unroll
        for (int c = 0; c < TD_MAXC; ++c)
            if (c < C) v_recon[(int64_t)at * C + c] = tt_ex[c] / tt_se;
    }
    acc_pos = td_sum64(acc_pos);
    acc_v = td_sum64(acc_v);
    if (lane == 0) {
        const int cnt = e - b < 1 ? 1 : e - b;          // an empty graph: 0 / 1
        loss_pos_g[g] = acc_pos / (float)cnt;
        loss_v_g[g] = acc_v / (float)cnt;
    }
}

// scalars[0..2] = mean_g loss_pos_g, mean_g loss_v_g, loss_pos + w loss_v.  Thread k adds its graphs k, k + 256, ... in ascending order, then
// the 256 partial sums fold in halves: the order of every addition is a function of B alone.
__global__ __launch_bounds__(LOSS_MEAN_THREADS) void loss_mean_kernel(const float *__restrict__ loss_pos_g,
                                                                      const float *__restrict__ loss_v_g, int B, float w,
                                                                      float *__restrict__ scalars) {
    __shared__ float sp[LOSS_MEAN_THREADS], sv[LOSS_MEAN_THREADS];
    const int tid = threadIdx.x;
    float ap = 0.f, av = 0.f;
    for (int g = tid; g < B; g += LOSS_MEAN_THREADS) {
        ap += loss_pos_g[g];
        av += loss_v_g[g];
    }
    sp[tid] = ap;
    sv[tid] = av;
    __syncthreads();
    for (int h = LOSS_MEAN_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            sp[tid] += sp[tid + h];
            sv[tid] += sv[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float lp = sp[0] / (float)B, lv = sv[0] / (float)B;       // B == 0: nan, the mean of nothing
        scalars[0] = lp;
        scalars[1] = lv;
        scalars[2] = td_add_rn(lp, td_mul_rn(lv, w));
    }
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// Atom i is a positive of its own class c_i and of no other, so the pairs of all classes together are the N^2 ordered pairs (i, j) with
// label_j != c_i, compared on column c_i: lane = one i (c_i and s_i = scores[i][c_i] in registers), the rows j pass through LDS in tiles
// of 256 and every lane reads the same row at the same time (one LDS row per step, the lanes spread over its columns: at most C distinct
// words of one row, conflict-free at any stride).  The rows are C + 1 words apart, so that rows of 16 classes do not all start on one
// bank; with this mapping that pad is not needed -- it would be for a lane-per-row read of one column -- and the tile's writes, linear in
// k without it, spread over k + k / C with it, a few two-way conflicts per tile against 256 reads per lane.  Workgroup (x, y)
// takes the i of tile x against the j tiles y, y + gridDim.y, ...  Counts are integers: per lane, then per wave and class, then one atomic
// add per wave and class that has something to add -- the totals do not depend on the order.
__global__ __launch_bounds__(AUROC_TILE) void auroc_pairs_kernel(const float *__restrict__ scores, const int64_t *__restrict__ labels,
                                                                 int N, int C, unsigned long long *__restrict__ n_pos,
                                                                 unsigned long long *__restrict__ pairs2) {
    __shared__ float s_tile[AUROC_TILE * AUROC_STRIDE];
    __shared__ int l_tile[AUROC_TILE];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * AUROC_TILE + tid;
    int ci = -1;
    float si = 0.f;
    if (i < N) {
        const int64_t l = labels[i];
        if (l >= 0 && l < C) {                                      // a label outside [0, C) is in no class (a binding refuses it)
            ci = (int)l;
            si = scores[(int64_t)i * C + ci];
        }
    }
    const int col = ci < 0 ? 0 : ci;
    const int stride = C + 1;
    unsigned long long acc = 0;
    const int tiles = (N + AUROC_TILE - 1) / AUROC_TILE;
    for (int jt = blockIdx.y; jt < tiles; jt += gridDim.y) {
        const int j0 = jt * AUROC_TILE;
        const int rows = N - j0 < AUROC_TILE ? N - j0 : AUROC_TILE;
        __syncthreads();                                            // the previous tile is read out
        for (int k = tid; k < rows * C; k += AUROC_TILE) {
            const int r = k / C, c = k - r * C;
            s_tile[r * stride + c] = scores[(int64_t)j0 * C + k];
        }
        if (tid < rows) l_tile[tid] = (int)labels[j0 + tid];
        __syncthreads();
        unsigned int part = 0;                                      // at most 2 * 256 per tile
        for (int r = 0; r < rows; ++r) {
            const float sj = s_tile[r * stride + col];
            const unsigned int inc = si > sj ? 2u : (si == sj ? 1u : 0u);
            part += l_tile[r] != ci ? inc : 0u;
        }
        acc += part;
    }
    if (ci < 0) acc = 0;
    const unsigned long long one = ci >= 0 && blockIdx.y == 0 ? 1ull : 0ull;
    for (int c = 0; c < C; ++c) {                                   // wave-uniform trip count
        const unsigned long long p = wave_sum_u64(ci == c ? acc : 0ull);
        const unsigned long long n = wave_sum_u64(ci == c ? one : 0ull);
        if ((tid & 63) == 0) {
            if (p) atomicAdd(&pairs2[c], p);
            if (n) atomicAdd(&n_pos[c], n);
        }
    }
}

}  // namespace

// ---- C ABI (include/targetdiff_hip.h)
extern "C" int td_diffusion_loss(const td_model *m, const int32_t *d_t, const int32_t *d_ligand_ptr, int64_t N_l, int64_t B,
                                 const float *d_pos_0, const float *d_pos_t, const float *d_noise, const int64_t *d_v_0,
                                 const int64_t *d_v_t, const float *d_pred_pos, const float *d_pred_v, float loss_v_weight,
                                 float *d_pred_pos_noise, float *d_v_recon, float *d_loss_pos_graph, float *d_loss_v_graph,
                                 float *d_scalars, void *stream) {
    const char *who = "td_diffusion_loss";
    if (!m || N_l < 0 || B < 0 || N_l > 0x7fffffff / TD_MAXC || B > 0x7fffffff) {
        td_set_error("%s: bad argument (N_l = %lld, B = %lld)", who, (long long)N_l, (long long)B);
        return TD_EINVAL;
    }
    const int C = m->cfg.ligand_num_classes;
    if (C < 1 || C > TD_MAXC) { td_set_error("%s: %d classes, built for 1 .. %d", who, C, TD_MAXC); return TD_EINVAL; }
    if (!m->sched.abar) { td_set_error("%s: the model was created without alphas_cumprod (8 schedule arrays)", who); return TD_EINVAL; }
    const int mean_type = m->cfg.model_mean_type;
    if (mean_type == 1 && !d_noise) {
        td_set_error("%s: model_mean_type 'noise' needs d_noise, the draw x_t was made from", who);
        return TD_EINVAL;
    }
    if (!d_scalars || (B > 0 && (!d_t || !d_ligand_ptr || !d_loss_pos_graph || !d_loss_v_graph)) ||
        (N_l > 0 && (!d_pos_0 || !d_pos_t || !d_v_0 || !d_v_t || !d_pred_pos || !d_pred_v || !d_pred_pos_noise || !d_v_recon))) {
        td_set_error("%s: null pointer", who);
        return TD_EINVAL;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (B > 0) {
        diffusion_loss_kernel<<<dim3((unsigned)B), dim3(64), 0, s>>>(m->sched, m->cfg.num_timesteps, mean_type, d_t, d_ligand_ptr, C, d_pos_0,
                                                                    d_pos_t, d_noise, d_v_0, d_v_t, d_pred_pos, d_pred_v,
                                                                    d_pred_pos_noise, d_v_recon, d_loss_pos_graph, d_loss_v_graph);
        TD_CHECK_HIP(hipGetLastError());
    }
    loss_mean_kernel<<<dim3(1), dim3(LOSS_MEAN_THREADS), 0, s>>>(d_loss_pos_graph, d_loss_v_graph, (int)B, loss_v_weight, d_scalars);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

extern "C" int td_auroc(const float *d_scores, const int64_t *d_labels, int64_t N, int32_t C, int64_t *d_n_pos, int64_t *d_pairs2,
                        void *stream) {
    const char *who = "td_auroc";
    if (N < 0 || N > AUROC_MAX_N) {
        td_set_error("%s: N = %lld, the counts are built for 0 .. %lld rows", who, (long long)N, (long long)AUROC_MAX_N);
        return TD_EINVAL;
    }
    if (C < 1 || C > TD_MAXC) { td_set_error("%s: %d classes, built for 1 .. %d", who, (int)C, TD_MAXC); return TD_EINVAL; }
    if (!d_n_pos || !d_pairs2 || (N > 0 && (!d_scores || !d_labels))) { td_set_error("%s: null pointer", who); return TD_EINVAL; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    TD_CHECK_HIP(hipMemsetAsync(d_n_pos, 0, (size_t)C * sizeof(int64_t), s));
    TD_CHECK_HIP(hipMemsetAsync(d_pairs2, 0, (size_t)C * sizeof(int64_t), s));
    if (N == 0) return TD_OK;
    const int tiles = (int)((N + AUROC_TILE - 1) / AUROC_TILE);
    // enough workgroups to fill the device on a small N, at most one per pair of tiles
    int gy = tiles < 64 ? tiles : 64;
    while (gy > 1 && (int64_t)tiles * gy > 4096) gy >>= 1;
    auroc_pairs_kernel<<<dim3((unsigned)tiles, (unsigned)gy), dim3(AUROC_TILE), 0, s>>>(
        d_scores, d_labels, (int)N, (int)C, reinterpret_cast<unsigned long long *>(d_n_pos), reinterpret_cast<unsigned long long *>(d_pairs2));
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}
