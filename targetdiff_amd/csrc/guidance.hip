// Pocket-clash guidance (gfx950; DESIGN.md section 3, "Clash guidance"; no seam in the reference, which has no such mode).
//   * clash_kernel<SHIFT>   per ligand atom  D_i = w sum_j max(0, sigma_j - d_ij) (x0_i - p_j) / d_ij  over the graph's protein atoms,
//                           capped to length max_shift: the shift the guided posterior step adds to the denoiser's predicted x0
//   * clash_kernel<REPORT>  per graph: pairs with d_ij < sigma_j, E_g = 1/2 sum max(0, sigma_j - d_ij)^2, min d_ij
//   * clash_pack_kernel     a session's centred protein rows + the caller's radii as float4 (x, y, z, sigma)
// One workgroup of four waves per graph.  The graph's protein atoms pass through LDS as float4 (x, y, z, sigma) tiles of CG_TILE atoms; a
// wave owns one ligand atom per round (atom = round * 4 + wave), its 64 lanes stride over the tile's atoms and keep their partial sums in
// registers across tiles, and one fixed-order wave reduction (td_sum64: DPP inside a row of 16, then the two permlane swaps) closes the
// atom.  A lane's partial is a sum over j = lane, lane + 64, ... of its own graph's protein atoms in index order, so an atom's result
// depends on its graph alone -- not on the batch around it, not on the grid -- and there is no floating-point atomic anywhere.
// With a protein of more than one tile the tiles are staged again for every round (from L2: a round reads N_p float4); a pocket of the C2
// shape (about 570 atoms) is one tile, staged once.
#include "td_device.h"
#include "td_internal.h"

constexpr int CG_TILE = TD_CLASH_TILE;      // protein atoms per LDS tile: 16 KiB
constexpr int CG_WAVES = 4;
constexpr int CG_SHIFT = 0, CG_REPORT = 1;

template <int MODE>
__global__ __launch_bounds__(CG_WAVES * 64) void clash_kernel(TdClashArgs a, float *__restrict__ shift, int32_t *__restrict__ count,
                                                              float *__restrict__ energy, float *__restrict__ min_dist) {
    __shared__ float4 s_p[CG_TILE];
    __shared__ int s_cnt[CG_WAVES];
    __shared__ double s_en[CG_WAVES];
    __shared__ float s_mn[CG_WAVES];
    const int g = blockIdx.x;
    const int p0 = a.pptr[g], np = a.pptr[g + 1] - p0, l0 = a.lptr[g], nl = a.lptr[g + 1] - l0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // model_mean_type 'noise' inside a session step: x0 comes from the network's output and x_t at the graph's time step, by the device
    // function the posterior kernel uses (td_x0_of_output); the step index is read, never advanced, here
    int t = 0;
    if (a.mean_type == 1) {
        int s = *reinterpret_cast<const volatile int32_t *>(a.step);
        s = s < 0 ? 0 : (s >= a.num_steps ? a.num_steps - 1 : s);
        t = a.t_all[(size_t)s * a.B + g];
        t = t < 0 ? 0 : (t >= a.T ? a.T - 1 : t);
    }
    const int ntiles = (np + CG_TILE - 1) / CG_TILE;
    const int rounds = (nl + CG_WAVES - 1) / CG_WAVES;
    int cnt = 0;
    double en = 0.0;
    float mn = INFINITY;
    for (int r = 0; r < rounds; ++r) {
        const int i = r * CG_WAVES + wave;
        const bool have = i < nl;                     // wave-uniform
        float x = 0.f, y = 0.f, z = 0.f;
        if (have) {
            const size_t o = (size_t)(l0 + i) * 3;
            x = a.eval[o]; y = a.eval[o + 1]; z = a.eval[o + 2];
            if (a.mean_type == 1) {
                x = td_x0_of_output(a.rc, a.rm1, t, 1, x, a.xt[o]);
                y = td_x0_of_output(a.rc, a.rm1, t, 1, y, a.xt[o + 1]);
                z = td_x0_of_output(a.rc, a.rm1, t, 1, z, a.xt[o + 2]);
            }
        }
        float ax = 0.f, ay = 0.f, az = 0.f;
        for (int tl = 0; tl < ntiles; ++tl) {
            const int n = np - tl * CG_TILE < CG_TILE ? np - tl * CG_TILE : CG_TILE;
            if (ntiles > 1 || r == 0) {               // workgroup-uniform: one tile stays in LDS for every round
                __syncthreads();                      // the previous tile's readers are done
                for (int j = threadIdx.x; j < n; j += CG_WAVES * 64) {
                    const size_t pj = (size_t)p0 + (size_t)tl * CG_TILE + j;
                    s_p[j] = a.prot4 ? a.prot4[pj] : make_float4(a.ppos[pj * 3], a.ppos[pj * 3 + 1], a.ppos[pj * 3 + 2], a.sigma[pj]);
                }
                __syncthreads();
            }
            if (have) {
                for (int j = lane; j < n; j += 64) {
                    const float4 q = s_p[j];
                    if (MODE == CG_REPORT) {
                        // off the hot path (finished poses): fp64 throughout, so the count is the float64 count of the fp32 inputs
                        // and the energy is rounded once
                        const double ex = (double)x - (double)q.x, ey = (double)y - (double)q.y, ez = (double)z - (double)q.z;
                        const double dd = sqrt(ex * ex + ey * ey + ez * ez), pd = (double)q.w - dd;
                        mn = fminf(mn, (float)dd);
                        if (pd > 0.0) { ++cnt; en += 0.5 * pd * pd; }
                    } else {
                        const float dx = x - q.x, dy = y - q.y, dz = z - q.z;
                        // every product and sum spelled out: no contraction left to the compiler
                        const float d = sqrtf(fmaf(dz, dz, fmaf(dy, dy, td_mul_rn(dx, dx))));
                        const float pen = q.w - d;
                        if (pen > 0.f && d >= 1e-6f) {                // d < 1e-6: no direction, no contribution
                            const float f = pen / d;
                            ax = fmaf(f, dx, ax); ay = fmaf(f, dy, ay); az = fmaf(f, dz, az);
                        }
                    }
                }
            }
        }
        if (MODE == CG_SHIFT && have) {
            ax = td_sum64(ax); ay = td_sum64(ay); az = td_sum64(az);
            if (lane == 0) {
                float sx = td_mul_rn(a.w, ax), sy = td_mul_rn(a.w, ay), sz = td_mul_rn(a.w, az);
                if (a.max_shift > 0.f) {
                    const float nrm = sqrtf(fmaf(sz, sz, fmaf(sy, sy, td_mul_rn(sx, sx))));
                    if (nrm > a.max_shift) {
                        const float k = a.max_shift / nrm;
                        sx = td_mul_rn(sx, k); sy = td_mul_rn(sy, k); sz = td_mul_rn(sz, k);
                    }
                }
                const size_t o = (size_t)(l0 + i) * 3;
                shift[o] = sx; shift[o + 1] = sy; shift[o + 2] = sz;
            }
        }
    }
    if (MODE == CG_REPORT) {
        // lanes in a fixed butterfly, then the four waves in order
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            cnt += __shfl_xor(cnt, o);
            en += __shfl_xor(en, o);
            mn = fminf(mn, __shfl_xor(mn, o));
        }
        if (lane == 0) { s_cnt[wave] = cnt; s_en[wave] = en; s_mn[wave] = mn; }
        __syncthreads();
        if (threadIdx.x == 0) {
            int c = 0;
            double e = 0.0;
            float m = INFINITY;
            for (int wv = 0; wv < CG_WAVES; ++wv) { c += s_cnt[wv]; e += s_en[wv]; m = fminf(m, s_mn[wv]); }
            count[g] = c; energy[g] = (float)e; min_dist[g] = m;
        }
    }
}

int td_launch_clash_shift(const TdClashArgs &a, float *shift, hipStream_t s) {
    if (a.B == 0) return TD_OK;
    clash_kernel<CG_SHIFT><<<dim3((unsigned)a.B), dim3(CG_WAVES * 64), 0, s>>>(a, shift, nullptr, nullptr, nullptr);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

int td_launch_clash_report(const TdClashArgs &a, int32_t *count, float *energy, float *min_dist, hipStream_t s) {
    if (a.B == 0) return TD_OK;
    clash_kernel<CG_REPORT><<<dim3((unsigned)a.B), dim3(CG_WAVES * 64), 0, s>>>(a, nullptr, count, energy, min_dist);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

__global__ void clash_pack_kernel(const float4 *__restrict__ x4, const int32_t *__restrict__ prot_node, const float *__restrict__ sigma,
                                  int64_t Np, float4 *__restrict__ prot4) {
    const int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= Np) return;
    const float4 p = x4[prot_node[at]];
    prot4[at] = make_float4(p.x, p.y, p.z, sigma[at]);
}

int td_launch_clash_pack(const float4 *x4, const int32_t *prot_node, const float *sigma, int64_t Np, float4 *prot4, hipStream_t s) {
    if (Np == 0) return TD_OK;
    clash_pack_kernel<<<dim3((unsigned)((Np + 255) / 256)), dim3(256), 0, s>>>(x4, prot_node, sigma, Np, prot4);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}
