// Sample quality of ligand frames (gfx950; DESIGN.md section 3, "Sample quality").  Restates, per molecule, utils/evaluation/analyze.py
// check_stability (hs=False) and, per frame, the counts behind utils/evaluation/eval_bond_length.py get_pair_length_profile and the
// element Counter of scripts/evaluate_diffusion.py:80 -- all as integers:
//   * quality_kernel   one workgroup per (molecule, frame): nr_bonds per atom, stable atoms and the stable flag per molecule; for an
//                      included molecule its pairs i < j into the frame's pair-distance histograms and its atoms into the element counts
// The molecule passes through LDS as float4 (x, y, z, element) tiles of QL_TILE atoms.  A lane owns atom i and walks every j of the
// tile: both (i, j) and (j, i) are evaluated, by the same operations on the same squares, so nr_bonds needs no atomic; only j > i
// enters a histogram.  The distance is float64 on the widened fp32 coordinates with every product and sum rounded on its own (numpy's
// order: ((dx dx + dy dy) + dz dz), IEEE sqrt, 100 d), so an order flips exactly where the reference's flips.  Histograms and counts
// are 64-bit integer LDS atomics inside the workgroup and one integer global atomic per non-empty bin at its end: every output is
// independent of the grid and of the order of arrival, and there is no floating-point atomic anywhere.
#include "td_bond_rule.h"
#include "td_device.h"
#include "td_internal.h"

constexpr int QL_TILE = 256;        // atoms per LDS tile (4 KiB) = lanes per workgroup
constexpr int QL_THREADS = QL_TILE;
constexpr int QL_BINS = TD_QUALITY_BINS, QL_MAXP = TD_QUALITY_MAX_PROFILES;

// the bonds an element may hold (H C N O F P S Cl); the bond-length tables and the order of a pair: td_bond_rule.h
__constant__ const int8_t QL_ALLOWED[8] = {1, 4, 3, 2, 1, 5, 4, 1};

__global__ __launch_bounds__(QL_THREADS) void quality_kernel(TdQualityArgs a) {
    __shared__ float4 s_at[QL_TILE];
    __shared__ double s_thr[3][64];                    // bond length + margin per order and element pair
    __shared__ double s_edges[QL_MAXP][QL_BINS];
    __shared__ unsigned long long s_hist[QL_MAXP][QL_BINS];
    __shared__ unsigned long long s_cnt[8];
    __shared__ int s_elem[TD_QUALITY_MAX_CLASSES];
    __shared__ int s_stable;
    const int tid = threadIdx.x;
    const int s = blockIdx.x / a.B, g = blockIdx.x - s * a.B;
    const int l0 = a.lptr[g], n = a.lptr[g + 1] - l0;
    const bool inc = !a.include || a.include[(size_t)s * a.B + g] != 0;          // workgroup-uniform
    const int P = inc ? a.P : 0;
    td_bond_thresholds(s_thr, tid, QL_THREADS);
    if (tid < TD_QUALITY_MAX_CLASSES) s_elem[tid] = tid < a.K ? a.elem[tid] : -1;
    if (tid < 8) s_cnt[tid] = 0ull;
    if (tid == 0) s_stable = 0;
#pragma unroll
    for (int p = 0; p < QL_MAXP; ++p) {
        if (p < P) {
            for (int k = tid; k < QL_BINS; k += QL_THREADS) {
                s_hist[p][k] = 0ull;
                s_edges[p][k] = k < a.n_edges[p] ? a.edges[p][k] : 0.0;
            }
        }
    }
    __syncthreads();
    const float *pos = a.pos + (size_t)s * (size_t)a.Nl * 3;
    const int64_t *v = a.v + (size_t)s * (size_t)a.Nl;
    for (int c0 = 0; c0 < n; c0 += QL_THREADS) {              // workgroup-uniform
        const int i = c0 + tid;
        const bool have = i < n;
        double xi = 0.0, yi = 0.0, zi = 0.0;
        int ei = -1;
        if (have) {
            const size_t o = (size_t)(l0 + i) * 3;
            xi = (double)pos[o]; yi = (double)pos[o + 1]; zi = (double)pos[o + 2];
            const int64_t c = v[(size_t)(l0 + i)];
            ei = (c >= 0 && c < a.K) ? s_elem[(int)c] : -1;   // a class outside the table: no element, bonds with nothing
        }
        int nb = 0;
        for (int t0 = 0; t0 < n; t0 += QL_TILE) {
            const int m = n - t0 < QL_TILE ? n - t0 : QL_TILE;
            __syncthreads();                                  // the previous tile's readers are done
            if (tid < m) {
                const size_t o = (size_t)(l0 + t0 + tid) * 3;
                const int64_t c = v[(size_t)(l0 + t0 + tid)];
                const int e = (c >= 0 && c < a.K) ? s_elem[(int)c] : -1;
                s_at[tid] = make_float4(pos[o], pos[o + 1], pos[o + 2], __int_as_float(e));
            }
            __syncthreads();
            if (have && ei >= 0) {
                for (int jj = 0; jj < m; ++jj) {
                    const int j = t0 + jj;
                    const float4 q = s_at[jj];                // every lane reads the same address: an LDS broadcast
                    const int ej = __float_as_int(q.w);
                    if (j == i || ej < 0) continue;
                    double d;
                    nb += td_bond_order(xi, yi, zi, q.x, q.y, q.z, ei * 8 + ej, s_thr, d);
                    if (j > i) {
#pragma unroll
                        for (int p = 0; p < QL_MAXP; ++p) {
                            if (p < P) {
                                const int e1 = a.pe1[p], e2 = a.pe2[p];
                                const bool match = ((e1 < 0 || ei == e1) && (e2 < 0 || ej == e2)) || ((e1 < 0 || ej == e1) && (e2 < 0 || ei == e2));
                                if (match && d < a.cutoff[p]) atomicAdd(&s_hist[p][td_searchsorted_left(s_edges[p], a.n_edges[p], d)], 1ull);
                            }
                        }
                    }
                }
            }
        }
        if (have) {
            if (a.nr_bonds) a.nr_bonds[(size_t)s * (size_t)a.Nl + (size_t)(l0 + i)] = nb;
            if (ei >= 0) {
                if (nb > 0 && nb <= QL_ALLOWED[ei]) atomicAdd(&s_stable, 1);
                if (inc) atomicAdd(&s_cnt[ei], 1ull);
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int st = s_stable;
        a.stable_atoms[(size_t)s * a.B + g] = st;
        a.mol_stable[(size_t)s * a.B + g] = st == n ? 1 : 0;          // 0 atoms: stable; 1 atom: no partner, not stable
    }
    if (inc) {
        if (tid < 8 && s_cnt[tid]) atomicAdd(&a.counts[(size_t)s * 8 + tid], s_cnt[tid]);
#pragma unroll
        for (int p = 0; p < QL_MAXP; ++p) {
            if (p < P) {
                for (int k = tid; k < QL_BINS; k += QL_THREADS) {
                    const unsigned long long c = s_hist[p][k];
                    if (c) atomicAdd(&a.hist[((size_t)s * a.P + p) * QL_BINS + k], c);
                }
            }
        }
    }
}

int td_launch_quality(const TdQualityArgs &a, hipStream_t s) {
    if (a.S == 0) return TD_OK;
    if (a.P > 0) TD_CHECK_HIP(hipMemsetAsync(a.hist, 0, (size_t)a.S * a.P * QL_BINS * sizeof(unsigned long long), s));
    TD_CHECK_HIP(hipMemsetAsync(a.counts, 0, (size_t)a.S * 8 * sizeof(unsigned long long), s));
    if (a.B == 0) return TD_OK;
    quality_kernel<<<dim3((unsigned)((int64_t)a.S * a.B)), dim3(QL_THREADS), 0, s>>>(a);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}
