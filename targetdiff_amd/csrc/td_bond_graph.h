// What the kernels over the bond graph share (bonds.hip, rings.hip; DESIGN.md section 3, "Bond graph" and "Rings"): which molecule a
// workgroup has, the molecule in LDS, and the bit rows of the graph.  One copy, so that every kernel sees the same bonds.
#pragma once
#include "td_bond_rule.h"
#include "td_device.h"
#include "td_internal.h"

constexpr int BG_BINS = TD_BOND_BINS, BG_MAXP = TD_BOND_MAX_PROFILES, BG_SMALL = TD_BOND_SMALL_ATOMS, BG_MAX = TD_BOND_MAX_ATOMS;

// what a workgroup needs to know about its molecule; `mine`: this instantiation handles it
struct BgMol {
    int s, g, l0, n;
    size_t mol;
    bool bad, mine;
};

template <int MAXN>
__device__ __forceinline__ BgMol bg_molecule(const TdBondArgs &a) {
    BgMol m;
    m.s = blockIdx.x / a.B;
    m.g = blockIdx.x - m.s * a.B;
    m.l0 = a.lptr[m.g];
    const int l1 = a.lptr[m.g + 1];
    m.n = l1 - m.l0;
    m.mol = (size_t)m.s * a.B + m.g;
    m.bad = m.n > BG_MAX || (m.n > 0 && (m.l0 < 0 || (int64_t)l1 > a.Nl));
    const bool small = !m.bad && m.n <= BG_SMALL;             // n <= 0: an empty molecule, the small instantiation writes its zeros
    m.mine = (MAXN == BG_SMALL) == small;
    return m;
}

// The molecule into LDS, between the two barriers every kernel needs around it: the first publishes the class table, the thresholds and
// the kernel's own LDS initialisation, which each kernel writes just before, in the order its loads were measured in (a helper for the
// two table lines moves their loads in the ISA, EXPERIMENTS.md "Sample evaluation: one pack").  Atom tid as (x, y, z, code): code =
// element | aromatic << 8, or -1 for a class outside [0, K).
template <int MAXN>
__device__ __forceinline__ void bg_load(const TdBondArgs &a, const BgMol &m, const int *s_elem, float4 *s_at) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < m.n) {
        const size_t at = (size_t)m.s * (size_t)a.Nl + (size_t)(m.l0 + tid);
        const float *p = a.pos + at * 3;
        const int64_t c = a.v[at];
        int code = -1;
        if (c >= 0 && c < a.K) code = s_elem[(int)c] | ((int)((a.aromatic >> (int)c) & 1ull) << 8);
        s_at[tid] = make_float4(p[0], p[1], p[2], __int_as_float(code));
    }
    __syncthreads();
}

// category of a bond: its order, or 4 (aromatic) when both atoms' classes are aromatic and the order is 1 or 2
__device__ __forceinline__ int bg_category(int ci, int cj, int order) { return ((ci & cj) >> 8 & 1) && order <= 2 ? 4 : order; }

// The row of atom tid (< n): order > 0 with atom j sets bit j of s_row[w][tid] (word w of atom tid, so a wave's accesses are
// contiguous).  bond(j, cj, order, d) is called for every bond tid < j in ascending j; returns their number.
template <int MAXN, typename F>
__device__ __forceinline__ int bg_rows(int n, const float4 *s_at, const double (*s_thr)[64], unsigned long long (*s_row)[MAXN], F bond) {
    constexpr int W = MAXN / 64;
    const int tid = threadIdx.x;
    int up = 0;
    const float4 me = s_at[tid];
    const int ci = __float_as_int(me.w), ei = ci & 7;
    const double xi = (double)me.x, yi = (double)me.y, zi = (double)me.z;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        unsigned long long bits = 0ull;
        const int cnt = n - w * 64 < 64 ? n - w * 64 : 64;
        if (ci >= 0) {
            for (int jj = 0; jj < cnt; ++jj) {
                const int j = w * 64 + jj;
                const float4 q = s_at[j];                                   // every lane reads the same address: an LDS broadcast
                const int cj = __float_as_int(q.w), ej = cj & 7;
                if (j == tid || cj < 0) continue;
                double d;
                const int order = td_bond_order(xi, yi, zi, q.x, q.y, q.z, ei * 8 + ej, s_thr, d);
                if (order == 0) continue;
                bits |= 1ull << jj;
                if (j < tid) continue;
                ++up;
                bond(j, cj, order, d);
            }
        }
        s_row[w][tid] = bits;
    }
    return up;
}

// The workgroup's LDS histogram of n bins added to the global one: one integer atomic per non-empty bin
template <int MAXN>
__device__ __forceinline__ void bg_flush_hist(const unsigned int *s_hist, int n, unsigned long long *hist) {
    for (int k = threadIdx.x; k < n; k += MAXN) {
        const unsigned int c = s_hist[k];
        if (c) atomicAdd(&hist[k], (unsigned long long)c);
    }
}

// Inclusive scan of s_off[0 .. MAXN) by the whole workgroup (the per-atom counts of bonds tid < j: s_off[tid] - own count is the offset
// of atom tid's first bond within the molecule).  A barrier precedes it at the caller; one follows the last step.
template <int MAXN>
__device__ __forceinline__ void bg_scan(int *s_off) {
    const int tid = threadIdx.x;
    for (int d = 1; d < MAXN; d <<= 1) {
        const int t = tid >= d ? s_off[tid - d] : 0;
        __syncthreads();
        s_off[tid] += t;
        __syncthreads();
    }
}

// Both instantiations of a kernel over the M > 0 (frame, molecule) workgroups: each takes the molecules of its own size
template <typename Args>
int bg_launch_pair(void (*small)(Args), void (*large)(Args), const Args &a, int64_t M, hipStream_t s) {
    small<<<dim3((unsigned)M), dim3(BG_SMALL), 0, s>>>(a);
    TD_CHECK_HIP(hipGetLastError());
    large<<<dim3((unsigned)M), dim3(BG_MAX), 0, s>>>(a);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}
