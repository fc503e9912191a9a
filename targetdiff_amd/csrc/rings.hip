// Rings of ligand frames (gfx950, wave64; DESIGN.md section 3, "Rings"): per bond of the bond graph of bonds.hip the size of the
// smallest cycle through it, and what follows from that per atom, per molecule and per frame.
//   * ring_report_kernel  one workgroup per (frame, molecule), the molecule and its bit rows in LDS exactly as bond_graph_kernel
//                         builds them (td_bond_graph.h).  Lane i owns atom i and its bonds i < j in ascending j, the order of
//                         bond_list_kernel, so a workgroup scan of the per-atom counts puts the per-bond outputs at the offsets of
//                         td_bond_list.  Per bond a breadth-first search from i over the bit rows with the edge to j left out:
//                         visited / frontier / next are W = MAXN / 64 words each, indexed by unrolled compile-time indices only (they
//                         stay in registers); frontier bits are popped with __ffsll and the popped atoms' rows are ORed into next.
//                         Before a level is expanded the target is tested from its own side: j is reached at the next level exactly
//                         when row(j) & frontier is non-empty.  A triangle so costs W reads, and every search is spared its last and
//                         largest expansion.  The search starts one level in: the first frontier is row(i) without bit j, which is
//                         what expanding {i} with the edge masked gives.
// Every loop is bounded by the molecule's size (at most n levels, at most n pops per search), so a defect ends in a wrong number, not
// in a kernel that does not return.  Outputs are integers; integer LDS atomics for the counts, the mask and the per-atom minimum, one
// integer global atomic per set mask bit for ring_hist: nothing depends on the grid or on the order of arrival.  No floating point
// beyond td_bond_order.  The two instantiations and the answer to an oversize molecule (-1, -1, mask 0) are those of bonds.hip.
#include "td_bond_graph.h"

constexpr int RG_NONE = 0x7fffffff;

// Atoms of the smallest cycle through the bond (i, j): 1 + the shortest path from i to j without that edge; 0 when there is none.
template <int MAXN>
__device__ __forceinline__ int rg_bond_ring(const unsigned long long (*s_row)[MAXN], int n, int i, int j) {
    constexpr int W = MAXN / 64;
    unsigned long long vis[W], fr[W], nx[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        unsigned long long f = s_row[w][i];
        if (w == (j >> 6)) f &= ~(1ull << (j & 63));                            // the edge itself is left out
        fr[w] = f;
        vis[w] = w == (i >> 6) ? f | 1ull << (i & 63) : f;
    }
    int pops = 0;
    for (int size = 3; size <= n; ++size) {                                     // the frontier is size - 2 bonds away from i
        unsigned long long hit = 0ull, left = 0ull;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            hit |= s_row[w][j] & fr[w];
            left |= fr[w];
        }
        if (hit) return size;
        if (!left) return 0;
#pragma unroll
        for (int w = 0; w < W; ++w) nx[w] = 0ull;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            unsigned long long bits = fr[w];
            for (int k = 0; k < 64 && bits && pops < n; ++k) {
                const int at = w * 64 + __ffsll((long long)bits) - 1;
                bits &= bits - 1ull;
                ++pops;
#pragma unroll
                for (int u = 0; u < W; ++u) nx[u] |= s_row[u][at];
            }
        }
#pragma unroll
        for (int w = 0; w < W; ++w) {
            nx[w] &= ~vis[w];
            vis[w] |= nx[w];
            fr[w] = nx[w];
        }
    }
    return 0;
}

template <int MAXN>
__global__ __launch_bounds__(MAXN) void ring_report_kernel(TdBondArgs a) {
    constexpr int W = MAXN / 64;
    __shared__ float4 s_at[MAXN];
    __shared__ unsigned long long s_row[W][MAXN];
    __shared__ double s_thr[3][64];
    __shared__ int s_off[MAXN], s_ring[MAXN], s_elem[TD_QUALITY_MAX_CLASSES];
    __shared__ unsigned int s_mask;
    __shared__ int s_nrb, s_nra;
    const int tid = threadIdx.x;
    const BgMol m = bg_molecule<MAXN>(a);
    if (!m.mine) return;                                                        // workgroup-uniform
    const int n = m.n;
    if (m.bad) {                                                                // only the 512-lane instantiation gets here
        if (tid == 0) {
            a.ring_mask[m.mol] = 0u;
            a.n_ring_bonds[m.mol] = a.n_ring_atoms[m.mol] = -1;
        }
        return;
    }
    td_bond_thresholds(s_thr, tid, MAXN);
    if (tid < TD_QUALITY_MAX_CLASSES) s_elem[tid] = tid < a.K ? a.elem[tid] : -1;
    s_ring[tid] = RG_NONE;
    if (tid == 0) {
        s_mask = 0u;
        s_nrb = s_nra = 0;
    }
    bg_load<MAXN>(a, m, s_elem, s_at);
    int up = 0;
    if (tid < n) up = bg_rows<MAXN>(n, s_at, s_thr, s_row, [](int, int, int, double) {});
    const bool list = a.bond_ring || a.bond_category;                           // workgroup-uniform
    s_off[tid] = up;
    __syncthreads();
    if (list) bg_scan<MAXN>(s_off);                                             // inclusive scan of the per-atom counts

    // ---- the bonds tid < j, ascending in j
    if (up) {
        int64_t k = list ? a.bond_ptr[m.mol] + (int64_t)(s_off[tid] - up) : 0;
        const float4 me = s_at[tid];
        const int ci = __float_as_int(me.w), ei = ci & 7;
        const double xi = (double)me.x, yi = (double)me.y, zi = (double)me.z;
        int nrb = 0, low = RG_NONE;
        unsigned int mask = 0u;
        for (int w = tid >> 6; w < W; ++w) {
            unsigned long long bits = s_row[w][tid];
            if (w == (tid >> 6)) bits &= ~((2ull << (tid & 63)) - 1ull);        // j > tid only
            for (int c = 0; c < 64 && bits; ++c) {
                const int j = w * 64 + __ffsll((long long)bits) - 1;
                bits &= bits - 1ull;
                const int r = rg_bond_ring<MAXN>(s_row, n, tid, j);
                if (r) {
                    ++nrb;
                    mask |= 1u << (r < 31 ? r : 31);
                    low = r < low ? r : low;
                    atomicMin(&s_ring[j], r);
                }
                if (list && k >= 0 && k < a.capacity) {                         // offsets that are not this pack's own write nothing out of bounds
                    if (a.bond_ring) a.bond_ring[k] = (uint16_t)r;
                    if (a.bond_category) {
                        const float4 q = s_at[j];
                        const int cj = __float_as_int(q.w);
                        double d;
                        const int order = td_bond_order(xi, yi, zi, q.x, q.y, q.z, ei * 8 + (cj & 7), s_thr, d);
                        const int cat = bg_category(ci, cj, order);
                        a.bond_category[k] = (uint8_t)(cat == 4 && r != 5 && r != 6 ? order : cat);
                    }
                }
                ++k;
            }
        }
        if (nrb) {
            atomicAdd(&s_nrb, nrb);
            atomicOr(&s_mask, mask);
            atomicMin(&s_ring[tid], low);
        }
    }
    __syncthreads();
    if (tid < n) {
        const int r = s_ring[tid] == RG_NONE ? 0 : s_ring[tid];
        if (r) atomicAdd(&s_nra, 1);
        if (a.atom_ring) a.atom_ring[(size_t)m.s * (size_t)a.Nl + (size_t)(m.l0 + tid)] = r;
    }
    __syncthreads();
    const unsigned int mask = s_mask;
    if (tid == 0) {
        a.ring_mask[m.mol] = mask;
        a.n_ring_bonds[m.mol] = s_nrb;
        a.n_ring_atoms[m.mol] = s_nra;
    }
    const bool inc = !a.include || a.include[m.mol] != 0;                       // workgroup-uniform
    // bits 0 .. 2 of a mask are never set: entry 0 of the histogram counts the molecules without any ring
    if (inc && tid < TD_RING_BITS && (tid == 0 ? mask == 0u : (mask >> tid & 1u) != 0u))
        atomicAdd(&a.ring_hist[(size_t)m.s * TD_RING_BITS + tid], 1ull);
}

int td_launch_ring_report(const TdBondArgs &a, hipStream_t s) {
    const int64_t M = (int64_t)a.S * a.B;
    if (a.S > 0) TD_CHECK_HIP(hipMemsetAsync(a.ring_hist, 0, (size_t)a.S * TD_RING_BITS * sizeof(unsigned long long), s));
    if (M == 0) return TD_OK;
    return bg_launch_pair(ring_report_kernel<BG_SMALL>, ring_report_kernel<BG_MAX>, a, M, s);
}
