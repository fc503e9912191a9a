// Bond graph of ligand frames (gfx950, wave64; DESIGN.md section 3, "Bond graph").  The bond-length table of td_bond_rule.h, which
// quality.hip only sums into nr_bonds, kept as a graph per (frame, molecule):
//   * bond_graph_kernel  one workgroup per (frame, molecule), the molecule in LDS.  A lane owns atom i, evaluates its row of orders
//                        once and keeps it as a bit row in LDS (s_row[w][i]: word w of atom i, so a wave's accesses are contiguous).
//                        Bonds i < j of an included molecule enter the bond-length histograms on the way.  Fragments: min-label
//                        propagation over the bit rows with one pointer jump per sweep, until a workgroup-wide "changed" flag stays
//                        clear; a label ends as the smallest atom index of its component.
//   * bond_ptr_kernel    exclusive prefix of n_bonds over (frame, molecule) in one workgroup: a fixed order of additions.
//   * bond_list_kernel   the same rows again; a workgroup scan of the per-atom counts of bonds i < j gives every lane the offset at
//                        which it writes its own atom's bonds, so the list is ascending in (frame, molecule, i, j).
// Every loop is bounded by the molecule's size (propagation: at most n sweeps, which plain min-label propagation needs at worst), so
// a defect ends in a wrong number, not in a kernel that does not return.  Outputs are integers, or float64 values written by one lane;
// integer LDS and global atomics only: nothing depends on the grid or on the order of arrival.
// Two instantiations share the grid: 128 lanes for molecules of up to TD_BOND_SMALL_ATOMS atoms (ligands), 512 lanes up to
// TD_BOND_MAX_ATOMS; a workgroup whose molecule belongs to the other one returns at once.  A molecule above TD_BOND_MAX_ATOMS, or whose
// offsets leave [0, N_l], is answered with -1 by the 512-lane instantiation and contributes nothing else.
#include "td_bond_graph.h"

constexpr int BG_SCAN_THREADS = 1024;

template <int MAXN>
__global__ __launch_bounds__(MAXN) void bond_graph_kernel(TdBondArgs a) {
    constexpr int W = MAXN / 64;
    __shared__ float4 s_at[MAXN];
    __shared__ unsigned long long s_row[W][MAXN];
    __shared__ double s_thr[3][64];
    __shared__ unsigned int s_hist[BG_MAXP][BG_BINS];
    __shared__ int s_lab[MAXN], s_size[MAXN], s_elem[TD_QUALITY_MAX_CLASSES];
    __shared__ int s_changed[2], s_nb, s_nf, s_big;
    __shared__ int s_pe1[BG_MAXP], s_pe2[BG_MAXP], s_pcat[BG_MAXP], s_pn[BG_MAXP];   // the profiles: read per bond, by a run-time index
    __shared__ const double *s_pedges[BG_MAXP];
    const int tid = threadIdx.x;
    const BgMol m = bg_molecule<MAXN>(a);
    if (!m.mine) return;                                                        // workgroup-uniform
    const int n = m.n;
    if (m.bad) {                                                                // only the 512-lane instantiation gets here
        if (tid == 0) a.n_bonds[m.mol] = a.n_fragments[m.mol] = a.largest[m.mol] = -1;
        return;
    }
    const bool inc = !a.include || a.include[m.mol] != 0;                       // workgroup-uniform
    const int P = inc ? a.P : 0;
    td_bond_thresholds(s_thr, tid, MAXN);
    if (tid < TD_QUALITY_MAX_CLASSES) s_elem[tid] = tid < a.K ? a.elem[tid] : -1;
    if (tid < P) {
        s_pe1[tid] = a.pe1[tid]; s_pe2[tid] = a.pe2[tid]; s_pcat[tid] = a.pcat[tid]; s_pn[tid] = a.n_edges[tid];
        s_pedges[tid] = a.edges[tid];
    }
    for (int k = tid; k < P * BG_BINS; k += MAXN) (&s_hist[0][0])[k] = 0u;
    s_lab[tid] = tid;
    s_size[tid] = 0;
    if (tid < 2) s_changed[tid] = 0;
    if (tid == 0) s_nb = s_nf = s_big = 0;
    bg_load<MAXN>(a, m, s_elem, s_at);

    // ---- the row of atom tid (td_bond_graph.h); bonds tid < j are counted and enter the histograms
    int up = 0;
    if (tid < n) {
        const int ci = __float_as_int(s_at[tid].w), ei = ci & 7;
        up = bg_rows<MAXN>(n, s_at, s_thr, s_row, [&](int j, int cj, int order, double d) {
            const int ej = cj & 7, cat = bg_category(ci, cj, order);
            for (int p = 0; p < P; ++p) {
                const int e1 = s_pe1[p], e2 = s_pe2[p], pc = s_pcat[p];
                const bool match = ((e1 < 0 || ei == e1) && (e2 < 0 || ej == e2)) || ((e1 < 0 || ej == e1) && (e2 < 0 || ei == e2));
                if (match && (pc == 0 || pc == cat)) atomicAdd(&s_hist[p][td_searchsorted_left(s_pedges[p], s_pn[p], d)], 1u);
            }
        });
    }
    __syncthreads();

    // ---- fragments: label <- min(own, neighbours', label of that minimum), all reads of a sweep before all of its writes.  A label
    // is always an atom of the same component and never grows; plain propagation alone is done after n - 1 sweeps, so n bounds the loop.
    for (int it = 0; it < n; ++it) {
        int old = MAXN, lab = MAXN;
        if (tid < n) {
            old = lab = s_lab[tid];
#pragma unroll
            for (int w = 0; w < W; ++w) {
                unsigned long long bits = s_row[w][tid];
                for (int k = 0; k < 64 && bits; ++k) {
                    const int jj = __ffsll((long long)bits) - 1;
                    bits &= bits - 1ull;
                    const int other = s_lab[w * 64 + jj];
                    lab = other < lab ? other : lab;
                }
            }
            const int jump = s_lab[lab];
            lab = jump < lab ? jump : lab;
        }
        __syncthreads();
        if (lab < old) {
            s_lab[tid] = lab;
            s_changed[it & 1] = 1;
        }
        __syncthreads();
        const int changed = s_changed[it & 1];                                  // workgroup-uniform
        if (tid == 0) s_changed[(it & 1) ^ 1] = 0;                              // the next sweep's flag; its writers wait at that sweep's barrier
        if (!changed) break;
    }

    // ---- counts
    if (tid < n) {
        const int lab = s_lab[tid];
        atomicAdd(&s_size[lab], 1);
        if (lab == tid) atomicAdd(&s_nf, 1);
        if (up) atomicAdd(&s_nb, up);
        if (a.fragment) a.fragment[(size_t)m.s * (size_t)a.Nl + (size_t)(m.l0 + tid)] = lab;
    }
    __syncthreads();
    if (tid < n && s_size[tid] > 0) atomicMax(&s_big, s_size[tid]);
    __syncthreads();
    if (tid == 0) {
        a.n_bonds[m.mol] = s_nb;
        a.n_fragments[m.mol] = s_nf;
        a.largest[m.mol] = s_big;
    }
    bg_flush_hist<MAXN>(&s_hist[0][0], P * BG_BINS, a.hist + (size_t)m.s * a.P * BG_BINS);
}

// ptr[k] = sum of max(n_bonds[0 .. k), 0), k = 0 .. M: every lane sums a contiguous run, the 1024 run sums are scanned in LDS
__global__ __launch_bounds__(BG_SCAN_THREADS) void bond_ptr_kernel(const int32_t *n_bonds, int64_t M, int64_t *ptr) {
    __shared__ long long s_sum[BG_SCAN_THREADS];
    const int tid = threadIdx.x;
    const int64_t per = (M + BG_SCAN_THREADS - 1) / BG_SCAN_THREADS;
    const int64_t b = (int64_t)tid * per < M ? (int64_t)tid * per : M, e = b + per < M ? b + per : M;
    long long sum = 0;
    for (int64_t k = b; k < e; ++k) sum += n_bonds[k] > 0 ? n_bonds[k] : 0;
    s_sum[tid] = sum;
    __syncthreads();
    for (int d = 1; d < BG_SCAN_THREADS; d <<= 1) {
        const long long t = tid >= d ? s_sum[tid - d] : 0;
        __syncthreads();
        s_sum[tid] += t;
        __syncthreads();
    }
    long long run = s_sum[tid] - sum;
    for (int64_t k = b; k < e; ++k) {
        ptr[k] = run;
        run += n_bonds[k] > 0 ? n_bonds[k] : 0;
    }
    if (tid == BG_SCAN_THREADS - 1) ptr[M] = s_sum[tid];
}

template <int MAXN>
__global__ __launch_bounds__(MAXN) void bond_list_kernel(TdBondArgs a) {
    __shared__ float4 s_at[MAXN];
    __shared__ double s_thr[3][64];
    __shared__ int s_off[MAXN], s_elem[TD_QUALITY_MAX_CLASSES];
    const int tid = threadIdx.x;
    const BgMol m = bg_molecule<MAXN>(a);
    if (!m.mine || m.bad || m.n < 2) return;                                    // workgroup-uniform; an oversize molecule lists nothing
    const int n = m.n;
    td_bond_thresholds(s_thr, tid, MAXN);
    if (tid < TD_QUALITY_MAX_CLASSES) s_elem[tid] = tid < a.K ? a.elem[tid] : -1;
    bg_load<MAXN>(a, m, s_elem, s_at);
    float4 me = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    if (tid < n) me = s_at[tid];
    const int ci = __float_as_int(me.w), ei = ci & 7;
    const double xi = (double)me.x, yi = (double)me.y, zi = (double)me.z;
    int up = 0;
    if (ci >= 0) {
        for (int j = tid + 1; j < n; ++j) {
            const float4 q = s_at[j];
            const int cj = __float_as_int(q.w);
            if (cj < 0) continue;
            double d;
            up += td_bond_order(xi, yi, zi, q.x, q.y, q.z, ei * 8 + (cj & 7), s_thr, d) > 0 ? 1 : 0;
        }
    }
    s_off[tid] = up;
    __syncthreads();
    bg_scan<MAXN>(s_off);                                                       // inclusive scan of the per-atom counts
    if (up == 0) return;
    int64_t k = a.bond_ptr[m.mol] + (int64_t)(s_off[tid] - up);
    for (int j = tid + 1; j < n; ++j) {
        const float4 q = s_at[j];
        const int cj = __float_as_int(q.w);
        if (cj < 0) continue;
        double d;
        const int order = td_bond_order(xi, yi, zi, q.x, q.y, q.z, ei * 8 + (cj & 7), s_thr, d);
        if (order == 0) continue;
        if (k >= 0 && k < a.capacity) {                                         // offsets that are not this pack's own write nothing out of bounds
            a.bond_atoms[2 * k] = m.l0 + tid;
            a.bond_atoms[2 * k + 1] = m.l0 + j;
            a.bond_order[k] = (uint8_t)order;
            a.bond_category[k] = (uint8_t)bg_category(ci, cj, order);
            a.bond_length[k] = d;
        }
        ++k;
    }
}

int td_launch_bond_graph(const TdBondArgs &a, hipStream_t s) {
    const int64_t M = (int64_t)a.S * a.B;
    if (a.S > 0 && a.P > 0) TD_CHECK_HIP(hipMemsetAsync(a.hist, 0, (size_t)a.S * a.P * BG_BINS * sizeof(unsigned long long), s));
    if (M == 0) {
        if (a.bond_ptr) TD_CHECK_HIP(hipMemsetAsync(a.bond_ptr, 0, sizeof(int64_t), s));
        return TD_OK;
    }
    if (const int rc = bg_launch_pair(bond_graph_kernel<BG_SMALL>, bond_graph_kernel<BG_MAX>, a, M, s)) return rc;
    if (a.bond_ptr) {
        bond_ptr_kernel<<<dim3(1), dim3(BG_SCAN_THREADS), 0, s>>>(a.n_bonds, M, a.bond_ptr);
        TD_CHECK_HIP(hipGetLastError());
    }
    return TD_OK;
}

int td_launch_bond_list(const TdBondArgs &a, hipStream_t s) {
    const int64_t M = (int64_t)a.S * a.B;
    if (M == 0 || a.capacity == 0) return TD_OK;
    return bg_launch_pair(bond_list_kernel<BG_SMALL>, bond_list_kernel<BG_MAX>, a, M, s);
}
