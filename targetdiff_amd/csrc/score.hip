// Docking-style score of ligand frames (gfx950, wave64; DESIGN.md section 3, "Docking-style score"): per molecule the five unweighted
// sums of a Vina-style pair energy with its pocket, and its rotatable bonds.  The kernels form no energy: the weights and the rotor
// normalisation are the host's.  This is a score on this project's heuristic typing (no hydrogens, roles from valence deficits, no
// intramolecular term): it is not AutoDock Vina's number.
//   * score_kernel  one workgroup of four waves per (frame, molecule), the launch shape of interaction_kernel.  The molecule is staged
//                   into LDS (pw_stage) and every ligand atom's role follows from its bonds (ix_ligand_role, the one copy that
//                   interactions.hip reads).  Threads own protein atoms at stride 256 and walk the ligand heavy atoms as LDS broadcast
//                   reads.  r is the bond rule's distance (td_pair_dist2, IEEE sqrt), taken only where the pair can fall below the
//                   cutoff (pw_reject2); d = r - rsum[e_l][e_p] is the surface distance.  The five term values of a pair are float64
//                   with every product, sum and difference rounded on its own; each becomes llrint(ldexp(value, 24)) and is added
//                   to the thread's own int64 accumulator, so a molecule's sums are exact whatever the order of arrival.  The
//                   accumulators meet in LDS integer atomics.
//   * rotor_kernel  one workgroup per (frame, molecule) on the bit rows of the bond graph (td_bond_graph.h), both size instantiations
//                   as bonds.hip.  Lane i owns atom i: the number of its bonded heavy atoms, then its bonds i < j in ascending j,
//                   whose index in td_bond_list's order is the scan of the upward-bond counts plus the rank of j (geometry.hip).
// Every loop is bounded by the molecule's size or the pocket's.  All outputs are integers: nothing depends on the grid or on the order
// of arrival.  No floating-point atomic.  The answer to an oversize molecule (-1, INT64_MIN) is that of bonds.hip.
#include "td_score_terms.h"

#include <climits>

__global__ __launch_bounds__(SC_T) void score_kernel(TdScoreArgs g) {
    const TdBondArgs &a = g.b;
    __shared__ float4 s_at[BG_MAX];
    __shared__ int s_role[BG_MAX];                                              // -1: the atom takes no part (no class, or H)
    __shared__ double s_thr[3][64], s_rsum[8 * SC_PE];
    __shared__ int s_elem[TD_QUALITY_MAX_CLASSES];
    __shared__ unsigned long long s_sum[SC_TERMS];
    __shared__ int s_pairs;
    const int tid = threadIdx.x;
    const BgMol m = bg_molecule<BG_MAX>(a);                                     // one instantiation takes every size: m.mine is not used
    const TdProteinSide &ps = g.p;
    const int Np = ps.Np;
    if (m.bad) {                                                                // workgroup-uniform
        if (tid == 0) g.n_pairs[m.mol] = -1;
        if (tid < SC_TERMS) g.terms[m.mol * SC_TERMS + tid] = LLONG_MIN;
        return;
    }
    const int n = m.n;
    if (tid < TD_QUALITY_MAX_CLASSES) s_elem[tid] = tid < a.K ? a.elem[tid] : -1;
    td_bond_thresholds(s_thr, tid, SC_T);
    if (tid < 8 * SC_PE) s_rsum[tid] = g.rsum[tid];
    if (tid < SC_TERMS) s_sum[tid] = 0ull;
    if (tid == 0) s_pairs = 0;
    __syncthreads();
    pw_stage(a, m, s_elem, s_at);
    __syncthreads();
    for (int i = tid; i < n; i += SC_T) {
        const int el = __float_as_int(s_at[i].w);
        s_role[i] = el > IX_H ? ix_ligand_role(i, n, s_at, s_thr) : -1;
    }
    __syncthreads();

    long long acc[SC_TERMS] = {0, 0, 0, 0, 0};
    int pairs = 0;
    const int rounds = (Np + SC_T - 1) / SC_T;
    for (int r = 0; r < rounds; ++r) {
        const int j = r * SC_T + tid;
        int pr = -1, kp = 0, pe = 0;
        double X = 0.0, Y = 0.0, Z = 0.0;
        if (pw_protein_atom(ps, j, kp, X, Y, Z)) {
            pe = ps.pelem[j];
            pr = pe == 0 ? -1 : g.role[j];                                      // >= 0: the atom takes part, so its element is in range
        }
        if (__ballot(pr >= 0) == 0ull) continue;                                // wave-uniform
        for (int i = 0; i < n; ++i) {
            const int lr = s_role[i];                                           // every lane reads the same address: an LDS broadcast
            if (lr < 0) continue;                                               // wave-uniform
            const float4 q = s_at[i];
            const double d2 = td_pair_dist2(X, Y, Z, q.x, q.y, q.z);
            if (pr < 0 || !(d2 < g.reject2)) continue;
            const double rr = sqrt(d2);
            if (!(rr < g.cutoff)) continue;
            const double d = td_add_rn64(rr, -s_rsum[__float_as_int(q.w) * SC_PE + pe]);
            ++pairs;
            sc_pair_terms(d, lr, pr, acc);                                      // td_score_terms.h: the copy relax.hip minimises
        }
    }
#pragma unroll
    for (int t = 0; t < SC_TERMS; ++t)
        if (acc[t]) atomicAdd(&s_sum[t], (unsigned long long)acc[t]);
    if (pairs) atomicAdd(&s_pairs, pairs);
    __syncthreads();
    if (tid == 0) g.n_pairs[m.mol] = s_pairs;
    if (tid < SC_TERMS) g.terms[m.mol * SC_TERMS + tid] = (long long)s_sum[tid];
}

// heavy: a class in the table and an element other than H
__device__ __forceinline__ bool sc_heavy(int code) { return code >= 0 && (code & 7) != IX_H; }

template <int MAXN>
__global__ __launch_bounds__(MAXN) void rotor_kernel(TdScoreArgs g) {
    constexpr int W = MAXN / 64;
    const TdBondArgs &a = g.b;
    __shared__ float4 s_at[MAXN];
    __shared__ unsigned long long s_row[W][MAXN];
    __shared__ double s_thr[3][64];
    __shared__ int s_off[MAXN], s_hdeg[MAXN], s_elem[TD_QUALITY_MAX_CLASSES];
    __shared__ int s_cnt;
    const int tid = threadIdx.x;
    const BgMol m = bg_molecule<MAXN>(a);
    if (!m.mine) return;                                                        // workgroup-uniform
    if (m.bad) {                                                                // only the 512-lane instantiation gets here
        if (tid == 0) g.n_rot[m.mol] = -1;
        return;
    }
    const int n = m.n;
    td_bond_thresholds(s_thr, tid, MAXN);
    if (tid < TD_QUALITY_MAX_CLASSES) s_elem[tid] = tid < a.K ? a.elem[tid] : -1;
    if (tid == 0) s_cnt = 0;
    bg_load<MAXN>(a, m, s_elem, s_at);

    // ---- the row of atom tid, its bonds tid < j and its bonded heavy atoms
    int up = 0, hdeg = 0;
    if (tid < n) {
        up = bg_rows<MAXN>(n, s_at, s_thr, s_row, [](int, int, int, double) {});
#pragma unroll
        for (int w = 0; w < W; ++w) {
            unsigned long long bits = s_row[w][tid];
            for (int c = 0; c < 64 && bits; ++c) {
                hdeg += sc_heavy(__float_as_int(s_at[w * 64 + __ffsll((long long)bits) - 1].w)) ? 1 : 0;
                bits &= bits - 1ull;
            }
        }
    }
    s_hdeg[tid] = hdeg;
    s_off[tid] = up;
    __syncthreads();
    bg_scan<MAXN>(s_off);                                                       // inclusive scan of the per-atom counts of bonds tid < j

    int rot = 0;
    if (tid < n && up > 0 && hdeg >= 2) {
        const float4 me = s_at[tid];
        const int ei = __float_as_int(me.w) & 7;
        const double xi = (double)me.x, yi = (double)me.y, zi = (double)me.z;
        const int64_t first = a.bond_ptr[m.mol] + (int64_t)(tid > 0 ? s_off[tid - 1] : 0);
        int rank = 0;                                                           // of j among the bonds tid < j, ascending: td_bond_list's order
#pragma unroll
        for (int w = 0; w < W; ++w) {
            unsigned long long bits = s_row[w][tid];
            for (int c = 0; c < 64 && bits; ++c) {
                const int j = w * 64 + __ffsll((long long)bits) - 1;
                bits &= bits - 1ull;
                if (j < tid) continue;
                const int64_t idx = first + rank++;
                const float4 q = s_at[j];
                double d;
                if (td_bond_order(xi, yi, zi, q.x, q.y, q.z, ei * 8 + (__float_as_int(q.w) & 7), s_thr, d) != 1 || s_hdeg[j] < 2) continue;
                if (idx < 0 || idx >= a.capacity) continue;                     // offsets that are not this pack's own read nothing out of bounds
                rot += a.bond_ring[idx] == 0 ? 1 : 0;
            }
        }
    }
    if (rot) atomicAdd(&s_cnt, rot);
    __syncthreads();
    if (tid == 0) g.n_rot[m.mol] = s_cnt;
}

// The protein roles are resolved by the caller, on the same stream (td_launch_protein_roles); the pair kernel reads them.
int td_launch_score_report(const TdScoreArgs &args, hipStream_t s) {
    TdScoreArgs g = args;
    g.reject2 = pw_reject2(g.cutoff);
    const int64_t M = (int64_t)g.b.S * g.b.B;
    if (M == 0) return TD_OK;
    score_kernel<<<dim3((unsigned)M), dim3(SC_T), 0, s>>>(g);
    TD_CHECK_HIP(hipGetLastError());
    return td_launch_rotors(g, s);
}

// the rotor kernel alone, where the pack comes with its bond list (relax.hip counts the rotors of the input pose with it)
int td_launch_rotors(const TdScoreArgs &g, hipStream_t s) {
    const int64_t M = (int64_t)g.b.S * g.b.B;
    if (M == 0 || !g.b.bond_ptr) return TD_OK;
    return bg_launch_pair(rotor_kernel<BG_SMALL>, rotor_kernel<BG_MAX>, g, M, s);
}
