// Pocket contacts of ligand frames (gfx950, wave64; DESIGN.md section 3, "Pocket contacts"): which protein atoms every molecule of a
// pack touches, how many of its atoms are buried, and how many pairs are closer than a clash threshold.
//   * pocket_kernel  one workgroup of four waves per (frame, molecule).  The molecule is staged once into LDS as (x, y, z, element
//                    index); threads own protein atoms at stride 256 (a coalesced read of the pocket, which stays in L2 across the
//                    grid) and walk the molecule's atoms as LDS broadcast reads.  The squared distance is the bond rule's
//                    (td_pair_dist2); its root is taken only where the pair can fall below a limit (see td_launch_pocket_report) and,
//                    for min_dist, once of the workgroup's smallest squared distance: the IEEE root is monotone, so the smallest root
//                    is the root of the smallest square.
//                    The contacted-protein-atom word of 64 atoms is a wave ballot: wave w of round r produces word 4 r + w, so no
//                    atomic is needed for the bits, and n_pocket_atoms and n_ref_common are popcounts.  The per-ligand-atom counts
//                    (one add per wave and atom, of the ballot's popcount) and the 8 x n_kinds histogram are LDS integer atomics, taken
//                    only on a hit; an included molecule adds its histogram to the global one once at its end, and one to the frequency
//                    of every protein atom it touches.
// Every loop is bounded by the molecule's size or the pocket's.  All outputs but min_dist are integers and min_dist is a minimum:
// nothing depends on the grid or on the order of arrival.  No floating-point atomic.  The answer to an oversize molecule (-1) is that
// of bonds.hip.
#include "td_pocket_walk.h"

constexpr int PK_T = PW_T, PK_WAVES = PW_WAVES, PK_E = TD_POCKET_ELEMENTS, PK_K = TD_POCKET_MAX_KINDS;

__global__ __launch_bounds__(PK_T) void pocket_kernel(TdPocketArgs g) {
    const TdBondArgs &a = g.b;
    __shared__ float4 s_at[BG_MAX];
    __shared__ int s_acon[BG_MAX], s_acl[BG_MAX];
    __shared__ unsigned int s_hist[8 * PK_K];
    __shared__ double s_thr[8 * PK_E], s_min[PK_WAVES];
    __shared__ int s_elem[TD_QUALITY_MAX_CLASSES];
    __shared__ int s_cnt[6];                                                    // contacts, clashes, pocket atoms, common, contact atoms, clash atoms
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BgMol m = bg_molecule<BG_MAX>(a);                                     // one instantiation takes every size: m.mine is not used
    const TdProteinSide &ps = g.p;
    const int Np = ps.Np, nk = ps.n_kinds;
    if (m.bad) {                                                                // workgroup-uniform
        if (tid == 0) {
            g.n_contacts[m.mol] = g.n_contact_atoms[m.mol] = g.n_pocket_atoms[m.mol] = -1;
            if (g.clash) g.n_clashes[m.mol] = g.n_clash_atoms[m.mol] = -1;
            if (ps.ref_bits) g.n_ref_common[m.mol] = -1;
            g.min_dist[m.mol] = std::numeric_limits<double>::infinity();
        }
        pw_no_bits<1>(ps, m.mol);
        return;
    }
    const int n = m.n;
    const bool inc = !a.include || a.include[m.mol] != 0;                       // workgroup-uniform
    if (tid < TD_QUALITY_MAX_CLASSES) s_elem[tid] = tid < a.K ? a.elem[tid] : -1;
    if (tid < 8 * PK_E) s_thr[tid] = g.clash_thr[tid];
    for (int k = tid; k < 8 * nk; k += PK_T) s_hist[k] = 0u;
    for (int i = tid; i < n; i += PK_T) s_acon[i] = s_acl[i] = 0;
    if (tid < 6) s_cnt[tid] = 0;
    __syncthreads();
    pw_stage(a, m, s_elem, s_at);
    __syncthreads();

    int nc = 0, ncl = 0, pocket = 0, common = 0;
    double min2 = std::numeric_limits<double>::infinity();
    const int rounds = (Np + PK_T - 1) / PK_T;
    for (int r = 0; r < rounds; ++r) {
        const int j = r * PK_T + tid;
        bool act = false, touched = false;
        int ep = 0, kp = 0;
        double X = 0.0, Y = 0.0, Z = 0.0;
        if (pw_protein_atom(ps, j, kp, X, Y, Z)) {
            ep = ps.pelem[j];
            act = pw_takes_part(ep, kp, nk);
        }
        if (__ballot(act) != 0ull) {                                            // wave-uniform: the last round leaves whole waves without an atom
            for (int i = 0; i < n; ++i) {
                const float4 q = s_at[i];                                       // every lane reads the same address: an LDS broadcast
                const int el = __float_as_int(q.w);
                if (el < 0) continue;                                           // wave-uniform
                const double d2 = td_pair_dist2(X, Y, Z, q.x, q.y, q.z);
                if (!act) continue;
                min2 = d2 < min2 ? d2 : min2;
                if (!(d2 < g.reject2)) continue;
                const double d = sqrt(d2);
                const bool con = d < g.cutoff, cl = g.clash && d < s_thr[el * PK_E + ep];
                const unsigned long long mcon = __ballot(con), mcl = __ballot(cl);          // over the lanes that came this far
                if (con) {
                    ++nc;
                    touched = true;
                    atomicAdd(&s_hist[el * nk + kp], 1u);
                    if (__ffsll((long long)mcon) - 1 == lane) atomicAdd(&s_acon[i], __popcll(mcon));
                }
                if (cl) {
                    ++ncl;
                    if (__ffsll((long long)mcl) - 1 == lane) atomicAdd(&s_acl[i], __popcll(mcl));
                }
            }
        }
        pw_word<1>(ps, m.mol, 0, PK_WAVES * r + wave, touched, pocket, common);
        if (inc && touched) atomicAdd(&ps.pocket_freq[(size_t)m.s * (size_t)Np + j], 1);
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(min2, off);
        min2 = o < min2 ? o : min2;
    }
    if (lane == 0) s_min[wave] = min2;
    if (nc) atomicAdd(&s_cnt[0], nc);
    if (ncl) atomicAdd(&s_cnt[1], ncl);
    if (pocket) atomicAdd(&s_cnt[2], pocket);
    if (common) atomicAdd(&s_cnt[3], common);
    __syncthreads();
    for (int i = tid; i < n; i += PK_T) {
        const size_t at = (size_t)m.s * (size_t)a.Nl + (size_t)(m.l0 + i);
        const int c = s_acon[i], k = s_acl[i];
        if (g.atom_contacts) g.atom_contacts[at] = c;
        if (g.clash && g.atom_clash) g.atom_clash[at] = k;
        if (c) atomicAdd(&s_cnt[4], 1);
        if (k) atomicAdd(&s_cnt[5], 1);
    }
    if (inc) bg_flush_hist<PK_T>(s_hist, 8 * nk, ps.kind_hist + (size_t)m.s * (size_t)(8 * nk));
    __syncthreads();
    if (tid == 0) {
        g.n_contacts[m.mol] = s_cnt[0];
        g.n_contact_atoms[m.mol] = s_cnt[4];
        g.n_pocket_atoms[m.mol] = s_cnt[2];
        if (g.clash) {
            g.n_clashes[m.mol] = s_cnt[1];
            g.n_clash_atoms[m.mol] = s_cnt[5];
        }
        if (ps.ref_bits) g.n_ref_common[m.mol] = s_cnt[3];
        double lo = s_min[0];
        for (int w = 1; w < PK_WAVES; ++w) lo = s_min[w] < lo ? s_min[w] : lo;
        g.min_dist[m.mol] = sqrt(lo);                                           // +inf without pairs
    }
}

// The limit of the root (pw_reject2) is taken of L, the larger of the contact cutoff and the table's largest threshold; an infinite
// limit rejects nothing.
#ifndef TD_POCKET_EARLY_REJECT
#define TD_POCKET_EARLY_REJECT 1
#endif

int td_launch_pocket_report(const TdPocketArgs &args, hipStream_t s) {
    TdPocketArgs g = args;
    double L = g.cutoff;
    if (g.clash)
        for (int k = 0; k < 8 * PK_E; ++k) L = std::fmax(L, g.clash_thr[k]);
    g.reject2 = TD_POCKET_EARLY_REJECT ? pw_reject2(L) : std::numeric_limits<double>::infinity();
    return pw_launch(pocket_kernel, g, 8, 1, s);
}
