// Typed pocket interactions of ligand frames (gfx950, wave64; DESIGN.md section 3, "Pocket interactions"): which hydrogen bonds and
// hydrophobic contacts every molecule of a pack makes with its pocket.  Integer outputs only: no energy, no score.
//   * protein_role_kernel  one thread per protein atom, the pocket tiled through LDS 256 atoms at a time.  A protein atom takes part
//                          when its element, its kind and its role are in range; a carbon that takes part is hydrophobic when no
//                          nitrogen or oxygen that takes part lies closer than hetero_cutoff.  Writes role_out: the host table's donor
//                          and acceptor bits with that bit added, -1 for an atom that takes no part.
//   * interaction_kernel   one workgroup of four waves per (frame, molecule), the launch shape of pocket_kernel.  The molecule is
//                          staged once into LDS as (x, y, z, element index); every ligand atom's role follows from its bonds under
//                          the bond rule (td_bond_order over the molecule's atoms as LDS broadcast reads: the sum of the orders, the
//                          bonded hydrogens and the bonded N / O).  Threads then own protein atoms at stride 256 and walk the ligand
//                          atoms that have a role; the squared distance is the bond rule's (td_pair_dist2) and its root is taken only
//                          where the pair can fall below the larger cutoff (see td_launch_interaction_report).  The word of 64 protein
//                          atoms hit is a wave ballot per interaction type: wave w of round r produces word 4 r + w of each of the
//                          three planes, so no atomic is needed for the bits, and n_ref_common is a popcount.  The per-ligand-atom
//                          counts and the 3 x n_kinds histogram are LDS integer atomics, taken only on a hit; an included molecule
//                          adds its histogram to the global one once at its end, and one per type to the frequency of every protein
//                          atom it hits.
// Every loop is bounded by the molecule's size or the pocket's.  All outputs are integers: nothing depends on the grid or on the order
// of arrival.  No floating-point atomic.  The answer to an oversize molecule (-1) is that of bonds.hip.
#include "td_pocket_walk.h"

constexpr int IX_T = PW_T, IX_WAVES = PW_WAVES, IX_K = TD_POCKET_MAX_KINDS, IX_TYPES = TD_INTERACTION_TYPES;
constexpr int IX_PC = 1, IX_PN = 2, IX_PO = 3;                                  // and of the protein (H C N O S Se)

__global__ __launch_bounds__(IX_T) void protein_role_kernel(TdInteractionArgs g) {
    __shared__ float4 s_tile[IX_T];
    const TdProteinSide &ps = g.p;
    const int tid = threadIdx.x, Np = ps.Np, nk = ps.n_kinds;
    const int j = blockIdx.x * IX_T + tid;
    auto takes_part = [&](int at) { return pw_takes_part(ps.pelem[at], ps.pkind[at], nk) && g.prole[at] >= 0; };
    int role = -1;
    bool carbon = false;
    double X = 0.0, Y = 0.0, Z = 0.0;
    if (j < Np && takes_part(j)) {
        role = g.prole[j] & (TD_ROLE_DONOR | TD_ROLE_ACCEPTOR);
        carbon = ps.pelem[j] == IX_PC;
        const float *p = ps.ppos + (size_t)j * 3;
        X = (double)p[0]; Y = (double)p[1]; Z = (double)p[2];
    }
    bool polar_near = false;
    for (int t0 = 0; t0 < Np; t0 += IX_T) {                                     // workgroup-uniform
        const int k = t0 + tid;
        float4 q = make_float4(0.f, 0.f, 0.f, __int_as_float(0));
        if (k < Np) {
            const int e = ps.pelem[k];
            const float *p = ps.ppos + (size_t)k * 3;
            q = make_float4(p[0], p[1], p[2], __int_as_float((e == IX_PN || e == IX_PO) && takes_part(k) ? 1 : 0));
        }
        __syncthreads();                                                        // the last tile has been read
        s_tile[tid] = q;
        __syncthreads();
        const int cnt = Np - t0 < IX_T ? Np - t0 : IX_T;
        if (carbon && !polar_near)
            for (int i = 0; i < cnt; ++i) {
                const float4 t = s_tile[i];
                if (__float_as_int(t.w) && sqrt(td_pair_dist2(X, Y, Z, t.x, t.y, t.z)) < g.hetero_cutoff) polar_near = true;
            }
    }
    if (j < Np) g.role_out[j] = carbon && !polar_near ? role | TD_ROLE_HYDROPHOBIC : role;
}

__global__ __launch_bounds__(IX_T) void interaction_kernel(TdInteractionArgs g) {
    const TdBondArgs &a = g.b;
    __shared__ float4 s_at[BG_MAX];
    __shared__ int s_role[BG_MAX], s_ahb[BG_MAX], s_ahy[BG_MAX];
    __shared__ unsigned int s_hist[IX_TYPES * IX_K];
    __shared__ double s_thr[3][64];
    __shared__ int s_elem[TD_QUALITY_MAX_CLASSES];
    // donated, accepted, hbonds, hydrophobic pairs; atoms in an H-bond; donors, acceptors, hydrophobic atoms; common per type
    __shared__ int s_cnt[8 + IX_TYPES];
    const int tid = threadIdx.x, wave = tid >> 6;
    const BgMol m = bg_molecule<BG_MAX>(a);                                     // one instantiation takes every size: m.mine is not used
    const TdProteinSide &ps = g.p;
    const int Np = ps.Np, nk = ps.n_kinds;
    if (m.bad) {                                                                // workgroup-uniform
        if (tid == 0) {
            g.n_donated[m.mol] = g.n_accepted[m.mol] = g.n_hbonds[m.mol] = g.n_hydrophobic[m.mol] = g.n_hb_atoms[m.mol] = -1;
            g.n_donors[m.mol] = g.n_acceptors[m.mol] = g.n_hydrophobic_atoms[m.mol] = -1;
        }
        if (ps.ref_bits && tid < IX_TYPES) g.n_ref_common[m.mol * IX_TYPES + tid] = -1;
        pw_no_bits<IX_TYPES>(ps, m.mol);
        return;
    }
    const int n = m.n;
    const bool inc = !a.include || a.include[m.mol] != 0;                       // workgroup-uniform
    if (tid < TD_QUALITY_MAX_CLASSES) s_elem[tid] = tid < a.K ? a.elem[tid] : -1;
    td_bond_thresholds(s_thr, tid, IX_T);
    for (int k = tid; k < IX_TYPES * nk; k += IX_T) s_hist[k] = 0u;
    for (int i = tid; i < n; i += IX_T) s_ahb[i] = s_ahy[i] = 0;
    if (tid < 8 + IX_TYPES) s_cnt[tid] = 0;
    __syncthreads();
    pw_stage(a, m, s_elem, s_at);
    __syncthreads();
    for (int i = tid; i < n; i += IX_T) {
        const int role = ix_ligand_role(i, n, s_at, s_thr);
        s_role[i] = role;
        if (g.atom_role) g.atom_role[(size_t)m.s * (size_t)a.Nl + (size_t)(m.l0 + i)] = role;
        if (role & TD_ROLE_DONOR) atomicAdd(&s_cnt[5], 1);
        if (role & TD_ROLE_ACCEPTOR) atomicAdd(&s_cnt[6], 1);
        if (role & TD_ROLE_HYDROPHOBIC) atomicAdd(&s_cnt[7], 1);
    }
    __syncthreads();

    int nd = 0, na = 0, nhb = 0, nhy = 0, common[IX_TYPES] = {0, 0, 0};
    const int rounds = (Np + IX_T - 1) / IX_T;
    for (int r = 0; r < rounds; ++r) {
        const int j = r * IX_T + tid;
        int pr = -1, kp = 0, touched = 0;                                       // touched: bit t, hit by an interaction of type t
        double X = 0.0, Y = 0.0, Z = 0.0;
        if (pw_protein_atom(ps, j, kp, X, Y, Z)) pr = g.role_out[j];            // >= 0: the atom takes part, so its kind is in range
        if (__ballot(pr > 0) != 0ull) {                                         // wave-uniform: an atom without a role bit hits nothing
            for (int i = 0; i < n; ++i) {
                const int lr = s_role[i];                                       // every lane reads the same address: an LDS broadcast
                if (lr == 0) continue;                                          // wave-uniform
                const float4 q = s_at[i];
                const double d2 = td_pair_dist2(X, Y, Z, q.x, q.y, q.z);
                if (pr <= 0 || !(d2 < g.reject2)) continue;
                const double d = sqrt(d2);
                const bool hb = d < g.hbond_cutoff, hy = d < g.hydrophobic_cutoff;
                const bool t0 = hb && (lr & TD_ROLE_DONOR) && (pr & TD_ROLE_ACCEPTOR);
                const bool t1 = hb && (lr & TD_ROLE_ACCEPTOR) && (pr & TD_ROLE_DONOR);
                const bool t2 = hy && (lr & TD_ROLE_HYDROPHOBIC) && (pr & TD_ROLE_HYDROPHOBIC);
                if (t0) {
                    ++nd;
                    touched |= 1;
                    atomicAdd(&s_hist[kp], 1u);
                }
                if (t1) {
                    ++na;
                    touched |= 2;
                    atomicAdd(&s_hist[nk + kp], 1u);
                }
                if (t0 || t1) {                                                 // a pair of both types is one hydrogen bond
                    ++nhb;
                    atomicAdd(&s_ahb[i], 1);
                }
                if (t2) {
                    ++nhy;
                    touched |= 4;
                    atomicAdd(&s_hist[2 * nk + kp], 1u);
                    atomicAdd(&s_ahy[i], 1);
                }
            }
        }
        const int wi = IX_WAVES * r + wave;                                     // protein atoms 64 wi .. + 63; every lane is here
#pragma unroll
        for (int t = 0; t < IX_TYPES; ++t) {
            const bool hit = (touched >> t) & 1;
            int hits = 0;                                                       // the atoms hit are not reported
            pw_word<IX_TYPES>(ps, m.mol, t, wi, hit, hits, common[t]);
            if (inc && hit) atomicAdd(&ps.pocket_freq[((size_t)m.s * IX_TYPES + t) * (size_t)Np + j], 1);
        }
    }
    if (nd) atomicAdd(&s_cnt[0], nd);
    if (na) atomicAdd(&s_cnt[1], na);
    if (nhb) atomicAdd(&s_cnt[2], nhb);
    if (nhy) atomicAdd(&s_cnt[3], nhy);
#pragma unroll
    for (int t = 0; t < IX_TYPES; ++t)
        if (common[t]) atomicAdd(&s_cnt[8 + t], common[t]);
    __syncthreads();
    for (int i = tid; i < n; i += IX_T) {
        const size_t at = (size_t)m.s * (size_t)a.Nl + (size_t)(m.l0 + i);
        const int hb = s_ahb[i];
        if (g.atom_hbonds) g.atom_hbonds[at] = hb;
        if (g.atom_hydrophobic) g.atom_hydrophobic[at] = s_ahy[i];
        if (hb) atomicAdd(&s_cnt[4], 1);
    }
    if (inc) bg_flush_hist<IX_T>(s_hist, IX_TYPES * nk, ps.kind_hist + (size_t)m.s * (size_t)(IX_TYPES * nk));
    __syncthreads();
    if (tid == 0) {
        g.n_donated[m.mol] = s_cnt[0];
        g.n_accepted[m.mol] = s_cnt[1];
        g.n_hbonds[m.mol] = s_cnt[2];
        g.n_hydrophobic[m.mol] = s_cnt[3];
        g.n_hb_atoms[m.mol] = s_cnt[4];
        g.n_donors[m.mol] = s_cnt[5];
        g.n_acceptors[m.mol] = s_cnt[6];
        g.n_hydrophobic_atoms[m.mol] = s_cnt[7];
    }
    if (ps.ref_bits && tid < IX_TYPES) g.n_ref_common[m.mol * IX_TYPES + tid] = s_cnt[8 + tid];
}

// The limit of the root (pw_reject2) is taken of the larger of the two pair cutoffs.  The protein roles are resolved first, on the
// same stream; the pair kernel reads them.
int td_launch_interaction_report(const TdInteractionArgs &args, hipStream_t s) {
    TdInteractionArgs g = args;
    g.reject2 = pw_reject2(std::fmax(g.hbond_cutoff, g.hydrophobic_cutoff));
    if (const int rc = td_launch_protein_roles(g, s)) return rc;
    return pw_launch(interaction_kernel, g, IX_TYPES, IX_TYPES, s);
}

// The protein roles alone, for the reports that read them (score.hip): nothing is launched for an empty pocket
int td_launch_protein_roles(const TdInteractionArgs &g, hipStream_t s) {
    if (g.p.Np > 0) {
        protein_role_kernel<<<dim3((unsigned)((g.p.Np + IX_T - 1) / IX_T)), dim3(IX_T), 0, s>>>(g);
        TD_CHECK_HIP(hipGetLastError());
    }
    return TD_OK;
}
