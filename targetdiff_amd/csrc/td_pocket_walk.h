// What the kernels that walk a pocket share (pocket.hip, interactions.hip, score.hip; sasa.hip keeps its own walk and its own argument block;
// DESIGN.md section 3, "Pocket contacts"): one workgroup of four waves per (frame, molecule), the molecule staged in LDS, threads that
// own protein atoms at stride 256, and per bit plane the word of 64 protein atoms as a wave ballot.  One copy, so that the reports say
// the protein side alike.
#pragma once
#include "td_bond_graph.h"

#include <cmath>
#include <limits>

constexpr int PW_T = TD_POCKET_THREADS, PW_WAVES = PW_T / 64;

// does a protein atom take part: its element index is over H C N O S Se and its kind is one of the nk
__device__ __forceinline__ bool pw_takes_part(int e, int k, int nk) { return e >= 0 && e < TD_POCKET_ELEMENTS && k >= 0 && k < nk; }

// The molecule into LDS, atom i as (x, y, z, element index or -1 for a class outside [0, K)).  A barrier that publishes the class table
// s_elem precedes it at the caller and one follows it.
__device__ __forceinline__ void pw_stage(const TdBondArgs &a, const BgMol &m, const int *s_elem, float4 *s_at) {
    for (int i = threadIdx.x; i < m.n; i += PW_T) {
        const size_t at = (size_t)m.s * (size_t)a.Nl + (size_t)(m.l0 + i);
        const float *p = a.pos + at * 3;
        const int64_t c = a.v[at];
        s_at[i] = make_float4(p[0], p[1], p[2], __int_as_float(c >= 0 && c < a.K ? s_elem[(int)c] : -1));
    }
}

constexpr int IX_H = 0, IX_C = 1, IX_N = 2, IX_O = 3, IX_F = 4, IX_CL = 7;      // element indices of the ligand (H C N O F P S Cl)

// The role of ligand atom i (element index el >= 0) from its bonds: val the sum of the orders, n_h the bonded hydrogens, hetero the
// bonded N / O.  Only C, N and O need their bonds.
__device__ __forceinline__ int ix_ligand_role(int i, int n, const float4 *s_at, const double (*s_thr)[64]) {
    const float4 me = s_at[i];
    const int el = __float_as_int(me.w);
    if (el == IX_F || el == IX_CL) return TD_ROLE_HYDROPHOBIC;
    if (el != IX_C && el != IX_N && el != IX_O) return 0;                       // H, P, S, and a class outside the table (-1)
    const double xi = (double)me.x, yi = (double)me.y, zi = (double)me.z;
    int val = 0, n_h = 0, hetero = 0;
    for (int j = 0; j < n; ++j) {
        const float4 q = s_at[j];
        const int ej = __float_as_int(q.w);
        if (j == i || ej < 0) continue;
        double d;
        const int order = td_bond_order(xi, yi, zi, q.x, q.y, q.z, el * 8 + ej, s_thr, d);
        if (order == 0) continue;
        val += order;
        n_h += ej == IX_H;
        hetero += ej == IX_N || ej == IX_O;
    }
    if (el == IX_C) return hetero == 0 ? TD_ROLE_HYDROPHOBIC : 0;
    const int implicit = (el == IX_N ? 3 : 2) - val, h = n_h + (implicit > 0 ? implicit : 0);
    int role = h >= 1 ? TD_ROLE_DONOR : 0;
    if (el == IX_O || (h == 0 && val <= 3)) role |= TD_ROLE_ACCEPTOR;
    return role;
}

// the answer to an oversize molecule for its T planes of bit words: none set
template <int T>
__device__ __forceinline__ void pw_no_bits(const TdProteinSide &p, size_t mol) {
    if (p.bits)
        for (int w = threadIdx.x; w < T * p.W; w += PW_T) p.bits[mol * (size_t)(T * p.W) + w] = 0ull;
}

// protein atom j of a round: its kind and its position, widened; false past the end of the pocket, and nothing is read
__device__ __forceinline__ bool pw_protein_atom(const TdProteinSide &p, int j, int &kind, double &X, double &Y, double &Z) {
    if (j >= p.Np) return false;
    kind = p.pkind[j];
    const float *q = p.ppos + (size_t)j * 3;
    X = (double)q[0]; Y = (double)q[1]; Z = (double)q[2];
    return true;
}

// Plane t of T, word wi = 4 r + wave of round r: the protein atoms 64 wi .. + 63 that the molecule hits, as the wave's ballot -- every
// lane is here, so no atomic is needed.  Lane 0 writes the word and adds its popcount to `hits` and, with reference words, the bits
// in common to `common`; wi >= W: no atom of the pocket, the word is 0.
template <int T>
__device__ __forceinline__ void pw_word(const TdProteinSide &p, size_t mol, int t, int wi, bool hit, int &hits, int &common) {
    const unsigned long long word = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && wi < p.W) {
        if (p.bits) p.bits[(mol * T + t) * (size_t)p.W + wi] = word;
        hits += __popcll(word);
        if (p.ref_bits) common += __popcll(word & p.ref_bits[(size_t)t * p.W + wi]);
    }
}

// The limit of the root: with L the largest distance limit of the report, the float64 above rn(L L), which is >= L^2 in the reals (rn(L L)
// is within half an ulp of it).  A pair with d2 >= it has sqrt(d2) >= L in the reals, so its rounded root is >= L too (rounding is
// monotone and L is a float64): it is below no limit, and skipping its root removes nothing.  EXPERIMENTS.md "Pocket contacts" has what
// it saves.
inline double pw_reject2(double L) { return std::nextafter(L * L, std::numeric_limits<double>::infinity()); }

// The launch of a pair kernel over the M = S B (frame, molecule) workgroups, after kind_hist [S, rows, n_kinds] and pocket_freq
// [S, T, Np] are zeroed on the stream
template <typename Args>
int pw_launch(void (*kernel)(Args), const Args &g, int rows, int T, hipStream_t s) {
    const TdProteinSide &p = g.p;
    if (g.b.S > 0) {
        TD_CHECK_HIP(hipMemsetAsync(p.kind_hist, 0, (size_t)g.b.S * rows * p.n_kinds * sizeof(unsigned long long), s));
        if (p.Np > 0) TD_CHECK_HIP(hipMemsetAsync(p.pocket_freq, 0, (size_t)g.b.S * T * p.Np * sizeof(int32_t), s));
    }
    const int64_t M = (int64_t)g.b.S * g.b.B;
    if (M == 0) return TD_OK;
    kernel<<<dim3((unsigned)M), dim3(PW_T), 0, s>>>(g);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}
