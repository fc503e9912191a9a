// The term arithmetic of one counted pair of the docking-style score (score.hip, relax.hip; DESIGN.md section 3, "Docking-style score"
// and "Pose relaxation"): one copy, so that the relaxation minimises exactly what td_score_report reports.
#pragma once
#include "td_pocket_walk.h"

constexpr int SC_T = PW_T, SC_TERMS = TD_SCORE_TERMS, SC_PE = TD_POCKET_ELEMENTS;

// a term value in units of 2^-24: ldexp is exact, llrint rounds to nearest, ties to even
__device__ __forceinline__ long long sc_fixed(double value) { return llrint(ldexp(value, TD_SCORE_FRAC_BITS)); }

// what the derivative needs of a pair's terms: t = 2 d and e1 = exp(-t t), u = (d - 3) / 2 and e2 = exp(-u u), and whether the roles
// admit the hydrophobic and the hydrogen-bond term
struct ScPair {
    double t, e1, u, e2;
    bool hy, hb;
};

// The five term values of a pair at surface distance d, ligand role lr and protein role pr, each added to acc in units of 2^-24:
// float64 with every product, sum and difference rounded on its own.
__device__ __forceinline__ ScPair sc_pair_terms(double d, int lr, int pr, long long (&acc)[SC_TERMS]) {
    ScPair k;
    const double t = td_mul_rn64(d, 2.0);
    k.t = t;
    k.e1 = exp(-td_mul_rn64(t, t));
    acc[0] += sc_fixed(k.e1);
    const double u = td_add_rn64(d, -3.0) / 2.0;
    k.u = u;
    k.e2 = exp(-td_mul_rn64(u, u));
    acc[1] += sc_fixed(k.e2);
    if (d < 0.0) acc[2] += sc_fixed(td_mul_rn64(d, d));
    k.hy = (lr & TD_ROLE_HYDROPHOBIC) && (pr & TD_ROLE_HYDROPHOBIC);
    if (k.hy && d < 1.5) acc[3] += sc_fixed(d < 0.5 ? 1.0 : td_add_rn64(1.5, -d));
    k.hb = ((lr & TD_ROLE_DONOR) && (pr & TD_ROLE_ACCEPTOR)) || ((lr & TD_ROLE_ACCEPTOR) && (pr & TD_ROLE_DONOR));
    if (k.hb && d < 0.0) acc[4] += sc_fixed(d < -0.7 ? 1.0 : (-d) / 0.7);
    return k;
}
