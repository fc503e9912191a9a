// The bond-order rule of a pair of atoms ("Sample quality" and "Bond graph"): utils/evaluation/analyze.py
// get_bond_order on a float64 distance.  One copy, shared by quality.hip (which sums the orders) and bonds.hip (which keeps the bonds).
#pragma once
#include "td_device.h"

// Single, double and triple bond lengths in picometres (wiredchemist.com bond energies and lengths, the table the reference cites), as
// flat 8 x 8 matrices over H C N O F P S Cl; -1: no such bond.  The margins follow below.
__constant__ const int16_t TD_BOND_PM[3][64] = {
    {74,  109, 101, 96,  92,  144, 134, 127,     109, 154, 147, 143, 135, 184, 182, 177,     101, 147, 145, 140, 136, 177, 168, 175,
     96,  143, 140, 148, 142, 163, 151, 164,     92,  135, 136, 142, 142, 156, 158, 166,     144, 184, 177, 163, 156, 221, 210, 203,
     134, 182, 168, 151, 158, 210, 204, 207,     127, 177, 175, 164, 166, 203, 207, 199},
    {-1, -1,  -1,  -1,  -1, -1,  -1,  -1,        -1, 134, 129, 120, -1, -1,  160, -1,        -1, 129, 125, 121, -1, -1,  -1,  -1,
     -1, 120, 121, 121, -1, 150, -1,  -1,        -1, -1,  -1,  -1,  -1, -1,  -1,  -1,        -1, -1,  -1,  150, -1, -1,  186, -1,
     -1, 160, -1,  -1,  -1, 186, -1,  -1,        -1, -1,  -1,  -1,  -1, -1,  -1,  -1},
    {-1, -1,  -1,  -1,  -1, -1, -1, -1,          -1, 120, 116, 113, -1, -1, -1, -1,          -1, 116, 110, -1,  -1, -1, -1, -1,
     -1, 113, -1,  -1,  -1, -1, -1, -1,          -1, -1,  -1,  -1,  -1, -1, -1, -1,          -1, -1,  -1,  -1,  -1, -1, -1, -1,
     -1, -1,  -1,  -1,  -1, -1, -1, -1,          -1, -1,  -1,  -1,  -1, -1, -1, -1}};
__constant__ const int16_t TD_BOND_MARGIN[3] = {10, 5, 3};

// thr[k][e1 * 8 + e2] = bond length + margin of order k + 1 as float64, filled by the whole workgroup (a barrier follows at the caller)
__device__ __forceinline__ void td_bond_thresholds(double (*thr)[64], int tid, int threads) {
    for (int k = tid; k < 3 * 64; k += threads) thr[k >> 6][k & 63] = (double)(TD_BOND_PM[k >> 6][k & 63] + TD_BOND_MARGIN[k >> 6]);
}

// The squared distance of the rule: atom i at float64-widened (xi, yi, zi), atom j at fp32 (xj, yj, zj), (dx dx + dy dy) + dz dz in
// float64 with every product and sum rounded on its own.  The rule's distance is the IEEE sqrt of it; pocket.hip takes that root
// only of the pairs that can fall below a limit, and of a minimum once (the root is monotone).
__device__ __forceinline__ double td_pair_dist2(double xi, double yi, double zi, float xj, float yj, float zj) {
    const double dx = xi - (double)xj, dy = yi - (double)yj, dz = zi - (double)zj;
    return td_add_rn64(td_add_rn64(td_mul_rn64(dx, dx), td_mul_rn64(dy, dy)), td_mul_rn64(dz, dz));
}

// Order 0 / 1 / 2 / 3 of the pair (atom i at float64-widened (xi, yi, zi), atom j at fp32 (xj, yj, zj)) whose element pair is
// pr = e_i * 8 + e_j, and its distance d = sqrt((dx dx + dy dy) + dz dz) in float64 with every product and sum rounded on its own
// (numpy's order), IEEE sqrt, compared as D = 100 d: an order flips exactly where the reference's flips.  (i, j) and (j, i) give the
// same bits: the differences only change sign.
__device__ __forceinline__ int td_bond_order(double xi, double yi, double zi, float xj, float yj, float zj, int pr,
                                             const double (*thr)[64], double &d) {
    d = sqrt(td_pair_dist2(xi, yi, zi, xj, yj, zj));
    const double D = td_mul_rn64(100.0, d);
    if (D < thr[0][pr]) return D < thr[1][pr] ? (D < thr[2][pr] ? 3 : 2) : 1;
    return 0;
}
