// Rigid-body relaxation of ligand frames under the docking-style score (gfx950, wave64; DESIGN.md section 3, "Pose relaxation"): a local
// optimisation under this project's heuristic score, not AutoDock Vina's `minimize`.  Rigid-body only: three translations and three
// rotations, no torsions.
//   * relax_kernel  one workgroup of four waves per (frame, molecule), alive through every iteration: no host round trip, no grid-wide
//                   synchronisation.  Staged once into LDS: the molecule (pw_stage), the roles of the INPUT pose (ix_ligand_role; a rigid
//                   motion cannot change chemistry and rounding must not either), x0 = x - c0 in float64 for every atom (c0: the
//                   centroid of the scored atoms, summed in index order), and a compact list of the protein atoms that take part and lie
//                   within R_mol + cutoff + max_shift (+ slack) of c0, as float4 with element and role packed into w: a superset of what
//                   any reachable pose can count, so an evaluation reads no global memory.  More candidates than the list holds: the
//                   evaluation walks the pocket in global memory instead; the pairs and their arithmetic are the same, and so are the
//                   integers.
//                   An evaluation at the state (q, t): the pose fp32(R(q) x0 + (c0 + t)) into LDS, then threads own list entries at
//                   stride 256 and read the scored ligand atoms as LDS broadcasts (score_kernel's loop).  A counted pair adds its five
//                   term values (sc_pair_terms, the copy score_kernel runs) and the six components of its gradient, each rounded to
//                   units of 2^-24 and added as int64: f = dE/dd in float64 in a fixed operation order, g = f (x_l - x_p) / r, the
//                   components g and (x_l - c) x g.  The sums are exact whatever the order of arrival; they meet in LDS integer adds.
//                   Thread 0 then advances a BFGS iteration with an Armijo backtracking line search on the 6-vector, in float64
//                   (rx_advance), and publishes the next trial state or the stop.
// Every loop is bounded: the main loop by max_evals, a line search by TD_RELAX_TRIALS, the rest by the sizes.  No floating-point atomic,
// no device-side assert, no spin.  The answer to an oversize molecule (-1, INT64_MIN) is that of score.hip.
#include "td_score_terms.h"

#include <algorithm>
#include <climits>

constexpr int RX_T = SC_T, RX_DOF = TD_RELAX_DOF, RX_SUMS = SC_TERMS + RX_DOF;

// the optimiser's state, in LDS; thread 0 alone writes it.  qn, tn and stop are what the workgroup reads.
struct RxOpt {
    double H[RX_DOF * RX_DOF], g[RX_DOF], gn[RX_DOF], p[RX_DOF], y[RX_DOF], Hy[RX_DOF];
    double q[4], t[3], qn[4], tn[3], c0[3];
    double hr, reach2, f0, alpha, slope;
    long long terms[SC_TERMS];
    int pairs, steps, evals, status, trial, stop;
};

// the rotation matrix of a unit quaternion (w, x, y, z), every product and sum rounded on its own
__device__ __forceinline__ void rx_matrix(const double *q, double (&R)[9]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double xx = td_mul_rn64(x, x), yy = td_mul_rn64(y, y), zz = td_mul_rn64(z, z);
    const double xy = td_mul_rn64(x, y), xz = td_mul_rn64(x, z), yz = td_mul_rn64(y, z);
    const double wx = td_mul_rn64(w, x), wy = td_mul_rn64(w, y), wz = td_mul_rn64(w, z);
    R[0] = td_add_rn64(1.0, -td_mul_rn64(2.0, td_add_rn64(yy, zz)));
    R[1] = td_mul_rn64(2.0, td_add_rn64(xy, -wz));
    R[2] = td_mul_rn64(2.0, td_add_rn64(xz, wy));
    R[3] = td_mul_rn64(2.0, td_add_rn64(xy, wz));
    R[4] = td_add_rn64(1.0, -td_mul_rn64(2.0, td_add_rn64(xx, zz)));
    R[5] = td_mul_rn64(2.0, td_add_rn64(yz, -wx));
    R[6] = td_mul_rn64(2.0, td_add_rn64(xz, -wy));
    R[7] = td_mul_rn64(2.0, td_add_rn64(yz, wx));
    R[8] = td_add_rn64(1.0, -td_mul_rn64(2.0, td_add_rn64(xx, yy)));
}

// The pose of the state (q, t) into s_at: atom i at fp32(((R0 x0 + R1 y0) + R2 z0) + c), c = c0 + t; the element in w stays.
__device__ __forceinline__ void rx_pose(int n, const double *s_x0, const double *q, const double *t, const double *c0, float4 *s_at) {
    double R[9];
    rx_matrix(q, R);
    const double cx = td_add_rn64(c0[0], t[0]), cy = td_add_rn64(c0[1], t[1]), cz = td_add_rn64(c0[2], t[2]);
    for (int i = threadIdx.x; i < n; i += RX_T) {
        const double x = s_x0[3 * i], y = s_x0[3 * i + 1], z = s_x0[3 * i + 2];
        const double px = td_add_rn64(td_add_rn64(td_add_rn64(td_mul_rn64(R[0], x), td_mul_rn64(R[1], y)), td_mul_rn64(R[2], z)), cx);
        const double py = td_add_rn64(td_add_rn64(td_add_rn64(td_mul_rn64(R[3], x), td_mul_rn64(R[4], y)), td_mul_rn64(R[5], z)), cy);
        const double pz = td_add_rn64(td_add_rn64(td_add_rn64(td_mul_rn64(R[6], x), td_mul_rn64(R[7], y)), td_mul_rn64(R[8], z)), cz);
        s_at[i].x = (float)px; s_at[i].y = (float)py; s_at[i].z = (float)pz;
    }
}

// One protein atom (X, Y, Z), element pe, role pr >= 0, against the scored ligand atoms of the pose in s_at: terms, gradient, pairs.
// (cx, cy, cz): the centre the torque is taken about.
__device__ __forceinline__ void rx_protein_atom(const TdRelaxArgs &g, int n, const float4 *s_at, const int *s_role, const double *s_rsum,
                                                double X, double Y, double Z, int pe, int pr, double cx, double cy, double cz,
                                                long long (&acc)[SC_TERMS], long long (&grad)[RX_DOF], int &pairs) {
    for (int i = 0; i < n; ++i) {
        const int lr = s_role[i];                                               // every lane reads the same address: an LDS broadcast
        if (lr < 0) continue;
        const float4 q = s_at[i];
        const double d2 = td_pair_dist2(X, Y, Z, q.x, q.y, q.z);
        if (!(d2 < g.sc.reject2)) continue;
        const double rr = sqrt(d2);
        if (!(rr < g.sc.cutoff)) continue;
        const double d = td_add_rn64(rr, -s_rsum[__float_as_int(q.w) * SC_PE + pe]);
        ++pairs;
        const ScPair k = sc_pair_terms(d, lr, pr, acc);
        // f = dE/dd: zero on the flat pieces, at a breakpoint the piece that the term value takes, no derivative of the cutoff
        const double dg1 = td_mul_rn64(td_mul_rn64(-4.0, k.t), k.e1);
        const double dg2 = td_mul_rn64(-k.u, k.e2);
        const double drep = d < 0.0 ? k.t : 0.0;
        const double dhy = (k.hy && d < 1.5 && !(d < 0.5)) ? -1.0 : 0.0;
        const double dhb = (k.hb && d < 0.0 && !(d < -0.7)) ? -1.0 / 0.7 : 0.0;
        const double f = td_add_rn64(td_add_rn64(td_add_rn64(td_add_rn64(td_mul_rn64(g.w[0], dg1), td_mul_rn64(g.w[1], dg2)),
                                                             td_mul_rn64(g.w[2], drep)), td_mul_rn64(g.w[3], dhy)), td_mul_rn64(g.w[4], dhb));
        if (!(rr > 0.0)) continue;                                              // coincident atoms: no direction
        const double lx = (double)q.x, ly = (double)q.y, lz = (double)q.z;
        const double gx = td_mul_rn64(f, td_add_rn64(lx, -X) / rr), gy = td_mul_rn64(f, td_add_rn64(ly, -Y) / rr),
                     gz = td_mul_rn64(f, td_add_rn64(lz, -Z) / rr);
        const double ax = td_add_rn64(lx, -cx), ay = td_add_rn64(ly, -cy), az = td_add_rn64(lz, -cz);
        grad[0] += sc_fixed(gx);
        grad[1] += sc_fixed(gy);
        grad[2] += sc_fixed(gz);
        grad[3] += sc_fixed(td_add_rn64(td_mul_rn64(ay, gz), -td_mul_rn64(az, gy)));
        grad[4] += sc_fixed(td_add_rn64(td_mul_rn64(az, gx), -td_mul_rn64(ax, gz)));
        grad[5] += sc_fixed(td_add_rn64(td_mul_rn64(ax, gy), -td_mul_rn64(ay, gx)));
    }
}

__device__ __forceinline__ void rx_reset_H(RxOpt &o) {
    for (int k = 0; k < RX_DOF * RX_DOF; ++k) o.H[k] = 0.0;
    for (int k = 0; k < RX_DOF; ++k) o.H[k * RX_DOF + k] = k < 3 ? 1.0 : o.hr;
}

// p = -H g and the slope g . p
__device__ __forceinline__ void rx_direction(RxOpt &o) {
    double slope = 0.0;
    for (int i = 0; i < RX_DOF; ++i) {
        double v = 0.0;
        for (int j = 0; j < RX_DOF; ++j) v += o.H[i * RX_DOF + j] * o.g[j];
        o.p[i] = -v;
        slope += o.g[i] * -v;
    }
    o.slope = slope;
}

// The next trial of the running line search into (qn, tn), or the stop: out of evaluations (2), or TD_RELAX_TRIALS failed trials (1).  A
// trial whose centre leaves the ball of max_shift around c0 fails without an evaluation (4).  The rotation increment of omega is the
// normalised quaternion (1, omega / 2), composed on the left and renormalised: sqrt and division only.
__device__ __forceinline__ void rx_next_trial(RxOpt &o, const TdRelaxArgs &g) {
    for (; o.trial < TD_RELAX_TRIALS; ++o.trial, o.alpha *= 0.5) {
        if (o.evals >= g.max_evals) { o.status |= 2; o.stop = 1; return; }
        const double a = o.alpha;
        const double tx = o.t[0] + a * o.p[0], ty = o.t[1] + a * o.p[1], tz = o.t[2] + a * o.p[2];
        if (!(sqrt(tx * tx + ty * ty + tz * tz) <= g.max_shift)) { o.status |= 4; continue; }
        const double hx = 0.5 * a * o.p[3], hy = 0.5 * a * o.p[4], hz = 0.5 * a * o.p[5];
        const double nrm = sqrt(1.0 + (hx * hx + hy * hy + hz * hz));
        const double dw = 1.0 / nrm, dx = hx / nrm, dy = hy / nrm, dz = hz / nrm;
        const double qw = o.q[0], qx = o.q[1], qy = o.q[2], qz = o.q[3];
        const double w = dw * qw - dx * qx - dy * qy - dz * qz, x = dw * qx + dx * qw + dy * qz - dz * qy,
                     y = dw * qy - dx * qz + dy * qw + dz * qx, z = dw * qz + dx * qy - dy * qx + dz * qw;
        const double len = sqrt(w * w + x * x + y * y + z * z);
        if (!(len > 0.0) || !(len < 2.0)) continue;                             // not finite: a failed trial, no evaluation
        o.qn[0] = w / len; o.qn[1] = x / len; o.qn[2] = y / len; o.qn[3] = z / len;
        o.tn[0] = tx; o.tn[1] = ty; o.tn[2] = tz;
        return;
    }
    o.status |= 1;
    o.stop = 1;
}

// a new line search from the accepted state: the direction -H g, H reset to H0 where that is no descent direction; none even then: the
// gradient is zero, converged (1)
__device__ __forceinline__ void rx_line_search(RxOpt &o, const TdRelaxArgs &g) {
    rx_direction(o);
    if (!(o.slope < 0.0)) {
        rx_reset_H(o);
        rx_direction(o);
        if (!(o.slope < 0.0)) { o.status |= 1; o.stop = 1; return; }
    }
    o.alpha = 1.0;
    o.trial = 0;
    rx_next_trial(o, g);
}

// Thread 0, after an evaluation whose sums are in s_sum and s_pairs: the first one (`first`) fixes f0 and the gradient of the input pose;
// a later one is a trial of the line search, accepted when f1 - f0 < c1 alpha slope (Armijo) and then followed by the BFGS update of
// the inverse Hessian where s . y > 0.
__device__ __forceinline__ void rx_advance(RxOpt &o, const TdRelaxArgs &g, const unsigned long long *s_sum, int pairs, bool first, size_t mol) {
    double T[SC_TERMS], gn[RX_DOF];
    for (int k = 0; k < SC_TERMS; ++k) T[k] = ldexp((double)(long long)s_sum[k], -TD_SCORE_FRAC_BITS);
    for (int k = 0; k < RX_DOF; ++k) gn[k] = ldexp((double)(long long)s_sum[SC_TERMS + k], -TD_SCORE_FRAC_BITS);
    const double f1 = td_add_rn64(td_add_rn64(td_add_rn64(td_add_rn64(td_mul_rn64(g.w[0], T[0]), td_mul_rn64(g.w[1], T[1])),
                                                          td_mul_rn64(g.w[2], T[2])), td_mul_rn64(g.w[3], T[3])), td_mul_rn64(g.w[4], T[4]));
    ++o.evals;
    if (first) {
        for (int k = 0; k < SC_TERMS; ++k) {
            o.terms[k] = (long long)s_sum[k];
            g.terms_in[mol * SC_TERMS + k] = o.terms[k];
        }
        for (int k = 0; k < RX_DOF; ++k) {
            o.g[k] = gn[k];
            g.grad_in[mol * RX_DOF + k] = (long long)s_sum[SC_TERMS + k];
        }
        o.pairs = pairs;
        o.f0 = f1;
        if (o.steps >= g.max_steps) { o.status |= 2; o.stop = 1; return; }
        rx_line_search(o, g);
        return;
    }
    if (!(f1 - o.f0 < TD_RELAX_ARMIJO * o.alpha * o.slope)) {                  // failed: halve the step
        o.alpha *= 0.5;
        ++o.trial;
        rx_next_trial(o, g);
        return;
    }
    double sy = 0.0;
    for (int k = 0; k < RX_DOF; ++k) {
        o.y[k] = gn[k] - o.g[k];
        o.g[k] = gn[k];
        o.p[k] *= o.alpha;                                                      // s, the step taken
        sy += o.p[k] * o.y[k];
    }
    for (int k = 0; k < 4; ++k) o.q[k] = o.qn[k];
    for (int k = 0; k < 3; ++k) o.t[k] = o.tn[k];
    for (int k = 0; k < SC_TERMS; ++k) o.terms[k] = (long long)s_sum[k];
    o.pairs = pairs;
    o.f0 = f1;
    ++o.steps;
    if (o.steps >= g.max_steps) { o.status |= 2; o.stop = 1; return; }
    if (sy > 0.0) {                                                             // H += (1 + y'Hy / sy) s s' / sy - (Hy s' + s (Hy)') / sy
        double yHy = 0.0;
        for (int i = 0; i < RX_DOF; ++i) {
            double v = 0.0;
            for (int j = 0; j < RX_DOF; ++j) v += o.H[i * RX_DOF + j] * o.y[j];
            o.Hy[i] = v;
            yHy += o.y[i] * v;
        }
        const double r = 1.0 / sy, c = (1.0 + yHy * r) * r;
        for (int i = 0; i < RX_DOF; ++i)
            for (int j = 0; j < RX_DOF; ++j) o.H[i * RX_DOF + j] += c * o.p[i] * o.p[j] - r * (o.Hy[i] * o.p[j] + o.p[i] * o.Hy[j]);
    }
    rx_line_search(o, g);
}

__global__ __launch_bounds__(RX_T) void relax_kernel(TdRelaxArgs g) {
    const TdScoreArgs &sc = g.sc;
    const TdBondArgs &a = sc.b;
    extern __shared__ __attribute__((aligned(16))) float4 s_list[];             // [g.list_capacity]: (x, y, z, element | role << 8)
    __shared__ float4 s_at[BG_MAX];
    __shared__ double s_x0[BG_MAX * 3];
    __shared__ int s_role[BG_MAX];                                              // -1: the atom takes no part (no class, or H)
    __shared__ double s_thr[3][64], s_rsum[8 * SC_PE];
    __shared__ int s_elem[TD_QUALITY_MAX_CLASSES];
    __shared__ unsigned long long s_sum[RX_SUMS];
    __shared__ int s_pairs, s_cnt;
    __shared__ RxOpt o;
    const int tid = threadIdx.x;
    const BgMol m = bg_molecule<BG_MAX>(a);
    const TdProteinSide &ps = sc.p;
    const int Np = ps.Np;
    if (m.bad) {                                                                // workgroup-uniform; the positions are the launcher's copy
        if (tid == 0) {
            g.n_pairs_out[m.mol] = -1; g.status[m.mol] = -1; g.n_steps[m.mol] = 0; g.n_evals[m.mol] = 0;
        }
        if (tid < SC_TERMS) g.terms_in[m.mol * SC_TERMS + tid] = g.terms_out[m.mol * SC_TERMS + tid] = LLONG_MIN;
        if (tid < RX_DOF) g.grad_in[m.mol * RX_DOF + tid] = 0;
        if (tid < 7) g.transform[m.mol * 7 + tid] = tid == 0 ? 1.0 : 0.0;
        return;
    }
    const int n = m.n;
    if (tid < TD_QUALITY_MAX_CLASSES) s_elem[tid] = tid < a.K ? a.elem[tid] : -1;
    td_bond_thresholds(s_thr, tid, RX_T);
    if (tid < 8 * SC_PE) s_rsum[tid] = sc.rsum[tid];
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    pw_stage(a, m, s_elem, s_at);
    __syncthreads();
    for (int i = tid; i < n; i += RX_T) {
        const int el = __float_as_int(s_at[i].w);
        s_role[i] = el > IX_H ? ix_ligand_role(i, n, s_at, s_thr) : -1;
    }
    __syncthreads();
    if (tid == 0) {                                                             // c0: the scored atoms in index order
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int ns = 0;
        for (int i = 0; i < n; ++i)
            if (s_role[i] >= 0) { sx += (double)s_at[i].x; sy += (double)s_at[i].y; sz += (double)s_at[i].z; ++ns; }
        o.c0[0] = ns ? sx / (double)ns : 0.0; o.c0[1] = ns ? sy / (double)ns : 0.0; o.c0[2] = ns ? sz / (double)ns : 0.0;
    }
    __syncthreads();
    for (int i = tid; i < n; i += RX_T) {
        s_x0[3 * i] = td_add_rn64((double)s_at[i].x, -o.c0[0]);
        s_x0[3 * i + 1] = td_add_rn64((double)s_at[i].y, -o.c0[1]);
        s_x0[3 * i + 2] = td_add_rn64((double)s_at[i].z, -o.c0[2]);
    }
    __syncthreads();
    if (tid == 0) {
        double sum2 = 0.0, max2 = 0.0;
        int ns = 0;
        for (int i = 0; i < n; ++i)
            if (s_role[i] >= 0) {
                const double x = s_x0[3 * i], y = s_x0[3 * i + 1], z = s_x0[3 * i + 2];
                const double r2 = td_add_rn64(td_add_rn64(td_mul_rn64(x, x), td_mul_rn64(y, y)), td_mul_rn64(z, z));
                sum2 += r2;
                max2 = r2 > max2 ? r2 : max2;
                ++ns;
            }
        const double msq = ns ? sum2 / (double)ns : 0.0;
        o.hr = msq > 0.0 ? 1.0 / msq : 1.0;
        // what a reachable pose can count lies within R_mol + max_shift + cutoff of c0; the slack covers the fp32 rounding of a pose
        const double rmol = sqrt(max2);
        const double reach = rmol + sc.cutoff + g.max_shift + 1e-3 + 1e-6 * (fabs(o.c0[0]) + fabs(o.c0[1]) + fabs(o.c0[2]) + rmol + g.max_shift);
        o.reach2 = reach * reach;
        o.q[0] = o.qn[0] = 1.0;
        for (int k = 1; k < 4; ++k) o.q[k] = o.qn[k] = 0.0;
        for (int k = 0; k < 3; ++k) o.t[k] = o.tn[k] = 0.0;
        o.pairs = o.steps = o.evals = o.status = o.trial = o.stop = 0;
        o.f0 = o.alpha = o.slope = 0.0;
        rx_reset_H(o);
    }
    __syncthreads();
    const int cap = g.list_capacity;
    for (int j = tid; j < Np; j += RX_T) {
        int kp = 0;
        double X = 0.0, Y = 0.0, Z = 0.0;
        pw_protein_atom(ps, j, kp, X, Y, Z);
        const int pe = ps.pelem[j];
        const int pr = pe == 0 ? -1 : sc.role[j];                               // >= 0: the atom takes part, so its element is in range
        if (pr < 0) continue;
        const float *P = ps.ppos + (size_t)j * 3;
        if (!(td_pair_dist2(o.c0[0], o.c0[1], o.c0[2], P[0], P[1], P[2]) <= o.reach2)) continue;
        const int slot = atomicAdd(&s_cnt, 1);
        if (slot < cap) s_list[slot] = make_float4(P[0], P[1], P[2], __int_as_float(pe | (pr << 8)));
    }
    __syncthreads();
    const int cnt = s_cnt;
    const bool listed = cnt <= cap;                                             // workgroup-uniform

    for (int it = 0; it < g.max_evals; ++it) {
        if (tid < RX_SUMS) s_sum[tid] = 0ull;
        if (tid == 0) s_pairs = 0;
        if (it > 0) rx_pose(n, s_x0, o.qn, o.tn, o.c0, s_at);                   // the first evaluation is of the input pose itself
        __syncthreads();
        const double cx = td_add_rn64(o.c0[0], o.tn[0]), cy = td_add_rn64(o.c0[1], o.tn[1]), cz = td_add_rn64(o.c0[2], o.tn[2]);
        long long acc[SC_TERMS] = {0, 0, 0, 0, 0}, grad[RX_DOF] = {0, 0, 0, 0, 0, 0};
        int pairs = 0;
        if (listed) {
            for (int e = tid; e < cnt; e += RX_T) {
                const float4 P = s_list[e];
                const int code = __float_as_int(P.w);
                rx_protein_atom(g, n, s_at, s_role, s_rsum, (double)P.x, (double)P.y, (double)P.z, code & 0xff, code >> 8, cx, cy, cz, acc,
                                grad, pairs);
            }
        } else {
            for (int j = tid; j < Np; j += RX_T) {
                int kp = 0;
                double X = 0.0, Y = 0.0, Z = 0.0;
                pw_protein_atom(ps, j, kp, X, Y, Z);
                const int pe = ps.pelem[j];
                const int pr = pe == 0 ? -1 : sc.role[j];
                if (pr >= 0) rx_protein_atom(g, n, s_at, s_role, s_rsum, X, Y, Z, pe, pr, cx, cy, cz, acc, grad, pairs);
            }
        }
#pragma unroll
        for (int t = 0; t < SC_TERMS; ++t)
            if (acc[t]) atomicAdd(&s_sum[t], (unsigned long long)acc[t]);
#pragma unroll
        for (int t = 0; t < RX_DOF; ++t)
            if (grad[t]) atomicAdd(&s_sum[SC_TERMS + t], (unsigned long long)grad[t]);
        if (pairs) atomicAdd(&s_pairs, pairs);
        __syncthreads();
        if (tid == 0) rx_advance(o, g, s_sum, s_pairs, it == 0, m.mol);
        __syncthreads();
        if (o.stop) break;                                                      // workgroup-uniform
    }

    if (o.steps > 0) {                                                          // the molecule moved: the pose of the accepted state
        __syncthreads();
        rx_pose(n, s_x0, o.q, o.t, o.c0, s_at);
        __syncthreads();
        for (int i = tid; i < n; i += RX_T) {
            float *p = g.pos_out + ((size_t)m.s * (size_t)a.Nl + (size_t)(m.l0 + i)) * 3;
            p[0] = s_at[i].x; p[1] = s_at[i].y; p[2] = s_at[i].z;
        }
    }
    if (tid == 0) {
        g.n_pairs_out[m.mol] = o.pairs; g.n_steps[m.mol] = o.steps; g.n_evals[m.mol] = o.evals; g.status[m.mol] = o.status;
    }
    if (tid < SC_TERMS) g.terms_out[m.mol * SC_TERMS + tid] = o.terms[tid];
    if (tid < 7) g.transform[m.mol * 7 + tid] = tid < 4 ? o.q[tid] : o.t[tid - 4];
}

// The protein roles are resolved by the caller, on the same stream (td_launch_protein_roles); the rotor kernel counts the rotatable
// bonds of the input pose.
int td_launch_score_minimize(const TdRelaxArgs &args, hipStream_t s) {
    static TdLdsOnce once;
    TdRelaxArgs g = args;
    g.sc.reject2 = pw_reject2(g.sc.cutoff);
    const size_t coords = (size_t)g.sc.b.S * (size_t)g.sc.b.Nl * 3;
    if (coords) TD_CHECK_HIP(hipMemcpyAsync(g.pos_out, g.sc.b.pos, coords * sizeof(float), hipMemcpyDeviceToDevice, s));
    const int64_t M = (int64_t)g.sc.b.S * g.sc.b.B;
    if (M == 0) return TD_OK;
    g.list_capacity = std::max(0, std::min(std::min(g.list_capacity, TD_RELAX_LIST_CAPACITY), g.sc.p.Np));
    if (const int rc = td_set_lds(once, reinterpret_cast<const void *>(relax_kernel), (size_t)TD_RELAX_LIST_CAPACITY * sizeof(float4))) return rc;
    relax_kernel<<<dim3((unsigned)M), dim3(RX_T), (size_t)g.list_capacity * sizeof(float4), s>>>(g);
    TD_CHECK_HIP(hipGetLastError());
    return td_launch_rotors(g.sc, s);
}
