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
// The staging (rx_stage), one evaluation (rx_evaluate), rx_advance and the loop of the two (rx_descend) are device functions that the
// docking search at the end of this file (dock_kernel, dock_select_kernel; td_score_dock) runs too: each block of arithmetic is
// written once.
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

// Thread 0, after an evaluation whose sums are in s_sum and s_pairs: the first one (`first`) fixes f0 and the gradient of the state the
// descent starts from, and records its integers in terms_in [SC_TERMS] and grad_in [RX_DOF] where those are given (the input pose's);
// a later one is a trial of the line search, accepted when f1 - f0 < c1 alpha slope (Armijo) and then followed by the BFGS update of
// the inverse Hessian where s . y > 0.
__device__ __forceinline__ void rx_advance(RxOpt &o, const TdRelaxArgs &g, const unsigned long long *s_sum, int pairs, bool first,
                                           long long *terms_in, long long *grad_in) {
    double T[SC_TERMS], gn[RX_DOF];
    for (int k = 0; k < SC_TERMS; ++k) T[k] = ldexp((double)(long long)s_sum[k], -TD_SCORE_FRAC_BITS);
    for (int k = 0; k < RX_DOF; ++k) gn[k] = ldexp((double)(long long)s_sum[SC_TERMS + k], -TD_SCORE_FRAC_BITS);
    const double f1 = td_add_rn64(td_add_rn64(td_add_rn64(td_add_rn64(td_mul_rn64(g.w[0], T[0]), td_mul_rn64(g.w[1], T[1])),
                                                          td_mul_rn64(g.w[2], T[2])), td_mul_rn64(g.w[3], T[3])), td_mul_rn64(g.w[4], T[4]));
    ++o.evals;
    if (first) {
        for (int k = 0; k < SC_TERMS; ++k) {
            o.terms[k] = (long long)s_sum[k];
            if (terms_in) terms_in[k] = o.terms[k];
        }
        for (int k = 0; k < RX_DOF; ++k) {
            o.g[k] = gn[k];
            if (grad_in) grad_in[k] = (long long)s_sum[SC_TERMS + k];
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

// What a workgroup keeps of its molecule in LDS (the list of protein atoms is the kernel's dynamic LDS, after it)
struct RxStage {
    float4 at[BG_MAX];
    double x0[BG_MAX * 3];
    int role[BG_MAX];                                                           // -1: the atom takes no part (no class, or H)
    double thr[3][64], rsum[8 * SC_PE];
    int elem[TD_QUALITY_MAX_CLASSES];
    unsigned long long sum[RX_SUMS];
    int pairs, cnt;
    RxOpt o;
};

// Thread 0: the descent starts anew at the state (q, t), with its budget whole and H = H0
__device__ __forceinline__ void rx_begin(RxOpt &o, const double *q, const double *t, int status) {
    for (int k = 0; k < 4; ++k) o.q[k] = o.qn[k] = q[k];
    for (int k = 0; k < 3; ++k) o.t[k] = o.tn[k] = t[k];
    o.pairs = o.steps = o.evals = o.trial = o.stop = 0;
    o.status = status;
    o.f0 = o.alpha = o.slope = 0.0;
    rx_reset_H(o);
}

// The staging of a molecule that is not `bad`: the molecule, the roles of the input pose, c0, x0, hr and the reach, the state at the
// identity, and (with_list) the protein atoms within reach into s_list.  Returns the number of candidates, which exceeds
// g.list_capacity when the list does not hold them (workgroup-uniform).
__device__ __forceinline__ int rx_stage(const TdRelaxArgs &g, const BgMol &m, RxStage &sh, float4 *s_list, bool with_list) {
    const TdScoreArgs &sc = g.sc;
    const TdBondArgs &a = sc.b;
    const TdProteinSide &ps = sc.p;
    RxOpt &o = sh.o;
    const int tid = threadIdx.x, n = m.n, Np = ps.Np;
    if (tid < TD_QUALITY_MAX_CLASSES) sh.elem[tid] = tid < a.K ? a.elem[tid] : -1;
    td_bond_thresholds(sh.thr, tid, RX_T);
    if (tid < 8 * SC_PE) sh.rsum[tid] = sc.rsum[tid];
    if (tid == 0) sh.cnt = 0;
    __syncthreads();
    pw_stage(a, m, sh.elem, sh.at);
    __syncthreads();
    for (int i = tid; i < n; i += RX_T) {
        const int el = __float_as_int(sh.at[i].w);
        sh.role[i] = el > IX_H ? ix_ligand_role(i, n, sh.at, sh.thr) : -1;
    }
    __syncthreads();
    if (tid == 0) {                                                             // c0: the scored atoms in index order
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int ns = 0;
        for (int i = 0; i < n; ++i)
            if (sh.role[i] >= 0) { sx += (double)sh.at[i].x; sy += (double)sh.at[i].y; sz += (double)sh.at[i].z; ++ns; }
        o.c0[0] = ns ? sx / (double)ns : 0.0; o.c0[1] = ns ? sy / (double)ns : 0.0; o.c0[2] = ns ? sz / (double)ns : 0.0;
    }
    __syncthreads();
    for (int i = tid; i < n; i += RX_T) {
        sh.x0[3 * i] = td_add_rn64((double)sh.at[i].x, -o.c0[0]);
        sh.x0[3 * i + 1] = td_add_rn64((double)sh.at[i].y, -o.c0[1]);
        sh.x0[3 * i + 2] = td_add_rn64((double)sh.at[i].z, -o.c0[2]);
    }
    __syncthreads();
    if (tid == 0) {
        double sum2 = 0.0, max2 = 0.0;
        int ns = 0;
        for (int i = 0; i < n; ++i)
            if (sh.role[i] >= 0) {
                const double x = sh.x0[3 * i], y = sh.x0[3 * i + 1], z = sh.x0[3 * i + 2];
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
        const double q1[4] = {1.0, 0.0, 0.0, 0.0}, t0[3] = {0.0, 0.0, 0.0};
        rx_begin(o, q1, t0, 0);
    }
    __syncthreads();
    if (!with_list) return 0;
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
        const int slot = atomicAdd(&sh.cnt, 1);
        if (slot < cap) s_list[slot] = make_float4(P[0], P[1], P[2], __int_as_float(pe | (pr << 8)));
    }
    __syncthreads();
    return sh.cnt;
}

// One evaluation at the trial state (qn, tn): the sums into sh.sum and sh.pairs, published by the barrier it ends with.  `pose`: build
// the pose of (qn, tn) first; without it sh.at is evaluated as it stands (the input pose itself).
__device__ __forceinline__ void rx_evaluate(const TdRelaxArgs &g, int n, RxStage &sh, const float4 *s_list, int cnt, bool pose) {
    const TdScoreArgs &sc = g.sc;
    const TdProteinSide &ps = sc.p;
    const RxOpt &o = sh.o;
    const int tid = threadIdx.x;
    if (tid < RX_SUMS) sh.sum[tid] = 0ull;
    if (tid == 0) sh.pairs = 0;
    if (pose) rx_pose(n, sh.x0, o.qn, o.tn, o.c0, sh.at);
    __syncthreads();
    const double cx = td_add_rn64(o.c0[0], o.tn[0]), cy = td_add_rn64(o.c0[1], o.tn[1]), cz = td_add_rn64(o.c0[2], o.tn[2]);
    long long acc[SC_TERMS] = {0, 0, 0, 0, 0}, grad[RX_DOF] = {0, 0, 0, 0, 0, 0};
    int pairs = 0;
    if (cnt <= g.list_capacity) {                                               // workgroup-uniform
        for (int e = tid; e < cnt; e += RX_T) {
            const float4 P = s_list[e];
            const int code = __float_as_int(P.w);
            rx_protein_atom(g, n, sh.at, sh.role, sh.rsum, (double)P.x, (double)P.y, (double)P.z, code & 0xff, code >> 8, cx, cy, cz, acc,
                            grad, pairs);
        }
    } else {
        for (int j = tid; j < ps.Np; j += RX_T) {
            int kp = 0;
            double X = 0.0, Y = 0.0, Z = 0.0;
            pw_protein_atom(ps, j, kp, X, Y, Z);
            const int pe = ps.pelem[j];
            const int pr = pe == 0 ? -1 : sc.role[j];
            if (pr >= 0) rx_protein_atom(g, n, sh.at, sh.role, sh.rsum, X, Y, Z, pe, pr, cx, cy, cz, acc, grad, pairs);
        }
    }
#pragma unroll
    for (int t = 0; t < SC_TERMS; ++t)
        if (acc[t]) atomicAdd(&sh.sum[t], (unsigned long long)acc[t]);
#pragma unroll
    for (int t = 0; t < RX_DOF; ++t)
        if (grad[t]) atomicAdd(&sh.sum[SC_TERMS + t], (unsigned long long)grad[t]);
    if (pairs) atomicAdd(&sh.pairs, pairs);
    __syncthreads();
}

// The local optimisation from the state that rx_begin set, to its stop: at most max_evals evaluations.  `input_pose`: the state is the
// identity and sh.at holds the input pose, which the first evaluation takes as it stands; its integers go to terms_in and grad_in
// where those are given.  Ends behind a barrier: sh.o holds the accepted state, its terms, pairs, f0, steps, evals and status.
__device__ __forceinline__ void rx_descend(const TdRelaxArgs &g, int n, RxStage &sh, const float4 *s_list, int cnt, bool input_pose,
                                           long long *terms_in, long long *grad_in) {
    for (int it = 0; it < g.max_evals; ++it) {
        rx_evaluate(g, n, sh, s_list, cnt, it > 0 || !input_pose);
        if (threadIdx.x == 0) rx_advance(sh.o, g, sh.sum, sh.pairs, it == 0, terms_in, grad_in);
        __syncthreads();
        if (sh.o.stop) break;                                                   // workgroup-uniform
    }
}

// the pose of the state (q, t) to pos_out, through sh.at
__device__ __forceinline__ void rx_write_pose(const TdRelaxArgs &g, const BgMol &m, RxStage &sh, const double *q, const double *t) {
    __syncthreads();
    rx_pose(m.n, sh.x0, q, t, sh.o.c0, sh.at);
    __syncthreads();
    for (int i = threadIdx.x; i < m.n; i += RX_T) {
        float *p = g.pos_out + ((size_t)m.s * (size_t)g.sc.b.Nl + (size_t)(m.l0 + i)) * 3;
        p[0] = sh.at[i].x; p[1] = sh.at[i].y; p[2] = sh.at[i].z;
    }
}

// the answer to a molecule that is `bad` (workgroup-uniform); the positions are the launcher's copy
__device__ __forceinline__ void rx_refuse(const TdRelaxArgs &g, const BgMol &m, bool with_input) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        g.n_pairs_out[m.mol] = -1; g.status[m.mol] = -1; g.n_steps[m.mol] = 0; g.n_evals[m.mol] = 0;
    }
    if (tid < SC_TERMS) {
        g.terms_out[m.mol * SC_TERMS + tid] = LLONG_MIN;
        if (with_input) g.terms_in[m.mol * SC_TERMS + tid] = LLONG_MIN;
    }
    if (with_input && tid < RX_DOF) g.grad_in[m.mol * RX_DOF + tid] = 0;
    if (tid < 7) g.transform[m.mol * 7 + tid] = tid == 0 ? 1.0 : 0.0;
}

__global__ __launch_bounds__(RX_T) void relax_kernel(TdRelaxArgs g) {
    extern __shared__ __attribute__((aligned(16))) float4 s_list[];             // [g.list_capacity]: (x, y, z, element | role << 8)
    __shared__ RxStage sh;
    const int tid = threadIdx.x;
    const BgMol m = bg_molecule<BG_MAX>(g.sc.b);
    if (m.bad) { rx_refuse(g, m, true); return; }
    const int cnt = rx_stage(g, m, sh, s_list, true);
    const RxOpt &o = sh.o;
    rx_descend(g, m.n, sh, s_list, cnt, true, g.terms_in + m.mol * SC_TERMS, g.grad_in + m.mol * RX_DOF);
    if (o.steps > 0) rx_write_pose(g, m, sh, o.q, o.t);                         // the molecule moved: the pose of the accepted state
    if (tid == 0) {
        g.n_pairs_out[m.mol] = o.pairs; g.n_steps[m.mol] = o.steps; g.n_evals[m.mol] = o.evals; g.status[m.mol] = o.status;
    }
    if (tid < SC_TERMS) g.terms_out[m.mol * SC_TERMS + tid] = o.terms[tid];
    if (tid < 7) g.transform[m.mol * 7 + tid] = tid < 4 ? o.q[tid] : o.t[tid - 4];
}

// ---- the docking search (td_score_dock; DESIGN.md section 3, "Docking search"): a rigid-body global search under this project's
// heuristic score, not AutoDock Vina's `dock`: three translations and three rotations, no torsions.
//   * dock_kernel         one workgroup per (frame, molecule, chain), staged as relax_kernel's and alive through every round of its
//                         chain: mutate the chain's state with six of the caller's uniforms (dk_mutate), descend from there with the
//                         code above (a fresh H0 and a whole budget per round), accept by Metropolis on inter with the seventh, and
//                         remember the best.  Chain 0 starts with the plain relaxation of the input pose, so the search is never worse
//                         than td_score_minimize.  The chain's Metropolis state never leaves LDS.
//   * dock_select_kernel  one workgroup per (frame, molecule), a launch of its own behind the first on the stream: the chain with the
//                         lowest inter (formed from the integer terms in rx_advance's order; a tie goes to the lowest index), its pose
//                         rebuilt by rx_pose from its transform, and the molecule's outputs.
// Every loop is bounded: a chain runs (n_rounds + 1) descents of at most max_evals evaluations.  No device RNG, no floating-point
// atomic, no spin, no grid-wide synchronisation, no last-block-done pattern.
struct DkChain {
    double q[4], t[3], e_cur, best_q[4], best_t[3], best_e;
    long long best_terms[SC_TERMS];
    int best_pairs, best_status, accepts, steps, evals;
};

// The mutation of the state (q, t) by six uniforms u in [0, 1), every operation rounded on its own (the order is the header's):
// s_k = 2 u_k - 1; t_k += amplitude s_k; h_k = 0.5 ((amplitude s_{3+k}) sqrt(hr)); the increment (1, h) / sqrt(1 + ((hx hx + hy hy) +
// hz hz)) composed on the left, each component summed left to right, and divided by its length sqrt(((ww + xx) + yy) + zz).  A shift
// longer than max_shift, |t| = sqrt((tx tx + ty ty) + tz tz), is scaled by (max_shift / |t|) (1 - 2^-40): returns 4 then, else 0.
__device__ __forceinline__ int dk_mutate(double *q, double *t, const double *u, double amplitude, double hr, double max_shift) {
    double s[6];
    for (int k = 0; k < 6; ++k) s[k] = td_add_rn64(td_mul_rn64(2.0, u[k]), -1.0);
    for (int k = 0; k < 3; ++k) t[k] = td_add_rn64(t[k], td_mul_rn64(amplitude, s[k]));
    const double root = sqrt(hr);
    double h[3];
    for (int k = 0; k < 3; ++k) h[k] = td_mul_rn64(0.5, td_mul_rn64(td_mul_rn64(amplitude, s[3 + k]), root));
    const double nrm = sqrt(td_add_rn64(1.0, td_add_rn64(td_add_rn64(td_mul_rn64(h[0], h[0]), td_mul_rn64(h[1], h[1])), td_mul_rn64(h[2], h[2]))));
    const double dw = 1.0 / nrm, dx = h[0] / nrm, dy = h[1] / nrm, dz = h[2] / nrm;
    const double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
    const double w = td_add_rn64(td_add_rn64(td_add_rn64(td_mul_rn64(dw, qw), -td_mul_rn64(dx, qx)), -td_mul_rn64(dy, qy)), -td_mul_rn64(dz, qz));
    const double x = td_add_rn64(td_add_rn64(td_add_rn64(td_mul_rn64(dw, qx), td_mul_rn64(dx, qw)), td_mul_rn64(dy, qz)), -td_mul_rn64(dz, qy));
    const double y = td_add_rn64(td_add_rn64(td_add_rn64(td_mul_rn64(dw, qy), -td_mul_rn64(dx, qz)), td_mul_rn64(dy, qw)), td_mul_rn64(dz, qx));
    const double z = td_add_rn64(td_add_rn64(td_add_rn64(td_mul_rn64(dw, qz), td_mul_rn64(dx, qy)), -td_mul_rn64(dy, qx)), td_mul_rn64(dz, qw));
    const double len = sqrt(td_add_rn64(td_add_rn64(td_add_rn64(td_mul_rn64(w, w), td_mul_rn64(x, x)), td_mul_rn64(y, y)), td_mul_rn64(z, z)));
    q[0] = w / len; q[1] = x / len; q[2] = y / len; q[3] = z / len;
    const double norm = sqrt(td_add_rn64(td_add_rn64(td_mul_rn64(t[0], t[0]), td_mul_rn64(t[1], t[1])), td_mul_rn64(t[2], t[2])));
    if (!(norm > max_shift)) return 0;
    const double scale = td_mul_rn64(max_shift / norm, 1.0 - 0x1p-40);
    for (int k = 0; k < 3; ++k) t[k] = td_mul_rn64(t[k], scale);
    return 4;
}

// inter of integer terms, in the order rx_advance forms it
__device__ __forceinline__ double dk_inter(const TdRelaxArgs &g, const long long *terms) {
    double T[SC_TERMS];
    for (int k = 0; k < SC_TERMS; ++k) T[k] = ldexp((double)terms[k], -TD_SCORE_FRAC_BITS);
    return td_add_rn64(td_add_rn64(td_add_rn64(td_add_rn64(td_mul_rn64(g.w[0], T[0]), td_mul_rn64(g.w[1], T[1])), td_mul_rn64(g.w[2], T[2])),
                                   td_mul_rn64(g.w[3], T[3])), td_mul_rn64(g.w[4], T[4]));
}

__global__ __launch_bounds__(RX_T) void dock_kernel(TdDockArgs d) {
    const TdRelaxArgs &g = d.rx;
    extern __shared__ __attribute__((aligned(16))) float4 s_list[];
    __shared__ RxStage sh;
    __shared__ DkChain ch;
    const int tid = threadIdx.x, chain = blockIdx.y, C = d.n_chains;
    const BgMol m = bg_molecule<BG_MAX>(g.sc.b);
    const size_t slot = m.mol * (size_t)C + chain;
    if (m.bad) {                                                                // workgroup-uniform; dock_select_kernel answers for the molecule
        if (tid < SC_TERMS) d.chain_terms[slot * SC_TERMS + tid] = LLONG_MIN;
        if (tid < 7) d.chain_transform[slot * 7 + tid] = tid == 0 ? 1.0 : 0.0;
        if (tid < 3) d.chain_aux[slot * 3 + tid] = tid < 2 ? -1 : 0;
        if (tid == 0) { d.chain_accepts[slot] = 0; d.chain_evals[slot] = 0; }
        if (chain == 0 && tid < SC_TERMS) g.terms_in[m.mol * SC_TERMS + tid] = LLONG_MIN;
        if (chain == 0 && tid < RX_DOF) g.grad_in[m.mol * RX_DOF + tid] = 0;
        return;
    }
    const int cnt = rx_stage(g, m, sh, s_list, true);
    RxOpt &o = sh.o;
    if (tid == 0) {
        ch.q[0] = 1.0; ch.q[1] = ch.q[2] = ch.q[3] = 0.0;
        ch.t[0] = ch.t[1] = ch.t[2] = 0.0;
        ch.e_cur = ch.best_e = 0.0;
        ch.accepts = ch.steps = ch.evals = 0;
    }
    const double *draws = d.draws + slot * (size_t)(d.n_rounds + 1) * TD_DOCK_DRAWS;
    for (int r = 0; r <= d.n_rounds; ++r) {
        const bool input_pose = chain == 0 && r == 0;                           // the plain relaxation of the input pose
        const double *u = draws + (size_t)r * TD_DOCK_DRAWS;
        if (tid == 0 && !input_pose) {
            double q[4] = {ch.q[0], ch.q[1], ch.q[2], ch.q[3]}, t[3] = {ch.t[0], ch.t[1], ch.t[2]};
            const int capped = dk_mutate(q, t, u, d.amplitude, o.hr, g.max_shift);
            rx_begin(o, q, t, capped);
        }
        __syncthreads();
        rx_descend(g, m.n, sh, s_list, cnt, input_pose, input_pose ? g.terms_in + m.mol * SC_TERMS : nullptr,
                   input_pose ? g.grad_in + m.mol * RX_DOF : nullptr);
        if (tid == 0) {
            const double e = o.f0;
            ch.steps += o.steps;
            ch.evals += o.evals;
            if (r == 0 || e < ch.e_cur || u[6] < exp((ch.e_cur - e) / d.temperature)) {
                for (int k = 0; k < 4; ++k) ch.q[k] = o.q[k];
                for (int k = 0; k < 3; ++k) ch.t[k] = o.t[k];
                ch.e_cur = e;
                ++ch.accepts;
            }
            if (r == 0 || e < ch.best_e) {
                for (int k = 0; k < 4; ++k) ch.best_q[k] = o.q[k];
                for (int k = 0; k < 3; ++k) ch.best_t[k] = o.t[k];
                for (int k = 0; k < SC_TERMS; ++k) ch.best_terms[k] = o.terms[k];
                ch.best_e = e;
                ch.best_pairs = o.pairs;
                ch.best_status = o.status;
            }
        }
        __syncthreads();
    }
    if (tid < SC_TERMS) d.chain_terms[slot * SC_TERMS + tid] = ch.best_terms[tid];
    if (tid < 7) d.chain_transform[slot * 7 + tid] = tid < 4 ? ch.best_q[tid] : ch.best_t[tid - 4];
    if (tid == 0) {
        d.chain_accepts[slot] = ch.accepts; d.chain_evals[slot] = ch.evals;
        d.chain_aux[slot * 3] = ch.best_pairs; d.chain_aux[slot * 3 + 1] = ch.best_status; d.chain_aux[slot * 3 + 2] = ch.steps;
    }
}

__global__ __launch_bounds__(RX_T) void dock_select_kernel(TdDockArgs d) {
    const TdRelaxArgs &g = d.rx;
    __shared__ RxStage sh;
    __shared__ int s_best;
    __shared__ double s_tr[7];
    const int tid = threadIdx.x, C = d.n_chains;
    const BgMol m = bg_molecule<BG_MAX>(g.sc.b);
    if (m.bad) {
        rx_refuse(g, m, false);                                                 // terms_in and grad_in are chain 0's
        if (tid == 0) d.best_chain[m.mol] = 0;
        return;
    }
    rx_stage(g, m, sh, nullptr, false);
    if (tid == 0) {
        int best = 0, steps = 0, evals = 0;
        double e_best = 0.0;
        for (int c = 0; c < C; ++c) {
            const size_t slot = m.mol * (size_t)C + c;
            const double e = dk_inter(g, d.chain_terms + slot * SC_TERMS);
            if (c == 0 || e < e_best) { best = c; e_best = e; }
            steps += d.chain_aux[slot * 3 + 2];
            evals += d.chain_evals[slot];
        }
        const size_t slot = m.mol * (size_t)C + best;
        for (int k = 0; k < 7; ++k) s_tr[k] = d.chain_transform[slot * 7 + k];
        s_best = best;
        d.best_chain[m.mol] = best;
        g.n_pairs_out[m.mol] = d.chain_aux[slot * 3]; g.status[m.mol] = d.chain_aux[slot * 3 + 1];
        g.n_steps[m.mol] = steps; g.n_evals[m.mol] = evals;
    }
    __syncthreads();
    const size_t slot = m.mol * (size_t)C + s_best;
    if (tid < SC_TERMS) g.terms_out[m.mol * SC_TERMS + tid] = d.chain_terms[slot * SC_TERMS + tid];
    if (tid < 7) g.transform[m.mol * 7 + tid] = s_tr[tid];
    // the identity (the input pose relaxed no further) keeps the input's bytes, as td_score_minimize's zero steps do
    const bool moved = !(s_tr[0] == 1.0 && s_tr[1] == 0.0 && s_tr[2] == 0.0 && s_tr[3] == 0.0 && s_tr[4] == 0.0 && s_tr[5] == 0.0 && s_tr[6] == 0.0);
    if (moved) rx_write_pose(g, m, sh, s_tr, s_tr + 4);                         // workgroup-uniform
}

namespace {
// the copy of the positions that both entry points start with, and the clamp of the list
int rx_prepare(TdRelaxArgs &g, hipStream_t s) {
    g.sc.reject2 = pw_reject2(g.sc.cutoff);
    const size_t coords = (size_t)g.sc.b.S * (size_t)g.sc.b.Nl * 3;
    if (coords) TD_CHECK_HIP(hipMemcpyAsync(g.pos_out, g.sc.b.pos, coords * sizeof(float), hipMemcpyDeviceToDevice, s));
    g.list_capacity = std::max(0, std::min(std::min(g.list_capacity, TD_RELAX_LIST_CAPACITY), g.sc.p.Np));
    return TD_OK;
}
}  // namespace

// The protein roles are resolved by the caller, on the same stream (td_launch_protein_roles); the rotor kernel counts the rotatable
// bonds of the input pose.
int td_launch_score_minimize(const TdRelaxArgs &args, hipStream_t s) {
    static TdLdsOnce once;
    TdRelaxArgs g = args;
    if (const int rc = rx_prepare(g, s)) return rc;
    const int64_t M = (int64_t)g.sc.b.S * g.sc.b.B;
    if (M == 0) return TD_OK;
    if (const int rc = td_set_lds(once, reinterpret_cast<const void *>(relax_kernel), (size_t)TD_RELAX_LIST_CAPACITY * sizeof(float4))) return rc;
    relax_kernel<<<dim3((unsigned)M), dim3(RX_T), (size_t)g.list_capacity * sizeof(float4), s>>>(g);
    TD_CHECK_HIP(hipGetLastError());
    return td_launch_rotors(g.sc, s);
}

// chain_aux [S,B,C,3] int32 is the caller's scratch: the pairs and the status of each chain's best, and the chain's steps
int td_launch_score_dock(const TdDockArgs &args, hipStream_t s) {
    static TdLdsOnce once;
    TdDockArgs d = args;
    if (const int rc = rx_prepare(d.rx, s)) return rc;
    const int64_t M = (int64_t)d.rx.sc.b.S * d.rx.sc.b.B;
    if (M == 0) return TD_OK;
    if (const int rc = td_set_lds(once, reinterpret_cast<const void *>(dock_kernel), (size_t)TD_RELAX_LIST_CAPACITY * sizeof(float4))) return rc;
    dock_kernel<<<dim3((unsigned)M, (unsigned)d.n_chains), dim3(RX_T), (size_t)d.rx.list_capacity * sizeof(float4), s>>>(d);
    TD_CHECK_HIP(hipGetLastError());
    dock_select_kernel<<<dim3((unsigned)M), dim3(RX_T), 0, s>>>(d);
    TD_CHECK_HIP(hipGetLastError());
    return td_launch_rotors(d.rx.sc, s);
}
