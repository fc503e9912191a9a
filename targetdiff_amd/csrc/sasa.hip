// Solvent-accessible surface of ligand frames by Shrake-Rupley point counting (gfx950, wave64; DESIGN.md section 3, "Solvent-accessible
// surface"): every atom carries P test points on its expanded sphere (reach R = van der Waals radius + probe), a point is exposed when
// no other sphere holds it, and every output is a count of points.
//   * sasa_apo_kernel  once per call, one workgroup per protein atom: lane k of the workgroup owns point k.  Writes the apo-exposed
//                      points of the pocket alone (pocket_free, pocket_mask); wave w's ballot is mask word w.
//   * sasa_mol_kernel  one workgroup of four waves per (frame, molecule), in two instantiations as the bond graph's kernels: molecules
//                      of up to 128 atoms with a 256-atom chunk (22 KiB of LDS), larger ones with room for 512 atoms and a 512-atom
//                      chunk (53 KiB); both grids cover every molecule and each workgroup takes only its own kind.  The molecule is
//                      staged into LDS as float64 centres and element indices, with an exposed-point bit mask [n][4] beside it.
//                      Pass 1 clears the bits of points inside another atom of the molecule (the free counts).  The pocket is then scanned in rounds of 256 atoms; those that
//                      take part and lie within the cull distance of some ligand centre are compacted by ballot into an LDS chunk,
//                      and a full chunk (or the last) is processed before the scan goes on: there is no cap on their number.  Per
//                      chunk, pass 2 clears the ligand's bits against the chunk (the bound counts, after the last chunk) and pass 3
//                      walks the apo-exposed points of the chunk's atoms against the molecule (pocket_buried, bits, buried_sum).
// One routine, sa_clear, does all four tests.  A wave holds the <= 64 points of one mask word of one sphere; the candidate occluders
// of that sphere are found 64 at a time, one per lane, by their centre distance, and the wave then walks the ballot's set bits, every
// lane reading the same occluder (an LDS broadcast, or a uniform global load in the apo kernel).  It leaves when no point is left.
//
// Culling never changes a result.  Sphere a (centre c_a, reach R_a) can hold a point of sphere b only if, in the reals,
//     |c_a - c_b| < R_a + R_b + e,    e = 1e-6 R_b + 3 * 2^-52 (C + R_b) + 2^-50 R_a:
// the point is x = c_b + R_b u with two roundings per coordinate (error <= 3 * 2^-52 (C + R_b) for |coordinate| <= C) and |u| <= 1 +
// 5e-7 (the binding admits | |u|^2 - 1 | <= 1e-6), and D2 < R2_a with the five roundings of D2 and the one of R2_a, all relative (every
// term of D2 is non-negative), gives |x - c_a| < R_a (1 + 2^-50).  The cull distance is L = (R_a + R_b) (1 + TD_SASA_CULL_REL) +
// TD_SASA_CULL_ABS with both constants 1e-4: for |coordinate| <= C = 1e5, the bound the binding enforces (capi.SASA_COORD_MAX), e <
// 1e-4 (R_a + R_b) + 1e-10, so L exceeds the bound by more than 9e-5, five orders above the rounding of the cull's own float64
// distance (relative 2^-50).  A candidate is dropped only on `d2 > L L`; a NaN or an overflow keeps it.  The workgroup's shortlist uses
// the largest reach of the ligand table for R_b, which is no smaller than any atom's.
// Every loop is bounded by the molecule's size, the pocket's or P.  All outputs are integers, added with integer atomics or written
// by one owner: nothing depends on the grid or on the order of arrival.  No floating-point atomic.  The answer to an oversize molecule
// (-1) is that of bonds.hip.
#include "td_bond_graph.h"

constexpr int SA_T = TD_SASA_THREADS, SA_WAVES = SA_T / 64, SA_PMAX = TD_SASA_MAX_POINTS, SA_CH = TD_SASA_CHUNK, SA_E = TD_POCKET_ELEMENTS;
constexpr int SA_CH_SMALL = SA_T;
static_assert(SA_PMAX == 64 * SA_WAVES, "the apo kernel's wave w writes mask word w");
static_assert(SA_CH >= SA_T && SA_CH_SMALL >= SA_T, "a chunk takes at least one scan round");

__device__ __forceinline__ double sa_dist2(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = td_add_rn64(ax, -bx), dy = td_add_rn64(ay, -by), dz = td_add_rn64(az, -bz);
    return td_add_rn64(td_add_rn64(td_mul_rn64(dx, dx), td_mul_rn64(dy, dy)), td_mul_rn64(dz, dz));
}

// may a sphere of reach Ra hold a point of a sphere of reach Rb whose centre is at squared distance d2?  (see the head of the file)
__device__ __forceinline__ bool sa_near(double d2, double Ra, double Rb) {
    const double L = (Ra + Rb) * (1.0 + TD_SASA_CULL_REL) + TD_SASA_CULL_ABS;
    return !(d2 > L * L);
}

// point k of the sphere (c, R): c + R u_k, per coordinate one product and one add
__device__ __forceinline__ void sa_point(double cx, double cy, double cz, double R, const double *u, double &px, double &py, double &pz) {
    px = td_add_rn64(cx, td_mul_rn64(R, u[0]));
    py = td_add_rn64(cy, td_mul_rn64(R, u[1]));
    pz = td_add_rn64(cz, td_mul_rn64(R, u[2]));
}

// The wave's points (px, py, pz; `alive`: still exposed, false for a lane without a point) of the sphere (c, R), wave-uniform, against
// the m occluders that get(o, x, y, z, Ro, R2o) yields (false: occluder o takes no part); occluder `skip` is the sphere itself.
template <typename G>
__device__ __forceinline__ bool sa_clear(double px, double py, double pz, bool alive, double cx, double cy, double cz, double R, int m,
                                         int skip, G get) {
    const int lane = threadIdx.x & 63;
    for (int b0 = 0; b0 < m; b0 += 64) {                                        // wave-uniform
        if (__ballot(alive) == 0ull) break;
        const int o = b0 + lane;
        bool near = false;
        if (o < m && o != skip) {
            double x, y, z, Ro, R2o;
            if (get(o, x, y, z, Ro, R2o)) near = sa_near(sa_dist2(cx, cy, cz, x, y, z), Ro, R);
        }
        unsigned long long nb = __ballot(near);
        while (nb != 0ull && __ballot(alive) != 0ull) {                         // wave-uniform
            const int q = b0 + __ffsll((long long)nb) - 1;
            nb &= nb - 1ull;
            double x, y, z, Ro, R2o;
            get(q, x, y, z, Ro, R2o);                                           // every lane reads the same occluder
            if (sa_dist2(px, py, pz, x, y, z) < R2o) alive = false;
        }
    }
    return alive;
}

__global__ __launch_bounds__(SA_T) void sasa_apo_kernel(TdSasaArgs g) {
    __shared__ int s_cnt[SA_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = blockIdx.x, Np = g.Np, P = g.P;
    const int e = g.pelem[j];
    unsigned long long word = 0ull;
    if (e >= 0 && e < SA_E && wave * 64 < P) {                                  // wave-uniform
        const float *c = g.ppos + (size_t)j * 3;
        const double cx = (double)c[0], cy = (double)c[1], cz = (double)c[2], R = g.prot_R[e];
        const int k = wave * 64 + lane;
        double px = 0.0, py = 0.0, pz = 0.0;
        if (k < P) sa_point(cx, cy, cz, R, g.dirs + (size_t)k * 3, px, py, pz);
        const bool alive = sa_clear(px, py, pz, k < P, cx, cy, cz, R, Np, j, [&](int o, double &x, double &y, double &z, double &Ro, double &R2o) {
            const int eo = g.pelem[o];
            if (eo < 0 || eo >= SA_E) return false;
            const float *p = g.ppos + (size_t)o * 3;
            x = (double)p[0]; y = (double)p[1]; z = (double)p[2];
            Ro = g.prot_R[eo];
            R2o = td_mul_rn64(Ro, Ro);
            return true;
        });
        word = __ballot(alive);
    }
    if (lane == 0) {
        g.pocket_mask[(size_t)j * SA_WAVES + wave] = word;
        s_cnt[wave] = __popcll(word);
    }
    __syncthreads();
    if (tid == 0) {
        int c = 0;
        for (int w = 0; w < SA_WAVES; ++w) c += s_cnt[w];
        g.pocket_free[j] = c;
    }
}

template <int MAXN, int CH>
__global__ __launch_bounds__(SA_T) void sasa_mol_kernel(TdSasaArgs g) {
    const TdBondArgs &a = g.b;
    __shared__ double s_x[MAXN], s_y[MAXN], s_z[MAXN];                         // the molecule's centres, widened
    __shared__ int s_el[MAXN];                                                  // element index, -1 for a class outside [0, K)
    __shared__ unsigned long long s_mask[MAXN][4];                              // bit k & 63 of word k >> 6: point k is still exposed
    __shared__ double s_px[CH], s_py[CH], s_pz[CH];                             // the chunk of shortlisted protein atoms
    __shared__ int s_pe[CH], s_pj[CH];
    __shared__ double s_dir[SA_PMAX * 3];
    __shared__ double s_lR[8], s_lR2[8], s_pR[SA_E], s_pR2[SA_E];
    __shared__ int s_elem[TD_QUALITY_MAX_CLASSES];
    __shared__ int s_free[8], s_bound[8], s_pb[SA_E], s_wcnt[SA_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BgMol m = bg_molecule<MAXN>(a);
    if (!m.mine) return;                                                        // workgroup-uniform: the other instantiation has it
    const int Np = g.Np, P = g.P, W = g.W, nw = (P + 63) >> 6;
    if (m.bad) {                                                                // workgroup-uniform; the launcher has zeroed the words of bits
        if (tid < 8) g.n_free[m.mol * 8 + tid] = g.n_bound[m.mol * 8 + tid] = -1;
        if (tid < SA_E) g.pocket_buried[m.mol * SA_E + tid] = -1;
        return;
    }
    const int n = m.n;
    const bool inc = !a.include || a.include[m.mol] != 0;                       // workgroup-uniform
    if (tid < TD_QUALITY_MAX_CLASSES) s_elem[tid] = tid < a.K ? a.elem[tid] : -1;
    if (tid < 8) {
        const double R = g.lig_R[tid];
        s_lR[tid] = R; s_lR2[tid] = td_mul_rn64(R, R);
        s_free[tid] = s_bound[tid] = 0;
    }
    if (tid < SA_E) {
        const double R = g.prot_R[tid];
        s_pR[tid] = R; s_pR2[tid] = td_mul_rn64(R, R);
        s_pb[tid] = 0;
    }
    for (int k = tid; k < 3 * P; k += SA_T) s_dir[k] = g.dirs[k];
    __syncthreads();
    for (int i = tid; i < n; i += SA_T) {
        const size_t at = (size_t)m.s * (size_t)a.Nl + (size_t)(m.l0 + i);
        const float *p = a.pos + at * 3;
        const int64_t c = a.v[at];
        const int el = c >= 0 && c < a.K ? s_elem[(int)c] : -1;
        s_x[i] = (double)p[0]; s_y[i] = (double)p[1]; s_z[i] = (double)p[2];
        s_el[i] = el;
        for (int w = 0; w < 4; ++w) {
            const int left = P - 64 * w;
            s_mask[i][w] = el < 0 || left <= 0 ? 0ull : left >= 64 ? ~0ull : (1ull << left) - 1ull;
        }
    }
    __syncthreads();
    const auto ligand = [&](int o, double &x, double &y, double &z, double &Ro, double &R2o) {
        const int eo = s_el[o];
        if (eo < 0) return false;
        x = s_x[o]; y = s_y[o]; z = s_z[o];
        Ro = s_lR[eo]; R2o = s_lR2[eo];
        return true;
    };
    const auto chunk = [&](int o, double &x, double &y, double &z, double &Ro, double &R2o) {
        const int eo = s_pe[o];
        x = s_px[o]; y = s_py[o]; z = s_pz[o];
        Ro = s_pR[eo]; R2o = s_pR2[eo];
        return true;
    };
    // word w of ligand atom i against m occluders: item t = i nw + w belongs to wave t % 4 in every pass, so a word has one owner
    const auto ligand_item = [&](int t, int mocc, bool self, auto get) {
        const int i = t / nw, w = t - i * nw;
        const unsigned long long word = s_mask[i][w];
        if (word == 0ull) return;                                               // wave-uniform
        const int k = 64 * w + lane;
        const double cx = s_x[i], cy = s_y[i], cz = s_z[i], R = s_lR[s_el[i]];  // el >= 0: the word is not 0
        double px = 0.0, py = 0.0, pz = 0.0;
        if (k < P) sa_point(cx, cy, cz, R, s_dir + 3 * k, px, py, pz);
        const bool alive = sa_clear(px, py, pz, ((word >> lane) & 1ull) != 0ull, cx, cy, cz, R, mocc, self ? i : -1, get);
        const unsigned long long left = __ballot(alive);
        if (lane == 0) s_mask[i][w] = left;
    };
    // the exposed points of every atom by element into cnt (LDS, zeroed), and per atom into out when given
    const auto count = [&](int *cnt, int32_t *out) {
        for (int i = tid; i < n; i += SA_T) {
            const int c = __popcll(s_mask[i][0]) + __popcll(s_mask[i][1]) + __popcll(s_mask[i][2]) + __popcll(s_mask[i][3]);
            if (out) out[(size_t)m.s * (size_t)a.Nl + (size_t)(m.l0 + i)] = c;
            if (c) atomicAdd(&cnt[s_el[i]], c);
        }
    };

    for (int t = wave; t < n * nw; t += SA_WAVES) ligand_item(t, n, true, ligand);            // pass 1
    __syncthreads();
    count(s_free, g.atom_free);

    double maxR = 0.0;                                                          // the ligand table's largest reach
    for (int e = 0; e < 8; ++e) maxR = s_lR[e] > maxR ? s_lR[e] : maxR;
    int base = 0;
    while (base < Np) {                                                         // workgroup-uniform
        int cnt = 0;
        while (base < Np && cnt + SA_T <= CH) {                              // one scan round: 256 atoms of the pocket, the near ones kept
            const int j = base + tid;
            bool keep = false;
            int e = -1;
            double X = 0.0, Y = 0.0, Z = 0.0;
            if (j < Np) {
                e = g.pelem[j];
                if (e >= 0 && e < SA_E) {
                    const float *p = g.ppos + (size_t)j * 3;
                    X = (double)p[0]; Y = (double)p[1]; Z = (double)p[2];
                    const double R = s_pR[e];
                    for (int i = 0; i < n && !keep; ++i)
                        keep = s_el[i] >= 0 && sa_near(sa_dist2(X, Y, Z, s_x[i], s_y[i], s_z[i]), R, maxR);
                }
            }
            const unsigned long long kb = __ballot(keep);
            if (lane == 0) s_wcnt[wave] = __popcll(kb);
            __syncthreads();
            int off = cnt, tot = 0;
            for (int w = 0; w < SA_WAVES; ++w) {
                if (w < wave) off += s_wcnt[w];
                tot += s_wcnt[w];
            }
            if (keep) {
                const int q = off + __popcll(kb & ((1ull << lane) - 1ull));     // < cnt + 256 <= CH
                s_px[q] = X; s_py[q] = Y; s_pz[q] = Z;
                s_pe[q] = e; s_pj[q] = j;
            }
            cnt += tot;
            base += SA_T;
            __syncthreads();                                                    // s_wcnt is read; the chunk's new entries are written
        }
        const int lig_items = n * nw, items = lig_items + cnt * nw;
        for (int t = wave; t < items; t += SA_WAVES) {
            if (t < lig_items) {                                                // pass 2: the ligand's points against the chunk
                ligand_item(t, cnt, false, chunk);
                continue;
            }
            const int u = t - lig_items, q = u / nw, w = u - q * nw;            // pass 3: word w of chunk atom q against the molecule
            const int j = s_pj[q], e = s_pe[q];
            const unsigned long long word = g.pocket_mask[(size_t)j * 4 + w];
            if (word == 0ull) continue;                                         // wave-uniform
            const int k = 64 * w + lane;
            const double cx = s_px[q], cy = s_py[q], cz = s_pz[q], R = s_pR[e];
            double px = 0.0, py = 0.0, pz = 0.0;
            if (k < P) sa_point(cx, cy, cz, R, s_dir + 3 * k, px, py, pz);
            const bool alive = sa_clear(px, py, pz, ((word >> lane) & 1ull) != 0ull, cx, cy, cz, R, n, -1, ligand);
            const int buried = __popcll(word) - __popcll(__ballot(alive));
            if (lane == 0 && buried > 0) {
                atomicAdd(&s_pb[e], buried);
                if (g.bits) atomicOr(&g.bits[m.mol * (size_t)W + (j >> 6)], 1ull << (j & 63));
                if (inc) atomicAdd(&g.buried_sum[(size_t)m.s * (size_t)Np + j], (unsigned long long)buried);
            }
        }
        __syncthreads();                                                        // the chunk is free again
    }
    count(s_bound, g.atom_bound);
    __syncthreads();
    if (tid < 8) {
        g.n_free[m.mol * 8 + tid] = s_free[tid];
        g.n_bound[m.mol * 8 + tid] = s_bound[tid];
    }
    if (tid < SA_E) g.pocket_buried[m.mol * SA_E + tid] = s_pb[tid];
}

int td_launch_sasa_report(const TdSasaArgs &g, hipStream_t s) {
    const int64_t M = (int64_t)g.b.S * g.b.B;
    if (g.b.S > 0 && g.Np > 0) TD_CHECK_HIP(hipMemsetAsync(g.buried_sum, 0, (size_t)g.b.S * g.Np * sizeof(unsigned long long), s));
    if (M > 0 && g.W > 0 && g.bits) TD_CHECK_HIP(hipMemsetAsync(g.bits, 0, (size_t)M * g.W * sizeof(unsigned long long), s));
    if (g.Np > 0) {
        sasa_apo_kernel<<<dim3((unsigned)g.Np), dim3(SA_T), 0, s>>>(g);
        TD_CHECK_HIP(hipGetLastError());
    }
    if (M == 0) return TD_OK;
    sasa_mol_kernel<BG_SMALL, SA_CH_SMALL><<<dim3((unsigned)M), dim3(SA_T), 0, s>>>(g);
    TD_CHECK_HIP(hipGetLastError());
    sasa_mol_kernel<BG_MAX, SA_CH><<<dim3((unsigned)M), dim3(SA_T), 0, s>>>(g);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}
