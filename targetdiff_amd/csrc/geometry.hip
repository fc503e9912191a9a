// Local geometry of ligand frames (gfx950, wave64; DESIGN.md section 3, "Local geometry"): bond angles, torsion angles and internal
// clashes on the bond graph of bonds.hip.
//   * geometry_kernel  one workgroup per (frame, molecule), the molecule and its bit rows in LDS exactly as bond_graph_kernel builds
//                      them (td_bond_graph.h).  Lane i owns atom i.  From its row it takes its degree and, when that is at most
//                      TD_GEOM_MAX_DEGREE, the ascending list of its neighbours (s_nbr).  Angles: lane j is the centre and walks the
//                      pairs a < b of its list.  Torsions: a wave takes a central bond j < k and its 64 lanes are the pairs of j's
//                      list and k's (a ligand has fewer atoms than its workgroup has lanes: per-atom torsion loops would leave most
//                      of them idle behind the busiest one).  Both are binned by their cosine, float64 with every product and sum
//                      rounded on its own, so no acos / atan2 runs here and every output is an integer.  The index of a central bond
//                      in td_bond_list's order, for the ring filter, is the scan of the upward-bond counts plus the rank of k among
//                      j's upward neighbours (rings.hip).
//                      Clashes: the set of atoms within 3 bonds of atom i is three rounds of OR over the bit rows, W = MAXN / 64 words
//                      indexed by unrolled compile-time indices only (registers); lane i then walks all other atoms outside that set.
// Every loop is bounded by the molecule's size or by the degree cap (at most 28 angles per centre, 49 torsions per central bond), so a
// defect ends in a wrong number, not in a kernel that does not return.  Integer LDS atomics for the counts and histograms, one integer
// global atomic per non-empty bin: nothing depends on the grid or on the order of arrival.  The two instantiations and the answer to
// an oversize molecule (-1) are those of bonds.hip.
#include "td_bond_graph.h"

constexpr int GM_DEG = TD_GEOM_MAX_DEGREE, GM_MAXP = TD_GEOM_MAX_PROFILES, GM_BINS = TD_GEOM_BINS;

__device__ __forceinline__ double gm_dot(double ax, double ay, double az, double bx, double by, double bz) {
    return td_add_rn64(td_add_rn64(td_mul_rn64(ax, bx), td_mul_rn64(ay, by)), td_mul_rn64(az, bz));
}
// (a b) - (c d), each product and the difference rounded on its own
__device__ __forceinline__ double gm_det(double a, double b, double c, double d) { return td_add_rn64(td_mul_rn64(a, b), -td_mul_rn64(c, d)); }

__device__ __forceinline__ bool gm_z(int want, int e) { return want < 0 || want == e; }

template <int MAXN>
__global__ __launch_bounds__(MAXN) void geometry_kernel(TdGeomArgs g) {
    constexpr int W = MAXN / 64;
    const TdBondArgs &a = g.b;
    __shared__ float4 s_at[MAXN];
    __shared__ unsigned long long s_row[W][MAXN];
    __shared__ double s_thr[3][64], s_clash[64];
    __shared__ unsigned int s_hist[GM_MAXP][GM_BINS];
    __shared__ unsigned short s_nbr[MAXN][GM_DEG], s_deg[MAXN];
    __shared__ int s_off[MAXN], s_elem[TD_QUALITY_MAX_CLASSES];
    __shared__ int s_cnt[5];                                                    // angles, torsions, degenerate, crowded, clashes
    __shared__ int s_pkind[GM_MAXP], s_pz[GM_MAXP][4], s_pcat[GM_MAXP], s_pring[GM_MAXP], s_pn[GM_MAXP];
    __shared__ const double *s_pedges[GM_MAXP];
    const int tid = threadIdx.x;
    const BgMol m = bg_molecule<MAXN>(a);
    if (!m.mine) return;                                                        // workgroup-uniform
    const int n = m.n;
    if (m.bad) {                                                                // only the 512-lane instantiation gets here
        if (tid == 0) {
            g.n_angles[m.mol] = g.n_torsions[m.mol] = g.n_degenerate[m.mol] = g.n_crowded[m.mol] = -1;
            if (g.clash) g.n_clashes[m.mol] = -1;
        }
        return;
    }
    const bool inc = !a.include || a.include[m.mol] != 0;                       // workgroup-uniform
    const int P = inc ? g.P : 0;
    bool need_ring = false;                                                     // workgroup-uniform: some profile filters on the ring
    for (int p = 0; p < P; ++p) need_ring = need_ring || g.ring[p] != 0;
    td_bond_thresholds(s_thr, tid, MAXN);
    if (tid < 64) s_clash[tid] = g.clash_thr[tid];
    if (tid < TD_QUALITY_MAX_CLASSES) s_elem[tid] = tid < a.K ? a.elem[tid] : -1;
    if (tid < P) {
        s_pkind[tid] = g.kind[tid]; s_pcat[tid] = g.cat[tid]; s_pring[tid] = g.ring[tid]; s_pn[tid] = g.n_edges[tid];
        s_pedges[tid] = g.edges[tid];
        for (int q = 0; q < 4; ++q) s_pz[tid][q] = g.z[tid][q];
    }
    for (int k = tid; k < P * GM_BINS; k += MAXN) (&s_hist[0][0])[k] = 0u;
    if (tid < 5) s_cnt[tid] = 0;
    bg_load<MAXN>(a, m, s_elem, s_at);

    // ---- the row of atom tid, its degree and, under the cap, its neighbours in ascending order
    int up = 0, deg = 0;
    if (tid < n) {
        up = bg_rows<MAXN>(n, s_at, s_thr, s_row, [](int, int, int, double) {});
#pragma unroll
        for (int w = 0; w < W; ++w) deg += __popcll(s_row[w][tid]);
        if (deg <= GM_DEG) {
            int k = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                unsigned long long bits = s_row[w][tid];
                for (int c = 0; c < 64 && bits && k < GM_DEG; ++c) {
                    s_nbr[tid][k++] = (unsigned short)(w * 64 + __ffsll((long long)bits) - 1);
                    bits &= bits - 1ull;
                }
            }
        }
    }
    s_deg[tid] = (unsigned short)deg;
    s_off[tid] = up;
    __syncthreads();
    if (need_ring) bg_scan<MAXN>(s_off);                                        // inclusive scan of the per-atom counts of bonds tid < j

    int n_ang = 0, n_tor = 0, n_degen = 0;
    if (tid < n && deg >= 2 && deg <= GM_DEG) {
        const float4 me = s_at[tid];
        const int cj = __float_as_int(me.w), ej = cj & 7;
        const double xj = (double)me.x, yj = (double)me.y, zj = (double)me.z;

        // ---- angles (i, tid, k), i < k
        for (int ia = 0; ia < deg; ++ia) {
            const float4 pi = s_at[s_nbr[tid][ia]];
            const int ei = __float_as_int(pi.w) & 7;
            const double ux = (double)pi.x - xj, uy = (double)pi.y - yj, uz = (double)pi.z - zj;
            const double uu = gm_dot(ux, uy, uz, ux, uy, uz);
            for (int ib = ia + 1; ib < deg; ++ib) {
                const float4 pk = s_at[s_nbr[tid][ib]];
                const int ek = __float_as_int(pk.w) & 7;
                const double wx = (double)pk.x - xj, wy = (double)pk.y - yj, wz = (double)pk.z - zj;
                const double den = td_mul_rn64(uu, gm_dot(wx, wy, wz, wx, wy, wz));
                if (den == 0.0) { ++n_degen; continue; }
                ++n_ang;
                if (P == 0) continue;
                const double c = gm_dot(ux, uy, uz, wx, wy, wz) / sqrt(den);
                for (int p = 0; p < P; ++p) {
                    if (s_pkind[p] != 1 || !gm_z(s_pz[p][1], ej)) continue;
                    const int z0 = s_pz[p][0], z2 = s_pz[p][2];
                    if ((gm_z(z0, ei) && gm_z(z2, ek)) || (gm_z(z0, ek) && gm_z(z2, ei)))
                        atomicAdd(&s_hist[p][td_searchsorted_left(s_pedges[p], s_pn[p], c)], 1u);
                }
            }
        }
    }

    // ---- torsions (i, j, k, l): a wave takes a slot (j, place ka in j's list) and, when that is a central bond j < k with both ends
    // under the cap, its 64 lanes are the pairs (place of i in j's list, place of l in k's list): one step per central bond
    {
        static_assert(GM_DEG == 8, "a slot is j * 8 + ka, a lane ia * 8 + lb");
        const int ia = (tid & 63) >> 3, lb = tid & 7;
        for (int slot = tid >> 6; slot < n * GM_DEG; slot += MAXN / 64) {
            const int j = slot >> 3, ka = slot & 7, dj = s_deg[j];              // wave-uniform down to the lane's own pair
            if (dj > GM_DEG || ka >= dj) continue;
            const int k = s_nbr[j][ka];
            if (k < j) continue;
            const int dk = s_deg[k];
            if (dk > GM_DEG || ia >= dj || lb >= dk) continue;
            const int i = s_nbr[j][ia], l = s_nbr[k][lb];
            if (i == k || l == j || l == i) continue;
            const float4 pj = s_at[j], pk = s_at[k], pi = s_at[i], pl = s_at[l];
            const int cj = __float_as_int(pj.w), ck = __float_as_int(pk.w), ej = cj & 7, ek = ck & 7;
            const int ei = __float_as_int(pi.w) & 7, el = __float_as_int(pl.w) & 7;
            const double xj = (double)pj.x, yj = (double)pj.y, zj = (double)pj.z;
            const double b1x = xj - (double)pi.x, b1y = yj - (double)pi.y, b1z = zj - (double)pi.z;
            const double b2x = (double)pk.x - xj, b2y = (double)pk.y - yj, b2z = (double)pk.z - zj;
            const double b3x = (double)pl.x - (double)pk.x, b3y = (double)pl.y - (double)pk.y, b3z = (double)pl.z - (double)pk.z;
            const double n1x = gm_det(b1y, b2z, b1z, b2y), n1y = gm_det(b1z, b2x, b1x, b2z), n1z = gm_det(b1x, b2y, b1y, b2x);
            const double n2x = gm_det(b2y, b3z, b2z, b3y), n2y = gm_det(b2z, b3x, b2x, b3z), n2z = gm_det(b2x, b3y, b2y, b3x);
            const double den = td_mul_rn64(gm_dot(n1x, n1y, n1z, n1x, n1y, n1z), gm_dot(n2x, n2y, n2z, n2x, n2y, n2z));
            if (den == 0.0) { ++n_degen; continue; }
            ++n_tor;
            if (P == 0) continue;
            const double c = gm_dot(n1x, n1y, n1z, n2x, n2y, n2z) / sqrt(den);
            double d;
            const int cat = bg_category(cj, ck, td_bond_order(xj, yj, zj, pk.x, pk.y, pk.z, ej * 8 + ek, s_thr, d));
            int rs = 0;                                                         // 1: the central bond is in no ring, 2: it is in one, 0: not known
            if (need_ring) {
                int lower = 0;                                                  // j's neighbours below j: the rank of k among the upward ones is ka - lower
                for (int q = 0; q < ka; ++q) lower += s_nbr[j][q] < j ? 1 : 0;
                const int64_t idx = a.bond_ptr[m.mol] + (int64_t)(j > 0 ? s_off[j - 1] : 0) + (int64_t)(ka - lower);
                if (idx >= 0 && idx < a.capacity) rs = a.bond_ring[idx] ? 2 : 1;   // offsets that are not this pack's own read nothing out of bounds
            }
            for (int p = 0; p < P; ++p) {
                if (s_pkind[p] != 2) continue;
                const int *z = s_pz[p];
                const bool fwd = gm_z(z[0], ei) && gm_z(z[1], ej) && gm_z(z[2], ek) && gm_z(z[3], el);
                const bool rev = gm_z(z[0], el) && gm_z(z[1], ek) && gm_z(z[2], ej) && gm_z(z[3], ei);
                if (!fwd && !rev) continue;
                if ((s_pcat[p] != 0 && s_pcat[p] != cat) || (s_pring[p] != 0 && s_pring[p] != rs)) continue;
                atomicAdd(&s_hist[p][td_searchsorted_left(s_pedges[p], s_pn[p], c)], 1u);
            }
        }
    }

    // ---- clashes: pairs of atoms with a class, more than 3 bonds apart, closer than the table's threshold
    int mine = 0, pairs = 0;
    if (g.clash && tid < n && __float_as_int(s_at[tid].w) >= 0) {
        unsigned long long reach[W], fr[W], nx[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            fr[w] = s_row[w][tid];
            reach[w] = w == (tid >> 6) ? fr[w] | 1ull << (tid & 63) : fr[w];
        }
        for (int round = 0; round < 2; ++round) {                               // within 2 bonds, then within 3
#pragma unroll
            for (int w = 0; w < W; ++w) nx[w] = 0ull;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                unsigned long long bits = fr[w];
                for (int c = 0; c < 64 && bits; ++c) {
                    const int at = w * 64 + __ffsll((long long)bits) - 1;
                    bits &= bits - 1ull;
#pragma unroll
                    for (int u = 0; u < W; ++u) nx[u] |= s_row[u][at];
                }
            }
#pragma unroll
            for (int w = 0; w < W; ++w) {
                nx[w] &= ~reach[w];
                reach[w] |= nx[w];
                fr[w] = nx[w];
            }
        }
        const float4 me = s_at[tid];
        const int ei = __float_as_int(me.w) & 7;
        const double xi = (double)me.x, yi = (double)me.y, zi = (double)me.z;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const int cnt = n - w * 64 < 64 ? n - w * 64 : 64;
            for (int jj = 0; jj < cnt; ++jj) {
                if (reach[w] >> jj & 1ull) continue;
                const int j = w * 64 + jj;
                const float4 q = s_at[j];
                const int cq = __float_as_int(q.w), eq = cq & 7;
                if (cq < 0) continue;
                double d;
                td_bond_order(xi, yi, zi, q.x, q.y, q.z, ei * 8 + eq, s_thr, d);
                if (d < s_clash[j > tid ? ei * 8 + eq : eq * 8 + ei]) {         // the table is read as the pair's lower atom first
                    ++mine;
                    pairs += j > tid ? 1 : 0;
                }
            }
        }
    }
    if (n_ang) atomicAdd(&s_cnt[0], n_ang);
    if (n_tor) atomicAdd(&s_cnt[1], n_tor);
    if (n_degen) atomicAdd(&s_cnt[2], n_degen);
    if (deg > GM_DEG) atomicAdd(&s_cnt[3], 1);
    if (pairs) atomicAdd(&s_cnt[4], pairs);
    if (g.clash && g.atom_clash && tid < n) g.atom_clash[(size_t)m.s * (size_t)a.Nl + (size_t)(m.l0 + tid)] = mine;
    __syncthreads();
    if (tid == 0) {
        g.n_angles[m.mol] = s_cnt[0];
        g.n_torsions[m.mol] = s_cnt[1];
        g.n_degenerate[m.mol] = s_cnt[2];
        g.n_crowded[m.mol] = s_cnt[3];
        if (g.clash) g.n_clashes[m.mol] = s_cnt[4];
    }
    bg_flush_hist<MAXN>(&s_hist[0][0], P * GM_BINS, g.hist + (size_t)m.s * g.P * GM_BINS);
}

int td_launch_geometry_report(const TdGeomArgs &g, hipStream_t s) {
    const int64_t M = (int64_t)g.b.S * g.b.B;
    if (g.b.S > 0 && g.P > 0) TD_CHECK_HIP(hipMemsetAsync(g.hist, 0, (size_t)g.b.S * g.P * GM_BINS * sizeof(unsigned long long), s));
    if (M == 0) return TD_OK;
    return bg_launch_pair(geometry_kernel<BG_SMALL>, geometry_kernel<BG_MAX>, g, M, s);
}
