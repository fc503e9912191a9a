// Fingerprints of ligand frames (gfx950, wave64; DESIGN.md section 3, "Fingerprints and diversity"): the bond graph of bonds.hip turned
// into something that compares between molecules, and the molecules of a frame compared.
//   * fingerprint_kernel  one workgroup per (frame, molecule), the molecule and its bit rows in LDS exactly as bond_graph_kernel builds
//                         them (td_bond_graph.h).  Lane i owns atom i.  A circular, Morgan-style refinement on uint64 hashes: id_0 from
//                         the atom's own invariant (atomic number, aromatic class, degree, valence), then per round the commutative sum
//                         of the hashed (neighbour id, bond category) pairs folded into the atom's id.  The ids are double-buffered in
//                         LDS: round r reads buffer (r - 1) & 1 and writes buffer r & 1, so the one barrier that ends a round is also
//                         the one that frees the buffer the next round writes.  A lane walks its own row only (popped with __ffsll,
//                         so always in ascending j) and takes each bond's category from td_bond_order once, as ring_report_kernel
//                         does for its list: the categories of the lane's first FP_CACHED bonds stay in one 64-bit register, two
//                         bits each, and only an atom with more bonds than that derives the further ones again in every round.  No
//                         further bit planes, 50 KiB of LDS at 512 atoms.  Bit id mod 2048 of every valid atom and every round
//                         0 .. radius goes into the LDS bitset by integer atomicOr; the key hashes the multiset of the ids after
//                         key_rounds rounds.
//   * similarity_kernel   one wave per (frame, molecule a): lane l takes the partners b = l, l + 64, ...; c = popcount(fp_a & fp_b)
//                         over the 32 words, T = c / (n_a + n_b - c) in float64.  The terms of a 64-partner chunk go through LDS and
//                         lane 0 adds them in ascending b, one add per term: sim_sum does not depend on the grid.  The maximum and the
//                         first equal key are order-free reductions.
// Every loop is bounded: the rounds by the argument (at most TD_FP_MAX_ROUNDS), the neighbours by the 64 bits of W words, the partners by
// B.  A defect ends in a wrong number, not in a kernel that does not return.  All arithmetic is on wrapping uint64 and int32 except the
// one division of T and td_bond_order; integer LDS atomics only (or, add): nothing depends on the order of arrival.  The two
// instantiations and the answer to an oversize molecule (n_bits -1, words and key 0) are those of bonds.hip.
#include "td_bond_graph.h"

constexpr int FP_CACHED = 32;                                                   // bonds per atom whose category is kept in a register

// the splitmix64 finaliser
__device__ __forceinline__ unsigned long long fp_mix(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

template <int MAXN>
__global__ __launch_bounds__(MAXN) void fingerprint_kernel(TdBondArgs a) {
    constexpr int W = MAXN / 64;
    __shared__ float4 s_at[MAXN];
    __shared__ unsigned long long s_row[W][MAXN];
    __shared__ double s_thr[3][64];
    __shared__ unsigned long long s_id[2][MAXN];
    __shared__ unsigned long long s_fp[TD_FP_WORDS];
    __shared__ unsigned long long s_sum;
    __shared__ int s_elem[TD_QUALITY_MAX_CLASSES];
    __shared__ int s_valid, s_bonds, s_pop;
    const int tid = threadIdx.x;
    const BgMol m = bg_molecule<MAXN>(a);
    if (!m.mine) return;                                                        // workgroup-uniform
    const int n = m.n;
    if (m.bad) {                                                                // only the 512-lane instantiation gets here
        if (tid < TD_FP_WORDS) a.fp_words[m.mol * TD_FP_WORDS + tid] = 0ull;
        if (tid == 0) {
            a.fp_bits[m.mol] = -1;
            a.fp_key[m.mol] = 0ull;
        }
        return;
    }
    td_bond_thresholds(s_thr, tid, MAXN);
    if (tid < TD_QUALITY_MAX_CLASSES) s_elem[tid] = tid < a.K ? a.elem[tid] : -1;
    if (tid < TD_FP_WORDS) s_fp[tid] = 0ull;
    s_id[0][tid] = s_id[1][tid] = 0ull;
    if (tid == 0) {
        s_sum = 0ull;
        s_valid = s_bonds = s_pop = 0;
    }
    bg_load<MAXN>(a, m, s_elem, s_at);
    int up = 0;
    if (tid < n) up = bg_rows<MAXN>(n, s_at, s_thr, s_row, [](int, int, int, double) {});   // a lane reads back its own row only

    const float4 me = tid < n ? s_at[tid] : make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    const int ci = __float_as_int(me.w), ei = ci & 7;
    const bool valid = tid < n && ci >= 0;                                      // an atom of no class takes no part; it has no bonds
    const double xi = (double)me.x, yi = (double)me.y, zi = (double)me.z;
    const unsigned long long mc1 = fp_mix(1ull), mc2 = fp_mix(2ull), mc3 = fp_mix(3ull), mc4 = fp_mix(4ull);
    unsigned long long id = 0ull, cats = 0ull;                                  // cats: category - 1 of the lane's bond k at bits 2 k, k < FP_CACHED
    if (valid) {
        int degree = 0, valence = 0;
        for (int w = 0; w < W; ++w) {
            unsigned long long bits = s_row[w][tid];
            for (int c = 0; c < 64 && bits; ++c) {
                const int j = w * 64 + __ffsll((long long)bits) - 1;
                bits &= bits - 1ull;
                const float4 q = s_at[j];
                const int cj = __float_as_int(q.w);
                double d;
                const int order = td_bond_order(xi, yi, zi, q.x, q.y, q.z, ei * 8 + (cj & 7), s_thr, d);
                if (degree < FP_CACHED) cats |= (unsigned long long)(bg_category(ci, cj, order) - 1) << (2 * degree);
                valence += order;
                ++degree;
            }
        }
        const unsigned long long Z = 0x11100F0908070601ull >> (8 * ei) & 0xffull;   // H C N O F P S Cl
        id = fp_mix(Z | (unsigned long long)(ci >> 8 & 1) << 8 | (unsigned long long)degree << 16 | (unsigned long long)valence << 24);
        s_id[0][tid] = id;
        atomicOr(&s_fp[id >> 6 & (TD_FP_WORDS - 1)], 1ull << (id & 63ull));
        atomicAdd(&s_valid, 1);
        if (up) atomicAdd(&s_bonds, up);
    }
    __syncthreads();

    // ---- the rounds: a.fp_rounds <= TD_FP_MAX_ROUNDS, checked by the entry point
    for (int r = 1; r <= a.fp_rounds; ++r) {
        const int cur = (r - 1) & 1;
        if (valid) {
            unsigned long long acc = 0ull;
            int k = 0;                                                          // the lane's bonds in ascending j, as round 0 met them
            for (int w = 0; w < W; ++w) {
                unsigned long long bits = s_row[w][tid];
                for (int c = 0; c < 64 && bits; ++c, ++k) {
                    const int j = w * 64 + __ffsll((long long)bits) - 1;
                    bits &= bits - 1ull;
                    int cat;
                    if (k < FP_CACHED) {
                        cat = (int)(cats >> (2 * k) & 3ull) + 1;
                    } else {
                        const float4 q = s_at[j];
                        const int cj = __float_as_int(q.w);
                        double d;
                        cat = bg_category(ci, cj, td_bond_order(xi, yi, zi, q.x, q.y, q.z, ei * 8 + (cj & 7), s_thr, d));
                    }
                    acc += fp_mix(s_id[cur][j] ^ (cat == 1 ? mc1 : cat == 2 ? mc2 : cat == 3 ? mc3 : mc4));
                }
            }
            id = fp_mix(fp_mix(id ^ (unsigned long long)r) + acc);
            s_id[cur ^ 1][tid] = id;
            if (r <= a.fp_radius) atomicOr(&s_fp[id >> 6 & (TD_FP_WORDS - 1)], 1ull << (id & 63ull));
        }
        __syncthreads();
    }

    if (valid) atomicAdd(&s_sum, fp_mix(id));
    if (tid < n && a.atom_key) a.atom_key[(size_t)m.s * (size_t)a.Nl + (size_t)(m.l0 + tid)] = id;
    __syncthreads();
    if (tid < TD_FP_WORDS) {
        const unsigned long long word = s_fp[tid];
        a.fp_words[m.mol * TD_FP_WORDS + tid] = word;
        atomicAdd(&s_pop, __popcll(word));
    }
    __syncthreads();
    if (tid == 0) {
        a.fp_bits[m.mol] = s_pop;
        a.fp_key[m.mol] = fp_mix(s_sum ^ fp_mix((unsigned long long)s_valid << 32 | (unsigned long long)s_bonds));
    }
}

int td_launch_fingerprint(const TdBondArgs &a, hipStream_t s) {
    const int64_t M = (int64_t)a.S * a.B;
    if (M == 0) return TD_OK;
    return bg_launch_pair(fingerprint_kernel<BG_SMALL>, fingerprint_kernel<BG_MAX>, a, M, s);
}

__global__ __launch_bounds__(64) void similarity_kernel(TdSimArgs a) {
    __shared__ unsigned long long s_a[TD_FP_WORDS];
    __shared__ double s_t[64];
    const int lane = threadIdx.x;
    const int s = blockIdx.x / a.B, g = blockIdx.x - s * a.B;
    const size_t mol = (size_t)blockIdx.x, row = (size_t)s * a.B;
    if (lane < TD_FP_WORDS) s_a[lane] = a.words[mol * TD_FP_WORDS + lane];
    __syncthreads();
    const int na = a.bits[mol];
    const unsigned long long ka = a.key[mol];
    // a refused molecule (n_bits < 0) is never included: it has no fingerprint
    const bool inc_a = na >= 0 && (!a.include || a.include[mol] != 0);          // wave-uniform
    double sum = 0.0, best = 0.0;
    int first = 0x7fffffff;
    for (int b0 = 0; b0 < a.B; b0 += 64) {
        const int b = b0 + lane;
        double t = -1.0;                                                        // no term: every T is >= 0
        if (b < a.B) {
            const unsigned long long *wb = a.words + (row + b) * TD_FP_WORDS;
            int c = 0;
#pragma unroll 8
            for (int w = 0; w < TD_FP_WORDS; ++w) c += __popcll(s_a[w] & wb[w]);
            if (a.common) a.common[mol * (size_t)a.B + b] = c;
            const int nb = a.bits[row + b];
            if (inc_a && nb >= 0 && (!a.include || a.include[row + b] != 0)) {
                if (a.key[row + b] == ka && b < first) first = b;               // a lane's b ascend: it keeps its first
                if (b != g) {
                    const int uni = na + nb - c;
                    t = uni > 0 ? (double)c / (double)uni : 0.0;
                }
            }
        }
        s_t[lane] = t;
        __syncthreads();
        if (lane == 0) {
            const int cnt = a.B - b0 < 64 ? a.B - b0 : 64;
            for (int k = 0; k < cnt; ++k) {                                     // ascending b, one add per term
                const double x = s_t[k];
                if (x >= 0.0) {
                    sum += x;
                    best = x > best ? x : best;
                }
            }
        }
        __syncthreads();
    }
    // the smallest b over the lanes: lane l holds the smallest of l, l + 64, ...
    for (int off = 32; off > 0; off >>= 1) {
        const int other = __shfl_xor(first, off, 64);
        first = other < first ? other : first;
    }
    if (lane == 0) {
        a.sim_sum[mol] = sum;
        a.sim_max[mol] = best;
        a.first_equal[mol] = inc_a ? first : -1;
    }
    if (a.query_common) {
        for (int q = lane; q < a.Q; q += 64) {
            const unsigned long long *wq = a.q_words + (size_t)q * TD_FP_WORDS;
            int c = 0;
#pragma unroll 8
            for (int w = 0; w < TD_FP_WORDS; ++w) c += __popcll(s_a[w] & wq[w]);
            a.query_common[mol * (size_t)a.Q + q] = c;
        }
    }
}

int td_launch_fingerprint_similarity(const TdSimArgs &a, hipStream_t s) {
    const int64_t M = (int64_t)a.S * a.B;
    if (M == 0) return TD_OK;
    similarity_kernel<<<dim3((unsigned)M), dim3(64), 0, s>>>(a);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}
