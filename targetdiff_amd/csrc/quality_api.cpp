// C ABI of libtargetdiff_hip.so: sample quality of ligand frames (td_quality_report).  See include/targetdiff_hip.h for the contract.
#include "td_device.h"
#include "td_internal.h"

// element index 0..7 (H C N O F P S Cl) of an atomic number, -1 for any other
int td_element_index(int z) {
    static const int Z[8] = {1, 6, 7, 8, 9, 15, 16, 17};
    for (int e = 0; e < 8; ++e)
        if (Z[e] == z) return e;
    return -1;
}

int td_profile_element(int z) {
    const int e = z == 0 ? -1 : td_element_index(z);
    return z != 0 && e < 0 ? -2 : e;
}

int td_check_pack(const char *who, int64_t S, int64_t N_l, int64_t B, const int32_t *class_atomic_number, int32_t K, int8_t *elem) {
    if (S < 0 || B < 0 || N_l < 0 || N_l > 0x7fffffff || S > 0x7fffffff || B > 0x7fffffff || S * B > 0x7fffffff) {
        td_set_error("%s: bad argument (S = %lld, B = %lld, N_l = %lld; S * B and N_l must fit 31 bits)", who, (long long)S, (long long)B,
                     (long long)N_l);
        return TD_EINVAL;
    }
    if (K < 1 || K > TD_QUALITY_MAX_CLASSES || !class_atomic_number) {
        td_set_error("%s: the class table must have 1 .. %d entries (got %d)", who, TD_QUALITY_MAX_CLASSES, (int)K);
        return TD_EINVAL;
    }
    for (int c = 0; c < K; ++c) {
        const int e = td_element_index(class_atomic_number[c]);
        if (e < 0) {
            td_set_error("%s: class %d has atomic number %d, outside the bond-length table (H C N O F P S Cl)", who, c,
                         (int)class_atomic_number[c]);
            return TD_EINVAL;
        }
        elem[c] = (int8_t)e;
    }
    return TD_OK;
}

extern "C" int td_quality_report(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                                 const int32_t *class_atomic_number, int32_t K, const uint8_t *d_include,
                                 const td_pair_profile *profiles, int32_t P, int32_t *d_nr_bonds, int32_t *d_stable_atoms,
                                 uint8_t *d_mol_stable, int64_t *d_hist, int64_t *d_counts, void *stream) {
    const char *who = "td_quality_report";
    TdQualityArgs a;
    if (const int rc = td_check_pack(who, S, N_l, B, class_atomic_number, K, a.elem)) return rc;
    if (P < 0 || P > TD_QUALITY_MAX_PROFILES || (P > 0 && !profiles)) {
        td_set_error("%s: 0 .. %d pair profiles (got %d)", who, TD_QUALITY_MAX_PROFILES, (int)P);
        return TD_EINVAL;
    }
    for (int p = 0; p < P; ++p) {
        const td_pair_profile &pf = profiles[p];
        const int e1 = td_profile_element(pf.z1), e2 = td_profile_element(pf.z2);
        if (e1 < -1 || e2 < -1) {
            td_set_error("%s: profile %d names an atomic number outside the table (%d, %d; 0 = any)", who, p, (int)pf.z1, (int)pf.z2);
            return TD_EINVAL;
        }
        if (pf.n_edges < 1 || pf.n_edges > TD_QUALITY_BINS - 1 || !pf.d_edges) {
            td_set_error("%s: profile %d needs 1 .. %d edges (got %d)", who, p, TD_QUALITY_BINS - 1, (int)pf.n_edges);
            return TD_EINVAL;
        }
        if (!(pf.cutoff > 0.0)) { td_set_error("%s: profile %d: the cutoff must be > 0", who, p); return TD_EINVAL; }
        a.pe1[p] = e1; a.pe2[p] = e2; a.n_edges[p] = pf.n_edges; a.cutoff[p] = pf.cutoff; a.edges[p] = pf.d_edges;
    }
    if (S > 0 && (!d_counts || (P > 0 && !d_hist))) { td_set_error("%s: null pointer", who); return TD_EINVAL; }
    if (S > 0 && B > 0 && (!d_ligand_ptr || !d_stable_atoms || !d_mol_stable || (N_l > 0 && (!d_pos || !d_v)))) {
        td_set_error("%s: null pointer", who);
        return TD_EINVAL;
    }
    a.pos = d_pos; a.v = d_v; a.lptr = d_ligand_ptr; a.include = d_include; a.Nl = N_l;
    a.S = (int)S; a.B = (int)B; a.K = K; a.P = P;
    a.nr_bonds = d_nr_bonds; a.stable_atoms = d_stable_atoms; a.mol_stable = d_mol_stable;
    a.hist = reinterpret_cast<unsigned long long *>(d_hist); a.counts = reinterpret_cast<unsigned long long *>(d_counts);
    return td_launch_quality(a, static_cast<hipStream_t>(stream));
}
