// C ABI of libtargetdiff_hip.so: the bond graph of ligand frames, its rings, its fingerprints, its local geometry and the contacts with
// the pocket, the typed interactions with it, the docking-style score and the surface it buries (td_bond_graph, td_bond_list,
// td_ring_report, td_fingerprint, td_fingerprint_similarity, td_geometry_report, td_pocket_report, td_interaction_report,
// td_score_report, td_score_minimize, td_score_dock, td_sasa_report).  See
// include/targetdiff_hip.h for the contract.
#include <cmath>
#include <initializer_list>

#include "td_device.h"
#include "td_internal.h"
#include "td_api.h"

namespace {
// the checks and the fields the entry points share: sizes, the class table, the aromatic flags and, of the entry points that take the
// bond list's offsets, its length
int bond_pack(const char *who, TdBondArgs &a, const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l,
              int64_t B, const int32_t *class_atomic_number, int32_t K, const uint8_t *class_aromatic, int64_t n_bonds = 0) {
    if (n_bonds < 0) { td_set_error("%s: bad argument (n_bonds = %lld)", who, (long long)n_bonds); return TD_EINVAL; }
    if (const int rc = td_check_pack(who, S, N_l, B, class_atomic_number, K, a.elem)) return rc;
    for (int c = 0; c < K; ++c)
        if (class_aromatic && class_aromatic[c]) a.aromatic |= 1ull << c;
    if (S > 0 && B > 0 && (!d_ligand_ptr || (N_l > 0 && (!d_pos || !d_v)))) {
        td_set_error("%s: null pointer", who);
        return TD_EINVAL;
    }
    a.pos = d_pos; a.v = d_v; a.lptr = d_ligand_ptr; a.Nl = N_l;
    a.S = (int)S; a.B = (int)B; a.K = K; a.capacity = n_bonds;
    return TD_OK;
}

// The protein side that the contact and the interaction report share, checked and filled: N_p with S * planes * N_p (`fits`: what the
// entry point's message says must fit), the number of kinds, the pocket's arrays and the sums by kind and by protein atom.
int protein_side(const char *who, TdProteinSide &p, int64_t S, int64_t N_p, int planes, const char *fits, const float *d_protein_pos,
                 const int32_t *d_protein_elem, const int32_t *d_protein_kind, int32_t n_kinds, const uint64_t *d_ref_bits, uint64_t *d_bits,
                 int64_t *d_kind_hist, int32_t *d_pocket_freq) {
    if (N_p < 0 || N_p > 0x7fffffff / TD_BOND_MAX_ATOMS || S * planes * N_p > 0x7fffffff) {      // a molecule's pairs are counted in an int32
        td_set_error("%s: bad argument (N_p = %lld; %s must fit 31 bits)", who, (long long)N_p, fits);
        return TD_EINVAL;
    }
    if (n_kinds < 1 || n_kinds > TD_POCKET_MAX_KINDS) {
        td_set_error("%s: 1 .. %d kinds of protein atoms (got %d)", who, TD_POCKET_MAX_KINDS, (int)n_kinds);
        return TD_EINVAL;
    }
    if ((N_p > 0 && (!d_protein_pos || !d_protein_elem || !d_protein_kind)) || (S > 0 && (!d_kind_hist || (N_p > 0 && !d_pocket_freq)))) {
        td_set_error("%s: null pointer", who);
        return TD_EINVAL;
    }
    p.ppos = d_protein_pos; p.pelem = d_protein_elem; p.pkind = d_protein_kind;
    p.Np = (int)N_p; p.W = (int)((N_p + 63) / 64); p.n_kinds = n_kinds;
    p.ref_bits = reinterpret_cast<const unsigned long long *>(d_ref_bits);
    p.bits = reinterpret_cast<unsigned long long *>(d_bits); p.kind_hist = reinterpret_cast<unsigned long long *>(d_kind_hist);
    p.pocket_freq = d_pocket_freq;
    return TD_OK;
}
}  // namespace

extern "C" int td_bond_graph(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                             const int32_t *class_atomic_number, int32_t K, const uint8_t *d_include, const uint8_t *class_aromatic,
                             const td_bond_profile *profiles, int32_t P, int32_t *d_n_bonds, int32_t *d_n_fragments,
                             int32_t *d_largest_fragment, int32_t *d_fragment, int64_t *d_bond_hist, int64_t *d_bond_ptr, void *stream) {
    const char *who = "td_bond_graph";
    TdBondArgs a;
    if (P < 0 || P > TD_BOND_MAX_PROFILES || (P > 0 && !profiles)) {
        td_set_error("%s: 0 .. %d bond profiles (got %d)", who, TD_BOND_MAX_PROFILES, (int)P);
        return TD_EINVAL;
    }
    for (int p = 0; p < P; ++p) {
        const td_bond_profile &pf = profiles[p];
        const int e1 = td_profile_element(pf.z1), e2 = td_profile_element(pf.z2);
        if (e1 < -1 || e2 < -1) {
            td_set_error("%s: profile %d names an atomic number outside the table (%d, %d; 0 = any)", who, p, (int)pf.z1, (int)pf.z2);
            return TD_EINVAL;
        }
        if (pf.category < 0 || pf.category > 4) {
            td_set_error("%s: profile %d: the category must be 0 (any), 1, 2, 3 or 4 (got %d)", who, p, (int)pf.category);
            return TD_EINVAL;
        }
        if (pf.n_edges < 1 || pf.n_edges > TD_BOND_BINS - 1 || !pf.d_edges) {
            td_set_error("%s: profile %d needs 1 .. %d edges (got %d)", who, p, TD_BOND_BINS - 1, (int)pf.n_edges);
            return TD_EINVAL;
        }
        a.pe1[p] = (int8_t)e1; a.pe2[p] = (int8_t)e2; a.pcat[p] = (int8_t)pf.category; a.n_edges[p] = (int16_t)pf.n_edges;
        a.edges[p] = pf.d_edges;
    }
    if (const int rc = bond_pack(who, a, d_pos, d_v, d_ligand_ptr, S, N_l, B, class_atomic_number, K, class_aromatic)) return rc;
    if ((S > 0 && P > 0 && !d_bond_hist) || (S > 0 && B > 0 && (!d_n_bonds || !d_n_fragments || !d_largest_fragment))) {
        td_set_error("%s: null pointer", who);
        return TD_EINVAL;
    }
    a.include = d_include; a.P = P;
    a.n_bonds = d_n_bonds; a.n_fragments = d_n_fragments; a.largest = d_largest_fragment; a.fragment = d_fragment;
    a.hist = reinterpret_cast<unsigned long long *>(d_bond_hist); a.bond_ptr = d_bond_ptr;
    return td_launch_bond_graph(a, static_cast<hipStream_t>(stream));
}

extern "C" int td_bond_list(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                            const int32_t *class_atomic_number, int32_t K, const uint8_t *class_aromatic, const int64_t *d_bond_ptr,
                            int64_t n_bonds, int32_t *d_bond_atoms, uint8_t *d_bond_order, uint8_t *d_bond_category,
                            double *d_bond_length, void *stream) {
    const char *who = "td_bond_list";
    TdBondArgs a;
    if (const int rc = bond_pack(who, a, d_pos, d_v, d_ligand_ptr, S, N_l, B, class_atomic_number, K, class_aromatic, n_bonds)) return rc;
    if (S > 0 && B > 0 && n_bonds > 0 && (!d_bond_ptr || !d_bond_atoms || !d_bond_order || !d_bond_category || !d_bond_length)) {
        td_set_error("%s: null pointer", who);
        return TD_EINVAL;
    }
    a.bond_ptr = const_cast<int64_t *>(d_bond_ptr);
    a.bond_atoms = d_bond_atoms; a.bond_order = d_bond_order; a.bond_category = d_bond_category; a.bond_length = d_bond_length;
    return td_launch_bond_list(a, static_cast<hipStream_t>(stream));
}

extern "C" int td_ring_report(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                              const int32_t *class_atomic_number, int32_t K, const uint8_t *d_include, const uint8_t *class_aromatic,
                              const int64_t *d_bond_ptr, int64_t n_bonds, uint32_t *d_ring_mask, int32_t *d_n_ring_bonds,
                              int32_t *d_n_ring_atoms, int32_t *d_atom_ring, int64_t *d_ring_hist, uint16_t *d_bond_ring,
                              uint8_t *d_bond_category, void *stream) {
    const char *who = "td_ring_report";
    TdBondArgs a;
    if (const int rc = bond_pack(who, a, d_pos, d_v, d_ligand_ptr, S, N_l, B, class_atomic_number, K, class_aromatic, n_bonds)) return rc;
    if ((d_bond_ring || d_bond_category) && !d_bond_ptr) {
        td_set_error("%s: the per-bond outputs need d_bond_ptr of td_bond_graph", who);
        return TD_EINVAL;
    }
    if ((S > 0 && !d_ring_hist) || (S > 0 && B > 0 && (!d_ring_mask || !d_n_ring_bonds || !d_n_ring_atoms))) {
        td_set_error("%s: null pointer", who);
        return TD_EINVAL;
    }
    a.include = d_include;
    a.bond_ptr = const_cast<int64_t *>(d_bond_ptr);
    a.ring_mask = d_ring_mask; a.n_ring_bonds = d_n_ring_bonds; a.n_ring_atoms = d_n_ring_atoms; a.atom_ring = d_atom_ring;
    a.ring_hist = reinterpret_cast<unsigned long long *>(d_ring_hist); a.bond_ring = d_bond_ring; a.bond_category = d_bond_category;
    return td_launch_ring_report(a, static_cast<hipStream_t>(stream));
}

extern "C" int td_fingerprint(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                              const int32_t *class_atomic_number, int32_t K, const uint8_t *class_aromatic, int32_t radius,
                              int32_t key_rounds, int64_t *d_fp_words, int32_t *d_n_bits, int64_t *d_key, int64_t *d_atom_key,
                              void *stream) {
    const char *who = "td_fingerprint";
    TdBondArgs a;
    if (radius < 0 || radius > TD_FP_MAX_RADIUS || key_rounds < radius || key_rounds > TD_FP_MAX_ROUNDS) {
        td_set_error("%s: 0 <= radius <= %d and radius <= key_rounds <= %d (got %d, %d)", who, TD_FP_MAX_RADIUS, TD_FP_MAX_ROUNDS, (int)radius,
                     (int)key_rounds);
        return TD_EINVAL;
    }
    if (const int rc = bond_pack(who, a, d_pos, d_v, d_ligand_ptr, S, N_l, B, class_atomic_number, K, class_aromatic)) return rc;
    if (S > 0 && B > 0 && (!d_fp_words || !d_n_bits || !d_key)) {
        td_set_error("%s: null pointer", who);
        return TD_EINVAL;
    }
    a.fp_radius = radius; a.fp_rounds = key_rounds;
    a.fp_words = reinterpret_cast<unsigned long long *>(d_fp_words); a.fp_bits = d_n_bits;
    a.fp_key = reinterpret_cast<unsigned long long *>(d_key); a.atom_key = reinterpret_cast<unsigned long long *>(d_atom_key);
    return td_launch_fingerprint(a, static_cast<hipStream_t>(stream));
}

extern "C" int td_fingerprint_similarity(const int64_t *d_fp_words, const int32_t *d_n_bits, const int64_t *d_key, int64_t S, int64_t B,
                                         const uint8_t *d_include, const int64_t *d_q_words, int64_t Q, double *d_sim_sum,
                                         double *d_sim_max, int32_t *d_first_equal, int32_t *d_common, int32_t *d_query_common,
                                         void *stream) {
    const char *who = "td_fingerprint_similarity";
    if (S < 0 || B < 0 || Q < 0 || S > 0x7fffffff || B > 0x7fffffff || Q > 0x7fffffff || S * B > 0x7fffffff) {
        td_set_error("%s: bad argument (S = %lld, B = %lld, Q = %lld; S * B and Q must fit 31 bits)", who, (long long)S, (long long)B,
                     (long long)Q);
        return TD_EINVAL;
    }
    if (Q > 0 && (!d_q_words || (S > 0 && B > 0 && !d_query_common))) {
        td_set_error("%s: a query set needs d_q_words and d_query_common", who);
        return TD_EINVAL;
    }
    if (S > 0 && B > 0 && (!d_fp_words || !d_n_bits || !d_key || !d_sim_sum || !d_sim_max || !d_first_equal)) {
        td_set_error("%s: null pointer", who);
        return TD_EINVAL;
    }
    TdSimArgs a;
    a.words = reinterpret_cast<const unsigned long long *>(d_fp_words); a.bits = d_n_bits;
    a.key = reinterpret_cast<const unsigned long long *>(d_key); a.include = d_include;
    a.q_words = reinterpret_cast<const unsigned long long *>(d_q_words);
    a.S = (int)S; a.B = (int)B; a.Q = (int)Q;
    a.sim_sum = d_sim_sum; a.sim_max = d_sim_max; a.first_equal = d_first_equal; a.common = d_common;
    a.query_common = Q > 0 ? d_query_common : nullptr;
    return td_launch_fingerprint_similarity(a, static_cast<hipStream_t>(stream));
}

extern "C" int td_geometry_report(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                                  const int32_t *class_atomic_number, int32_t K, const uint8_t *d_include, const uint8_t *class_aromatic,
                                  const td_geometry_profile *profiles, int32_t P, const int64_t *d_bond_ptr, int64_t n_bonds,
                                  const uint16_t *d_bond_ring, const double *clash_threshold, int32_t *d_n_angles, int32_t *d_n_torsions,
                                  int32_t *d_n_degenerate, int32_t *d_n_crowded, int32_t *d_n_clashes, int32_t *d_atom_clash,
                                  int64_t *d_hist, void *stream) {
    const char *who = "td_geometry_report";
    TdGeomArgs g;
    if (P < 0 || P > TD_GEOM_MAX_PROFILES || (P > 0 && !profiles)) {
        td_set_error("%s: 0 .. %d geometry profiles (got %d)", who, TD_GEOM_MAX_PROFILES, (int)P);
        return TD_EINVAL;
    }
    for (int p = 0; p < P; ++p) {
        const td_geometry_profile &pf = profiles[p];
        if (pf.kind != 1 && pf.kind != 2) {
            td_set_error("%s: profile %d: the kind must be 1 (angle) or 2 (torsion) (got %d)", who, p, (int)pf.kind);
            return TD_EINVAL;
        }
        for (int q = 0; q < 4; ++q) {
            const int e = td_profile_element(pf.z[q]);
            if (e < -1) {
                td_set_error("%s: profile %d names an atomic number outside the table (%d; 0 = any)", who, p, (int)pf.z[q]);
                return TD_EINVAL;
            }
            g.z[p][q] = (int8_t)e;
        }
        if (pf.category < 0 || pf.category > 4 || pf.ring < 0 || pf.ring > 2) {
            td_set_error("%s: profile %d: the category must be 0 (any) .. 4 and the ring filter 0 (any), 1 or 2 (got %d, %d)", who, p,
                         (int)pf.category, (int)pf.ring);
            return TD_EINVAL;
        }
        if (pf.kind == 1 && (pf.z[3] != 0 || pf.category != 0 || pf.ring != 0)) {
            td_set_error("%s: profile %d: an angle has three elements (z[3] = 0) and no category or ring filter", who, p);
            return TD_EINVAL;
        }
        if (pf.ring != 0 && (!d_bond_ptr || !d_bond_ring)) {
            td_set_error("%s: profile %d: the ring filter needs d_bond_ptr of td_bond_graph and d_bond_ring of td_ring_report", who, p);
            return TD_EINVAL;
        }
        if (pf.n_edges < 1 || pf.n_edges > TD_GEOM_BINS - 1 || !pf.d_edges) {
            td_set_error("%s: profile %d needs 1 .. %d edges (got %d)", who, p, TD_GEOM_BINS - 1, (int)pf.n_edges);
            return TD_EINVAL;
        }
        g.kind[p] = (int8_t)pf.kind; g.cat[p] = (int8_t)pf.category; g.ring[p] = (int8_t)pf.ring; g.n_edges[p] = (int16_t)pf.n_edges;
        g.edges[p] = pf.d_edges;
    }
    if (const int rc = bond_pack(who, g.b, d_pos, d_v, d_ligand_ptr, S, N_l, B, class_atomic_number, K, class_aromatic, n_bonds)) return rc;
    if ((S > 0 && P > 0 && !d_hist) ||
        (S > 0 && B > 0 && (!d_n_angles || !d_n_torsions || !d_n_degenerate || !d_n_crowded || (clash_threshold && !d_n_clashes)))) {
        td_set_error("%s: null pointer", who);
        return TD_EINVAL;
    }
    g.b.include = d_include; g.P = P;
    g.b.bond_ptr = const_cast<int64_t *>(d_bond_ptr); g.b.bond_ring = const_cast<uint16_t *>(d_bond_ring);
    if (clash_threshold) {
        g.clash = true;
        for (int k = 0; k < 64; ++k) g.clash_thr[k] = clash_threshold[k];
    }
    g.n_angles = d_n_angles; g.n_torsions = d_n_torsions; g.n_degenerate = d_n_degenerate; g.n_crowded = d_n_crowded;
    g.n_clashes = d_n_clashes; g.atom_clash = d_atom_clash;
    g.hist = reinterpret_cast<unsigned long long *>(d_hist);
    return td_launch_geometry_report(g, static_cast<hipStream_t>(stream));
}

extern "C" int td_pocket_report(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                                const int32_t *class_atomic_number, int32_t K, const uint8_t *d_include, const float *d_protein_pos,
                                const int32_t *d_protein_elem, const int32_t *d_protein_kind, int64_t N_p, int32_t n_kinds,
                                double contact_cutoff, const double *clash_threshold, const uint64_t *d_ref_bits, int32_t *d_n_contacts,
                                int32_t *d_n_contact_atoms, int32_t *d_n_pocket_atoms, int32_t *d_n_clashes, int32_t *d_n_clash_atoms,
                                double *d_min_dist, int32_t *d_n_ref_common, int32_t *d_atom_contacts, int32_t *d_atom_clash,
                                uint64_t *d_bits, int64_t *d_kind_hist, int32_t *d_pocket_freq, void *stream) {
    const char *who = "td_pocket_report";
    TdPocketArgs g;
    if (const int rc = bond_pack(who, g.b, d_pos, d_v, d_ligand_ptr, S, N_l, B, class_atomic_number, K, nullptr)) return rc;
    if (const int rc = protein_side(who, g.p, S, N_p, 1, "512 N_p and S * N_p", d_protein_pos, d_protein_elem, d_protein_kind, n_kinds,
                                    d_ref_bits, d_bits, d_kind_hist, d_pocket_freq)) return rc;
    if (!std::isfinite(contact_cutoff) || !(contact_cutoff > 0.0)) {
        td_set_error("%s: the contact cutoff must be finite and > 0", who);
        return TD_EINVAL;
    }
    if (S > 0 && B > 0 && (!d_n_contacts || !d_n_contact_atoms || !d_n_pocket_atoms || !d_min_dist ||
                           (clash_threshold && (!d_n_clashes || !d_n_clash_atoms)) || (d_ref_bits && !d_n_ref_common))) {
        td_set_error("%s: null pointer", who);
        return TD_EINVAL;
    }
    g.b.include = d_include;
    g.cutoff = contact_cutoff;
    if (clash_threshold) {
        g.clash = true;
        for (int k = 0; k < 8 * TD_POCKET_ELEMENTS; ++k) g.clash_thr[k] = clash_threshold[k];
    }
    g.n_contacts = d_n_contacts; g.n_contact_atoms = d_n_contact_atoms; g.n_pocket_atoms = d_n_pocket_atoms;
    g.n_clashes = d_n_clashes; g.n_clash_atoms = d_n_clash_atoms; g.min_dist = d_min_dist; g.n_ref_common = d_n_ref_common;
    g.atom_contacts = d_atom_contacts; g.atom_clash = d_atom_clash;
    return td_launch_pocket_report(g, static_cast<hipStream_t>(stream));
}

extern "C" int td_interaction_report(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                                     const int32_t *class_atomic_number, int32_t K, const uint8_t *d_include, const float *d_protein_pos,
                                     const int32_t *d_protein_elem, const int32_t *d_protein_kind, const int32_t *d_protein_role,
                                     int64_t N_p, int32_t n_kinds, double hbond_cutoff, double hydrophobic_cutoff, double hetero_cutoff,
                                     const uint64_t *d_ref_bits, int32_t *d_protein_role_out, int32_t *d_n_donated, int32_t *d_n_accepted,
                                     int32_t *d_n_hbonds, int32_t *d_n_hydrophobic, int32_t *d_n_hb_atoms, int32_t *d_n_donors,
                                     int32_t *d_n_acceptors, int32_t *d_n_hydrophobic_atoms, int32_t *d_n_ref_common, int32_t *d_atom_role,
                                     int32_t *d_atom_hbonds, int32_t *d_atom_hydrophobic, uint64_t *d_bits, int64_t *d_kind_hist,
                                     int32_t *d_pocket_freq, void *stream) {
    const char *who = "td_interaction_report";
    TdInteractionArgs g;
    if (const int rc = bond_pack(who, g.b, d_pos, d_v, d_ligand_ptr, S, N_l, B, class_atomic_number, K, nullptr)) return rc;
    if (const int rc = protein_side(who, g.p, S, N_p, TD_INTERACTION_TYPES, "512 N_p and 3 S * N_p", d_protein_pos, d_protein_elem,
                                    d_protein_kind, n_kinds, d_ref_bits, d_bits, d_kind_hist, d_pocket_freq)) return rc;
    for (const double c : {hbond_cutoff, hydrophobic_cutoff, hetero_cutoff})
        if (!std::isfinite(c) || !(c > 0.0)) {
            td_set_error("%s: the hbond, hydrophobic and hetero cutoffs must be finite and > 0", who);
            return TD_EINVAL;
        }
    if ((N_p > 0 && (!d_protein_role || !d_protein_role_out)) ||
        (S > 0 && B > 0 && (!d_n_donated || !d_n_accepted || !d_n_hbonds || !d_n_hydrophobic || !d_n_hb_atoms || !d_n_donors ||
                            !d_n_acceptors || !d_n_hydrophobic_atoms || (d_ref_bits && !d_n_ref_common)))) {
        td_set_error("%s: null pointer", who);
        return TD_EINVAL;
    }
    g.b.include = d_include;
    g.prole = d_protein_role;
    g.hbond_cutoff = hbond_cutoff; g.hydrophobic_cutoff = hydrophobic_cutoff; g.hetero_cutoff = hetero_cutoff;
    g.role_out = d_protein_role_out;
    g.n_donated = d_n_donated; g.n_accepted = d_n_accepted; g.n_hbonds = d_n_hbonds; g.n_hydrophobic = d_n_hydrophobic;
    g.n_hb_atoms = d_n_hb_atoms; g.n_donors = d_n_donors; g.n_acceptors = d_n_acceptors; g.n_hydrophobic_atoms = d_n_hydrophobic_atoms;
    g.n_ref_common = d_n_ref_common;
    g.atom_role = d_atom_role; g.atom_hbonds = d_atom_hbonds; g.atom_hydrophobic = d_atom_hydrophobic;
    return td_launch_interaction_report(g, static_cast<hipStream_t>(stream));
}

namespace {
// The arguments of td_score_report, td_score_minimize and td_score_dock by side, the members in the order of the C argument lists: an
// exported symbol brace-initialises them from its flat list, once, and everything below it passes the structs.  ScoreSide: the inputs the
// three share (the pack, the aromatic flags, the pocket, the cutoffs, the radius sums, the rotor inputs) and the two outputs score_side
// fills; RelaxSide: the optimiser's; DockSide: the search's.
struct ScoreSide {
    const float *d_pos; const int64_t *d_v; const int32_t *d_ligand_ptr; int64_t S, N_l, B; const int32_t *class_atomic_number; int32_t K;
    const uint8_t *class_aromatic; const float *d_protein_pos; const int32_t *d_protein_elem, *d_protein_kind, *d_protein_role; int64_t N_p;
    int32_t n_kinds; double cutoff, hetero_cutoff; const double *rsum; const int64_t *d_bond_ptr; int64_t n_bonds; const uint16_t *d_bond_ring;
    int32_t *d_protein_role_out, *d_n_rot;
};
struct RelaxSide {
    const double *weights; int32_t max_steps, max_evals; double max_shift; int32_t list_capacity; float *d_pos_out; int64_t *d_terms_in;
    int64_t *d_terms_out; int32_t *d_n_pairs_out, *d_n_steps, *d_n_evals, *d_status; double *d_transform; int64_t *d_grad_in;
};
struct DockSide {
    int32_t n_chains, n_rounds; double amplitude, temperature; const double *d_draws; int32_t *d_best_chain; int64_t *d_chain_terms;
    double *d_chain_transform; int32_t *d_chain_accepts, *d_chain_evals;
};

// What the three entry points share: the pack, the pocket, the cutoffs, the radius sums and the rotor inputs checked and filled into g,
// and the protein roles resolved on the stream.  The outputs of each (beyond d_protein_role_out and d_n_rot) are its own.
int score_side(const char *who, TdScoreArgs &g, const ScoreSide &in, hipStream_t stream) {
    if (const int rc = bond_pack(who, g.b, in.d_pos, in.d_v, in.d_ligand_ptr, in.S, in.N_l, in.B, in.class_atomic_number, in.K,
                                 in.class_aromatic, in.n_bonds)) return rc;
    if (in.N_p < 0 || in.N_p > 0x7fffffff / TD_BOND_MAX_ATOMS) {                // a molecule's pairs are counted in an int32
        td_set_error("%s: bad argument (N_p = %lld; 512 N_p must fit 31 bits)", who, (long long)in.N_p);
        return TD_EINVAL;
    }
    if (in.n_kinds < 1 || in.n_kinds > TD_POCKET_MAX_KINDS) {
        td_set_error("%s: 1 .. %d kinds of protein atoms (got %d)", who, TD_POCKET_MAX_KINDS, (int)in.n_kinds);
        return TD_EINVAL;
    }
    for (const double c : {in.cutoff, in.hetero_cutoff})
        if (!std::isfinite(c) || !(c > 0.0)) {
            td_set_error("%s: the cutoff and the hetero cutoff must be finite and > 0", who);
            return TD_EINVAL;
        }
    if (!in.rsum) { td_set_error("%s: null pointer", who); return TD_EINVAL; }
    for (int k = 0; k < 8 * TD_POCKET_ELEMENTS; ++k) {
        if (!std::isfinite(in.rsum[k]) || !(in.rsum[k] > 0.0) || !(in.rsum[k] <= 6.0)) {
            td_set_error("%s: every radius sum must be in (0, 6] (entry %d)", who, k);
            return TD_EINVAL;
        }
        g.rsum[k] = in.rsum[k];
    }
    // the rotor inputs come together: the offsets of td_bond_graph, the length of the list and, where it has entries, the ring sizes
    const bool rotors = in.d_bond_ptr != nullptr;
    if ((!rotors && (in.d_bond_ring || in.n_bonds != 0)) || (rotors && in.n_bonds > 0 && !in.d_bond_ring)) {
        td_set_error("%s: d_bond_ptr, n_bonds and d_bond_ring are given together or not at all", who);
        return TD_EINVAL;
    }
    if ((in.N_p > 0 && (!in.d_protein_pos || !in.d_protein_elem || !in.d_protein_kind || !in.d_protein_role || !in.d_protein_role_out)) ||
        (in.S > 0 && in.B > 0 && rotors && !in.d_n_rot)) {
        td_set_error("%s: null pointer", who);
        return TD_EINVAL;
    }
    TdInteractionArgs roles;
    TdProteinSide &p = roles.p;
    p.ppos = in.d_protein_pos; p.pelem = in.d_protein_elem; p.pkind = in.d_protein_kind;
    p.Np = (int)in.N_p; p.W = (int)((in.N_p + 63) / 64); p.n_kinds = in.n_kinds;
    roles.prole = in.d_protein_role; roles.hetero_cutoff = in.hetero_cutoff; roles.role_out = in.d_protein_role_out;
    if (const int rc = td_launch_protein_roles(roles, stream)) return rc;
    g.p = p;
    g.role = in.d_protein_role_out;
    g.cutoff = in.cutoff;
    g.b.bond_ptr = const_cast<int64_t *>(in.d_bond_ptr); g.b.bond_ring = const_cast<uint16_t *>(in.d_bond_ring);
    g.n_rot = in.d_n_rot;
    return TD_OK;
}

// What td_score_minimize and td_score_dock share: the optimiser's arguments and outputs checked and filled into g, then score_side.
int relax_side(const char *who, TdRelaxArgs &g, const ScoreSide &in, const RelaxSide &rx, hipStream_t stream) {
    if (rx.max_steps < 0 || rx.max_evals < 1 || rx.list_capacity < 0) {
        td_set_error("%s: bad argument (max_steps = %d must be >= 0, max_evals = %d must be >= 1)", who, (int)rx.max_steps, (int)rx.max_evals);
        return TD_EINVAL;
    }
    if (!std::isfinite(rx.max_shift) || !(rx.max_shift > 0.0)) {
        td_set_error("%s: max_shift must be finite and > 0", who);
        return TD_EINVAL;
    }
    if (!rx.weights) { td_set_error("%s: null pointer", who); return TD_EINVAL; }
    for (int k = 0; k < TD_SCORE_TERMS; ++k) {
        if (!std::isfinite(rx.weights[k])) { td_set_error("%s: the weights must be finite (weight %d)", who, k); return TD_EINVAL; }
        g.w[k] = rx.weights[k];
    }
    if ((in.S > 0 && in.N_l > 0 && (!rx.d_pos_out || rx.d_pos_out == in.d_pos)) ||
        (in.S > 0 && in.B > 0 && (!rx.d_terms_in || !rx.d_terms_out || !rx.d_n_pairs_out || !rx.d_n_steps || !rx.d_n_evals || !rx.d_status ||
                                  !rx.d_transform || !rx.d_grad_in))) {
        td_set_error("%s: null pointer (d_pos_out may not be d_pos)", who);
        return TD_EINVAL;
    }
    if (const int rc = score_side(who, g.sc, in, stream)) return rc;
    g.max_steps = rx.max_steps; g.max_evals = rx.max_evals; g.max_shift = rx.max_shift; g.list_capacity = rx.list_capacity;
    g.pos_out = rx.d_pos_out;
    g.terms_in = reinterpret_cast<long long *>(rx.d_terms_in); g.terms_out = reinterpret_cast<long long *>(rx.d_terms_out);
    g.n_pairs_out = rx.d_n_pairs_out; g.n_steps = rx.d_n_steps; g.n_evals = rx.d_n_evals; g.status = rx.d_status;
    g.transform = rx.d_transform; g.grad_in = reinterpret_cast<long long *>(rx.d_grad_in);
    return TD_OK;
}

// td_score_dock's own: the search's arguments and outputs checked and filled into d, then relax_side.
int dock_side(const char *who, TdDockArgs &d, const ScoreSide &in, const RelaxSide &rx, const DockSide &dk, hipStream_t stream) {
    if (dk.n_chains < 1 || dk.n_chains > TD_DOCK_MAX_CHAINS || dk.n_rounds < 0 || dk.n_rounds > TD_DOCK_MAX_ROUNDS) {
        td_set_error("%s: bad argument (n_chains = %d must be in 1 .. %d, n_rounds = %d in 0 .. %d)", who, (int)dk.n_chains, TD_DOCK_MAX_CHAINS,
                     (int)dk.n_rounds, TD_DOCK_MAX_ROUNDS);
        return TD_EINVAL;
    }
    if (!std::isfinite(dk.amplitude) || !(dk.amplitude > 0.0) || !std::isfinite(dk.temperature) || !(dk.temperature > 0.0)) {
        td_set_error("%s: amplitude and temperature must be finite and > 0", who);
        return TD_EINVAL;
    }
    if (in.S > 0 && in.B > 0 &&
        (!dk.d_draws || !dk.d_best_chain || !dk.d_chain_terms || !dk.d_chain_transform || !dk.d_chain_accepts || !dk.d_chain_evals)) {
        td_set_error("%s: null pointer", who);
        return TD_EINVAL;
    }
    if (const int rc = relax_side(who, d.rx, in, rx, stream)) return rc;
    d.n_chains = dk.n_chains; d.n_rounds = dk.n_rounds; d.amplitude = dk.amplitude; d.temperature = dk.temperature; d.draws = dk.d_draws;
    d.best_chain = dk.d_best_chain; d.chain_terms = reinterpret_cast<long long *>(dk.d_chain_terms); d.chain_transform = dk.d_chain_transform;
    d.chain_accepts = dk.d_chain_accepts; d.chain_evals = dk.d_chain_evals;
    return TD_OK;
}
}  // namespace

extern "C" int td_score_report(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                               const int32_t *class_atomic_number, int32_t K, const uint8_t *class_aromatic, const float *d_protein_pos,
                               const int32_t *d_protein_elem, const int32_t *d_protein_kind, const int32_t *d_protein_role, int64_t N_p,
                               int32_t n_kinds, double cutoff, double hetero_cutoff, const double *rsum, const int64_t *d_bond_ptr,
                               int64_t n_bonds, const uint16_t *d_bond_ring, int32_t *d_protein_role_out, int64_t *d_terms,
                               int32_t *d_n_pairs, int32_t *d_n_rot, void *stream) {
    const char *who = "td_score_report";
    const ScoreSide in{d_pos, d_v, d_ligand_ptr, S, N_l, B, class_atomic_number, K, class_aromatic, d_protein_pos, d_protein_elem,
                       d_protein_kind, d_protein_role, N_p, n_kinds, cutoff, hetero_cutoff, rsum, d_bond_ptr, n_bonds, d_bond_ring,
                       d_protein_role_out, d_n_rot};
    if (S > 0 && B > 0 && (!d_terms || !d_n_pairs)) { td_set_error("%s: null pointer", who); return TD_EINVAL; }
    TdScoreArgs g;
    if (const int rc = score_side(who, g, in, static_cast<hipStream_t>(stream))) return rc;
    g.terms = reinterpret_cast<long long *>(d_terms); g.n_pairs = d_n_pairs;
    return td_launch_score_report(g, static_cast<hipStream_t>(stream));
}

// td_score_minimize with the capacity of the LDS list as an argument (0 .. TD_RELAX_LIST_CAPACITY; 0: every molecule walks the pocket in
// global memory): for the tests that show the two walks give the same bytes.  Not part of the public ABI (no declaration in
// include/targetdiff_hip.h).
extern "C" __attribute__((visibility("default"))) int td_internal_score_minimize_capacity(
    const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B, const int32_t *class_atomic_number,
    int32_t K, const uint8_t *class_aromatic, const float *d_protein_pos, const int32_t *d_protein_elem, const int32_t *d_protein_kind,
    const int32_t *d_protein_role, int64_t N_p, int32_t n_kinds, double cutoff, double hetero_cutoff, const double *rsum,
    const int64_t *d_bond_ptr, int64_t n_bonds, const uint16_t *d_bond_ring, const double *weights, int32_t max_steps, int32_t max_evals,
    double max_shift, int32_t *d_protein_role_out, int32_t *d_n_rot, float *d_pos_out, int64_t *d_terms_in, int64_t *d_terms_out,
    int32_t *d_n_pairs_out, int32_t *d_n_steps, int32_t *d_n_evals, int32_t *d_status, double *d_transform, int64_t *d_grad_in, void *stream,
    int32_t list_capacity) {
    const ScoreSide in{d_pos, d_v, d_ligand_ptr, S, N_l, B, class_atomic_number, K, class_aromatic, d_protein_pos, d_protein_elem,
                       d_protein_kind, d_protein_role, N_p, n_kinds, cutoff, hetero_cutoff, rsum, d_bond_ptr, n_bonds, d_bond_ring,
                       d_protein_role_out, d_n_rot};
    const RelaxSide rx{weights, max_steps, max_evals, max_shift, list_capacity, d_pos_out, d_terms_in, d_terms_out, d_n_pairs_out, d_n_steps,
                       d_n_evals, d_status, d_transform, d_grad_in};
    TdRelaxArgs g;
    if (const int rc = relax_side("td_score_minimize", g, in, rx, static_cast<hipStream_t>(stream))) return rc;
    return td_launch_score_minimize(g, static_cast<hipStream_t>(stream));
}

extern "C" int td_score_minimize(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                                 const int32_t *class_atomic_number, int32_t K, const uint8_t *class_aromatic, const float *d_protein_pos,
                                 const int32_t *d_protein_elem, const int32_t *d_protein_kind, const int32_t *d_protein_role, int64_t N_p,
                                 int32_t n_kinds, double cutoff, double hetero_cutoff, const double *rsum, const int64_t *d_bond_ptr,
                                 int64_t n_bonds, const uint16_t *d_bond_ring, const double *weights, int32_t max_steps, int32_t max_evals,
                                 double max_shift, int32_t *d_protein_role_out, int32_t *d_n_rot, float *d_pos_out, int64_t *d_terms_in,
                                 int64_t *d_terms_out, int32_t *d_n_pairs_out, int32_t *d_n_steps, int32_t *d_n_evals, int32_t *d_status,
                                 double *d_transform, int64_t *d_grad_in, void *stream) {
    return td_internal_score_minimize_capacity(d_pos, d_v, d_ligand_ptr, S, N_l, B, class_atomic_number, K, class_aromatic, d_protein_pos,
                                               d_protein_elem, d_protein_kind, d_protein_role, N_p, n_kinds, cutoff, hetero_cutoff, rsum,
                                               d_bond_ptr, n_bonds, d_bond_ring, weights, max_steps, max_evals, max_shift, d_protein_role_out,
                                               d_n_rot, d_pos_out, d_terms_in, d_terms_out, d_n_pairs_out, d_n_steps, d_n_evals, d_status,
                                               d_transform, d_grad_in, stream, TD_RELAX_LIST_CAPACITY);
}

// td_score_dock with the capacity of the LDS list as a last argument, as td_internal_score_minimize_capacity; not part of the public ABI.
extern "C" __attribute__((visibility("default"))) int td_internal_score_dock_capacity(
    const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
    const int32_t *class_atomic_number, int32_t K, const uint8_t *class_aromatic, const float *d_protein_pos, const int32_t *d_protein_elem,
    const int32_t *d_protein_kind, const int32_t *d_protein_role, int64_t N_p, int32_t n_kinds, double cutoff, double hetero_cutoff,
    const double *rsum, const int64_t *d_bond_ptr, int64_t n_bonds, const uint16_t *d_bond_ring, const double *weights, int32_t max_steps,
    int32_t max_evals, double max_shift, int32_t n_chains, int32_t n_rounds, double amplitude, double temperature, const double *d_draws,
    int32_t *d_protein_role_out, int32_t *d_n_rot, float *d_pos_out, int64_t *d_terms_in, int64_t *d_terms_out, int32_t *d_n_pairs_out,
    int32_t *d_n_steps, int32_t *d_n_evals, int32_t *d_status, double *d_transform, int64_t *d_grad_in, int32_t *d_best_chain,
    int64_t *d_chain_terms, double *d_chain_transform, int32_t *d_chain_accepts, int32_t *d_chain_evals, void *stream, int32_t list_capacity) {
    const char *who = "td_score_dock";
    const ScoreSide in{d_pos, d_v, d_ligand_ptr, S, N_l, B, class_atomic_number, K, class_aromatic, d_protein_pos, d_protein_elem,
                       d_protein_kind, d_protein_role, N_p, n_kinds, cutoff, hetero_cutoff, rsum, d_bond_ptr, n_bonds, d_bond_ring,
                       d_protein_role_out, d_n_rot};
    const RelaxSide rx{weights, max_steps, max_evals, max_shift, list_capacity, d_pos_out, d_terms_in, d_terms_out, d_n_pairs_out, d_n_steps,
                       d_n_evals, d_status, d_transform, d_grad_in};
    const DockSide dk{n_chains, n_rounds, amplitude, temperature, d_draws, d_best_chain, d_chain_terms, d_chain_transform, d_chain_accepts,
                      d_chain_evals};
    TdDockArgs d;
    if (const int rc = dock_side(who, d, in, rx, dk, static_cast<hipStream_t>(stream))) return rc;
    tdapi::AsyncScratch scratch(static_cast<hipStream_t>(stream));               // given back in stream order, behind the selection
    if (const int rc = scratch.take(&d.chain_aux, (size_t)S * (size_t)B * (size_t)n_chains * 3 * sizeof(int32_t), who)) return rc;
    return td_launch_score_dock(d, static_cast<hipStream_t>(stream));
}

extern "C" int td_score_dock(
    const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
    const int32_t *class_atomic_number, int32_t K, const uint8_t *class_aromatic, const float *d_protein_pos, const int32_t *d_protein_elem,
    const int32_t *d_protein_kind, const int32_t *d_protein_role, int64_t N_p, int32_t n_kinds, double cutoff, double hetero_cutoff,
    const double *rsum, const int64_t *d_bond_ptr, int64_t n_bonds, const uint16_t *d_bond_ring, const double *weights, int32_t max_steps,
    int32_t max_evals, double max_shift, int32_t n_chains, int32_t n_rounds, double amplitude, double temperature, const double *d_draws,
    int32_t *d_protein_role_out, int32_t *d_n_rot, float *d_pos_out, int64_t *d_terms_in, int64_t *d_terms_out, int32_t *d_n_pairs_out,
    int32_t *d_n_steps, int32_t *d_n_evals, int32_t *d_status, double *d_transform, int64_t *d_grad_in, int32_t *d_best_chain,
    int64_t *d_chain_terms, double *d_chain_transform, int32_t *d_chain_accepts, int32_t *d_chain_evals, void *stream) {
    return td_internal_score_dock_capacity(d_pos, d_v, d_ligand_ptr, S, N_l, B, class_atomic_number, K, class_aromatic, d_protein_pos,
                                           d_protein_elem, d_protein_kind, d_protein_role, N_p, n_kinds, cutoff, hetero_cutoff, rsum, d_bond_ptr,
                                           n_bonds, d_bond_ring, weights, max_steps, max_evals, max_shift, n_chains, n_rounds, amplitude,
                                           temperature, d_draws, d_protein_role_out, d_n_rot, d_pos_out, d_terms_in, d_terms_out, d_n_pairs_out,
                                           d_n_steps, d_n_evals, d_status, d_transform, d_grad_in, d_best_chain, d_chain_terms,
                                           d_chain_transform, d_chain_accepts, d_chain_evals, stream, TD_RELAX_LIST_CAPACITY);
}

extern "C" int td_sasa_report(const float *d_pos, const int64_t *d_v, const int32_t *d_ligand_ptr, int64_t S, int64_t N_l, int64_t B,
                              const int32_t *class_atomic_number, int32_t K, const uint8_t *d_include, const float *d_protein_pos,
                              const int32_t *d_protein_elem, int64_t N_p, const double *ligand_reach, const double *protein_reach,
                              const double *d_dirs, int32_t P, int32_t *d_free, int32_t *d_bound, int32_t *d_pocket_buried,
                              int32_t *d_atom_free, int32_t *d_atom_bound, uint64_t *d_bits, int32_t *d_pocket_free,
                              uint64_t *d_pocket_mask, int64_t *d_pocket_buried_sum, void *stream) {
    const char *who = "td_sasa_report";
    TdSasaArgs g;
    if (const int rc = bond_pack(who, g.b, d_pos, d_v, d_ligand_ptr, S, N_l, B, class_atomic_number, K, nullptr)) return rc;
    if (N_p < 0 || N_p > 0x7fffffff / TD_BOND_MAX_ATOMS || S * N_p > 0x7fffffff || S * B > 0x7fffffff / 8) {   // points are counted in an int32
        td_set_error("%s: bad argument (N_p = %lld; 512 N_p, S * N_p and 8 S * B must fit 31 bits)", who, (long long)N_p);
        return TD_EINVAL;
    }
    if (P < 1 || P > TD_SASA_MAX_POINTS || !d_dirs) {
        td_set_error("%s: 1 .. %d directions (got %d)", who, TD_SASA_MAX_POINTS, (int)P);
        return TD_EINVAL;
    }
    if (!ligand_reach || !protein_reach) { td_set_error("%s: null pointer", who); return TD_EINVAL; }
    for (int e = 0; e < 8 + TD_POCKET_ELEMENTS; ++e) {
        const double R = e < 8 ? ligand_reach[e] : protein_reach[e - 8];
        if (!std::isfinite(R) || !(R > 0.0)) {
            td_set_error("%s: every reach must be finite and > 0", who);
            return TD_EINVAL;
        }
        (e < 8 ? g.lig_R[e] : g.prot_R[e - 8]) = R;
    }
    if (N_p > 0 && (!d_protein_pos || !d_protein_elem || !d_pocket_free || !d_pocket_mask || (S > 0 && !d_pocket_buried_sum))) {
        td_set_error("%s: null pointer", who);
        return TD_EINVAL;
    }
    if (S > 0 && B > 0 && (!d_free || !d_bound || !d_pocket_buried)) { td_set_error("%s: null pointer", who); return TD_EINVAL; }
    g.b.include = d_include;
    g.ppos = d_protein_pos; g.pelem = d_protein_elem; g.dirs = d_dirs;
    g.Np = (int)N_p; g.W = (int)((N_p + 63) / 64); g.P = P;
    g.n_free = d_free; g.n_bound = d_bound; g.pocket_buried = d_pocket_buried;
    g.atom_free = d_atom_free; g.atom_bound = d_atom_bound;
    g.bits = reinterpret_cast<unsigned long long *>(d_bits);
    g.pocket_free = d_pocket_free; g.pocket_mask = reinterpret_cast<unsigned long long *>(d_pocket_mask);
    g.buried_sum = reinterpret_cast<unsigned long long *>(d_pocket_buried_sum);
    return td_launch_sasa_report(g, static_cast<hipStream_t>(stream));
}
