"""CPU-only checks of the typed pocket interactions ("Pocket interactions"):

  1. the restatement tests/_interactions_ref.py against cases counted by hand, with every output written out: the ligand roles of small
     planted molecules, the protein table for all 20 residues, a carbon exactly at the hetero cutoff, a pair that donates and accepts
     at once, and strictness at each of the three cutoffs;
  2. the library exports td_interaction_report and the ABI version stays 5;
  3. every ValueError of capi.interaction_report and of quality.sample_interactions, reached without a device;
  4. quality.pocket_roles and the arithmetic of quality.InteractionReport on planted raw outputs, and merged;
  5. tools/evaluate_samples.py --interactions and tools/export_sdf.py --min-hbonds with the bindings patched by the restatements, and
     the tool's output without the flag.
tests/test_gpu_interactions.py compares the kernel with the restatement.
"""
import types

import numpy as np
import pytest
import torch

import _interactions_ref as IR
import _pocket_ref as PR
from targetdiff_amd import capi, quality, workloads
from test_bonds_host import load_tool, parse_sdf
from test_pocket_host import assert_same, pocket_data, save_with_pockets
from test_rings_host import ringed_result
from test_sample_pack_host import numpy_binding  # noqa: F401  (the fixture that patches the other bindings)

CLASS_Z = quality.class_atomic_numbers('add_aromatic')
BASIC_Z = quality.class_atomic_numbers('basic')
H, C, N_, O, F, P, S, CL = 0, 1, 3, 5, 7, 8, 10, 12                             # classes of 'add_aromatic'
D, A, HY = IR.DONOR, IR.ACCEPTOR, IR.HYDROPHOBIC
f32 = np.float32


def roles(atoms, class_z=CLASS_Z):
    """the restatement's roles of one molecule given as [(class, x, y, z)]"""
    pos = np.asarray([a[1:] for a in atoms], f32).reshape(-1, 3)
    return IR.ligand_roles(pos, np.asarray([a[0] for a in atoms], np.int64), class_z).tolist()


def test_ligand_roles_of_planted_molecules():
    # bond lengths of the rule, in A: C-N single < 1.57, double < 1.34, triple < 1.19; C-O single < 1.53, double < 1.25; C-C single < 1.64;
    # N-H < 1.11
    assert (D, A, HY) == (1, 2, 4) == (quality.ROLE_DONOR, quality.ROLE_ACCEPTOR, quality.ROLE_HYDROPHOBIC)
    assert roles([(N_, 0, 0, 0)]) == [D]                                         # an isolated N: val 0, three implied hydrogens
    assert roles([(N_, 0, 0, 0), (C, 1.45, 0, 0)]) == [D, 0]                     # val 1: two implied; the carbon has a bonded N
    assert roles([(N_, 0, 0, 0), (C, 1.25, 0, 0)]) == [D, 0]                     # val 2 (a double bond): one implied
    assert roles([(N_, 0, 0, 0), (C, 1.15, 0, 0)]) == [A, 0]                     # val 3 (a triple bond): no hydrogen, an acceptor
    assert roles([(N_, 0, 0, 0), (C, 1.15, 0, 0), (C, -1.45, 0, 0)]) == [0, 0, 0]            # val 4: neither
    assert roles([(O, 0, 0, 0)]) == [D | A]                                      # val 0: water-like
    assert roles([(O, 0, 0, 0), (C, 1.40, 0, 0)]) == [D | A, 0]                  # val 1: a hydroxyl
    assert roles([(O, 0, 0, 0), (C, 1.20, 0, 0)]) == [A, 0]                      # val 2: a carbonyl
    assert roles([(O, 0, 0, 0), (C, 1.40, 0, 0), (C, -1.40, 0, 0)]) == [A, 0, 0]             # val 2: an ether
    assert roles([(C, 0, 0, 0), (C, 1.5, 0, 0)]) == [HY, HY]                     # a C next to C only
    assert roles([(C, 0, 0, 0), (C, 1.5, 0, 0), (O, 2.9, 0, 0)]) == [HY, 0, D | A]           # and its neighbour next to an O
    assert roles([(C, 0, 0, 0)]) == [HY]
    assert roles([(F, 0, 0, 0), (CL, 5, 0, 0), (P, 10, 0, 0), (S, 15, 0, 0), (H, 20, 0, 0)]) == [HY, HY, 0, 0, 0]
    assert roles([(F, 0, 0, 0), (C, 1.3, 0, 0)]) == [HY, HY]                     # a halogen is no hetero neighbour
    # a class outside [0, K) bonds with nothing and has no role: the N beside it keeps val 0
    assert roles([(N_, 0, 0, 0), (13, 1.45, 0, 0)]) == [D, 0] and roles([(N_, 0, 0, 0), (-1, 1.15, 0, 0)]) == [D, 0]
    # explicit hydrogens, with the 'basic' table (H C N O F P S Cl = classes 0 .. 7): the nitrile N with a hydrogen on it is a donor
    # and no acceptor; an N with one hydrogen and nothing else has that one and two implied
    assert roles([(2, 0, 0, 0), (1, 1.15, 0, 0)], BASIC_Z) == [A, 0]
    assert roles([(2, 0, 0, 0), (1, 1.15, 0, 0), (0, -1.0, 0, 0)], BASIC_Z) == [D, 0, 0]
    assert roles([(2, 0, 0, 0), (0, 1.0, 0, 0)], BASIC_Z) == [D, 0]
    assert roles([(3, 0, 0, 0), (1, 1.20, 0, 0), (0, -0.95, 0, 0)], BASIC_Z) == [D | A, 0, 0]  # O with val 3 and a hydrogen: both
    assert roles([]) == []


# residue -> (side-chain N, side-chain O) by the table; every backbone N donates except PRO's, every backbone O accepts
TABLE = {'ALA': (0, A), 'CYS': (0, A), 'ASP': (0, A), 'GLU': (0, A), 'PHE': (0, A), 'GLY': (0, A), 'HIS': (D | A, A), 'ILE': (0, A),
         'LYS': (D, A), 'LEU': (0, A), 'MET': (0, A), 'ASN': (D, A), 'PRO': (0, A), 'GLN': (D, A), 'ARG': (D, A), 'SER': (0, D | A),
         'THR': (0, D | A), 'VAL': (0, A), 'TRP': (D, A), 'TYR': (0, D | A)}


@pytest.mark.parametrize('table', [IR.pocket_roles, quality.pocket_roles], ids=['restatement', 'quality'])
def test_protein_table_for_all_twenty_residues(table):
    assert tuple(TABLE) == workloads.AA_NAMES == IR.AA
    for k, aa in enumerate(workloads.AA_NAMES):
        # backbone N, backbone O, side-chain N, side-chain O, side-chain C, backbone C, S, Se, H
        element = np.asarray([7, 8, 7, 8, 6, 6, 16, 34, 1])
        bb = np.asarray([1, 1, 0, 0, 0, 1, 0, 0, 0], bool)
        feat = workloads.featurize_protein(element, np.full(9, k), bb)
        sc_n, sc_o = TABLE[aa]
        got = table(feat)
        assert got.dtype == np.int32 and got.tolist() == [0 if aa == 'PRO' else D, A, sc_n, sc_o, 0, 0, 0, 0, -1], aa
        assert table(feat, hydrogens=True).tolist()[-1] == 0
    feat = workloads.featurize_protein(np.asarray([8, 15, 7]), np.asarray([0, 0, 0]), np.asarray([1, 1, 1], bool))
    feat[2, 6:26] = 0                                                           # P is no element of the feature; a row without a residue bit
    assert table(feat).tolist() == [A, -1, -1] and table(torch.from_numpy(feat) if table is quality.pocket_roles else feat).tolist() == [A, -1, -1]
    assert table(np.zeros((0, 27))).shape == (0,)


def test_pocket_roles_refuses_another_feature_width():
    with pytest.raises(ValueError, match=r'protein feature is \[n, 27\]'):
        quality.pocket_roles(np.zeros((3, 26)))
    assert quality.ROLE_NAMES == {1: 'donor', 2: 'acceptor', 4: 'hydrophobic'} and quality.INTERACTION_NAMES == ('donated', 'accepted', 'hydrophobic')


def test_a_carbon_exactly_at_the_hetero_cutoff_and_just_below_it():
    below = np.nextafter(f32(1.75), f32(0))
    # carbons 0, 2, 4, 6 with a nitrogen at exactly 1.75 A, at the fp32 below, an oxygen at the fp32 below that takes no part, none
    ppos = np.asarray([(0, 0, 0), (1.75, 0, 0), (10, 0, 0), (10, below, 0), (20, 0, 0), (20, 0, below), (30, 0, 0)], f32)
    pelem = np.asarray([1, 2, 1, 2, 1, 3, 1], np.int32)
    pkind = np.asarray([0, 0, 0, 0, 0, -1, 0], np.int32)
    prole = np.asarray([0, D, 0, D, 0, A, 0], np.int32)
    assert IR.protein_roles(ppos, pelem, pkind, prole, 1).tolist() == [HY, D, 0, D, HY, -1, HY]
    assert IR.protein_roles(ppos, pelem, pkind, prole, 1, float(np.nextafter(1.75, 9.0))).tolist() == [0, D, 0, D, HY, -1, HY]
    assert IR.protein_roles(ppos, pelem, pkind, prole, 1, float(below)).tolist() == [HY, D, HY, D, HY, -1, HY]
    # the role -1, the element -1 and a kind past n_kinds take an atom out; the table's bits above 2 are ignored; the oxygen beside
    # carbon 4 now takes part
    assert IR.protein_roles(ppos, pelem, np.asarray([0, 0, 0, 1, 0, 0, 0]), np.asarray([0, -1, 0, D, 7, A, 0]), 1).tolist() == [HY, -1, HY, -1, 3, A, HY]
    assert IR.protein_roles(ppos, pelem, np.asarray([0, 0, 0, 1, 0, -1, 0]), np.asarray([0, -1, 0, D, 7, A, 0]), 1).tolist() == [HY, -1, HY, -1, 3 | HY, -1, HY]
    assert IR.protein_roles(ppos, np.asarray([1, 2, -1, 2, 6, 3, 1]), pkind, prole, 1).tolist() == [HY, D, -1, D, -1, -1, HY]
    assert IR.protein_roles(np.zeros((0, 3), f32), [], [], [], 1).shape == (0,)


def hand_case():
    """a hydroxyl on a two-carbon chain beside seven protein atoms"""
    return dict(pos=np.asarray([[(0, 0, 0), (1.4, 0, 0), (2.9, 0, 0)]], f32), v=np.asarray([[O, C, C]], np.int64), ptr=np.asarray([0, 3], np.int32),
                ppos=np.asarray([(0, 0, 3), (0, 3.2, 0), (2.9, 0, 4), (0, 0, 4.4), (2.9, 0, -4), (0, -3.5, 0), (-3, 0, 0)], f32),
                pelem=np.asarray([3, 2, 1, 1, 1, 3, 3], np.int32), pkind=np.asarray([0, 1, 2, 2, -1, 3, 3], np.int32),
                prole=np.asarray([D | A, D, 0, 0, 0, A, A], np.int32))


def ref(c, n_kinds=4, **kw):
    return IR.interaction_report(c['pos'], c['v'], c['ptr'], CLASS_Z, c['ppos'], c['pelem'], c['pkind'], c['prole'], n_kinds, **kw)


def test_restatement_against_a_case_counted_by_hand():
    # ligand: O (hydroxyl: donor and acceptor), C bonded to it (no role), C bonded to that one (hydrophobic)
    # protein: 0 SER OG at 3 A of the O; 1 a backbone N at 3.2 A; 2 a carbon 4 A from the last C; 3 a carbon 1.4 A from atom 0 (not
    # hydrophobic); 4 a carbon of kind -1; 5 an acceptor O at exactly 3.5 A; 6 an acceptor O at 3 A
    ref_bits = np.stack([PR.pack_bits([0, 0, 0, 0, 0, 1, 1]), PR.pack_bits([0, 1, 0, 0, 0, 0, 0]), PR.pack_bits([0, 0, 0, 1, 0, 0, 0])])
    r = ref(hand_case(), ref_bits=ref_bits)
    assert r['protein_role'].tolist() == [D | A, D, HY, 0, -1, A, A] and r['atom_role'].tolist() == [[D | A, 0, HY]]
    assert r['n_donated'].tolist() == [[2]] and r['n_accepted'].tolist() == [[2]] and r['n_hbonds'].tolist() == [[3]]      # O - OG is both
    assert r['n_hydrophobic'].tolist() == [[1]] and r['n_hb_atoms'].tolist() == [[1]]
    assert r['n_donors'].tolist() == [[1]] and r['n_acceptors'].tolist() == [[1]] and r['n_hydrophobic_atoms'].tolist() == [[1]]
    assert r['atom_hbonds'].tolist() == [[3, 0, 0]] and r['atom_hydrophobic'].tolist() == [[0, 0, 1]]
    assert r['bits'].tolist() == [[[[0b1000001], [0b0000011], [0b0000100]]]]
    assert r['n_ref_common'].tolist() == [[[1, 1, 0]]]
    assert r['kind_hist'].tolist() == [[[1, 0, 0, 1], [1, 1, 0, 0], [0, 0, 1, 0]]]
    assert r['pocket_freq'].tolist() == [[[1, 0, 0, 0, 0, 0, 1], [1, 1, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0]]]
    want = dict(protein_role=np.int32, n_hbonds=np.int32, n_ref_common=np.int32, atom_role=np.int32, atom_hbonds=np.int32, bits=np.int64,
                kind_hist=np.int64, pocket_freq=np.int32)
    assert {k: r[k].dtype for k in want} == want and set(r) == set(IR.KEYS)
    # not included: the sums over molecules are empty, the rest is as before; no reference words: no n_ref_common
    r = ref(hand_case(), include=np.zeros((1, 1), bool))
    assert not r['kind_hist'].any() and not r['pocket_freq'].any() and r['n_hbonds'].tolist() == [[3]] and r['n_ref_common'] is None
    # the O of another class table entry that is outside it: no roles, no bonds, the first carbon turns hydrophobic
    c = hand_case()
    c['v'][0, 0] = 13
    r = ref(c)
    assert r['atom_role'].tolist() == [[0, HY, HY]] and r['n_hbonds'].tolist() == [[0]]
    assert r['n_hydrophobic'].tolist() == [[2]] and r['atom_hydrophobic'].tolist() == [[0, 1, 1]]      # protein atom 2 is sqrt(1.5^2 + 4^2) = 4.27 from it
    # wider cutoffs: the acceptor at 3.5 A comes in; the carbon that lost its neighbour (role -1 for atom 0) turns hydrophobic
    c = hand_case()
    c['prole'][0] = -1
    r = ref(c, hbond_cutoff=3.6, hydrophobic_cutoff=5.3)                          # the last C to protein atom 3: sqrt(2.9^2 + 4.4^2) = 5.27
    assert r['protein_role'].tolist() == [-1, D, HY, HY, -1, A, A] and r['n_donated'].tolist() == [[2]] and r['n_accepted'].tolist() == [[1]]
    assert r['n_hbonds'].tolist() == [[3]] and r['bits'][0, 0, :, 0].tolist() == [0b1100000, 0b0000010, 0b0001100]
    assert r['n_hydrophobic'].tolist() == [[2]] and r['atom_hydrophobic'].tolist() == [[0, 0, 2]]
    assert ref(c, hbond_cutoff=3.6, hydrophobic_cutoff=5.2)['n_hydrophobic'].tolist() == [[1]]
    # an oversize molecule answers -1 and adds nothing
    big = IR.build_case(3, 20, [3, 513])
    r = IR.interaction_report(big['pos'], big['v'], big['ptr'], CLASS_Z, big['ppos'], big['pelem'], big['pkind'], big['prole'], 40,
                              ref_bits=np.zeros((3, 1), np.int64))
    assert all((r[k][:, 1] == -1).all() and (r[k][:, 0] >= 0).all() for k in IR.MOL_KEYS + ('n_ref_common',))
    assert not r['bits'][:, 1].any() and not r['atom_role'][:, 3:].any()


def test_a_pair_that_donates_and_accepts_at_once_is_one_hydrogen_bond():
    c = dict(pos=np.asarray([[(0, 0, 0), (1.4, 0, 0)]], f32), v=np.asarray([[O, C]], np.int64), ptr=np.asarray([0, 2], np.int32),
             ppos=np.asarray([(0, 0, 3)], f32), pelem=np.asarray([3], np.int32), pkind=np.asarray([0], np.int32), prole=np.asarray([D | A], np.int32))
    r = ref(c, n_kinds=1)
    assert (r['n_donated'][0, 0], r['n_accepted'][0, 0], r['n_hbonds'][0, 0], r['n_hb_atoms'][0, 0]) == (1, 1, 1, 1)
    assert r['atom_hbonds'].tolist() == [[1, 0]] and r['bits'][0, 0].tolist() == [[1], [1], [0]] and r['kind_hist'].tolist() == [[[1], [1], [0]]]


@pytest.mark.parametrize('which, at, cls, pelem, prole', [('hbond_cutoff', 3.5, O, 3, A), ('hbond_cutoff', 3.5, O, 2, D), ('hydrophobic_cutoff', 4.5, F, 1, 0)])
def test_restatement_is_strict_at_the_pair_cutoffs(which, at, cls, pelem, prole):
    t = 0 if prole == A else 1 if prole == D else 2
    lo, hi = np.nextafter(f32(at), f32(0)), np.nextafter(f32(at), f32(9))
    c = dict(pos=np.zeros((1, 1, 3), f32), v=np.asarray([[cls]], np.int64), ptr=np.asarray([0, 1], np.int32),
             ppos=np.asarray([(at, 0, 0), (0, lo, 0), (0, 0, hi)], f32), pelem=np.full(3, pelem, np.int32), pkind=np.asarray([0, 1, 2], np.int32),
             prole=np.full(3, prole, np.int32))
    word = lambda **kw: int(ref(c, **kw)['bits'][0, 0, t, 0])
    assert word() == 0b010                                                       # d == cutoff is no interaction, the fp32 below it is one
    assert word(**{which: float(np.nextafter(at, 9.0))}) == 0b011                # the float64 above the cutoff lets d == cutoff in
    assert word(**{which: float(np.nextafter(at, 0.0))}) == 0b010
    assert word(**{which: float(lo)}) == 0 and word(**{which: float(np.nextafter(np.float64(hi), 9.0))}) == 0b111
    assert [int(x) for x in ref(c)['bits'][0, 0, :, 0]] == [0b010 if k == t else 0 for k in range(3)]


def test_library_exports_the_entry_point_and_the_abi_version_stays():
    lib = capi.load_library()
    assert hasattr(lib, 'td_interaction_report') and 'td_interaction_report' in capi.SIGNATURES
    assert len(capi.SIGNATURES['td_interaction_report'][1]) == 36
    assert lib.td_abi_version() == capi.ABI_VERSION == 5
    assert (capi.ROLE_DONOR, capi.ROLE_ACCEPTOR, capi.ROLE_HYDROPHOBIC, capi.INTERACTION_TYPES) == (1, 2, 4, 3)


def cpu_args(c, n_kinds=40, **kw):
    t = torch.as_tensor
    return [t(c['pos']), t(c['v']), t(c['ptr']), CLASS_Z, t(c['ppos']), t(c['pelem']), t(c['pkind']), t(c['prole']), n_kinds], kw


def test_binding_refuses_bad_arguments_before_anything_is_launched():
    c = IR.build_case(0, 70, [4, 9], S=2, dead=False)

    def refused(match, edit=None, check=True, **kw):
        a, kw = cpu_args(c, **kw)
        if edit:
            edit(a)
        with pytest.raises(ValueError, match=match):
            capi.interaction_report(*a, check=check, **kw)

    def put(i, x):
        return lambda a: a.__setitem__(i, x)

    refused(r'pos / v must be', put(0, torch.zeros(2, 13, 2)))
    refused(r'prefix offsets', put(2, torch.tensor([0, 9, 4], dtype=torch.int32)))
    refused(r'v must be in', put(1, torch.full((2, 13), 13)))
    refused(r'at most 512', lambda a: (a.__setitem__(0, torch.zeros(1, 513, 3)), a.__setitem__(1, torch.zeros(1, 513, dtype=torch.int64)),
                                      a.__setitem__(2, torch.tensor([0, 513], dtype=torch.int32))))
    refused(r'include must be', include=torch.ones(2, 3, dtype=torch.bool))
    refused(r'protein_pos must be \[N_p, 3\]', put(4, torch.zeros(70, 4)))
    refused(r'protein_elem / protein_kind must be \[70\]', put(5, torch.zeros(69, dtype=torch.int32)))
    refused(r'protein_elem / protein_kind must be \[70\]', put(6, torch.zeros(70, 1, dtype=torch.int32)))
    refused(r'fp32 / int32 / int32', put(4, torch.zeros(70, 3, dtype=torch.float64)))
    refused(r'fp32 / int32 / int32', put(5, torch.zeros(70, dtype=torch.int64)))
    refused(r'device of the pack', put(4, torch.zeros(70, 3, device='meta')))
    refused(r'protein_role must be \[70\] int32', put(7, torch.zeros(69, dtype=torch.int32)))
    refused(r'protein_role must be \[70\] int32', put(7, torch.zeros(70, dtype=torch.int64)))
    refused(r'device of the pack', put(7, torch.zeros(70, dtype=torch.int32, device='meta')))
    refused(r'device of the pack', ref_bits=torch.zeros(3, 2, dtype=torch.int64, device='meta'))
    for n_kinds in (0, 65):
        refused(r'n_kinds is 1 \.\. 64', n_kinds=n_kinds)
    for name in ('hbond', 'hydrophobic', 'hetero'):
        for cutoff in (0.0, -1.0, float('inf'), float('nan')):
            refused(rf'the {name} cutoff must be finite and > 0', **{name + '_cutoff': cutoff})
    refused(r'ref_bits must be \[3, 2\] int64', ref_bits=torch.zeros(2, dtype=torch.int64))
    refused(r'ref_bits must be \[3, 2\] int64', ref_bits=torch.zeros(3, 3, dtype=torch.int64))
    refused(r'ref_bits must be \[3, 2\] int64', ref_bits=torch.zeros(3, 2, dtype=torch.int32))
    refused(r'protein_elem must be in \[-1, 6\)', put(5, torch.full((70,), 6, dtype=torch.int32)))
    refused(r'protein_kind must be in \[-1, 40\)', put(6, torch.full((70,), 40, dtype=torch.int32)))
    refused(r'protein_kind must be in \[-1, 6\)', n_kinds=6)
    refused(r'protein_role must be -1 or a sum of DONOR = 1 and ACCEPTOR = 2', put(7, torch.full((70,), 4, dtype=torch.int32)))
    refused(r'protein_role must be -1 or a sum of DONOR = 1 and ACCEPTOR = 2', put(7, torch.full((70,), -2, dtype=torch.int32)))
    # check=False skips the looks at the values, not the ones at shapes and types; what passes them needs a device
    refused(r'n_kinds is 1 \.\. 64', n_kinds=65, check=False)
    refused(r'the hetero cutoff must be finite', hetero_cutoff=0.0, check=False)
    a, _ = cpu_args(c, n_kinds=6)
    with pytest.raises(RuntimeError, match='must live on a HIP device'):
        capi.interaction_report(*a, check=False)


@pytest.fixture
def interaction_binding(numpy_binding, monkeypatch):  # noqa: F811
    """numpy_binding, and capi.interaction_report and capi.pocket_report patched by their restatements too"""
    def patched(name, fn):
        def binding(*a, **kw):
            numpy_binding.append((name, kw.get('check')))
            return fn(*a, **kw)
        return binding

    monkeypatch.setattr(capi, 'interaction_report', patched('interaction_report', IR.torch_interaction_report))
    monkeypatch.setattr(capi, 'pocket_report', patched('pocket_report', PR.torch_pocket_report))
    return numpy_binding


def test_sample_interactions_refuses_a_result_without_a_pocket(interaction_binding):
    res = ringed_result(1, [5, 7], 2)
    with pytest.raises(ValueError, match='carries no pocket'):
        quality.sample_interactions(res, device='cpu')
    with pytest.raises(ValueError, match='carries no pocket'):
        quality.sample_interactions({'data': None, 'pred_ligand_pos_traj': res[2], 'pred_ligand_v_traj': res[3]}, device='cpu')
    pack = quality.SamplePack(res, device='cpu')
    with pytest.raises(ValueError, match=r'protein positions must be \[60, 3\]'):
        pack.interactions((torch.zeros(59, 3), pocket_data().protein_atom_feature))
    with pytest.raises(ValueError, match=r'protein feature is \[n, 27\]'):
        pack.interactions((torch.zeros(3, 3), torch.zeros(3, 26)))
    with pytest.raises(ValueError, match='include is'):
        pack.interactions(pocket_data(), include='stable')
    with pytest.raises(ValueError, match='one molecule'):
        pack.interactions(pocket_data(), reference_ligand=(np.zeros((2, 4, 3), f32), np.zeros(4, np.int64)))
    with pytest.raises(ValueError, match='hbond cutoff'):
        pack.interactions(pocket_data(), hbond_cutoff=0.0)
    assert not [c for c in interaction_binding if c[0] == 'interaction_report' and c[1] is None]      # only calls that were refused


def planted_raw():
    """two frames of four molecules of sizes 4, 0, 2, 5 (11 atoms) in a pocket of 70 atoms; the second frame has no interaction"""
    hist = np.zeros((2, 3, 4), np.int64)
    hist[0, 0, 0], hist[0, 0, 1], hist[0, 1, 3], hist[0, 2, 2], hist[0, 2, 0] = 2, 1, 2, 5, 1
    role = np.asarray([[D, A, HY, 0, D | A, 0, HY, HY, D | A, A, 0], [D, 0, HY, 0, 0, 0, HY, HY, D | A, HY, 0]])
    bits = np.zeros((2, 4, 3, 2), np.int64)
    bits[0, 0, 0], bits[0, 0, 1], bits[0, 0, 2] = [0b11, 0], [0b100, 0], [0b1111, 1]
    bits[0, 3, 0], bits[0, 3, 2] = [0b10, 0], [0b11000, 0]
    return dict(n_donated=np.asarray([[2, 0, 0, 1], [0] * 4]), n_accepted=np.asarray([[2, 0, 0, 0], [0] * 4]), n_hbonds=np.asarray([[3, 0, 0, 1], [0] * 4]),
                n_hydrophobic=np.asarray([[4, 0, 0, 2], [0] * 4]), n_hb_atoms=np.asarray([[2, 0, 0, 1], [0] * 4]), atom_role=role,
                n_ref_common=np.asarray([[[2, 1, 3], [0, 0, 0], [0, 0, 0], [1, 0, 0]], np.zeros((4, 3), int)]), bits=bits, kind_hist=hist,
                pocket_freq=np.zeros((2, 3, 70), np.int32))


def test_interaction_report_arithmetic():
    names, sizes = ('A.sc', 'A.bb', 'B.sc', 'B.bb'), [4, 0, 2, 5]
    rep = quality.InteractionReport.from_outputs(planted_raw(), np.ones((2, 4), bool), sizes, names, ref_sizes=[4, 0, 6])
    assert rep.num_frames == 2 and rep.n_samples == 4 and rep.n_included.tolist() == [4, 4]
    assert rep.mean_hbonds(0) == 4 / 4 and rep.mean_donated(0) == 3 / 4 and rep.mean_accepted(0) == 2 / 4 and rep.mean_hydrophobic(0) == 6 / 4
    assert rep.no_hbond(0) == 2 / 4 and rep.no_hbond(1) == 1.0                   # an empty molecule has no hydrogen bond
    assert rep.sum_polar_atoms.tolist() == [5, 2] and rep.polar_in_hbond(0) == 3 / 5 and rep.polar_in_hbond(1) == 0.0
    assert rep.kind_profile('donated', 0) == {'A.sc': 2 / 3, 'A.bb': 1 / 3, 'B.sc': 0.0, 'B.bb': 0.0} and rep.kind_profile(2, 0)['B.sc'] == 5 / 6
    assert rep.kind_profile('accepted', 1) is None and rep.interaction_frequency(0).shape == (3, 70)
    rec0, rec2 = np.asarray([2, 0, 0, 1]) / 4, np.asarray([3, 0, 0, 0]) / 6
    tan0 = np.asarray([2 / (2 + 4 - 2), 0.0, 0.0, 1 / (1 + 4 - 1)])
    tan2 = np.asarray([3 / (5 + 6 - 3), 0.0, 0.0, 0 / (2 + 6 - 0)])
    got = rep.reference_recovery(0)
    assert got['ref_donated_recovery_mean'] == rec0.sum() / 4 and got['ref_donated_recovery_median'] == float(np.median(rec0))
    assert got['ref_donated_recovery_max'] == 0.5 and got['ref_donated_tanimoto'] == tan0.sum() / 4
    assert got['ref_hydrophobic_recovery_mean'] == rec2.sum() / 4 and got['ref_hydrophobic_recovery_max'] == 0.5 and got['ref_hydrophobic_tanimoto'] == tan2.sum() / 4
    assert all(np.isnan(got[f'ref_accepted_{k}']) for k in ('recovery_mean', 'recovery_median', 'recovery_max', 'tanimoto'))      # nothing to recover
    assert rep.n_ref.tolist() == [[1, 0, 1], [1, 0, 1]]
    s = rep.summary(-1)
    assert list(s)[:6] == ['mean_hbonds', 'mean_donated', 'mean_accepted', 'mean_hydrophobic', 'no_hbond', 'polar_in_hbond'] and len(s) == 18
    assert s['mean_hbonds'] == 0.0 and s['no_hbond'] == 1.0 and s['ref_donated_recovery_max'] == 0.0
    lines = rep.lines(0)
    assert lines[0] == 'mean_hbonds:\t1.0000' and 'ref_accepted_tanimoto:\tNone' in lines
    assert lines[-5:] == ['donated A.sc:\t0.6667', 'donated A.bb:\t0.3333', 'accepted B.bb:\t1.0000', 'hydrophobic B.sc:\t0.8333', 'hydrophobic A.sc:\t0.1667']
    assert not any(x.startswith(('donated', 'accepted', 'hydrophobic')) for x in rep.lines(1))
    # an include mask: only the first and the third molecule of frame 0, nothing of frame 1
    inc = np.asarray([[True, False, True, False], [False] * 4])
    part = quality.InteractionReport.from_outputs(planted_raw(), inc, sizes, names, ref_sizes=[4, 0, 6])
    assert part.n_included.tolist() == [2, 0] and part.mean_hbonds(0) == 3 / 2 and part.no_hbond(0) == 1 / 2 and part.polar_in_hbond(0) == 2 / 3
    assert part.reference_recovery(0)['ref_donated_recovery_mean'] == (2 / 4 + 0) / 2
    assert all(np.isnan(x) for x in part.summary(1).values()) and np.isnan(part.interaction_frequency(1)).all() and part.n_ref[1].tolist() == [0, 0, 0]
    # no reference gives no keys
    raw = {k: x for k, x in planted_raw().items() if k not in ('n_ref_common', 'bits')}
    plain = quality.InteractionReport.from_outputs(raw, np.ones((2, 4), bool), sizes, names)
    assert plain.reference_recovery(0) == {} and list(plain.summary(0)) == list(s)[:6] and plain.sum_ref is None


def test_interaction_report_merged():
    names, sizes = ('A.sc', 'A.bb', 'B.sc', 'B.bb'), [4, 0, 2, 5]
    a = quality.InteractionReport.from_outputs(planted_raw(), np.ones((2, 4), bool), sizes, names, ref_sizes=[4, 0, 6])
    raw = planted_raw()
    raw['pocket_freq'] = np.zeros((2, 3, 9), np.int64)                          # another pocket, of nine atoms
    b = quality.InteractionReport.from_outputs(raw, np.asarray([[True, False, True, False], [False] * 4]), sizes, names, ref_sizes=[0, 0, 6])
    m = quality.InteractionReport.merged([a, b])
    assert m.n_samples == 8 and m.n_included.tolist() == [6, 4] and m.mean_hbonds(0) == (4 + 3) / 6 and m.mean_hydrophobic(0) == (6 + 4) / 6
    assert m.polar_in_hbond(0) == (3 + 2) / (5 + 3) and np.array_equal(m.kind_hist, a.kind_hist + b.kind_hist) and m.interaction_frequency(0) is None
    assert m.n_ref[0].tolist() == [1, 0, 2]
    assert m.reference_recovery(0)['ref_donated_recovery_mean'] == a.reference_recovery(0)['ref_donated_recovery_mean']    # b's had none
    assert m.reference_recovery(0)['ref_hydrophobic_recovery_mean'] == (3 / 6 / 4 + 3 / 6 / 2) / 2
    one = quality.InteractionReport.merged([a])
    assert np.array_equal(one.interaction_frequency(0), a.interaction_frequency(0))
    np.testing.assert_equal(one.summary(0), a.summary(0))
    plain = quality.InteractionReport.from_outputs({k: x for k, x in planted_raw().items() if k not in ('n_ref_common', 'bits')},
                                                   np.ones((2, 4), bool), sizes, names)
    with pytest.raises(ValueError, match='do not merge'):
        quality.InteractionReport.merged([a, plain])
    with pytest.raises(ValueError, match='do not merge'):
        quality.InteractionReport.merged([a, quality.InteractionReport.from_outputs(planted_raw(), np.ones((2, 4), bool), sizes, names[::-1], [4, 0, 6])])


def typed_result(seed, sizes, T):
    """test_rings_host.ringed_result with oxygens, fluorines and chlorines among its carbons and nitrogens: every role occurs"""
    res = ringed_result(seed, sizes, T)
    rng = np.random.default_rng(seed + 100)
    for v in res[3]:
        v[...] = np.where(rng.random(v.shape) < 0.4, rng.choice([O, F, CL], v.shape), v)
    for k in range(len(res[1])):
        res[1][k] = res[3][k][-1]
    return res


def typed_pocket(seed, n_p=60):
    """test_pocket_host.pocket_data, looser (a scale of 0.7, not 0.4): some of its carbons have no N or O within 1.75 A"""
    c = PR.build_case(seed, n_p, [30], dead=False)
    rng = np.random.default_rng(seed)
    feat = workloads.featurize_protein(np.asarray(workloads.PROTEIN_ELEMENTS)[np.maximum(c['pelem'], 1)], rng.integers(0, 20, n_p), rng.random(n_p) < 0.5)
    return types.SimpleNamespace(protein_pos=torch.from_numpy(c['ppos'] * f32(0.7)), protein_atom_feature=torch.from_numpy(feat))


def expected_report(res, data, eval_step, reference_ligand=None, include=None, **cutoffs):
    """InteractionReport of a result through the restatement alone"""
    frames = slice(None) if eval_step == 'all' else slice(len(res[2][0]) - 1, None)
    sizes = [p.shape[1] for p in res[2]]
    pos = np.concatenate([p[frames] for p in res[2]], 1).astype(f32)
    v = np.concatenate([x[frames] for x in res[3]], 1)
    elem, kind, names = quality.pocket_kinds(data.protein_atom_feature)
    pocket = (data.protein_pos.numpy(), elem, kind, IR.pocket_roles(data.protein_atom_feature.numpy()), 40)
    bits = ref_sizes = None
    if reference_ligand is not None:
        q = IR.interaction_report(reference_ligand[0][None], reference_ligand[1][None], [0, len(reference_ligand[1])], CLASS_Z, *pocket, **cutoffs)
        bits = q['bits'][0, 0]
        ref_sizes = PR.unpack_bits(bits, len(elem)).sum(-1)
    w = IR.interaction_report(pos, v, np.cumsum([0] + sizes), CLASS_Z, *pocket, include=include, ref_bits=bits, **cutoffs)
    inc = np.ones(w['n_hbonds'].shape, bool) if include is None else include
    return quality.InteractionReport.from_outputs({k: x for k, x in w.items() if x is not None}, inc, sizes, names, ref_sizes), w


def test_sample_interactions_and_the_tool(interaction_binding, tmp_path, capsys):
    results = {10: typed_result(5, [6, 9, 14], 3), 2: typed_result(6, [4, 11, 5, 1], 3)}
    pockets = {10: typed_pocket(1), 2: typed_pocket(2, 45)}
    ligand = (np.asarray(results[10][2][0][-1], f32), np.asarray(results[10][3][0][-1], np.int64))
    for i, res in results.items():
        as_dict = {'data': pockets[i], 'pred_ligand_pos_traj': res[2], 'pred_ligand_v_traj': res[3]}
        for eval_step in (-1, 'all'):
            want, _ = expected_report(res, pockets[i], eval_step, ligand)
            assert want.sum_hbonds[-1] > 0 and want.sum_hydrophobic[-1] > 0 and want.sum_donated[-1] > 0 and want.sum_accepted[-1] > 0
            assert_same(quality.sample_interactions(as_dict, eval_step, reference_ligand=ligand, device='cpu'), want)
            assert_same(quality.SamplePack(res, eval_step, device='cpu').interactions(pockets[i]), expected_report(res, pockets[i], eval_step)[0])
    mask = np.asarray([[True, False, True]] * 3)
    assert_same(quality.SamplePack(results[10], 'all', device='cpu').interactions(pockets[10], mask),
                expected_report(results[10], pockets[10], 'all', None, mask)[0])
    # the stateless function returns the raw outputs
    x = quality.pocket_interactions(pockets[10].protein_pos, pockets[10].protein_atom_feature, ligand[0], ligand[1],
                                    ligand_ptr=torch.tensor([0, 6], dtype=torch.int32), return_bits=True, device='cpu')
    w = expected_report(([ligand[0]], [ligand[1]], [ligand[0][None].astype(np.float64)], [ligand[1][None]]), pockets[10], -1)[1]
    for k in IR.KEYS:
        assert (w[k] is None and getattr(x, k) is None) or np.array_equal(getattr(x, k).numpy(), w[k]), k
    # the tool: one pack per file, the reference ligand's call first, the host's look with the pack's first call only
    save_with_pockets(tmp_path, results, pockets)
    np.savez(tmp_path / 'ref.npz', ligand_pos=ligand[0], ligand_v=ligand[1])
    tool = load_tool('evaluate_samples')
    del interaction_binding[:]
    capsys.readouterr()
    out = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--interactions', '--eval_step', 'all', '--include', 'complete',
                     '--reference_npz', str(tmp_path / 'ref.npz')])
    assert [c[0] for c in interaction_binding].count('interaction_report') == 4 and [c[0] for c in interaction_binding].count('pack') == 2
    assert [c for c in interaction_binding if c[0] == 'interaction_report'][1::2] == [('interaction_report', False)] * 2      # the graph looked first
    reports = []
    for i in (2, 10):
        res = results[i]
        complete = quality.SamplePack(res, 'all', device='cpu').mask('complete').numpy()
        reports.append(expected_report(res, pockets[i], 'all', ligand, complete)[0])
    want = quality.InteractionReport.merged(reports)
    printed = capsys.readouterr().out.split('\n')
    assert printed[7:7 + len(want.lines(-1))] == want.lines(-1) and printed[7].startswith('mean_hbonds:\t')
    nan_none = lambda x: None if x != x else x
    assert out['interactions']['mean_hbonds'] == nan_none(want.mean_hbonds(-1)) and out['interactions']['num_included'] == int(want.n_included[-1])
    assert out['interactions']['ref_hydrophobic_recovery_mean'] == nan_none(want.reference_recovery(-1)['ref_hydrophobic_recovery_mean'])
    assert len(out['interactions']['curve']) == 3 and out['interactions']['hbond_cutoff'] == 3.5 and out['interactions']['hydrophobic_cutoff'] == 4.5
    assert {t: sum(h.values()) for t, h in out['interactions']['kind_hist'].items()} == \
        dict(donated=want.sum_donated[-1], accepted=want.sum_accepted[-1], hydrophobic=want.sum_hydrophobic[-1])
    # other limits reach the report
    base = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--interactions'])
    out2 = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--interactions', '--hbond_cutoff', '5', '--hydrophobic_cutoff', '6'])
    assert out2['interactions']['mean_hbonds'] > base['interactions']['mean_hbonds'] > 0
    assert out2['interactions']['mean_hydrophobic'] > base['interactions']['mean_hydrophobic'] > 0
    assert 'ref_donated_recovery_mean' not in out2['interactions'] and 'curve' not in out2['interactions'] and 'pocket' not in out2


def test_the_tool_without_the_flag_prints_what_it_printed(interaction_binding, tmp_path, capsys):
    results = {10: typed_result(5, [6, 9, 14], 3), 2: typed_result(6, [4, 11, 5, 1], 3)}
    save_with_pockets(tmp_path, results, {10: typed_pocket(1), 2: None})          # a file without a pocket is fine without the flag
    tool = load_tool('evaluate_samples')
    del interaction_binding[:]
    capsys.readouterr()
    out = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu'])
    lines = capsys.readouterr().out.rstrip('\n').split('\n')
    assert [x.split(':')[0].split('!')[0] for x in lines] == ['Load generated data done', 'Evaluate done', 'mol_stable', 'atm_stable', 'JSD_CC_2A',
                                                              'JSD_All_12A', 'Atom type JS', 'wrote ' + str(tmp_path / 'eval_results' / 'quality.json')]
    assert 'interactions' not in out and interaction_binding == [('pack', None), ('quality_report', True)] * 2
    with pytest.raises(SystemExit, match='carries no pocket'):
        tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--interactions'])


def test_export_sdf_writes_only_the_molecules_with_enough_hydrogen_bonds(interaction_binding, tmp_path):
    res = typed_result(5, [6, 9, 14, 3], 3)
    res[2][3] = (res[2][3].astype(f32) + f32(40)).astype(np.float64)            # the last sample has left the pocket: no hydrogen bond
    res[0][3] = res[2][3][-1]
    data = typed_pocket(1)
    save_with_pockets(tmp_path, {4: res}, {4: data})
    hbonds = expected_report(res, data, -1)[1]['n_hbonds'][0]
    assert hbonds[3] == 0 and hbonds.max() >= 2
    tool = load_tool('export_sdf')
    for least in (1, 2, int(hbonds.max()) + 1):
        out = tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / f'sdf{least}'), '--device', 'cpu', '--min-hbonds', str(least)])
        keep = hbonds >= least
        assert out['result_4']['min_hbonds'] == keep.sum() == out['result_4']['written']
        recs = parse_sdf(open(tmp_path / f'sdf{least}' / 'result_4.sdf').read())
        assert [len(atoms) for _, atoms, _, _ in recs] == [n for n, ok in zip([6, 9, 14, 3], keep) if ok]
    both = tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'both'), '--device', 'cpu', '--min-hbonds', '1', '--pocket-clash-free'])
    assert both['result_4']['written'] <= min(both['result_4']['min_hbonds'], both['result_4']['pocket_clash_free'])
    plain = tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'plain'), '--device', 'cpu'])
    assert plain['result_4']['written'] == 4 and 'min_hbonds' not in plain['result_4']
