"""CPU-only checks of the pocket contact report ("Pocket contacts"):

  1. the restatement tests/_pocket_ref.py against cases counted by hand, with every output written out;
  2. the library exports td_pocket_report and the ABI version stays 5;
  3. every ValueError of capi.pocket_report and of quality.sample_pocket, reached without a device;
  4. quality.pocket_kinds, quality.pocket_clash_thresholds and the arithmetic of quality.PocketReport on planted raw outputs;
  5. tools/evaluate_samples.py --pocket and tools/export_sdf.py --pocket-clash-free with the bindings patched by the restatements, and
     the tool's output without the flag.
tests/test_gpu_pocket.py compares the kernel with the restatement.
"""
import types

import numpy as np
import pytest
import torch

import _pocket_ref as PR
from targetdiff_amd import capi, quality, workloads
from test_bonds_host import load_tool, parse_sdf
from test_rings_host import ringed_result
from test_sample_pack_host import numpy_binding  # noqa: F401  (the fixture that patches the other bindings)

CLASS_Z = quality.class_atomic_numbers('add_aromatic')
C, N_, O = 1, 3, 5                                                             # classes of 'add_aromatic'


def hand_case():
    """three ligand atoms beside four protein atoms on a lattice"""
    return dict(pos=np.asarray([[(0, 0, 2), (3, 0, 2), (0, 0, 10)]], np.float32), v=np.asarray([[C, N_, O]], np.int64),
                ptr=np.asarray([0, 3], np.int32), ppos=np.asarray([(0, 0, 0), (3, 0, 0), (0, 5, 0), (10, 0, 0)], np.float32),
                pelem=np.asarray([1, 2, 3, 4], np.int32), pkind=np.asarray([0, 1, 2, 1], np.int32))


def ref(c, cutoff=4.0, table=None, include=None, ref_bits=None, n_kinds=3):
    return PR.pocket_report(c['pos'], c['v'], c['ptr'], CLASS_Z, c['ppos'], c['pelem'], c['pkind'], n_kinds, cutoff, table, include, ref_bits)


def test_restatement_against_a_case_counted_by_hand():
    # distances: L0-P0 2, L0-P1 sqrt 13, L1-P0 sqrt 13, L1-P1 2; every other pair is farther than 5
    # thresholds at tolerance 0.5: C-C 2.9, C-N 2.75, N-N 2.6: the two pairs at 2 A clash
    r = ref(hand_case(), table=PR.clash_table(), ref_bits=PR.pack_bits([False, True, True, False]))
    assert r['n_contacts'].tolist() == [[4]] and r['n_contact_atoms'].tolist() == [[2]] and r['n_pocket_atoms'].tolist() == [[2]]
    assert r['n_clashes'].tolist() == [[2]] and r['n_clash_atoms'].tolist() == [[2]] and r['min_dist'].tolist() == [[2.0]]
    assert r['n_ref_common'].tolist() == [[1]]
    assert r['atom_contacts'].tolist() == [[2, 2, 0]] and r['atom_clash'].tolist() == [[1, 1, 0]]
    assert r['bits'].tolist() == [[[0b0011]]] and r['pocket_freq'].tolist() == [[1, 1, 0, 0]]
    hist = np.zeros((1, 8, 3), np.int64)
    hist[0, 1, 0] = hist[0, 1, 1] = hist[0, 2, 0] = hist[0, 2, 1] = 1          # carbon and nitrogen, each with kinds 0 and 1
    assert np.array_equal(r['kind_hist'], hist)
    assert {k: r[k].dtype for k in ('n_contacts', 'min_dist', 'bits', 'kind_hist', 'pocket_freq', 'atom_contacts')} == \
        dict(n_contacts=np.int32, min_dist=np.float64, bits=np.int64, kind_hist=np.int64, pocket_freq=np.int32, atom_contacts=np.int32)
    # a longer cutoff reaches P2 from L0 (sqrt 29 = 5.39) and not from L1 (sqrt 38 = 6.16)
    r = ref(hand_case(), cutoff=5.5)
    assert r['n_contacts'].tolist() == [[5]] and r['bits'].tolist() == [[[0b0111]]] and r['kind_hist'][0, 1, 2] == 1
    assert r['n_clashes'] is None and r['atom_clash'] is None and r['n_ref_common'] is None
    # not included: the sums over molecules are empty, the rest is as before
    r = ref(hand_case(), include=np.zeros((1, 1), bool))
    assert not r['kind_hist'].any() and not r['pocket_freq'].any() and r['n_contacts'].tolist() == [[4]]
    # a protein atom of kind -1 or element -1, a ligand atom of no class
    c = hand_case()
    c['pkind'][0], c['pelem'][1], c['v'][0, 0] = -1, -1, 13
    r = ref(c, cutoff=8.0)
    assert r['n_contacts'].tolist() == [[2]] and r['atom_contacts'].tolist() == [[0, 2, 0]] and r['bits'].tolist() == [[[0b1100]]]
    assert r['min_dist'][0, 0] == np.sqrt(9.0 + 25.0 + 4.0)


def test_restatement_is_strict_at_the_cutoff():
    c = dict(pos=np.zeros((1, 1, 3), np.float32), v=np.asarray([[C]], np.int64), ptr=np.asarray([0, 1], np.int32),
             ppos=np.asarray([(4, 0, 0), (0, np.nextafter(np.float32(4), np.float32(0)), 0), (0, 0, np.nextafter(np.float32(4), np.float32(9)))], np.float32),
             pelem=np.ones(3, np.int32), pkind=np.asarray([0, 1, 2], np.int32))
    assert ref(c)['bits'].tolist() == [[[0b010]]]                               # d == cutoff is no contact, the fp32 below it is one
    assert ref(c, cutoff=float(np.nextafter(4.0, 9.0)))['bits'].tolist() == [[[0b011]]]      # the float64 above the cutoff lets d == 4 in
    assert ref(c, cutoff=float(np.nextafter(4.0, 0.0)))['bits'].tolist() == [[[0b010]]]
    table = np.full((8, 6), 4.0)
    assert ref(c, cutoff=1.0, table=table)['n_clashes'].tolist() == [[1]]
    table[1, 1] = np.nextafter(4.0, 9.0)
    assert ref(c, cutoff=1.0, table=table)['n_clashes'].tolist() == [[2]]
    assert PR.unpack_bits(PR.pack_bits(np.arange(130) % 7 == 0), 130).tolist() == (np.arange(130) % 7 == 0).tolist()
    assert PR.pack_bits(np.arange(130) == 64).tolist() == [0, 1, 0] and PR.pack_bits(np.arange(64) == 63).view(np.uint64)[0] == 1 << 63


def test_library_exports_the_entry_point_and_the_abi_version_stays():
    lib = capi.load_library()
    assert hasattr(lib, 'td_pocket_report') and 'td_pocket_report' in capi.SIGNATURES
    assert len(capi.SIGNATURES['td_pocket_report'][1]) == 30
    assert lib.td_abi_version() == capi.ABI_VERSION == 5


def cpu_args(c, n_kinds=40, cutoff=4.0, table=None, include=None, ref_bits=None):
    t = torch.as_tensor
    return [t(c['pos']), t(c['v']), t(c['ptr']), CLASS_Z, t(c['ppos']), t(c['pelem']), t(c['pkind']), n_kinds, cutoff, table, include, ref_bits]


def test_binding_refuses_bad_arguments_before_anything_is_launched():
    c = PR.build_case(0, 70, [4, 9], S=2, dead=False)

    def refused(match, edit=None, check=True, **kw):
        a = cpu_args(c, **kw)
        if edit:
            edit(a)
        with pytest.raises(ValueError, match=match):
            capi.pocket_report(*a, check=check)

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
    refused(r'fp32 / int32 / int32', put(6, torch.zeros(70, dtype=torch.int64)))
    refused(r'device of the pack', put(4, torch.zeros(70, 3, device='meta')))
    refused(r'device of the pack', ref_bits=torch.zeros(2, dtype=torch.int64, device='meta'))
    for n_kinds in (0, 65):
        refused(r'n_kinds is 1 \.\. 64', n_kinds=n_kinds)
    for cutoff in (0.0, -1.0, float('inf'), float('nan')):
        refused(r'cutoff must be finite and > 0', cutoff=cutoff)
    refused(r'finite \[8, 6\] table', table=np.zeros((8, 8)))
    refused(r'finite \[8, 6\] table', table=np.zeros((6, 8)))
    refused(r'finite \[8, 6\] table', table=np.full((8, 6), np.inf))
    refused(r'ref_bits must be \[2\] int64', ref_bits=torch.zeros(3, dtype=torch.int64))
    refused(r'ref_bits must be \[2\] int64', ref_bits=torch.zeros(2, dtype=torch.int32))
    refused(r'protein_elem must be in \[-1, 6\)', put(5, torch.full((70,), 6, dtype=torch.int32)))
    refused(r'protein_elem must be in \[-1, 6\)', put(5, torch.full((70,), -2, dtype=torch.int32)))
    refused(r'protein_kind must be in \[-1, 40\)', put(6, torch.full((70,), 40, dtype=torch.int32)))
    refused(r'protein_kind must be in \[-1, 6\)', n_kinds=6)
    # check=False skips the looks at the values, not the ones at shapes and types; what passes them needs a device
    refused(r'n_kinds is 1 \.\. 64', n_kinds=65, check=False)
    with pytest.raises(RuntimeError, match='must live on a HIP device'):
        capi.pocket_report(*cpu_args(c, n_kinds=6), check=False)


def pocket_data(seed=0, n_p=60, n=30):
    """a pocket around the origin, where ringed_result's clouds are, as the object a result file carries"""
    c = PR.build_case(seed, n_p, [n], dead=False)
    rng = np.random.default_rng(seed)
    feat = workloads.featurize_protein(np.asarray(workloads.PROTEIN_ELEMENTS)[np.maximum(c['pelem'], 1)], rng.integers(0, 20, n_p), rng.random(n_p) < 0.5)
    return types.SimpleNamespace(protein_pos=torch.from_numpy(c['ppos'] * np.float32(0.4)), protein_atom_feature=torch.from_numpy(feat))


def test_sample_pocket_refuses_a_result_without_a_pocket():
    res = ringed_result(1, [5, 7], 2)
    with pytest.raises(ValueError, match='carries no pocket'):
        quality.sample_pocket(res, device='cpu')
    as_dict = {'data': None, 'pred_ligand_pos_traj': res[2], 'pred_ligand_v_traj': res[3]}
    with pytest.raises(ValueError, match='carries no pocket'):
        quality.sample_pocket(as_dict, device='cpu')
    pack = quality.SamplePack(res, device='cpu')
    with pytest.raises(ValueError, match='no pocket'):
        pack.pocket(types.SimpleNamespace(protein_pos=torch.zeros(3, 3)))
    with pytest.raises(ValueError, match=r'protein positions must be \[60, 3\]'):
        pack.pocket((torch.zeros(59, 3), pocket_data().protein_atom_feature))
    with pytest.raises(ValueError, match=r'protein feature is \[n, 27\]'):
        pack.pocket((torch.zeros(3, 3), torch.zeros(3, 26)))
    with pytest.raises(ValueError, match="by 'residue' or by 'element'"):
        pack.pocket(pocket_data(), kinds='atom')
    with pytest.raises(ValueError, match='include is'):
        pack.pocket(pocket_data(), include='stable')
    with pytest.raises(ValueError, match='one molecule'):
        pack.pocket(pocket_data(), reference_ligand=(np.zeros((2, 4, 3), np.float32), np.zeros(4, np.int64)))


def test_pocket_kinds():
    element = np.asarray([6, 7, 8, 16, 34, 1, 15, 6])                           # the seventh is no element of the table: no bit
    aa, bb = np.asarray([0, 0, 5, 19, 19, 3, 2, 7]), np.asarray([0, 1, 1, 0, 1, 0, 1, 1], bool)
    feat = workloads.featurize_protein(element, aa, bb)
    elem, kind, names = quality.pocket_kinds(feat)
    assert elem.dtype == kind.dtype == np.int32 and elem.tolist() == [1, 2, 3, 4, 5, 0, -1, 1]
    assert kind.tolist() == [0, 1, 11, 38, 39, -1, 5, 15]                        # 2 * residue + backbone; the hydrogen takes no part
    assert len(names) == 40 and names[:2] == ('ALA.sc', 'ALA.bb') and names[11] == 'GLY.bb' and names[38:] == ('TYR.sc', 'TYR.bb')
    assert quality.pocket_kinds(feat, hydrogens=True)[1].tolist() == [0, 1, 11, 38, 39, 6, 5, 15]
    elem2, kind2, names2 = quality.pocket_kinds(torch.from_numpy(feat), 'element')
    assert elem2.tolist() == elem.tolist() and kind2.tolist() == [1, 2, 3, 4, 5, -1, -1, 1] and names2 == ('H', 'C', 'N', 'O', 'S', 'Se')
    assert quality.pocket_kinds(feat, 'element', hydrogens=True)[1].tolist() == [1, 2, 3, 4, 5, 0, -1, 1]
    none = feat.copy()
    none[0, 6:26] = 0                                                           # a row without a residue bit
    assert quality.pocket_kinds(none)[1][0] == -1
    assert quality.pocket_kinds(feat.astype(np.int8))[1].tolist() == kind.tolist() and quality.pocket_kinds(np.zeros((0, 27)))[0].shape == (0,)


def test_clash_threshold_table():
    t = quality.pocket_clash_thresholds()
    assert t.shape == (8, 6) and t.dtype == np.float64 and np.array_equal(t, PR.clash_table())
    assert t[1, 1] == (1.7 + 1.7) - 0.5 and t[2, 3] == (1.55 + 1.52) - 0.5 and t[7, 5] == (1.75 + 1.9) - 0.5 and t[0, 0] == (1.2 + 1.2) - 0.5
    assert quality.DEFAULT_CONTACT_CUTOFF == 4.0 and quality.DEFAULT_CLASH_TOLERANCE == 0.5
    assert np.array_equal(quality.pocket_clash_thresholds(0.0), t + 0.5) or np.allclose(quality.pocket_clash_thresholds(0.0), t + 0.5, rtol=0, atol=1e-15)
    assert quality.pocket_clash_thresholds(0.5, {34: 2.0, 6: 1.8})[1, 5] == (1.8 + 2.0) - 0.5
    for bad in ({35: 1.85}, {6: -1.0}):
        with pytest.raises(ValueError, match='radii are non-negative'):
            quality.pocket_clash_thresholds(0.5, bad)
    with pytest.raises(ValueError, match='tolerance is finite'):
        quality.pocket_clash_thresholds(float('nan'))


def planted_raw():
    """two frames of four molecules of sizes 4, 0, 2, 5; the second frame touches nothing"""
    inf = np.inf
    hist = np.zeros((2, 8, 4), np.int64)
    hist[0, 1, 0], hist[0, 1, 1], hist[0, 3, 3] = 6, 3, 3                       # kinds 1 and 3 are of the backbone
    return dict(n_contacts=np.asarray([[7, 0, 0, 5], [0, 0, 0, 0]]), n_contact_atoms=np.asarray([[3, 0, 0, 5], [0, 0, 0, 0]]),
                n_pocket_atoms=np.asarray([[4, 0, 0, 2], [0, 0, 0, 0]]), n_clashes=np.asarray([[2, 0, 0, 0], [0, 0, 0, 0]]),
                min_dist=np.asarray([[1.5, inf, 6.0, 2.5], [9.0, inf, 8.0, 7.0]]), n_ref_common=np.asarray([[2, 0, 0, 1], [0, 0, 0, 0]]),
                kind_hist=hist, pocket_freq=np.asarray([[1, 1, 2, 1, 1, 0], [0, 0, 0, 0, 0, 0]]))


def test_pocket_report_arithmetic():
    names, backbone, sizes = ('A.sc', 'A.bb', 'B.sc', 'B.bb'), [False, True, False, True], [4, 0, 2, 5]
    rep = quality.PocketReport.from_outputs(planted_raw(), np.ones((2, 4), bool), sizes, names, backbone, ref_size=4)
    assert rep.num_frames == 2 and rep.n_samples == 4 and rep.n_included.tolist() == [4, 4]
    assert rep.clash_free(0) == 3 / 4 and rep.mean_clashes(0) == 2 / 4 and rep.mean_contacts(0) == 12 / 4
    assert rep.buried_share(0) == (3 / 4 + 0 / 2 + 5 / 5) / 3                    # the empty molecule is in no mean of shares
    assert rep.no_contact(0) == 2 / 4 and rep.no_contact(1) == 1.0              # an empty molecule touches nothing
    assert rep.mean_min_dist(0) == (1.5 + 6.0 + 2.5) / 3 and rep.mean_min_dist(1) == (9.0 + 8.0 + 7.0) / 3
    assert rep.contact_profile(0) == {'A.sc': 6 / 12, 'A.bb': 3 / 12, 'B.sc': 0.0, 'B.bb': 3 / 12} and rep.contact_profile(1) is None
    assert rep.backbone_share(0) == 6 / 12 and np.isnan(rep.backbone_share(1))
    assert rep.contact_frequency(0).tolist() == [1 / 4, 1 / 4, 2 / 4, 1 / 4, 1 / 4, 0.0]
    rec = np.asarray([2, 0, 0, 1]) / 4
    tan = np.asarray([2 / (4 + 4 - 2), 0 / 4, 0 / 4, 1 / (2 + 4 - 1)])
    assert rep.reference_recovery(0) == dict(ref_recovery_mean=rec.sum() / 4, ref_recovery_median=float(np.median(rec)), ref_recovery_max=0.5,
                                             ref_tanimoto=tan.sum() / 4)
    s = rep.summary(-1)
    assert list(s) == ['pocket_clash_free', 'pocket_mean_clashes', 'mean_contacts', 'buried_share', 'no_contact', 'mean_min_dist',
                       'backbone_share', 'ref_recovery_mean', 'ref_recovery_median', 'ref_recovery_max', 'ref_tanimoto']
    assert s['pocket_clash_free'] == 1.0 and s['mean_contacts'] == 0.0 and s['ref_recovery_max'] == 0.0 and np.isnan(s['backbone_share'])
    lines = rep.lines(0)
    assert lines[0] == 'pocket_clash_free:\t0.7500' and lines[-3:] == ['contacts A.sc:\t0.5000', 'contacts A.bb:\t0.2500', 'contacts B.bb:\t0.2500']
    assert 'backbone_share:\tNone' in rep.lines(1) and not any(x.startswith('contacts ') for x in rep.lines(1))
    # an include mask: only the first and the third molecule of frame 0, nothing of frame 1
    inc = np.asarray([[True, False, True, False], [False] * 4])
    raw = planted_raw()
    raw['pocket_freq'] = np.asarray([[1, 1, 1, 1, 0, 0], [0] * 6])
    part = quality.PocketReport.from_outputs(raw, inc, sizes, names, backbone, ref_size=4)
    assert part.n_included.tolist() == [2, 0] and part.clash_free(0) == 1 / 2 and part.mean_contacts(0) == 7 / 2 and part.no_contact(0) == 1 / 2
    assert part.buried_share(0) == (3 / 4 + 0 / 2) / 2 and part.contact_frequency(0).tolist() == [0.5, 0.5, 0.5, 0.5, 0.0, 0.0]
    empty = part.summary(1)                                                     # an empty include set: every share is NaN
    assert all(np.isnan(x) for x in empty.values()) and np.isnan(part.contact_frequency(1)).all() and part.n_ref.tolist() == [1, 0]
    # a reference that touches nothing gives NaN, not a division by zero; no reference gives no keys
    none = quality.PocketReport.from_outputs(planted_raw(), np.ones((2, 4), bool), sizes, names, backbone, ref_size=0)
    assert all(np.isnan(x) for x in none.reference_recovery(0).values()) and none.n_ref.tolist() == [0, 0]
    raw = planted_raw()
    del raw['n_ref_common']
    plain = quality.PocketReport.from_outputs(raw, np.ones((2, 4), bool), sizes, names, backbone)
    assert plain.reference_recovery(0) == {} and 'ref_tanimoto' not in plain.summary(0)
    by_element = quality.PocketReport.from_outputs(raw, np.ones((2, 4), bool), sizes, names, None)
    assert np.isnan(by_element.backbone_share(0))


def test_pocket_report_merged():
    names, backbone, sizes = ('A.sc', 'A.bb', 'B.sc', 'B.bb'), [False, True, False, True], [4, 0, 2, 5]
    a = quality.PocketReport.from_outputs(planted_raw(), np.ones((2, 4), bool), sizes, names, backbone, ref_size=4)
    raw = planted_raw()
    raw['pocket_freq'] = np.zeros((2, 9), np.int64)                             # another pocket, of nine atoms
    b = quality.PocketReport.from_outputs(raw, np.asarray([[True, False, True, False], [False] * 4]), sizes, names, backbone, ref_size=0)
    m = quality.PocketReport.merged([a, b])
    assert m.n_samples == 8 and m.n_included.tolist() == [6, 4] and m.clash_free(0) == (3 + 1) / 6 and m.mean_contacts(0) == (12 + 7) / 6
    assert m.buried_share(0) == ((3 / 4 + 0 / 2 + 5 / 5) + (3 / 4 + 0 / 2)) / 5 and m.mean_min_dist(0) == (10.0 + 7.5) / 5
    assert np.array_equal(m.kind_hist, a.kind_hist + b.kind_hist) and m.contact_frequency(0) is None
    assert m.n_ref.tolist() == [1, 1] and m.reference_recovery(0) == a.reference_recovery(0)      # b's reference touched nothing
    one = quality.PocketReport.merged([a])
    assert np.array_equal(one.contact_frequency(0), a.contact_frequency(0)) and one.summary(0) == a.summary(0)
    plain = quality.PocketReport.from_outputs({k: x for k, x in planted_raw().items() if k != 'n_ref_common'}, np.ones((2, 4), bool), sizes,
                                              names, backbone)
    with pytest.raises(ValueError, match='do not merge'):
        quality.PocketReport.merged([a, plain])
    with pytest.raises(ValueError, match='do not merge'):
        quality.PocketReport.merged([a, quality.PocketReport.from_outputs(planted_raw(), np.ones((2, 4), bool), sizes, names[::-1], backbone, 4)])


@pytest.fixture
def pocket_binding(numpy_binding, monkeypatch):  # noqa: F811
    """numpy_binding, and capi.pocket_report patched by its restatement too"""
    def binding(*a, **kw):
        numpy_binding.append(('pocket_report', kw.get('check')))
        return PR.torch_pocket_report(*a, **kw)

    monkeypatch.setattr(capi, 'pocket_report', binding)
    return numpy_binding


def save_with_pockets(tmp_path, results, pockets):
    for i, r in results.items():
        torch.save({'data': pockets[i], 'pred_ligand_pos': r[0], 'pred_ligand_v': r[1], 'pred_ligand_pos_traj': r[2], 'pred_ligand_v_traj': r[3],
                    'time': r[6]}, tmp_path / f'result_{i}.pt')


def expected_report(res, data, eval_step, reference_ligand=None, include=None):
    """PocketReport of a result through the restatement alone"""
    frames = slice(None) if eval_step == 'all' else slice(len(res[2][0]) - 1, None)
    sizes = [p.shape[1] for p in res[2]]
    pos = np.concatenate([p[frames] for p in res[2]], 1).astype(np.float32)
    v = np.concatenate([x[frames] for x in res[3]], 1)
    ptr = np.cumsum([0] + sizes)
    elem, kind, names = quality.pocket_kinds(data.protein_atom_feature)
    ppos = data.protein_pos.numpy()
    bits = size = None
    if reference_ligand is not None:
        q = PR.pocket_report(reference_ligand[0][None], reference_ligand[1][None], [0, len(reference_ligand[1])], CLASS_Z, ppos, elem, kind, 40, 4.0)
        bits, size = q['bits'][0, 0], int(q['n_pocket_atoms'][0, 0])
    w = PR.pocket_report(pos, v, ptr, CLASS_Z, ppos, elem, kind, 40, 4.0, PR.clash_table(), include, bits)
    inc = np.ones(w['n_contacts'].shape, bool) if include is None else include
    return quality.PocketReport.from_outputs({k: x for k, x in w.items() if x is not None}, inc, sizes, names, [n.endswith('.bb') for n in names], size)


def assert_same(got, want):
    assert vars(got).keys() == vars(want).keys()
    for k, x in vars(want).items():
        if isinstance(x, np.ndarray):
            assert np.array_equal(getattr(got, k), x, equal_nan=x.dtype.kind == 'f'), k
        else:
            assert getattr(got, k) == x, k


def test_sample_pocket_and_the_tool(pocket_binding, tmp_path, capsys):
    results = {10: ringed_result(5, [6, 9, 14], 3), 2: ringed_result(6, [4, 11, 5, 1], 3)}
    pockets = {10: pocket_data(1), 2: pocket_data(2, 45)}
    ligand = (np.asarray(results[10][2][0][-1], np.float32), np.asarray(results[10][3][0][-1], np.int64))
    for i, res in results.items():
        as_dict = {'data': pockets[i], 'pred_ligand_pos_traj': res[2], 'pred_ligand_v_traj': res[3]}
        for eval_step in (-1, 'all'):
            want = expected_report(res, pockets[i], eval_step, ligand)
            assert want.sum_contacts[-1] > 0 and want.sum_clashes[-1] > 0
            assert_same(quality.sample_pocket(as_dict, eval_step, reference_ligand=ligand, device='cpu'), want)
            assert_same(quality.SamplePack(res, eval_step, device='cpu').pocket(pockets[i]), expected_report(res, pockets[i], eval_step))
    mask = np.asarray([[True, False, True]] * 3)
    assert_same(quality.SamplePack(results[10], 'all', device='cpu').pocket(pockets[10], mask), expected_report(results[10], pockets[10], 'all', None, mask))
    # the tool: one pack per file, the reference ligand's call first, the host's look with the pack's first call only
    save_with_pockets(tmp_path, results, pockets)
    np.savez(tmp_path / 'ref.npz', ligand_pos=ligand[0], ligand_v=ligand[1])
    tool = load_tool('evaluate_samples')
    del pocket_binding[:]
    capsys.readouterr()
    out = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--pocket', '--eval_step', 'all', '--reference_npz', str(tmp_path / 'ref.npz')])
    assert pocket_binding == [('pack', None), ('pocket_report', None), ('pocket_report', True), ('quality_report', False)] * 2
    want = quality.PocketReport.merged([expected_report(results[i], pockets[i], 'all', ligand) for i in (2, 10)])
    printed = capsys.readouterr().out.split('\n')
    assert printed[7:7 + len(want.lines(-1))] == want.lines(-1) and printed[7].startswith('pocket_clash_free:\t')
    assert out['pocket']['mean_contacts'] == want.mean_contacts(-1) and out['pocket']['ref_recovery_mean'] == want.reference_recovery(-1)['ref_recovery_mean']
    assert out['pocket']['num_included'] == 7 and len(out['pocket']['curve']) == 3 and out['pocket']['contact_cutoff'] == 4.0
    assert sum(out['pocket']['kind_hist'].values()) == want.sum_contacts[-1]
    # other limits reach the report
    out2 = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--pocket', '--contact_cutoff', '6', '--clash_tolerance', '0'])
    assert out2['pocket']['mean_contacts'] > out['pocket']['mean_contacts'] and out2['pocket']['pocket_mean_clashes'] > out['pocket']['pocket_mean_clashes']
    assert 'ref_recovery_mean' not in out2['pocket'] and 'curve' not in out2['pocket']


def test_the_tool_without_the_flag_prints_what_it_printed(pocket_binding, tmp_path, capsys):
    results = {10: ringed_result(5, [6, 9, 14], 3), 2: ringed_result(6, [4, 11, 5, 1], 3)}
    save_with_pockets(tmp_path, results, {10: pocket_data(1), 2: None})          # a file without a pocket is fine without the flag
    tool = load_tool('evaluate_samples')
    del pocket_binding[:]
    capsys.readouterr()
    out = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu'])
    lines = capsys.readouterr().out.rstrip('\n').split('\n')
    assert [x.split(':')[0].split('!')[0] for x in lines] == ['Load generated data done', 'Evaluate done', 'mol_stable', 'atm_stable', 'JSD_CC_2A',
                                                              'JSD_All_12A', 'Atom type JS', 'wrote ' + str(tmp_path / 'eval_results' / 'quality.json')]
    assert 'pocket' not in out and pocket_binding == [('pack', None), ('quality_report', True)] * 2
    with pytest.raises(SystemExit, match='carries no pocket'):
        tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--pocket'])


def test_export_sdf_writes_only_the_molecules_without_a_protein_clash(pocket_binding, tmp_path):
    res = ringed_result(5, [6, 9, 14, 3], 3)
    res[2][3] = (res[2][3].astype(np.float32) + np.float32(40)).astype(np.float64)      # the last sample has left the pocket: no clash
    res[0][3] = res[2][3][-1]
    data = pocket_data(1)
    save_with_pockets(tmp_path, {4: res}, {4: data})
    want = expected_report(res, data, -1)
    elem, kind, _ = quality.pocket_kinds(data.protein_atom_feature)
    pos = np.concatenate([p[-1:] for p in res[2]], 1).astype(np.float32)
    w = PR.pocket_report(pos, np.concatenate([x[-1:] for x in res[3]], 1), np.cumsum([0, 6, 9, 14, 3]), CLASS_Z, data.protein_pos.numpy(), elem, kind,
                         40, 4.0, PR.clash_table())
    free = w['n_clashes'][0] == 0
    assert free[3] and not free.all() and want.n_clash_free[-1] == free.sum()
    tool = load_tool('export_sdf')
    out = tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'sdf'), '--device', 'cpu', '--pocket-clash-free'])
    assert out['result_4']['pocket_clash_free'] == free.sum() == out['result_4']['written']
    recs = parse_sdf(open(tmp_path / 'sdf' / 'result_4.sdf').read())
    assert [len(atoms) for _, atoms, _, _ in recs] == [n for n, ok in zip([6, 9, 14, 3], free) if ok]
    plain = tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'sdf2'), '--device', 'cpu'])
    assert plain['result_4']['written'] == 4 and 'pocket_clash_free' not in plain['result_4']
