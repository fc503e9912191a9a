"""CPU-only checks of the solvent-accessible-surface report ("Solvent-accessible surface"):

  1. the restatement tests/_sasa_ref.py against hand cases: an isolated atom, two atoms that do not meet, an atom enclosed by six, and
     two equal spheres swept apart -- the exposed count never falls, and the exposed fraction follows the analytic cap (1 + d / 2R) / 2
     to the restatement's own largest deviation (measured once on the CPU, EXPERIMENTS.md "SASA") plus one point;
  2. the library exports td_sasa_report and the ABI version stays 5;
  3. every ValueError of capi.sasa_report, of the helpers of quality and of quality.sample_sasa, reached without a device, and a CPU
     tensor refused before anything is allocated;
  4. the arithmetic of quality.SasaReport on planted counts;
  5. tools/evaluate_samples.py --sasa and tools/export_sdf.py --min-buried-share with the bindings patched by the restatements.
tests/test_gpu_sasa.py compares the kernel with the restatement.
"""
import types

import numpy as np
import pytest
import torch

import _sasa_ref as SR
from targetdiff_amd import capi, quality, workloads
from test_bonds_host import load_tool, parse_sdf
from test_rings_host import ringed_result
from test_sample_pack_host import numpy_binding  # noqa: F401  (the fixture that patches the other bindings)

CLASS_Z = quality.class_atomic_numbers('add_aromatic')
C, N_, O = 1, 3, 5                                                             # classes of 'add_aromatic'
LIG_R, PROT_R = SR.reaches()
NO_POCKET = dict(ppos=np.zeros((0, 3), np.float32), pelem=np.zeros(0, np.int32))
SWEEP_MAX_DEVIATION = 0.0074975                                                # of the restatement at P = 256, measured: EXPERIMENTS.md "SASA"


def ref(c, dirs=None, include=None):
    return SR.sasa_report(c['pos'], c['v'], c['ptr'], CLASS_Z, c['ppos'], c['pelem'], LIG_R, PROT_R, SR.directions(96) if dirs is None else dirs,
                          include)


def molecule(atoms, cls, **pocket):
    atoms = np.asarray(atoms, np.float32).reshape(-1, 3)
    return dict(dict(pos=atoms[None], v=np.asarray(cls, np.int64)[None], ptr=np.asarray([0, len(atoms)], np.int32)), **(pocket or NO_POCKET))


def test_the_directions_and_the_reaches_of_the_package_are_the_restatements():
    for P in (1, 2, 63, 96, 256):
        d = quality.sasa_directions(P)
        assert d.shape == (P, 3) and d.dtype == np.float64 and d.tobytes() == SR.directions(P).tobytes()
        assert np.abs((d * d).sum(1) - 1.0).max() < 1e-12
    assert quality.sasa_directions().shape == (96, 3) and quality.SASA_POINTS == 96 and quality.SASA_PROBE == 1.4
    z = quality.sasa_directions(4)[:, 2]
    assert z.tolist() == [0.75, 0.25, -0.25, -0.75]
    lr, pr = quality.sasa_reaches()
    assert np.array_equal(lr, LIG_R) and np.array_equal(pr, PROT_R) and lr[1] == 1.7 + 1.4 and pr[5] == 1.9 + 1.4 and lr.shape == (8,) and pr.shape == (6,)
    assert quality.sasa_reaches(0.0)[0].tolist() == [1.2, 1.7, 1.55, 1.52, 1.47, 1.8, 1.8, 1.75]
    assert quality.sasa_reaches(1.0, {6: 2.0, 34: 2.0})[0][1] == 3.0 and quality.sasa_reaches(1.0, {34: 2.0})[1][5] == 3.0


def test_an_isolated_atom_is_wholly_exposed_and_its_area_is_that_of_its_sphere():
    for P in (1, 96, 256):
        r = ref(molecule([(1, 2, 3)], [C]), SR.directions(P))
        assert r['free'].tolist() == [[[0, P, 0, 0, 0, 0, 0, 0]]] and r['bound'].tolist() == r['free'].tolist() and r['atom_free'].tolist() == [[P]]
        area = quality.sasa_areas(r['free'][0, 0], LIG_R, P)
        assert abs(area[0] - 4.0 * np.pi * 3.1 ** 2) < 1e-9 and area[1] == 0.0 and area[2] == area[0]
    r = ref(molecule([(1, 2, 3)], [13]))                                         # a class outside the table takes no part
    assert not r['free'].any() and not r['atom_free'].any()
    assert {k: r[k].dtype for k in SR.KEYS} == dict(free=np.int32, bound=np.int32, pocket_buried=np.int32, atom_free=np.int32, atom_bound=np.int32,
                                                    bits=np.int64, pocket_free=np.int32, pocket_mask=np.int64, pocket_buried_sum=np.int64)


def test_two_atoms_that_do_not_meet_occlude_nothing():
    touching = np.nextafter(np.float32(LIG_R[1] + LIG_R[3]), np.float32(99))     # the fp32 above R_C + R_O
    for d in (touching, np.float32(7), np.float32(50)):
        r = ref(molecule([(0, 0, 0), (d, 0, 0)], [C, O]))
        assert r['atom_free'].tolist() == [[96, 96]] and r['free'][0, 0].tolist() == [0, 96, 0, 96, 0, 0, 0, 0]
    closer = ref(molecule([(0, 0, 0), (2, 0, 0)], [C, O]))
    assert (closer['atom_free'] < 96).all() and (closer['atom_free'] > 48).all()
    # the same pair as a ligand atom and a protein atom: free sees the ligand alone, bound and the pocket's buried points see both
    pair = ref(molecule([(0, 0, 0)], [C], ppos=np.asarray([(2, 0, 0)], np.float32), pelem=np.asarray([3], np.int32)))
    assert pair['free'][0, 0, 1] == 96 and pair['bound'][0, 0, 1] == closer['atom_free'][0, 0] and pair['pocket_free'].tolist() == [96]
    assert pair['pocket_buried'][0, 0].tolist() == [0, 0, 0, 96 - closer['atom_free'][0, 1], 0, 0] and pair['bits'].tolist() == [[[1]]]
    assert pair['pocket_buried_sum'].tolist() == [[96 - closer['atom_free'][0, 1]]] and pair['pocket_mask'].view(np.uint64).tolist() == [[2 ** 64 - 1, 2 ** 32 - 1, 0, 0]]
    out = ref(molecule([(0, 0, 0)], [C], ppos=np.asarray([(2, 0, 0)], np.float32), pelem=np.asarray([3], np.int32)), include=np.zeros((1, 1), bool))
    assert not out['pocket_buried_sum'].any() and out['pocket_buried'].tolist() == pair['pocket_buried'].tolist()


def test_an_atom_enclosed_by_six_has_no_exposed_point():
    six = [(1.5, 0, 0), (-1.5, 0, 0), (0, 1.5, 0), (0, -1.5, 0), (0, 0, 1.5), (0, 0, -1.5)]
    r = ref(molecule([(0, 0, 0)] + six, [N_] + [C] * 6), SR.directions(256))
    assert r['atom_free'][0, 0] == 0 and (r['atom_free'][0, 1:] > 0).all() and r['free'][0, 0, 2] == 0
    # enclosed by the pocket instead: free, and not bound; the cage of protein atoms alone has an apo surface, part of it buried
    cage = ref(molecule([(0, 0, 0)], [N_], ppos=np.asarray(six, np.float32), pelem=np.ones(6, np.int32)), SR.directions(256))
    assert cage['free'][0, 0, 2] == 256 and cage['bound'][0, 0, 2] == 0 and (cage['pocket_free'] == r['atom_free'][0, 1:] + cage['pocket_buried_sum'][0]).all()
    dead = ref(molecule([(0, 0, 0)], [N_], ppos=np.asarray(six, np.float32), pelem=np.full(6, -1, np.int32)), SR.directions(256))
    assert dead['bound'][0, 0, 2] == 256 and not dead['pocket_free'].any()


def sweep():
    """two carbons d apart, d = 0.05 .. 7 A in fp32, P = 256: the exposed points of both (of 512) per d"""
    ds = (np.arange(1, 141) * 0.05).astype(np.float32)
    dirs = SR.directions(256)
    return ds, np.asarray([int(ref(molecule([(0, 0, 0), (d, 0, 0)], [C, C]), dirs)['free'][0, 0, 1]) for d in ds])


def test_two_equal_spheres_swept_apart():
    ds, counts = sweep()
    assert (np.diff(counts) >= 0).all() and counts[0] < 270 and counts[-1] == 512
    R = LIG_R[1]
    analytic = np.minimum(1.0, (1.0 + ds.astype(np.float64) / (2.0 * R)) / 2.0)
    deviation = np.abs(counts / 512.0 - analytic).max()
    print(f'largest deviation from the analytic cap fraction: {deviation!r}')
    assert deviation <= SWEEP_MAX_DEVIATION + 1.0 / 256.0


def test_library_exports_the_entry_point_and_the_abi_version_stays():
    lib = capi.load_library()
    assert hasattr(lib, 'td_sasa_report') and 'td_sasa_report' in capi.SIGNATURES
    assert len(capi.SIGNATURES['td_sasa_report'][1]) == 26
    assert lib.td_abi_version() == capi.ABI_VERSION == 5


def cpu_args(c, lig=LIG_R, prot=PROT_R, dirs=None, include=None):
    t = torch.as_tensor
    return [t(c['pos']), t(c['v']), t(c['ptr']), CLASS_Z, t(c['ppos']), t(c['pelem']), lig, prot, t(SR.directions(96) if dirs is None else dirs), include]


def test_binding_refuses_bad_arguments_before_anything_is_launched():
    c = SR.build_case(0, 70, [4, 9], S=2, dead=False)

    def refused(match, edit=None, check=True, **kw):
        a = cpu_args(c, **kw)
        if edit:
            edit(a)
        with pytest.raises(ValueError, match=match):
            capi.sasa_report(*a, check=check)

    def put(i, x):
        return lambda a: a.__setitem__(i, x)

    refused(r'pos / v must be', put(0, torch.zeros(2, 13, 2)))
    refused(r'prefix offsets', put(2, torch.tensor([0, 9, 4], dtype=torch.int32)))
    refused(r'v must be in', put(1, torch.full((2, 13), 13)))
    refused(r'at most 512', lambda a: (a.__setitem__(0, torch.zeros(1, 513, 3)), a.__setitem__(1, torch.zeros(1, 513, dtype=torch.int64)),
                                      a.__setitem__(2, torch.tensor([0, 513], dtype=torch.int32))))
    refused(r'include must be', include=torch.ones(2, 3, dtype=torch.bool))
    refused(r'protein_pos must be \[N_p, 3\]', put(4, torch.zeros(70, 4)))
    refused(r'protein_elem must be \[70\]', put(5, torch.zeros(69, dtype=torch.int32)))
    refused(r'fp32 / int32', put(4, torch.zeros(70, 3, dtype=torch.float64)))
    refused(r'fp32 / int32', put(5, torch.zeros(70, dtype=torch.int64)))
    refused(r'device of the pack', put(4, torch.zeros(70, 3, device='meta')))
    refused(r'device of the pack', put(8, torch.zeros(96, 3, dtype=torch.float64, device='meta')))
    refused(r'dirs must be \[P, 3\]', dirs=np.zeros((96, 2)))
    refused(r'dirs must be \[P, 3\]', dirs=np.zeros((0, 3)))
    refused(r'dirs must be \[P, 3\]', dirs=SR.directions(256).repeat(2, 0)[:257])
    refused(r'dirs must be float64', dirs=SR.directions(96).astype(np.float32))
    for bad in (np.zeros(7), np.full(8, np.nan), np.full(8, np.inf), np.zeros(8), -LIG_R, np.zeros((8, 1))):
        refused(r'ligand_reach is \[8\], finite and > 0', lig=bad)
    for bad in (np.zeros(8), np.full(6, np.inf), np.zeros(6)):
        refused(r'protein_reach is \[6\], finite and > 0', prot=bad)
    refused(r'protein_elem must be in \[-1, 6\)', put(5, torch.full((70,), 6, dtype=torch.int32)))
    refused(r'protein_elem must be in \[-1, 6\)', put(5, torch.full((70,), -2, dtype=torch.int32)))
    nan = SR.directions(96)
    nan[5, 1] = np.nan
    refused(r'finite unit vectors', dirs=nan)
    refused(r'finite unit vectors', dirs=SR.directions(96) * 1.001)
    refused(r'finite unit vectors', dirs=np.zeros((4, 3)))
    far = c['pos'].copy()
    far[1, 3, 2] = 1.5e5
    refused(r'pos must be finite with \|coordinate\| <= 100000', put(0, torch.as_tensor(far)))
    far[1, 3, 2] = np.nan
    refused(r'pos must be finite', put(0, torch.as_tensor(far)))
    pfar = c['ppos'].copy()
    pfar[0, 0] = -np.inf
    refused(r'protein_pos must be finite', put(4, torch.as_tensor(pfar)))
    assert capi.SASA_COORD_MAX == 1.0e5 and capi.SASA_MAX_POINTS == 256 and capi.SASA_CULL_REL == capi.SASA_CULL_ABS == 1e-4
    # check=False skips the looks at the values, not the ones at shapes and types; what passes them needs a device: a CPU tensor is
    # refused when the arguments are formed, before an output is allocated
    refused(r'dirs must be float64', dirs=SR.directions(96).astype(np.float32), check=False)
    allocated = []
    empty = torch.empty
    try:
        torch.empty = lambda *a, **kw: allocated.append(a) or empty(*a, **kw)
        with pytest.raises(RuntimeError, match='must live on a HIP device'):
            capi.sasa_report(*cpu_args(c), check=False)
        with pytest.raises(RuntimeError, match='must live on a HIP device'):
            capi.sasa_report(*cpu_args(c))
    finally:
        torch.empty = empty
    assert allocated == []


def test_the_helpers_refuse_bad_arguments():
    for P in (0, 257, -1):
        with pytest.raises(ValueError, match=r'1 \.\. 256 points'):
            quality.sasa_directions(P)
    for bad in ({35: 1.85}, {6: -1.0}):
        with pytest.raises(ValueError, match='radii are non-negative'):
            quality.sasa_reaches(1.4, bad)
    for probe in (-0.1, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='probe radius is finite and >= 0'):
            quality.sasa_reaches(probe)
    with pytest.raises(ValueError, match='must be > 0'):
        quality.sasa_reaches(0.0, {1: 0.0})


def pocket_data(seed=0, n_p=60, n=30):
    """a pocket around the origin, where ringed_result's clouds are, as the object a result file carries; one atom in ten a hydrogen"""
    c = SR.build_case(seed, n_p, [n], dead=False)
    rng = np.random.default_rng(seed)
    feat = workloads.featurize_protein(np.asarray(workloads.PROTEIN_ELEMENTS)[c['pelem']], rng.integers(0, 20, n_p), rng.random(n_p) < 0.5)
    return types.SimpleNamespace(protein_pos=torch.from_numpy(c['ppos']), protein_atom_feature=torch.from_numpy(feat))


def test_sample_sasa_refuses_a_result_without_a_pocket():
    res = ringed_result(1, [5, 7], 2)
    with pytest.raises(ValueError, match='carries no pocket'):
        quality.sample_sasa(res, device='cpu')
    as_dict = {'data': None, 'pred_ligand_pos_traj': res[2], 'pred_ligand_v_traj': res[3]}
    with pytest.raises(ValueError, match='carries no pocket'):
        quality.sample_sasa(as_dict, device='cpu')
    pack = quality.SamplePack(res, device='cpu')
    with pytest.raises(ValueError, match='no pocket'):
        pack.sasa(types.SimpleNamespace(protein_pos=torch.zeros(3, 3)))
    with pytest.raises(ValueError, match=r'protein positions must be \[60, 3\]'):
        pack.sasa((torch.zeros(59, 3), pocket_data().protein_atom_feature))
    with pytest.raises(ValueError, match='include is'):
        pack.sasa(pocket_data(), include='stable')
    with pytest.raises(ValueError, match=r'1 \.\. 256 points'):
        pack.sasa(pocket_data(), points=300)
    with pytest.raises(ValueError, match='probe radius'):
        pack.sasa(pocket_data(), probe=-1.0)


def planted_raw():
    """two frames of three molecules; the second frame is out of the pocket"""
    free = np.zeros((2, 3, 8), np.int64)
    bound = np.zeros((2, 3, 8), np.int64)
    free[0, 0, [1, 2, 3]], bound[0, 0, [1, 2, 3]] = (200, 48, 96), (100, 0, 48)
    free[0, 1, [1, 7]], bound[0, 1, [1, 7]] = (96, 96), (96, 24)
    free[1] = free[0]                                                           # the third molecule is empty: nothing free
    bound[1] = free[1]
    pb = np.zeros((2, 3, 6), np.int64)
    pb[0, 0, [1, 2, 3]], pb[0, 1, [1, 4]] = (30, 10, 20), (5, 0)
    bits = np.zeros((2, 3, 1), np.int64)
    bits[0, 0, 0], bits[0, 1, 0] = 0b01111, 0b10001
    return dict(free=free, bound=bound, pocket_buried=pb, bits=bits, pocket_buried_sum=np.asarray([[30, 10, 20, 0, 5], [0] * 5]))


def area(counts, reach, P=96):
    return float((np.asarray(counts, np.float64) * (4.0 * np.pi * np.asarray(reach) ** 2 / P)).sum())


def test_sasa_report_arithmetic():
    raw = planted_raw()
    ref_lig = dict(free=np.asarray([0, 96, 0, 96, 0, 0, 0, 0]), bound=np.asarray([0, 24, 0, 48, 0, 0, 0, 0]), pocket_buried=np.asarray([0, 40, 0, 8, 0, 0]),
                   bits=np.asarray([0b00111], np.int64))
    rep = quality.SasaReport.from_outputs(raw, np.ones((2, 3), bool), LIG_R, PROT_R, 96, 1.4, ref_lig)
    assert rep.num_frames == 2 and rep.n_samples == 3 and rep.n_included.tolist() == [3, 3] and rep.points == 96 and rep.probe == 1.4
    f0, f1 = area(raw['free'][0, 0], LIG_R), area(raw['free'][0, 1], LIG_R)
    b0, b1 = area(raw['bound'][0, 0], LIG_R), area(raw['bound'][0, 1], LIG_R)
    u0, u1 = area(raw['free'][0, 0] - raw['bound'][0, 0], LIG_R), area(raw['free'][0, 1] - raw['bound'][0, 1], LIG_R)
    close = lambda a, b: abs(a - b) <= 1e-12 * max(1.0, abs(b))
    assert close(rep.free_area(0), (f0 + f1) / 3) and close(rep.bound_area(0), (b0 + b1) / 3) and close(rep.buried_area(0), (u0 + u1) / 3)
    assert close(rep.buried_share(0), (u0 / f0 + u1 / f1 + 0.0) / 3)             # the empty molecule: nothing free, share 0
    polar0 = area([0, 0, 48, 96, 0, 0, 0, 0], LIG_R)
    assert close(rep.free_area(0, 1), polar0 / 3) and close(rep.free_area(0, 2), (f0 + f1 - polar0) / 3)
    assert close(rep.buried_area(0, 1), area([0, 0, 48, 48, 0, 0, 0, 0], LIG_R) / 3)
    assert close(rep.free_area(0, 1) + rep.free_area(0, 2), rep.free_area(0))
    p0, p1 = area(raw['pocket_buried'][0, 0], PROT_R), area(raw['pocket_buried'][0, 1], PROT_R)
    assert close(rep.pocket_buried_area(0), (p0 + p1) / 3) and close(rep.pocket_buried_polar_share(0), area([0, 0, 10, 20, 0, 0], PROT_R) / (p0 + p1))
    assert rep.buries_nothing(0) == 1 / 3 and rep.buries_nothing(1) == 1.0 and rep.buried_area(1) == 0.0 and rep.buried_share(1) == 0.0
    assert np.isnan(rep.pocket_buried_polar_share(1)) and rep.pocket_map(0).tolist() == [10.0, 10 / 3, 20 / 3, 0.0, 5 / 3]
    # the reference ligand: its own numbers, and the recovery of the three protein atoms it buries
    own = rep.reference(0)
    rf, rb = area(ref_lig['free'], LIG_R), area(ref_lig['bound'], LIG_R)
    assert close(own['ref_sasa_free'], rf) and close(own['ref_sasa_bound'], rb) and close(own['ref_sasa_buried'], rf - rb)
    assert close(own['ref_sasa_buried_share'], (rf - rb) / rf) and close(own['ref_pocket_buried_area'], area(ref_lig['pocket_buried'], PROT_R))
    rec, tan = np.asarray([3, 1, 0]) / 3, np.asarray([3 / (4 + 3 - 3), 1 / (2 + 3 - 1), 0.0])
    assert own['ref_recovery_mean'] == rec.sum() / 3 and own['ref_recovery_median'] == float(np.median(rec)) and own['ref_recovery_max'] == 1.0
    assert own['ref_tanimoto'] == tan.sum() / 3 and rep.reference(1)['ref_recovery_max'] == 0.0
    s = rep.summary(0)
    assert list(s) == ['sasa_free', 'sasa_bound', 'sasa_buried', 'sasa_buried_share', 'sasa_free_polar', 'sasa_bound_polar', 'sasa_buried_polar',
                       'sasa_free_apolar', 'sasa_bound_apolar', 'sasa_buried_apolar', 'pocket_buried_area', 'pocket_buried_polar_share',
                       'buries_nothing', 'ref_sasa_free', 'ref_sasa_bound', 'ref_sasa_buried', 'ref_sasa_buried_share', 'ref_pocket_buried_area',
                       'ref_recovery_mean', 'ref_recovery_median', 'ref_recovery_max', 'ref_tanimoto']
    assert rep.lines(0)[0] == f'sasa_free:\t{(f0 + f1) / 3:.4f}' and 'pocket_buried_polar_share:\tNone' in rep.lines(1)
    # an include mask; an empty set gives NaN
    inc = np.asarray([[True, False, False], [False] * 3])
    part = quality.SasaReport.from_outputs(raw, inc, LIG_R, PROT_R, 96, 1.4, ref_lig)
    assert part.n_included.tolist() == [1, 0] and close(part.free_area(0), f0) and close(part.buried_share(0), u0 / f0) and part.buries_nothing(0) == 0.0
    assert part.reference(0)['ref_recovery_mean'] == 1.0 and part.n_ref.tolist() == [1, 0]
    assert all(np.isnan(x) for k, x in part.summary(1).items() if not k.startswith('ref_sasa') and k != 'ref_pocket_buried_area')
    # no reference: no keys; a reference that buries nothing: NaN, not a division by zero
    plain = quality.SasaReport.from_outputs({k: x for k, x in raw.items() if k != 'bits'}, np.ones((2, 3), bool), LIG_R, PROT_R, 96)
    assert plain.reference(0) == {} and 'ref_tanimoto' not in plain.summary(0) and plain.probe is None
    none = quality.SasaReport.from_outputs(raw, np.ones((2, 3), bool), LIG_R, PROT_R, 96, 1.4, dict(ref_lig, bits=np.zeros(1, np.int64)))
    assert np.isnan(none.reference(0)['ref_recovery_mean']) and none.reference(0)['ref_sasa_free'] == own['ref_sasa_free']
    # merged: the sums add, the map belongs to one pocket
    m = quality.SasaReport.merged([rep, part])
    assert m.n_samples == 6 and m.n_included.tolist() == [4, 3] and close(m.free_area(0), (f0 + f1 + f0) / 4) and m.pocket_map(0) is None
    assert close(m.reference(0)['ref_recovery_mean'], (rec.sum() / 3 + 1.0) / 2) and close(m.reference(0)['ref_sasa_free'], rf)
    assert quality.SasaReport.merged([rep]).summary(0) == rep.summary(0)
    for other in (plain, quality.SasaReport.from_outputs(raw, np.ones((2, 3), bool), LIG_R, PROT_R, 64, 1.4, ref_lig),
                  quality.SasaReport.from_outputs(raw, np.ones((2, 3), bool), LIG_R, PROT_R, 96, 1.0, ref_lig)):
        with pytest.raises(ValueError, match='do not merge'):
            quality.SasaReport.merged([rep, other])


@pytest.fixture
def sasa_binding(numpy_binding, monkeypatch):  # noqa: F811
    """numpy_binding, and capi.sasa_report patched by its restatement too"""
    def binding(*a, **kw):
        numpy_binding.append(('sasa_report', kw.get('check')))
        return SR.torch_sasa_report(*a, **kw)

    monkeypatch.setattr(capi, 'sasa_report', binding)
    return numpy_binding


def save_with_pockets(tmp_path, results, pockets):
    for i, r in results.items():
        torch.save({'data': pockets[i], 'pred_ligand_pos': r[0], 'pred_ligand_v': r[1], 'pred_ligand_pos_traj': r[2], 'pred_ligand_v_traj': r[3],
                    'time': r[6]}, tmp_path / f'result_{i}.pt')


def packed(res, eval_step):
    frames = slice(None) if eval_step == 'all' else slice(len(res[2][0]) - 1, None)
    sizes = [p.shape[1] for p in res[2]]
    return (np.concatenate([p[frames] for p in res[2]], 1).astype(np.float32), np.concatenate([x[frames] for x in res[3]], 1),
            np.cumsum([0] + sizes), sizes)


def expected_report(res, data, eval_step, reference_ligand=None, include=None, probe=1.4, points=96):
    """SasaReport of a result through the restatement alone"""
    pos, v, ptr, sizes = packed(res, eval_step)
    _, elem, _ = quality.pocket_kinds(data.protein_atom_feature, 'element')      # hydrogens left out: kind -1
    lr, pr = SR.reaches(probe)
    ppos, dirs = data.protein_pos.numpy(), SR.directions(points)
    own = None
    if reference_ligand is not None:
        q = SR.sasa_report(reference_ligand[0][None], reference_ligand[1][None], [0, len(reference_ligand[1])], CLASS_Z, ppos, elem, lr, pr, dirs)
        own = {k: q[k][0, 0] for k in ('free', 'bound', 'pocket_buried', 'bits')}
    w = SR.sasa_report(pos, v, ptr, CLASS_Z, ppos, elem, lr, pr, dirs, include)
    inc = np.ones(w['free'].shape[:2], bool) if include is None else include
    if own is None:
        del w['bits']
    return quality.SasaReport.from_outputs(w, inc, lr, pr, points, float(probe), own)


def assert_same(got, want):
    assert vars(got).keys() == vars(want).keys()
    for k, x in vars(want).items():
        if isinstance(x, np.ndarray):
            assert np.array_equal(getattr(got, k), x, equal_nan=x.dtype.kind == 'f'), k
        else:
            assert getattr(got, k) == x, k


def test_sample_sasa_and_the_tool(sasa_binding, tmp_path, capsys):
    results = {10: ringed_result(5, [6, 9, 14], 3), 2: ringed_result(6, [4, 11, 5, 1], 3)}
    pockets = {10: pocket_data(1), 2: pocket_data(2, 45)}
    assert (pockets[10].protein_atom_feature[:, 0] != 0).any()                   # a hydrogen is in the pocket, and is left out
    ligand = (np.asarray(results[10][2][0][-1], np.float32), np.asarray(results[10][3][0][-1], np.int64))
    for i, res in results.items():
        as_dict = {'data': pockets[i], 'pred_ligand_pos_traj': res[2], 'pred_ligand_v_traj': res[3]}
        for eval_step in (-1, 'all'):
            want = expected_report(res, pockets[i], eval_step, ligand)
            assert want.sum_buried[-1, 0] > 0 and want.sum_bound[-1, 0] > 0 and want.sum_pocket[-1, 0] > 0
            assert_same(quality.sample_sasa(as_dict, eval_step, reference_ligand=ligand, device='cpu'), want)
            assert_same(quality.SamplePack(res, eval_step, device='cpu').sasa(pockets[i]), expected_report(res, pockets[i], eval_step))
    mask = np.asarray([[True, False, True]] * 3)
    assert_same(quality.SamplePack(results[10], 'all', device='cpu').sasa(pockets[10], mask), expected_report(results[10], pockets[10], 'all', None, mask))
    assert_same(quality.sample_sasa({'data': pockets[2], 'pred_ligand_pos_traj': results[2][2], 'pred_ligand_v_traj': results[2][3]}, -1, probe=1.0,
                                    points=64, device='cpu'), expected_report(results[2], pockets[2], -1, probe=1.0, points=64))
    # pocket_sasa: the raw counts and the areas per molecule
    pos, v, ptr, _ = packed(results[10], -1)
    s = quality.pocket_sasa(pockets[10].protein_pos, pockets[10].protein_atom_feature, pos, v, ligand_ptr=torch.as_tensor(ptr, dtype=torch.int32),
                            return_bits=True, device='cpu')
    _, elem, _ = quality.pocket_kinds(pockets[10].protein_atom_feature, 'element')
    w = SR.sasa_report(pos, v, ptr, CLASS_Z, pockets[10].protein_pos.numpy(), elem, LIG_R, PROT_R, SR.directions(96))
    for k in SR.KEYS:
        assert np.array_equal(getattr(s, k).numpy(), w[k]), k
    fa = quality.sasa_areas(w['free'], LIG_R, 96)[..., 0]
    ba = quality.sasa_areas(w['bound'], LIG_R, 96)[..., 0]
    assert np.array_equal(s.free_area.numpy(), fa) and np.array_equal(s.bound_area.numpy(), ba) and np.allclose(s.buried_area.numpy(), fa - ba, rtol=0, atol=1e-9)
    assert np.allclose(s.buried_share.numpy(), (fa - ba) / fa, rtol=0, atol=1e-12) and s.points == 96
    with_h = quality.pocket_sasa(pockets[10].protein_pos, pockets[10].protein_atom_feature, pos, v, ligand_ptr=torch.as_tensor(ptr, dtype=torch.int32),
                                 hydrogens=True, device='cpu')
    assert int(with_h.bound.sum()) < int(s.bound.sum()) and (with_h.pocket_free.numpy()[elem == -1] > 0).any() and with_h.bits is None
    # the tool: one pack per file, the reference ligand's call first, the host's look with the pack's call
    save_with_pockets(tmp_path, results, pockets)
    np.savez(tmp_path / 'ref.npz', ligand_pos=ligand[0], ligand_v=ligand[1])
    tool = load_tool('evaluate_samples')
    del sasa_binding[:]
    capsys.readouterr()
    out = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--sasa', '--eval_step', 'all', '--reference_npz', str(tmp_path / 'ref.npz')])
    assert sasa_binding == [('pack', None), ('sasa_report', None), ('sasa_report', True), ('quality_report', False)] * 2
    want = quality.SasaReport.merged([expected_report(results[i], pockets[i], 'all', ligand) for i in (2, 10)])
    printed = capsys.readouterr().out.split('\n')
    assert printed[7:7 + len(want.lines(-1))] == want.lines(-1) and printed[7].startswith('sasa_free:\t')
    assert out['sasa']['sasa_buried'] == want.buried_area(-1) and out['sasa']['ref_recovery_mean'] == want.reference(-1)['ref_recovery_mean']
    assert out['sasa']['num_included'] == 7 and len(out['sasa']['curve']) == 3 and out['sasa']['probe'] == 1.4 and out['sasa']['points'] == 96
    # other conventions reach the report; 'complete' restricts the molecules
    out2 = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--sasa', '--probe', '0.5', '--sasa_points', '32'])
    assert out2['sasa']['sasa_free'] < out['sasa']['sasa_free'] and out2['sasa']['points'] == 32 and 'ref_recovery_mean' not in out2['sasa']
    assert 'curve' not in out2['sasa']
    out3 = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--sasa', '--include', 'complete'])
    assert out3['sasa']['num_included'] < 7
    with pytest.raises(SystemExit, match=r'1 \.\. 256 points'):
        tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--sasa', '--sasa_points', '500'])


def test_the_tool_without_the_flag_prints_what_it_printed(sasa_binding, tmp_path, capsys):
    results = {10: ringed_result(5, [6, 9, 14], 3), 2: ringed_result(6, [4, 11, 5, 1], 3)}
    save_with_pockets(tmp_path, results, {10: pocket_data(1), 2: None})          # a file without a pocket is fine without the flag
    tool = load_tool('evaluate_samples')
    del sasa_binding[:]
    capsys.readouterr()
    out = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu'])
    lines = capsys.readouterr().out.rstrip('\n').split('\n')
    assert [x.split(':')[0].split('!')[0] for x in lines] == ['Load generated data done', 'Evaluate done', 'mol_stable', 'atm_stable', 'JSD_CC_2A',
                                                              'JSD_All_12A', 'Atom type JS', 'wrote ' + str(tmp_path / 'eval_results' / 'quality.json')]
    assert 'sasa' not in out and sasa_binding == [('pack', None), ('quality_report', True)] * 2
    with pytest.raises(SystemExit, match='carries no pocket'):
        tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--sasa'])


def test_export_sdf_writes_only_the_molecules_that_are_buried_enough(sasa_binding, tmp_path):
    res = ringed_result(5, [6, 9, 14, 3], 3)
    res[2][3] = (res[2][3].astype(np.float32) + np.float32(40)).astype(np.float64)      # the last sample has left the pocket: nothing buried
    res[0][3] = res[2][3][-1]
    data = pocket_data(1)
    save_with_pockets(tmp_path, {4: res}, {4: data})
    pos, v, ptr, sizes = packed(res, -1)
    _, elem, _ = quality.pocket_kinds(data.protein_atom_feature, 'element')
    w = SR.sasa_report(pos, v, ptr, CLASS_Z, data.protein_pos.numpy(), elem, LIG_R, PROT_R, SR.directions(96))
    fa = quality.sasa_areas(w['free'], LIG_R, 96)[0, :, 0]
    share = quality.sasa_areas(w['free'] - w['bound'], LIG_R, 96)[0, :, 0] / fa
    assert share[3] == 0.0 and (share[:3] > 0).all()
    limit = float(np.sort(share)[2])                                            # two of the four reach it
    enough = share >= limit
    assert enough.sum() == 2
    tool = load_tool('export_sdf')
    out = tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'sdf'), '--device', 'cpu', '--min-buried-share', repr(limit)])
    assert out['result_4']['min_buried_share'] == 2 == out['result_4']['written']
    recs = parse_sdf(open(tmp_path / 'sdf' / 'result_4.sdf').read())
    assert [len(atoms) for _, atoms, _, _ in recs] == [n for n, ok in zip(sizes, enough) if ok]
    plain = tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'sdf2'), '--device', 'cpu'])
    assert plain['result_4']['written'] == 4 and 'min_buried_share' not in plain['result_4']
    everything = tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'sdf3'), '--device', 'cpu', '--min-buried-share', '0'])
    assert everything['result_4']['written'] == 4
    for bad in ('1.5', '-0.1'):
        with pytest.raises(SystemExit, match='is a share'):
            tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'sdf4'), '--device', 'cpu', '--min-buried-share', bad])
