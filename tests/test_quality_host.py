"""CPU-only checks of the sample-quality feature (targetdiff_amd.quality, td_quality_report's host side).

  1. tests/_quality_ref.py -- the numpy restatement the GPU tests use where no fixture can exist -- is pinned to every fixture made
     with the reference itself (tools/make_golden_quality.py): integers with array_equal, distributions bit for bit, Jensen-Shannon
     values through their squares (a divergence is a sum of <= 202 float64 terms of magnitude <= 1, rounding below 1e-13; the
     square root would amplify that near zero), identical inputs exactly 0.
  2. class tables, argument checks and the binding's signature; TD_ABI_VERSION stays 5.
  3. sample_quality's packing of a ragged 7-tuple and tools/evaluate_samples.py, with the binding patched by the restatement.
"""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import _quality_ref as QR
from conftest import ROOT, load_golden
from targetdiff_amd import capi, quality

CLASS_Z = quality.class_atomic_numbers('add_aromatic')
PROFILES = quality.default_profiles()
NAMES = quality.PROFILE_NAMES


def test_restatement_matches_reference_docked():
    g = load_golden('quality_docked.npz')
    r = QR.quality_report(g['pos'], g['v'], g['ptr'], CLASS_Z, PROFILES)
    QR.check_against_fixture(r, g)
    assert g['mol_stable'][0].tolist() == [1, 0, 0, 0, 0] and g['stable_atoms'][0, 0] == 25
    assert 'Br written as Cl' in str(g['note'])


def test_restatement_matches_reference_thresholds():
    g = load_golden('quality_thresholds.npz')
    assert g['ptr'].size == 426 and int(g['fp32_flips']) >= 100
    r = QR.quality_report(g['pos'], g['v'], g['ptr'], CLASS_Z, PROFILES)
    QR.check_against_fixture(r, g)
    assert set(g['nr_bonds'][0].tolist()) == {0, 1, 2, 3}


def test_restatement_matches_reference_sizes():
    g = load_golden('quality_sizes.npz')
    sizes = np.diff(g['ptr']).tolist()
    assert sizes[:8] == [0, 1, 2, 63, 64, 65, 130, 300] and sizes[8] > 2 * 256
    r = QR.quality_report(g['pos'], g['v'], g['ptr'], CLASS_Z, PROFILES, g['include'])
    QR.check_against_fixture(r, g)
    assert g['n_CC_2A'][2] == 0 and g['n_All_12A'][2] == 1            # an empty profile beside a filled one
    assert g['mol_stable'][:, 0].all() and not g['mol_stable'][:, 1].any()          # 0 atoms: stable; 1 atom: not


def test_restatement_matches_reference_trajectory():
    g = load_golden('quality_traj.npz')
    t = load_golden('sample_small_1000.npz')
    r = QR.quality_report(t['pos_traj'], t['v_traj'].astype(np.int64), g['ptr'], CLASS_Z, PROFILES)
    np.testing.assert_array_equal(r['stable_atoms'], g['stable_atoms'])
    np.testing.assert_array_equal(r['mol_stable'], g['mol_stable'])
    np.testing.assert_array_equal(r['hist'][:, 1, :101], g['hist_All_12A'])
    np.testing.assert_array_equal(r['hist'][:, 1].sum(1), g['n_All_12A'])
    np.testing.assert_array_equal(r['hist'][:, 0].sum(1), g['n_CC_2A'])
    np.testing.assert_array_equal(r['counts'], g['counts'])


@pytest.mark.parametrize('name', ['quality_docked.npz', 'quality_thresholds.npz', 'quality_sizes.npz'])
def test_jensen_shannon_matches_reference(name):
    g = load_golden(name)
    ref = load_golden('quality_reference_distributions.npz')
    assert ref['CC_2A'].shape == ref['All_12A'].shape == (101,) and ref['atom_type'].shape == (7,)
    r = QR.quality_report(g['pos'], g['v'], g['ptr'], CLASS_Z, PROFILES, g['include'] if 'include' in g else None)
    B = g['ptr'].size - 1
    rep = quality.QualityReport(r['mol_stable'].sum(1), r['stable_atoms'].sum(1), B, int(g['ptr'][-1]), r['hist'], r['counts'], PROFILES,
                                {k: ref[k] for k in ('CC_2A', 'All_12A', 'atom_type')})
    seen = 0
    for s in range(g['pos'].shape[0]):
        js = rep.js(s)
        for p, n in enumerate(NAMES):
            want = g['js_' + n][s]
            if np.isnan(want):
                assert js['JSD_' + n] is None and rep.distribution(n, s) is None
                continue
            seen += 1
            assert abs(js['JSD_' + n] ** 2 - want ** 2) <= 1e-12
            assert abs(QR.js_squared(ref[n], QR.normalised(r['hist'][s, p], 100)) - want ** 2) <= 1e-12
            np.testing.assert_array_equal(rep.distribution(n, s), g['dist_' + n][s])
        want = g['js_atom_type'][s]
        assert abs(js['atom_type_js'] ** 2 - want ** 2) <= 1e-12
        assert abs(QR.js_squared(ref['atom_type'], QR.atom_type_distribution(r['counts'][s])) - want ** 2) <= 1e-12
    assert seen >= 1
    # fractions as the reference forms them
    np.testing.assert_array_equal(rep.mol_stable, g['mol_stable'].sum(1) / float(B))
    np.testing.assert_array_equal(rep.atm_stable, g['stable_atoms'].sum(1) / float(g['ptr'][-1]))
    p = ref['All_12A']
    assert quality.jensenshannon(p, p) == 0.0 and QR.js_squared(p, p) == 0.0
    assert quality.jensenshannon(p, 4.0 * p) == 0.0                     # both are normalised first (a power of two: the same bits)
    q = np.zeros(101)
    q[0] = 1.0
    assert abs(quality.jensenshannon(q, np.roll(q, 1)) ** 2 - np.log(2.0)) <= 1e-12       # disjoint supports: ln 2
    # a report without reference distributions carries histograms and no distance
    bare = quality.QualityReport(r['mol_stable'].sum(1), r['stable_atoms'].sum(1), B, int(g['ptr'][-1]), r['hist'], r['counts'], PROFILES)
    assert bare.js(0) == {'JSD_CC_2A': None, 'JSD_All_12A': None, 'atom_type_js': None}


def test_class_tables():
    assert quality.class_atomic_numbers('basic') == (1, 6, 7, 8, 9, 15, 16, 17)
    aro = quality.class_atomic_numbers('add_aromatic')
    assert len(aro) == 13 and aro == (1, 6, 6, 7, 7, 8, 8, 9, 15, 15, 16, 16, 17)
    assert quality.class_atomic_numbers([6, 8, 17]) == (6, 8, 17)
    with pytest.raises(ValueError):
        quality.class_atomic_numbers('full')
    with pytest.raises(ValueError, match='35'):
        quality.class_atomic_numbers([6, 35])


def test_argument_checks_before_any_device_work():
    pos = torch.zeros(2, 5, 3)
    v = torch.zeros(2, 5, dtype=torch.int64)
    ptr = torch.tensor([0, 2, 5], dtype=torch.int32)
    ok = lambda **kw: capi._quality_inputs(**dict(dict(pos=pos, v=v, ligand_ptr=ptr, class_z=CLASS_Z, include=None, profiles=PROFILES), **kw))
    S, Nl, B, cz, prof = ok()
    assert (S, Nl, B) == (2, 5, 2) and cz.dtype == np.int32 and len(prof) == 2 and prof[0][3].size == 100
    with pytest.raises(ValueError, match='35'):                                  # an element outside the table (the reference: KeyError)
        ok(class_z=[6, 35])
    with pytest.raises(ValueError, match='prefix offsets'):
        ok(ligand_ptr=torch.tensor([0, 3, 2], dtype=torch.int32))
    with pytest.raises(ValueError, match='prefix offsets'):
        ok(ligand_ptr=torch.tensor([0, 2, 4], dtype=torch.int32))
    with pytest.raises(ValueError, match=r'v must be in \[0, 13\)'):
        ok(v=torch.full((2, 5), 13, dtype=torch.int64))
    with pytest.raises(ValueError, match='at most 4'):
        ok(profiles=PROFILES + PROFILES + PROFILES[:1])
    with pytest.raises(ValueError, match='edges'):
        ok(profiles=((0, 0, 12.0, np.linspace(0, 12, 128)),))
    with pytest.raises(ValueError, match='ascending'):
        ok(profiles=((0, 0, 12.0, [0.0, 2.0, 1.0]),))
    with pytest.raises(ValueError):
        ok(profiles=((35, 0, 12.0, [0.0, 1.0]),))
    with pytest.raises(ValueError):
        ok(class_z=list(range(65)))
    with pytest.raises(ValueError):
        ok(include=torch.ones(2, 3, dtype=torch.bool))
    with pytest.raises(ValueError):
        ok(pos=torch.zeros(2, 5, 2))
    # float64 positions: only what round-trips through fp32
    p32 = torch.randn(4, 3)
    assert quality._fp32_positions(p32.double(), 'cpu').dtype == torch.float32
    with pytest.raises(ValueError, match='round-trip'):
        quality._fp32_positions(p32.double() + 1e-12, 'cpu')
    with pytest.raises(ValueError):
        quality._fp32_positions(p32.half(), 'cpu')
    with pytest.raises(ValueError, match='one of the two'):
        quality._pack(p32, torch.zeros(4, dtype=torch.int64), None, None, 'cpu')
    with pytest.raises(ValueError, match='sorted'):
        quality._pack(p32, torch.zeros(4, dtype=torch.int64), torch.tensor([0, 1, 0, 1]), None, 'cpu')
    _, _, lp = quality._pack(p32, torch.zeros(4, dtype=torch.int64), torch.tensor([0, 0, 2, 2]), None, 'cpu')
    assert lp.tolist() == [0, 2, 2, 4] and lp.dtype == torch.int32
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU path'):
            capi.quality_report(pos, v, ptr, CLASS_Z)


def test_library_entry_point_and_its_checks():
    """the signature in capi.SIGNATURES, the export, the host-side refusals of the C ABI, and the ABI version"""
    lib = capi.load_library()
    assert hasattr(lib, 'td_quality_report') and len(capi.SIGNATURES['td_quality_report'][1]) == 17
    assert lib.td_abi_version() == capi.ABI_VERSION == 5
    assert ctypes.sizeof(capi.TdPairProfile) == 32
    header = open(os.path.join(ROOT, 'include', 'targetdiff_hip.h')).read()
    assert 'int td_quality_report(' in header and '#define TD_ABI_VERSION 5' in header
    cz = (ctypes.c_int32 * 13)(*CLASS_Z)
    prof = (capi.TdPairProfile * 5)()
    call = lambda S=1, B=1, K=13, P=0, table=cz: lib.td_quality_report(None, None, None, S, 0, B, table, K, None, ctypes.cast(prof, ctypes.c_void_p),
                                                                      P, None, None, None, None, None, None)
    assert call(S=-1) == -1
    assert call(K=0) == -1 and call(K=65) == -1 and b'class table' in lib.td_last_error()
    assert call(P=5) == -1 and b'pair profiles' in lib.td_last_error()
    assert call(S=1 << 20, B=1 << 20) == -1
    bad = (ctypes.c_int32 * 13)(*([6] * 12 + [35]))
    assert call(table=bad) == -1 and b'atomic number 35' in lib.td_last_error()
    prof[0] = capi.TdPairProfile(6, 6, 2.0, 128, 0, None)
    assert call(P=1) == -1 and b'edges' in lib.td_last_error()
    prof[0] = capi.TdPairProfile(6, 35, 2.0, 100, 0, 8)
    assert call(P=1) == -1 and b'atomic number' in lib.td_last_error()
    assert call() == -1 and b'null pointer' in lib.td_last_error()              # S = B = 1 without outputs


@pytest.fixture
def numpy_binding(monkeypatch):
    calls = []

    def binding(*a, **kw):
        calls.append((a, kw))
        return QR.torch_binding(*a, **kw)

    monkeypatch.setattr(capi, 'quality_report', binding)
    return calls


def ragged_result(seed, sizes, T):
    """a 7-tuple as sample_diffusion_ligand returns it: float64 positions holding fp32 values, one entry per sample"""
    rng = np.random.default_rng(seed)
    pos_traj = [rng.normal(0, 1.2, (T, n, 3)).astype(np.float32).astype(np.float64) for n in sizes]
    v_traj = [rng.integers(0, 13, (T, n)) for n in sizes]
    return ([p[-1] for p in pos_traj], [v[-1] for v in v_traj], pos_traj, v_traj, [], [], [0.0])


def expected_report(result, frames, include=None):
    pos = np.concatenate([p[frames].astype(np.float32) for p in result[2]], axis=1)
    v = np.concatenate([x[frames] for x in result[3]], axis=1)
    ptr = np.cumsum([0] + [p.shape[1] for p in result[2]])
    r = QR.quality_report(pos, v, ptr, CLASS_Z, PROFILES)
    if include == 'stable':
        r2 = QR.quality_report(pos, v, ptr, CLASS_Z, PROFILES, r['mol_stable'])
        r['hist'], r['counts'] = r2['hist'], r2['counts']
    return r


def test_sample_quality_packs_a_ragged_result(numpy_binding):
    sizes, T = [7, 3, 12, 1, 9], 4
    res = ragged_result(3, sizes, T)
    for eval_step, frames in ((-1, slice(T - 1, T)), (1, slice(1, 2)), ('all', slice(0, T))):
        rep = quality.sample_quality(res, eval_step, device='cpu', reference={})
        want = expected_report(res, frames)
        np.testing.assert_array_equal(rep.hist, want['hist'])
        np.testing.assert_array_equal(rep.counts, want['counts'])
        np.testing.assert_array_equal(rep.stable_mols, want['mol_stable'].sum(1))
        np.testing.assert_array_equal(rep.stable_atoms, want['stable_atoms'].sum(1))
        assert rep.n_samples == 5 and rep.n_atoms == 32 and rep.num_frames == (T if eval_step == 'all' else 1)
        np.testing.assert_array_equal(rep.atm_stable, want['stable_atoms'].sum(1) / 32.0)
    assert len(numpy_binding) == 3                                       # one call per report
    (pos, v, ptr, *_), _ = numpy_binding[-1]
    assert tuple(pos.shape) == (T, 32, 3) and pos.dtype == torch.float32 and tuple(v.shape) == (T, 32) and ptr.tolist() == [0, 7, 10, 22, 23, 32]
    # the result_{i}.pt dictionary form, 'stable' (two calls) and an explicit mask
    d = {'pred_ligand_pos_traj': res[2], 'pred_ligand_v_traj': res[3]}
    rep = quality.sample_quality(d, 'all', include='stable', device='cpu', reference={})
    want = expected_report(res, slice(0, T), 'stable')
    np.testing.assert_array_equal(rep.hist, want['hist'])
    np.testing.assert_array_equal(rep.counts, want['counts'])
    np.testing.assert_array_equal(rep.stable_atoms, want['stable_atoms'].sum(1))
    assert len(numpy_binding) == 5
    mask = np.zeros((T, 5), bool)
    mask[:, 2] = True
    rep = quality.sample_quality(res, 'all', include=mask, device='cpu', reference={})
    only = QR.quality_report(np.stack([p.astype(np.float32) for p in res[2][2]]), res[3][2], [0, 12], CLASS_Z, PROFILES)
    np.testing.assert_array_equal(rep.hist, only['hist'])
    with pytest.raises(ValueError, match='round-trip'):
        quality.sample_quality((None, None, [res[2][0] + 1e-9], [res[3][0]], [], [], []), device='cpu')
    # stability() on one frame and on a stack
    ok, ns, nb = quality.stability(res[2][0][-1], res[3][0][-1], batch_ligand=np.zeros(7, np.int64), return_nr_bonds=True, device='cpu')
    one = QR.molecule(res[2][0][-1].astype(np.float32), np.asarray(CLASS_Z)[res[3][0][-1]])
    assert bool(ok[0]) == one[0] and int(ns[0]) == one[1] and nb.tolist() == one[2].tolist()
    ok2, ns2 = quality.stability(res[2][0], res[3][0], ligand_ptr=[0, 7], device='cpu')
    assert tuple(ok2.shape) == (T, 1) and ok2.dtype == torch.bool and int(ns2[-1, 0]) == one[1]


def test_evaluate_samples_tool(numpy_binding, tmp_path, capsys):
    spec = importlib.util.spec_from_file_location('evaluate_samples', os.path.join(ROOT, 'tools', 'evaluate_samples.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    results = {10: ragged_result(5, [6, 9], 3), 2: ragged_result(6, [4, 11, 5], 3)}
    for i, r in results.items():
        torch.save({'data': None, 'pred_ligand_pos': r[0], 'pred_ligand_v': r[1], 'pred_ligand_pos_traj': r[2], 'pred_ligand_v_traj': r[3],
                    'time': r[6]}, tmp_path / f'result_{i}.pt')
    assert [os.path.basename(f) for f in tool.result_files(str(tmp_path))] == ['result_2.pt', 'result_10.pt']       # numeric order
    gold = load_golden('quality_reference_distributions.npz')
    out = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--reference_npz', os.path.join(ROOT, 'tests', 'golden',
                                                                                                        'quality_reference_distributions.npz')])
    text = capsys.readouterr().out
    for name in ('mol_stable:\t', 'atm_stable:\t', 'JSD_CC_2A:\t', 'JSD_All_12A:\t', 'Atom type JS: '):
        assert name in text, name
    want = [expected_report(results[i], slice(2, 3)) for i in (2, 10)]
    hist = sum(w['hist'] for w in want)
    assert out['num_samples'] == 5 and out['num_atoms'] == 35 and out['num_examples'] == 2
    assert out['atm_stable'] == sum(int(w['stable_atoms'].sum()) for w in want) / 35.0
    assert out['mol_stable'] == sum(int(w['mol_stable'].sum()) for w in want) / 5.0
    assert out['hist']['All_12A'] == hist[0, 1, :101].tolist()
    assert abs(out['JSD_All_12A'] ** 2 - QR.js_squared(gold['All_12A'], QR.normalised(hist[0, 1], 100))) <= 1e-12
    saved = json.load(open(tmp_path / 'eval_results' / 'quality.json'))
    assert saved['mol_stable'] == out['mol_stable'] and 'curve' not in saved
    # the curve, first example only
    out = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--eval_step', 'all', '--eval_num_examples', '1'])
    assert out['num_examples'] == 1 and len(out['curve']) == 3 and out['curve'][-1]['atm_stable'] == out['atm_stable']
    assert out['JSD_All_12A'] is None or quality.reference_distributions() is not None
    w = expected_report(results[2], slice(0, 3))
    assert [c['atm_stable'] for c in out['curve']] == (w['stable_atoms'].sum(1) / 20.0).tolist()
