"""CPU-only checks of the bond graph (targetdiff_amd.quality.bond_graph, td_bond_graph / td_bond_list's host side).

  1. tests/_bonds_ref.py -- the numpy restatement the GPU tests use where no fixture can exist -- is pinned to every fixture made with
     the reference itself (tools/make_golden_bonds.py): integers and float64 lengths with array_equal, distributions bit for bit,
     Jensen-Shannon values through their squares (1e-12, the tolerance tests/test_quality_host.py derives).
  2. the ABI surface and the refusals of the library and of the binding; TD_ABI_VERSION stays 5.
  3. sample_connectivity, sample_quality(include='complete'), tools/evaluate_samples.py --connectivity and tools/export_sdf.py with
     the bindings patched by the restatement; the written SD file parses back to the same atoms, coordinates and bonds.
"""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import _bonds_ref as BR
import _quality_ref as QR
from conftest import ROOT, load_golden
from targetdiff_amd import capi, molfile, quality

CLASS_Z = quality.class_atomic_numbers('add_aromatic')
AROMATIC = quality.class_aromatic('add_aromatic')
PROFILES = quality.default_bond_profiles()


def fixture_pack(name):
    g = load_golden(f'bonds_{name}.npz')
    q = g if 'pos' in g else load_golden(f'quality_{name}.npz')
    return g, q['pos'], q['v'], q['ptr'], (g['include'] if 'include' in g else None)


def test_tables_match_the_reference_configuration():
    ref = load_golden('bonds_reference_distributions.npz')
    assert quality.BOND_TYPES == BR.BOND_TYPES == tuple(tuple(int(x) for x in t) for t in ref['bond_types'])
    np.testing.assert_array_equal(PROFILES[0][3], ref['distance_bins'])                 # formed here as the reference forms them
    np.testing.assert_array_equal(BR.DISTANCE_BINS, ref['distance_bins'])
    assert ref['distributions'].shape == (8, len(ref['distance_bins']) + 1) and len(ref['distance_bins']) <= 127
    assert [c for c, a in enumerate(AROMATIC) if a] == [2, 4, 6, 9, 11] and AROMATIC == BR.CLASS_AROMATIC
    assert not any(quality.class_aromatic('basic')) and len(quality.class_aromatic('basic')) == 8
    assert quality.class_aromatic([6, 8, 17]) == (False, False, False)
    with pytest.raises(ValueError):
        quality.class_aromatic('full')
    assert quality.bond_type_name((6, 7, 4)) == '6-7|4'
    assert quality.reference_bond_distributions() is None or set(quality.reference_bond_distributions()) == set(quality.BOND_TYPES)


@pytest.mark.parametrize('name', ['docked', 'thresholds', 'sizes'])
def test_restatement_matches_reference(name):
    g, pos, v, ptr, include = fixture_pack(name)
    r = BR.bond_graph(pos, v, ptr, CLASS_Z, AROMATIC, PROFILES, include)
    BR.check_against_fixture(r, g)
    # the orders of all pairs, bonded or not, in (frame, molecule, i, j) order
    orders = [BR.molecule(pos[s, a:b], v[s, a:b], CLASS_Z, AROMATIC)['order'][np.triu_indices(b - a, 1)]
              for s in range(pos.shape[0]) for a, b in zip(ptr[:-1], ptr[1:])]
    np.testing.assert_array_equal(np.concatenate(orders), g['pair_order'])
    assert r['bond_ptr'][-1] == len(r['bond_order']) == g['n_bonds'].sum()
    if name == 'docked':
        rings = r['n_bonds'] - np.diff(ptr)[None] + r['n_fragments']
        assert (r['n_bonds'][0, 0], r['n_fragments'][0, 0], rings[0, 0]) == (27, 1, 3)
        assert r['n_fragments'][0, 1:].tolist() == [3, 3, 8, 16]
        assert 4 in r['bond_category'] and set(r['bond_order'].tolist()) == {1, 2, 3}
    if name == 'thresholds':
        assert set(r['n_fragments'][0].tolist()) == {1, 2}
    if name == 'sizes':
        assert r['n_fragments'][:, 0].tolist() == [0, 0, 0] and r['largest_fragment'][:, 0].tolist() == [0, 0, 0]


@pytest.mark.parametrize('name', ['docked', 'sizes'])
def test_jensen_shannon_matches_reference(name):
    g, pos, v, ptr, include = fixture_pack(name)
    ref = load_golden('bonds_reference_distributions.npz')
    reference = {t: d for t, d in zip(quality.BOND_TYPES, ref['distributions'])}
    r = BR.bond_graph(pos, v, ptr, CLASS_Z, AROMATIC, PROFILES, include)
    nf, big, n = r['n_fragments'].astype(np.int64), r['largest_fragment'].astype(np.float64), np.diff(ptr).astype(np.float64)
    share = np.divide(big, n[None], out=np.zeros_like(big), where=n[None] > 0)
    rep = quality.ConnectivityReport((nf == 1).sum(1), nf.sum(1), share.sum(1), len(n), int((n > 0).sum()), r['bond_hist'], PROFILES, reference)
    seen = 0
    for s in range(pos.shape[0]):
        js = rep.js(s)
        for p, t in enumerate(quality.BOND_TYPES):
            want = g['profile_js'][s, p]
            key = 'JSD_' + quality.bond_type_name(t)
            if np.isnan(want):
                assert js[key] is None and rep.distribution(t, s) is None and g['profile_n'][s, p] == 0
                continue
            seen += 1
            assert abs(js[key] ** 2 - want ** 2) <= 1e-12
            np.testing.assert_array_equal(rep.distribution(t, s), g['profile_dist'][s, p])
    assert seen >= 1
    assert rep.complete.tolist() == ((nf == 1).sum(1) / float(len(n))).tolist()
    bare = quality.ConnectivityReport((nf == 1).sum(1), nf.sum(1), share.sum(1), len(n), int((n > 0).sum()), r['bond_hist'], PROFILES)
    assert all(x is None for x in bare.js(0).values()) and len(bare.js(0)) == 8


def test_library_entry_points_and_their_checks():
    lib = capi.load_library()
    assert hasattr(lib, 'td_bond_graph') and len(capi.SIGNATURES['td_bond_graph'][1]) == 19
    assert hasattr(lib, 'td_bond_list') and len(capi.SIGNATURES['td_bond_list'][1]) == 16
    assert lib.td_abi_version() == capi.ABI_VERSION == 5
    assert ctypes.sizeof(capi.TdBondProfile) == 24
    header = open(os.path.join(ROOT, 'include', 'targetdiff_hip.h')).read()
    assert 'int td_bond_graph(' in header and 'int td_bond_list(' in header and '#define TD_ABI_VERSION 5' in header
    cz = (ctypes.c_int32 * 13)(*CLASS_Z)
    prof = (capi.TdBondProfile * 17)()
    call = lambda S=1, B=1, K=13, P=0, table=cz: lib.td_bond_graph(None, None, None, S, 0, B, table, K, None, None, ctypes.cast(prof, ctypes.c_void_p),
                                                                  P, None, None, None, None, None, None, None)
    assert call(S=-1) == -1 and b'bad argument' in lib.td_last_error()
    assert call(B=-1) == -1
    assert call(K=0) == -1 and call(K=65) == -1 and b'class table' in lib.td_last_error()
    assert call(P=17) == -1 and b'bond profiles' in lib.td_last_error()
    assert call(S=1 << 20, B=1 << 20) == -1
    bad = (ctypes.c_int32 * 13)(*([6] * 12 + [35]))
    assert call(table=bad) == -1 and b'atomic number 35' in lib.td_last_error()
    prof[0] = capi.TdBondProfile(6, 6, 1, 128, 8)
    assert call(P=1) == -1 and b'edges' in lib.td_last_error()
    prof[0] = capi.TdBondProfile(6, 6, 1, 0, 8)
    assert call(P=1) == -1 and b'edges' in lib.td_last_error()
    prof[0] = capi.TdBondProfile(6, 6, 5, 100, 8)
    assert call(P=1) == -1 and b'category' in lib.td_last_error()
    prof[0] = capi.TdBondProfile(6, 6, -1, 100, 8)
    assert call(P=1) == -1 and b'category' in lib.td_last_error()
    prof[0] = capi.TdBondProfile(6, 35, 1, 100, 8)
    assert call(P=1) == -1 and b'atomic number' in lib.td_last_error()
    assert call() == -1 and b'null pointer' in lib.td_last_error()              # S = B = 1 without outputs
    lst = lambda S=1, B=1, K=13, nb=1: lib.td_bond_list(None, None, None, S, 0, B, cz, K, None, None, nb, None, None, None, None, None)
    assert lst(S=-1) == -1 and lst(K=65) == -1 and lst(nb=-1) == -1 and b'n_bonds' in lib.td_last_error()
    assert lst() == -1 and b'null pointer' in lib.td_last_error()
    assert lst(S=0) == 0 and call(S=0) == 0                                      # no work: nothing is touched


def test_binding_refusals_before_any_device_work():
    pos = torch.zeros(2, 5, 3)
    v = torch.zeros(2, 5, dtype=torch.int64)
    ptr = torch.tensor([0, 2, 5], dtype=torch.int32)
    ok = lambda **kw: capi._bond_inputs(**dict(dict(pos=pos, v=v, ligand_ptr=ptr, class_z=CLASS_Z, class_aromatic=AROMATIC, include=None,
                                                   profiles=PROFILES), **kw))
    S, Nl, B, cz, aro, prof = ok()
    assert (S, Nl, B) == (2, 5, 2) and cz.dtype == np.int32 and aro.dtype == np.uint8 and aro.tolist() == [int(a) for a in AROMATIC]
    assert len(prof) == 8 and prof[2][:3] == (6, 6, 4)
    assert ok(class_aromatic=None)[4] is None
    big = dict(pos=torch.zeros(1, 513, 3), v=torch.zeros(1, 513, dtype=torch.int64))
    with pytest.raises(ValueError, match='513 atoms'):
        ok(ligand_ptr=torch.tensor([0, 513], dtype=torch.int32), **big)
    assert ok(ligand_ptr=torch.tensor([0, 1, 513], dtype=torch.int32), **big)[2] == 2          # 512 atoms pass
    with pytest.raises(ValueError, match='prefix offsets'):
        ok(ligand_ptr=torch.tensor([0, 3, 2], dtype=torch.int32))
    with pytest.raises(ValueError, match='prefix offsets'):
        ok(ligand_ptr=torch.tensor([0, 2, 4], dtype=torch.int32))
    with pytest.raises(ValueError, match='at most 16'):
        ok(profiles=PROFILES + PROFILES + PROFILES[:1])
    with pytest.raises(ValueError, match='ascending'):
        ok(profiles=((6, 6, 1, [1.0, 2.0, 1.5]),))
    with pytest.raises(ValueError, match='edges'):
        ok(profiles=((6, 6, 1, np.linspace(1, 2, 128)),))
    with pytest.raises(ValueError, match='category'):
        ok(profiles=((6, 6, 5, [1.0, 2.0]),))
    with pytest.raises(ValueError):
        ok(profiles=((6, 35, 1, [1.0, 2.0]),))
    with pytest.raises(ValueError, match='one flag per class'):
        ok(class_aromatic=[True, False])
    with pytest.raises(ValueError, match=r'v must be in \[0, 13\)'):
        ok(v=torch.full((2, 5), 13, dtype=torch.int64))
    with pytest.raises(ValueError):
        ok(include=torch.ones(2, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match='bond_ptr'):
        capi.bond_list(pos, v, ptr, CLASS_Z, AROMATIC, torch.zeros(4, dtype=torch.int64))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU path'):
            capi.bond_graph(pos, v, ptr, CLASS_Z, AROMATIC)
        with pytest.raises(RuntimeError, match='no CPU path'):
            capi.bond_list(pos, v, ptr, CLASS_Z, AROMATIC, torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="'complete'"):
        quality.sample_connectivity(([], [], [np.zeros((1, 2, 3))], [np.zeros((1, 2), np.int64)], [], [], []), include='stable', device='cpu')


@pytest.fixture
def numpy_binding(monkeypatch):
    calls = []

    def patched(name, fn):
        def binding(*a, **kw):
            calls.append((name, a, kw))
            return fn(*a, **kw)
        return binding

    monkeypatch.setattr(capi, 'bond_graph', patched('bond_graph', BR.torch_bond_graph))
    monkeypatch.setattr(capi, 'bond_list', patched('bond_list', BR.torch_bond_list))
    monkeypatch.setattr(capi, 'quality_report', patched('quality_report', QR.torch_binding))
    return calls


def ragged_result(seed, sizes, T):
    """a 7-tuple as sample_diffusion_ligand returns it: compact clouds, so that bonds, rings and fragments all occur"""
    rng = np.random.default_rng(seed)
    pos_traj = [rng.normal(0, 1.2, (T, n, 3)).astype(np.float32).astype(np.float64) for n in sizes]
    v_traj = [rng.integers(0, 13, (T, n)) for n in sizes]
    return ([p[-1] for p in pos_traj], [v[-1] for v in v_traj], pos_traj, v_traj, [], [], [0.0])


def packed(result, frames):
    pos = np.concatenate([p[frames].astype(np.float32) for p in result[2]], axis=1)
    v = np.concatenate([x[frames] for x in result[3]], axis=1)
    return pos, v, np.cumsum([0] + [p.shape[1] for p in result[2]])


def test_sample_connectivity_packs_a_ragged_result(numpy_binding):
    sizes, T = [7, 3, 12, 1, 9, 2], 4
    res = ragged_result(3, sizes, T)
    for eval_step, frames in ((-1, slice(T - 1, T)), (1, slice(1, 2)), ('all', slice(0, T))):
        pos, v, ptr = packed(res, frames)
        want = BR.bond_graph(pos, v, ptr, CLASS_Z, AROMATIC, PROFILES)
        con = quality.sample_connectivity(res, eval_step, device='cpu', reference={})
        np.testing.assert_array_equal(con.bond_hist, want['bond_hist'])
        np.testing.assert_array_equal(con.n_complete, (want['n_fragments'] == 1).sum(1))
        np.testing.assert_array_equal(con.mean_fragments, want['n_fragments'].sum(1) / 6.0)
        np.testing.assert_array_equal(con.mean_largest_share, (want['largest_fragment'] / np.asarray(sizes, np.float64)[None]).sum(1) / 6.0)
        assert con.num_frames == (T if eval_step == 'all' else 1) and con.n_samples == 6
        # include='complete': the bond graph's flags are the mask of both reports
        mask = want['n_fragments'] == 1
        con2 = quality.sample_connectivity(res, eval_step, include='complete', device='cpu', reference={})
        np.testing.assert_array_equal(con2.bond_hist, BR.bond_graph(pos, v, ptr, CLASS_Z, AROMATIC, PROFILES, mask)['bond_hist'])
        np.testing.assert_array_equal(con2.n_complete, con.n_complete)
        rep = quality.sample_quality(res, eval_step, include='complete', device='cpu', reference={})
        wq = QR.quality_report(pos, v, ptr, CLASS_Z, quality.default_profiles(), mask)
        np.testing.assert_array_equal(rep.hist, wq['hist'])
        np.testing.assert_array_equal(rep.counts, wq['counts'])
        np.testing.assert_array_equal(rep.stable_atoms, wq['stable_atoms'].sum(1))
        np.testing.assert_array_equal(rep.hist, quality.sample_quality(res, eval_step, include=mask, device='cpu', reference={}).hist)
    assert 0 < mask.sum() < mask.size                                         # the mask selects something and leaves something out
    name, (pos_t, v_t, ptr_t, *_), _ = numpy_binding[-1]
    assert name == 'quality_report' and tuple(pos_t.shape) == (T, 34, 3) and ptr_t.tolist() == [0, 7, 10, 22, 23, 32, 34]
    d = {'pred_ligand_pos_traj': res[2], 'pred_ligand_v_traj': res[3]}
    np.testing.assert_array_equal(quality.sample_connectivity(d, 'all', device='cpu', reference={}).bond_hist, con.bond_hist)
    # quality.bond_graph on one frame: fragments, rings and the bond list
    pos, v, ptr = packed(res, slice(T - 1, T))
    g = quality.bond_graph(pos[0], v[0], ligand_ptr=ptr, return_fragments=True, return_bonds=True, device='cpu')
    want = BR.bond_graph(pos, v, ptr, CLASS_Z, AROMATIC, PROFILES)
    np.testing.assert_array_equal(g.fragment.numpy(), want['fragment'])
    np.testing.assert_array_equal(g.rings.numpy(), want['n_bonds'] - np.diff(ptr)[None] + want['n_fragments'])
    np.testing.assert_array_equal(g.complete.numpy(), want['n_fragments'] == 1)
    np.testing.assert_array_equal(g.bond_atoms.numpy(), want['bond_atoms'])
    atoms, order, cat, length = g.molecule_bonds(-1, 2)
    a, b = want['bond_ptr'][2:4]
    np.testing.assert_array_equal(atoms, want['bond_atoms'][a:b] - 10)
    np.testing.assert_array_equal(length, want['bond_length'][a:b])
    batch = np.repeat(np.arange(6), sizes)
    g2 = quality.bond_graph(pos, v, batch_ligand=batch, device='cpu')
    np.testing.assert_array_equal(g2.n_bonds.numpy(), want['n_bonds'])
    assert g2.fragment is None and g2.bond_atoms is None


def parse_sdf(text):
    """[(name, [(symbol, x, y, z)], [(i, j, type)], {property: value})] of V2000 records"""
    out = []
    for rec in text.split('$$$$\n')[:-1]:
        lines = rec.split('\n')
        na, nb = int(lines[3][0:3]), int(lines[3][3:6])
        assert lines[3].rstrip().endswith('V2000')
        atoms = [(ln[31:34].strip(), float(ln[0:10]), float(ln[10:20]), float(ln[20:30])) for ln in lines[4:4 + na]]
        bonds = [(int(ln[0:3]) - 1, int(ln[3:6]) - 1, int(ln[6:9])) for ln in lines[4 + na:4 + na + nb]]
        assert lines[4 + na + nb] == 'M  END'
        rest = lines[5 + na + nb:]
        props = {rest[k][4:-1]: rest[k + 1] for k in range(0, len(rest) - 1, 3) if rest[k].startswith('>  <')}
        out.append((lines[0], atoms, bonds, props))
    return out


def load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'tools', name + '.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def save_results(tmp_path, results):
    for i, r in results.items():
        torch.save({'data': None, 'pred_ligand_pos': r[0], 'pred_ligand_v': r[1], 'pred_ligand_pos_traj': r[2], 'pred_ligand_v_traj': r[3],
                    'time': r[6]}, tmp_path / f'result_{i}.pt')


def test_export_sdf_tool_round_trips(numpy_binding, tmp_path, capsys):
    tool = load_tool('export_sdf')
    results = {10: ragged_result(5, [6, 9, 14], 3), 2: ragged_result(6, [4, 11, 5], 3)}
    save_results(tmp_path, results)
    sym = np.asarray([molfile.ELEMENT_SYMBOLS[z] for z in CLASS_Z])
    out = tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'sdf'), '--device', 'cpu'])
    assert list(out) == ['result_2', 'result_10'] and 'result_10.sdf' in capsys.readouterr().out
    for i, res in results.items():
        pos, v, ptr = packed(res, slice(2, 3))
        want = BR.bond_graph(pos, v, ptr, CLASS_Z, AROMATIC)
        recs = parse_sdf(open(tmp_path / 'sdf' / f'result_{i}.sdf').read())
        assert len(recs) == len(res[2]) == out[f'result_{i}']['written'] and out[f'result_{i}']['complete'] == int((want['n_fragments'] == 1).sum())
        for g, (name, atoms, bonds, props) in enumerate(recs):
            a, b = ptr[g], ptr[g + 1]
            assert name == f'sample_{g}' and [s for s, *_ in atoms] == sym[v[0, a:b]].tolist()
            np.testing.assert_array_equal(np.array([xyz for _, *xyz in atoms]), np.round(pos[0, a:b].astype(np.float64), 4))
            k0, k1 = want['bond_ptr'][g], want['bond_ptr'][g + 1]
            assert bonds == [(int(i - a), int(j - a), int(c)) for (i, j), c in zip(want['bond_atoms'][k0:k1], want['bond_category'][k0:k1])]
            assert int(props['n_fragments']) == want['n_fragments'][0, g]
    # --only-complete and --largest-fragment, first frame
    out = tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'sdf2'), '--device', 'cpu', '--eval_step', '0', '--only-complete',
                     '--largest-fragment', '--eval_num_examples', '1'])
    assert list(out) == ['result_2']
    pos, v, ptr = packed(results[2], slice(0, 1))
    want = BR.bond_graph(pos, v, ptr, CLASS_Z, AROMATIC)
    assert out['result_2']['written'] == int((want['n_fragments'] == 1).sum())
    out = tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'sdf3'), '--device', 'cpu', '--largest-fragment'])
    for i, res in results.items():
        pos, v, ptr = packed(res, slice(2, 3))
        want = BR.bond_graph(pos, v, ptr, CLASS_Z, AROMATIC)
        recs = parse_sdf(open(tmp_path / 'sdf3' / f'result_{i}.sdf').read())
        assert [len(r[1]) for r in recs] == want['largest_fragment'][0].tolist()
        for g, (_, atoms, bonds, _p) in enumerate(recs):
            lab = want['fragment'][0, ptr[g]:ptr[g + 1]]
            keep = lab == np.argmax(np.bincount(lab))
            assert [s for s, *_ in atoms] == sym[v[0, ptr[g]:ptr[g + 1]][keep]].tolist()
            assert len(bonds) >= len(atoms) - 1 and all(0 <= i < j < len(atoms) for i, j, _ in bonds)          # one connected piece
    with pytest.raises(ValueError):
        molfile.write_sdf(tmp_path / 'bad.sdf', [dict(symbols=['C'], pos=np.zeros((1, 3)), bonds=[(0, 1, 1)])])
    with pytest.raises(ValueError):
        molfile.write_sdf(tmp_path / 'bad.sdf', [dict(symbols=['C', 'C'], pos=np.zeros((2, 3)), bonds=[(0, 1, 5)])])


def test_evaluate_samples_connectivity(numpy_binding, tmp_path, capsys):
    tool = load_tool('evaluate_samples')
    results = {10: ragged_result(5, [6, 9], 3), 2: ragged_result(6, [4, 11, 5], 3)}
    save_results(tmp_path, results)
    ref = load_golden('bonds_reference_distributions.npz')
    q = load_golden('quality_reference_distributions.npz')
    npz = tmp_path / 'reference.npz'
    np.savez(npz, CC_2A=q['CC_2A'], All_12A=q['All_12A'], atom_type=q['atom_type'], bond_types=ref['bond_types'], bond_distributions=ref['distributions'])
    base = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--reference_npz', str(npz)])
    assert 'connectivity' not in base and 'complete:' not in capsys.readouterr().out          # the default output is unchanged
    out = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--reference_npz', str(npz), '--connectivity', '--eval_step', 'all'])
    text = capsys.readouterr().out
    for name in ('complete:\t', 'mean_fragments:\t', 'mean_largest_share:\t', 'JSD_6-6|1:\t', 'JSD_6-8|2:\t'):
        assert name in text, name
    want = [BR.bond_graph(*packed(results[i], slice(0, 3)), CLASS_Z, AROMATIC, PROFILES) for i in (2, 10)]
    nf = np.concatenate([w['n_fragments'] for w in want], axis=1)
    con = out['connectivity']
    assert [c['complete'] for c in con['curve']] == ((nf == 1).sum(1) / 5.0).tolist() and con['complete'] == con['curve'][-1]['complete']
    assert [c['mean_fragments'] for c in con['curve']] == (nf.sum(1) / 5.0).tolist()
    hist = sum(w['bond_hist'] for w in want)
    assert con['bond_hist']['6-6|1'] == hist[-1, 0, :len(BR.DISTANCE_BINS) + 1].tolist()
    for p, t in enumerate(quality.BOND_TYPES):
        key = 'JSD_' + quality.bond_type_name(t)
        if hist[-1, p].sum() == 0:
            assert con[key] is None
        else:
            assert abs(con[key] ** 2 - QR.js_squared(ref['distributions'][p], QR.normalised(hist[-1, p], len(BR.DISTANCE_BINS)))) <= 1e-12
    assert {k: base[k] for k in ('mol_stable', 'atm_stable', 'JSD_All_12A')} == {k: out[k] for k in ('mol_stable', 'atm_stable', 'JSD_All_12A')}
    saved = json.load(open(tmp_path / 'eval_results' / 'quality.json'))
    assert saved['connectivity']['complete'] == con['complete']
    # --include complete: the pair profiles over the one-piece samples only
    inc = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--include', 'complete'])
    wq = []
    for i in (2, 10):
        pos, v, ptr = packed(results[i], slice(2, 3))
        mask = BR.bond_graph(pos, v, ptr, CLASS_Z, AROMATIC)['n_fragments'] == 1
        wq.append(QR.quality_report(pos, v, ptr, CLASS_Z, quality.default_profiles(), mask))
    assert inc['hist']['All_12A'] == sum(w['hist'] for w in wq)[0, 1, :101].tolist() and inc['include'] == 'complete'
