"""CPU-only checks of the ring report (targetdiff_amd.quality.sample_rings, td_ring_report's host side).

  1. tests/_rings_ref.py -- the pure-Python restatement the GPU tests compare the kernel with -- against an independent party,
     networkx, on every molecule of the fixture packs, and against known answers on the docked ligand and its jittered copies.
  2. the ABI surface and the refusals of the library and of the binding; TD_ABI_VERSION stays 5.
  3. sample_rings, quality.bond_graph(rings=True), tools/evaluate_samples.py --rings and tools/export_sdf.py --ring-aromatic with the
     bindings patched by the restatements.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _bonds_ref as BR
import _rings_ref as RR
from conftest import ROOT, load_golden
from targetdiff_amd import capi, molfile, quality
from test_bonds_host import load_tool, packed, parse_sdf, ragged_result, save_results

CLASS_Z = quality.class_atomic_numbers('add_aromatic')
AROMATIC = quality.class_aromatic('add_aromatic')


def fixture_molecules():
    """(name, pos [n, 3], v [n]) of every molecule of the three packs; of the 1000-frame trajectory every 97th frame and the last"""
    for name in ('docked', 'sizes'):
        q = load_golden(f'quality_{name}.npz')
        for s in range(q['pos'].shape[0]):
            for g, (a, b) in enumerate(zip(q['ptr'][:-1], q['ptr'][1:])):
                if b - a <= RR.MAX_ATOMS:
                    yield f'{name}[{s},{g}]', q['pos'][s, a:b], q['v'][s, a:b]
    t, ptr = load_golden('sample_small_1000.npz'), load_golden('quality_traj.npz')['ptr']
    for s in sorted(set(range(0, 1000, 97)) | {999}):
        for g, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
            yield f'traj[{s},{g}]', t['pos_traj'][s, a:b], t['v_traj'][s, a:b].astype(np.int64)


def test_restatement_matches_networkx():
    nx = pytest.importorskip('networkx')
    seen_ring = seen_bridge = 0
    for name, pos, v in fixture_molecules():
        m = RR.molecule(pos, v, CLASS_Z, AROMATIC)
        G = nx.Graph()
        G.add_nodes_from(range(len(v)))
        G.add_edges_from(zip(m['i'].tolist(), m['j'].tolist()))
        for k, (i, j) in enumerate(zip(m['i'].tolist(), m['j'].tolist())):
            G.remove_edge(i, j)
            want = 1 + nx.shortest_path_length(G, i, j) if nx.has_path(G, i, j) else 0
            G.add_edge(i, j)
            assert m['ring'][k] == want, (name, i, j)
            seen_ring += want > 0
            seen_bridge += want == 0
        # every basis ring that is some bond's smallest ring is in the mask
        smallest = set(m['ring'][m['ring'] > 0].tolist())
        for cycle in nx.minimum_cycle_basis(G):
            if len(cycle) in smallest:
                assert m['mask'] >> min(len(cycle), 31) & 1, (name, len(cycle))
        # and the mask holds nothing else; an atom's size is the minimum over its bonds
        assert m['mask'] == sum({1 << min(r, 31) for r in smallest}), name
        for a in range(len(v)):
            mine = [int(r) for i, j, r in zip(m['i'], m['j'], m['ring']) if r and a in (i, j)]
            assert m['atom_ring'][a] == (min(mine) if mine else 0), (name, a)
        assert m['n_ring_atoms'] == int((m['atom_ring'] > 0).sum()) and m['n_ring_bonds'] == int((m['ring'] > 0).sum())
    assert seen_ring > 100 and seen_bridge > 100


def test_known_answers_on_the_docked_ligand():
    q = load_golden('quality_docked.npz')
    want = [(12, 3, 12, {3, 6}), (12, 0, 12, {6}), (15, 3, 6, {3, 6}), (17, 0, 0, set()), (5, 6, 0, {3})]
    ring_aromatic, class_aromatic = [], []
    for g, (a, b) in enumerate(zip(q['ptr'][:-1], q['ptr'][1:])):
        m = RR.molecule(q['pos'][0, a:b], q['v'][0, a:b], CLASS_Z, AROMATIC)
        bits = {k for k in range(32) if m['mask'] >> k & 1}
        assert ((m['ring'] == 0).sum(), (m['ring'] == 3).sum(), (m['ring'] == 6).sum(), bits) == want[g], g
        assert set(m['ring'].tolist()) <= {0, 3, 6}
        ring_aromatic.append(int((m['ring_cat'] == 4).sum()))
        class_aromatic.append(int((m['cat'] == 4).sum()))
        keep = m['cat'] != 4
        np.testing.assert_array_equal(m['ring_cat'][keep], m['cat'][keep])
        np.testing.assert_array_equal(m['ring_cat'][~keep & ~np.isin(m['ring'], (5, 6))], m['o'][~keep & ~np.isin(m['ring'], (5, 6))])
    assert ring_aromatic == [1, 1, 1, 0, 0] and class_aromatic == [1, 1, 1, 1, 0]          # molecule 3's aromatic bond lies in no ring
    r = RR.ring_report(q['pos'], q['v'], q['ptr'], CLASS_Z, AROMATIC)
    assert r['ring_hist'][0].tolist() == [1, 0, 0, 3, 0, 0, 3] + [0] * 25
    assert r['ring_mask'][0].tolist() == [72, 64, 72, 0, 8] and r['bond_ptr'][-1] == len(r['bond_ring']) == len(r['bond_category'])
    inc = np.array([[True, False, True, True, False]])
    assert RR.ring_report(q['pos'], q['v'], q['ptr'], CLASS_Z, AROMATIC, inc)['ring_hist'][0].tolist() == [1, 0, 0, 2, 0, 0, 2] + [0] * 25


def test_library_entry_point_and_its_checks():
    lib = capi.load_library()
    assert hasattr(lib, 'td_ring_report') and len(capi.SIGNATURES['td_ring_report'][1]) == 20
    assert lib.td_abi_version() == capi.ABI_VERSION == 5
    header = open(os.path.join(ROOT, 'include', 'targetdiff_hip.h')).read()
    assert 'int td_ring_report(' in header and '#define TD_ABI_VERSION 5' in header
    decl = header[header.index('int td_ring_report('):]
    assert decl[:decl.index(';')].count(',') == 19
    cz = (ctypes.c_int32 * 13)(*CLASS_Z)
    some = ctypes.c_void_p(8)                                                   # never dereferenced: every call below is refused first
    call = lambda S=1, B=1, K=13, nb=0, table=cz, bond_ptr=None, bond_ring=None, bond_cat=None, mask=None, hist=None: lib.td_ring_report(
        None, None, None, S, 0, B, table, K, None, None, bond_ptr, nb, mask, None, None, None, hist, bond_ring, bond_cat, None)
    assert call(S=-1) == -1 and b'bad argument' in lib.td_last_error()
    assert call(B=-1) == -1 and call(S=1 << 20, B=1 << 20) == -1
    assert call(nb=-1) == -1 and b'n_bonds' in lib.td_last_error()
    assert call(K=0) == -1 and call(K=65) == -1 and b'class table' in lib.td_last_error()
    assert call(table=None) == -1
    bad = (ctypes.c_int32 * 13)(*([6] * 12 + [35]))
    assert call(table=bad) == -1 and b'atomic number 35' in lib.td_last_error()
    assert call() == -1 and b'null pointer' in lib.td_last_error()              # S = B = 1 without a ligand_ptr
    assert call(S=1, B=0) == -1 and b'null pointer' in lib.td_last_error()      # frames need ring_hist
    assert call(S=0, bond_ring=some) == -1 and b'd_bond_ptr' in lib.td_last_error()
    assert call(S=0, bond_cat=some) == -1 and b'd_bond_ptr' in lib.td_last_error()
    assert call(S=0, bond_ring=some, bond_cat=some, bond_ptr=some) == 0         # no work: nothing is touched
    assert call(S=0) == 0 and call(S=0, B=5, nb=7) == 0


def test_binding_refusals_before_any_device_work():
    pos = torch.zeros(2, 5, 3)
    v = torch.zeros(2, 5, dtype=torch.int64)
    ptr = torch.tensor([0, 2, 5], dtype=torch.int32)
    with pytest.raises(ValueError, match='513 atoms'):
        capi.ring_report(torch.zeros(1, 513, 3), torch.zeros(1, 513, dtype=torch.int64), torch.tensor([0, 513], dtype=torch.int32), CLASS_Z, AROMATIC)
    with pytest.raises(ValueError, match='bond_ptr'):
        capi.ring_report(pos, v, ptr, CLASS_Z, AROMATIC, bond_ptr=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match='bond_ptr'):
        capi.ring_report(pos, v, ptr, CLASS_Z, AROMATIC, bond_ptr=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match='prefix offsets'):
        capi.ring_report(pos, v, torch.tensor([0, 3, 2], dtype=torch.int32), CLASS_Z, AROMATIC)
    with pytest.raises(ValueError, match='one flag per class'):
        capi.ring_report(pos, v, ptr, CLASS_Z, [True])
    with pytest.raises(ValueError):
        capi.ring_report(pos, v, ptr, CLASS_Z, AROMATIC, include=torch.ones(2, 3, dtype=torch.bool))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU path'):
            capi.ring_report(pos, v, ptr, CLASS_Z, AROMATIC)
    with pytest.raises(ValueError, match="'complete'"):
        quality.sample_rings(([], [], [np.zeros((1, 2, 3))], [np.zeros((1, 2), np.int64)], [], [], []), include='stable', device='cpu')


@pytest.fixture
def numpy_binding(monkeypatch):
    calls = []

    def patched(name, fn):
        def binding(*a, **kw):
            calls.append(name)
            return fn(*a, **kw)
        return binding

    monkeypatch.setattr(capi, 'bond_graph', patched('bond_graph', BR.torch_bond_graph))
    monkeypatch.setattr(capi, 'bond_list', patched('bond_list', BR.torch_bond_list))
    monkeypatch.setattr(capi, 'ring_report', patched('ring_report', RR.torch_ring_report))
    return calls


def ringed_result(seed, sizes, T):
    """test_bonds_host.ragged_result, tighter (sigma 0.9 A) and of carbons and nitrogens of both kinds: rings of several sizes and
    aromatic-class bonds inside and outside them"""
    rng = np.random.default_rng(seed)
    pos_traj = [rng.normal(0, 0.9, (T, n, 3)).astype(np.float32).astype(np.float64) for n in sizes]
    v_traj = [rng.integers(1, 5, (T, n)) for n in sizes]
    return ([p[-1] for p in pos_traj], [v[-1] for v in v_traj], pos_traj, v_traj, [], [], [0.0])


def test_sample_rings_packs_a_ragged_result(numpy_binding):
    sizes, T = [7, 3, 12, 1, 9, 2], 4
    res = ringed_result(3, sizes, T)
    n = np.asarray(sizes, np.float64)
    for eval_step, frames in ((-1, slice(T - 1, T)), (1, slice(1, 2)), ('all', slice(0, T))):
        pos, v, ptr = packed(res, frames)
        want = RR.ring_report(pos, v, ptr, CLASS_Z, AROMATIC)
        rep = quality.sample_rings(res, eval_step, device='cpu')
        np.testing.assert_array_equal(rep.ring_hist, want['ring_hist'])
        assert rep.num_frames == (T if eval_step == 'all' else 1) and rep.n_samples == 6 and rep.n_included.tolist() == [6] * rep.num_frames
        for s in range(rep.num_frames):
            assert rep.ring_ratio(s) == {k: want['ring_hist'][s, k] / 6 for k in range(3, 10)}
            assert rep.no_ring(s) == (want['ring_mask'][s] == 0).sum() / 6 and rep.large_ring(s) == (want['ring_mask'][s] >= 1024).sum() / 6
            assert rep.ring_atom_share(s) == (want['n_ring_atoms'][s] / n).sum() / 6
            assert set(rep.summary(s)) == {f'ring_{k}' for k in range(3, 10)} | {'no_ring', 'large_ring', 'ring_atom_share'}
        # include='complete': the bond graph's flags are the mask
        mask = BR.bond_graph(pos, v, ptr, CLASS_Z, AROMATIC)['n_fragments'] == 1
        rep2 = quality.sample_rings(res, eval_step, include='complete', device='cpu')
        np.testing.assert_array_equal(rep2.ring_hist, RR.ring_report(pos, v, ptr, CLASS_Z, AROMATIC, mask)['ring_hist'])
        np.testing.assert_array_equal(rep2.n_included, mask.sum(1))
        np.testing.assert_array_equal(rep2.ring_hist, quality.sample_rings(res, eval_step, include=mask, device='cpu').ring_hist)
        both = quality.RingReport.merged([rep, rep2])
        np.testing.assert_array_equal(both.ring_hist, rep.ring_hist + rep2.ring_hist)
        assert both.n_samples == 12 and both.n_included.tolist() == (6 + mask.sum(1)).tolist()
    assert 0 < mask.sum() < mask.size and want['ring_hist'][:, 3:].sum() > 0 and want['ring_hist'][:, 0].sum() > 0
    with pytest.raises(ValueError):
        quality.RingReport.merged([rep, quality.sample_rings(res, -1, device='cpu')])
    # quality.bond_graph: no ring launch by default, the same object as before; with rings the new fields
    pos, v, ptr = packed(res, slice(T - 1, T))
    del numpy_binding[:]
    g0 = quality.bond_graph(pos[0], v[0], ligand_ptr=ptr, return_bonds=True, device='cpu')
    assert numpy_binding == ['bond_graph', 'bond_list'] and g0.bond_ring is None and g0.ring_mask is None and len(g0.molecule_bonds(0, 2)) == 4
    g = quality.bond_graph(pos[0], v[0], ligand_ptr=ptr, return_bonds=True, rings=True, device='cpu')
    want = RR.ring_report(pos, v, ptr, CLASS_Z, AROMATIC)
    for k, t in (('ring_mask', g.ring_mask), ('n_ring_bonds', g.n_ring_bonds), ('n_ring_atoms', g.n_ring_atoms), ('atom_ring', g.atom_ring),
                 ('bond_ring', g.bond_ring), ('bond_category', g.ring_category), ('class_category', g.bond_category)):
        np.testing.assert_array_equal(t.numpy(), want[k], err_msg=k)
    atoms, order, cat, length, ring, ring_cat = g.molecule_bonds(-1, 2)
    a, b = want['bond_ptr'][2:4]
    np.testing.assert_array_equal(ring, want['bond_ring'][a:b])
    np.testing.assert_array_equal(ring_cat, want['bond_category'][a:b])
    np.testing.assert_array_equal(atoms, want['bond_atoms'][a:b] - 10)
    g1 = quality.bond_graph(pos[0], v[0], ligand_ptr=ptr, rings=True, device='cpu')          # without the list: no per-bond output
    assert g1.bond_ring is None and g1.ring_category is None
    np.testing.assert_array_equal(g1.atom_ring.numpy(), want['atom_ring'])


def test_export_sdf_ring_aromatic(numpy_binding, tmp_path):
    tool = load_tool('export_sdf')
    results = {10: ringed_result(5, [6, 9, 14], 3), 2: ringed_result(6, [4, 11, 5], 3)}
    save_results(tmp_path, results)
    tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'plain'), '--device', 'cpu'])
    assert 'ring_report' not in numpy_binding                                   # without the flag: no ring launch
    out = tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'ring'), '--device', 'cpu', '--ring-aromatic'])
    assert list(out) == ['result_2', 'result_10'] and numpy_binding.count('ring_report') == 2
    changed = 0
    for i, res in results.items():
        pos, v, ptr = packed(res, slice(2, 3))
        want = RR.ring_report(pos, v, ptr, CLASS_Z, AROMATIC)
        plain = parse_sdf(open(tmp_path / 'plain' / f'result_{i}.sdf').read())
        ring = parse_sdf(open(tmp_path / 'ring' / f'result_{i}.sdf').read())
        for g, ((_, atoms0, bonds0, _p0), (_, atoms1, bonds1, _p1)) in enumerate(zip(plain, ring)):
            k0, k1 = want['bond_ptr'][g], want['bond_ptr'][g + 1]
            assert atoms0 == atoms1 and [b[:2] for b in bonds0] == [b[:2] for b in bonds1]
            assert [b[2] for b in bonds1] == want['bond_category'][k0:k1].tolist()
            assert [b[2] for b in bonds0] == want['class_category'][k0:k1].tolist()
            changed += sum(b0[2] != b1[2] for b0, b1 in zip(bonds0, bonds1))
            in_ring = want['atom_ring'][0, ptr[g]:ptr[g + 1]] > 0
            assert all(in_ring[i] and in_ring[j] for i, j, t in bonds1 if t == 4)                  # no aromatic bond on an atom outside a ring
    assert changed > 0
    # --largest-fragment keeps the categories with their bonds
    tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'ring2'), '--device', 'cpu', '--ring-aromatic', '--largest-fragment'])
    assert len(parse_sdf(open(tmp_path / 'ring2' / 'result_2.sdf').read())) == 3
    pos, v, ptr = packed(results[2], slice(2, 3))
    g = quality.bond_graph(pos, v, ligand_ptr=ptr, return_fragments=True, return_bonds=True, device='cpu')
    with pytest.raises(ValueError, match='categories'):
        molfile.molecules_from_graph(g, pos, v, categories=np.zeros(1, np.uint8))


def test_evaluate_samples_rings(numpy_binding, tmp_path, capsys, monkeypatch):
    import _quality_ref as QR
    monkeypatch.setattr(capi, 'quality_report', QR.torch_binding)
    tool = load_tool('evaluate_samples')
    results = {10: ringed_result(5, [6, 9], 3), 2: ringed_result(6, [4, 11, 5], 3)}
    save_results(tmp_path, results)
    base = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu'])
    assert 'rings' not in base and 'ring size' not in capsys.readouterr().out and 'ring_report' not in numpy_binding
    out = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--rings', '--eval_step', 'all'])
    text = capsys.readouterr().out
    want = [RR.ring_report(*packed(results[i], slice(0, 3)), CLASS_Z, AROMATIC) for i in (2, 10)]
    hist = sum(w['ring_hist'] for w in want)
    for k in range(3, 10):
        assert f'ring size: {k} ratio: {hist[-1, k] / 5:.3f}\n' in text
        assert out['rings'][f'ring_{k}'] == hist[-1, k] / 5
    assert 'no_ring:\t' in text and 'large_ring:\t' in text and 'ring_atom_share:\t' in text
    assert out['rings']['ring_hist'] == hist[-1].tolist() and out['rings']['num_included'] == 5
    assert [c['ring_3'] for c in out['rings']['curve']] == (hist[:, 3] / 5).tolist() and hist[:, 3].sum() > 0
    assert {k: base[k] for k in ('mol_stable', 'atm_stable')} == {k: out[k] for k in ('mol_stable', 'atm_stable')}
    saved = json.load(open(tmp_path / 'eval_results' / 'quality.json'))
    assert saved['rings']['ring_hist'] == hist[-1].tolist()
    inc = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--rings', '--include', 'complete'])
    n_inc, h = 0, np.zeros(32, np.int64)
    for i in (2, 10):
        pos, v, ptr = packed(results[i], slice(2, 3))
        mask = BR.bond_graph(pos, v, ptr, CLASS_Z, AROMATIC)['n_fragments'] == 1
        n_inc += int(mask.sum())
        h += RR.ring_report(pos, v, ptr, CLASS_Z, AROMATIC, mask)['ring_hist'][0]
    assert inc['rings']['ring_hist'] == h.tolist() and inc['rings']['num_included'] == n_inc
