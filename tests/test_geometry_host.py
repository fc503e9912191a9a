"""CPU-only checks of the local geometry report (targetdiff_amd.quality.sample_geometry, td_geometry_report's host side).

  1. tests/_geometry_ref.py -- the numpy restatement the GPU tests compare the kernel with -- against independent parties on every
     molecule of the fixture packs: topological distance > 3 against networkx, angle and torsion values against a direct
     arctan2 computation, counts against a brute-force enumeration over atom triples and quadruples and against a degree formula.
  2. known answers on the docked ligand and its jittered copies.
  3. the ABI surface and the refusals of the library and of the binding; TD_ABI_VERSION stays 5.
  4. sample_geometry, geometry_reference, tools/evaluate_samples.py --geometry and tools/export_sdf.py --clash-free with the bindings
     patched by the restatements, the degree-to-cosine edge flip included.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _bonds_ref as BR
import _geometry_ref as GR
import _rings_ref as RR
from conftest import ROOT, load_golden
from targetdiff_amd import capi, molfile, quality
from test_bonds_host import load_tool, packed, parse_sdf, save_results
from test_rings_host import fixture_molecules, ringed_result

CLASS_Z = quality.class_atomic_numbers('add_aromatic')
AROMATIC = quality.class_aromatic('add_aromatic')
TABLE = GR.clash_table()


def test_restatement_far_apart_matches_networkx():
    nx = pytest.importorskip('networkx')
    far = near = 0
    for name, pos, v in fixture_molecules():
        m = GR.molecule(pos, v, CLASS_Z, AROMATIC, TABLE)
        n = len(v)
        G = nx.Graph()
        G.add_nodes_from(range(n))
        G.add_edges_from(zip(m['i'].tolist(), m['j'].tolist()))
        want = np.ones((n, n), bool)
        for a, reach in nx.all_pairs_shortest_path_length(G, cutoff=3):
            want[a, list(reach)] = False
        np.testing.assert_array_equal(m['far'], want, err_msg=name)
        # a clash: far apart, both with a class, closer than the table says; symmetric, nothing on the diagonal
        valid = m['z'] > 0
        e = np.asarray([GR.QR.ELEMENTS.index(z) if z else 0 for z in m['z']], np.int64)
        close = np.linalg.norm(pos[:, None].astype(np.float64) - pos[None].astype(np.float64), axis=2) < TABLE[e[:, None], e[None, :]] - 1e-9
        loose = np.linalg.norm(pos[:, None].astype(np.float64) - pos[None].astype(np.float64), axis=2) < TABLE[e[:, None], e[None, :]] + 1e-9
        assert (m['clash'] >= (want & close & valid[:, None] & valid[None, :])).all() and (m['clash'] <= (want & loose)).all(), name
        assert (m['clash'] == m['clash'].T).all() and not m['clash'].diagonal().any()
        far += int(m['clash'].sum())
        near += int((~want & close).sum()) - n
    assert far > 100 and near > 100


def test_restatement_values_match_a_direct_computation():
    n_ang = n_tor = 0
    for name, pos, v in fixture_molecules():
        m = GR.molecule(pos, v, CLASS_Z, AROMATIC)
        p = pos.astype(np.float64)
        for (i, j, k), c, bad in zip(m['ang'], m['ang_cos'], m['ang_bad']):
            u, w = p[i] - p[j], p[k] - p[j]
            theta = np.arctan2(np.linalg.norm(np.cross(u, w)), np.dot(u, w))
            assert not bad and 1e-3 < theta < np.pi - 1e-3, (name, i, j, k)             # no fixture angle is near a degenerate one
            assert abs(np.arccos(c) - theta) < 1e-9, (name, i, j, k)
            n_ang += 1
        for (i, j, k, l), c, bad in zip(m['tor'], m['tor_cos'], m['tor_bad']):
            b1, b2, b3 = p[j] - p[i], p[k] - p[j], p[l] - p[k]
            n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
            phi = abs(np.arctan2(np.linalg.norm(b2) * np.dot(b1, n2), np.dot(n1, n2)))     # the signed dihedral, its sign dropped
            assert not bad, (name, i, j, k, l)
            if 1e-3 < phi < np.pi - 1e-3:
                assert abs(np.arccos(c) - phi) < 1e-9, (name, i, j, k, l)
            else:
                assert abs(abs(c) - 1.0) < 1e-6
            n_tor += 1
    assert n_ang > 300 and n_tor > 300


def test_restatement_counts_match_brute_force():
    brute = 0
    for name, pos, v in fixture_molecules():
        m = GR.molecule(pos, v, CLASS_Z, AROMATIC)
        adj = m['order'] > 0
        n = len(v)
        deg = adj.sum(1)
        ok = deg <= GR.MAX_DEGREE
        np.testing.assert_array_equal(m['crowded'], ~ok)
        # from the degrees: C(d, 2) angles per centre; (d_j - 1)(d_k - 1) minus the common neighbours per central bond
        common = adj.astype(np.int64) @ adj.astype(np.int64)
        central = np.triu(adj, 1) & ok[:, None] & ok[None, :]
        assert len(m['ang']) == int((deg * (deg - 1) // 2)[ok].sum()), name
        assert len(m['tor']) == int((((deg[:, None] - 1) * (deg[None, :] - 1) - common) * central).sum()), name
        if n <= 65:
            I = np.arange(n)
            tri = adj[:, :, None] & adj[None, :, :]                                                                            # [i, j, k]: i-j and j-k
            tri = tri & (I[:, None, None] < I[None, None, :]) & ok[None, :, None]
            assert {tuple(t) for t in m['ang'].tolist()} == {tuple(t) for t in np.argwhere(tri).tolist()}, name
            quad = adj[:, :, None, None] & adj[None, :, :, None] & adj[None, None, :, :]                                       # i-j, j-k, k-l
            quad = quad & (I[None, :, None, None] < I[None, None, :, None]) & (I[:, None, None, None] != I[None, None, None, :])
            quad = quad & (I[:, None, None, None] != I[None, None, :, None]) & (I[None, :, None, None] != I[None, None, None, :])
            quad = quad & ok[None, :, None, None] & ok[None, None, :, None]
            assert {tuple(t) for t in m['tor'].tolist()} == {tuple(t) for t in np.argwhere(quad).tolist()}, name
            assert len(m['tor']) == len({tuple(t) for t in m['tor'].tolist()})
            brute += 1
        # the central bond's category and ring size are those of the bond list
        for (i, j, k, l), cat, ring in zip(m['tor'], m['tor_cat'], m['tor_ring']):
            b = np.nonzero((m['i'] == j) & (m['j'] == k))[0]
            assert len(b) == 1 and m['cat'][b[0]] == cat and m['ring'][b[0]] == ring
    assert brute > 20


def test_known_answers_on_the_docked_ligand():
    q = load_golden('quality_docked.npz')
    assert np.diff(q['ptr']).tolist() == [25] * 5
    r = GR.geometry_report(q['pos'], q['v'], q['ptr'], CLASS_Z, AROMATIC, (), None, TABLE)
    assert r['n_angles'][0].tolist() == [36, 29, 29, 13, 9] and r['n_torsions'][0].tolist() == [42, 34, 31, 8, 2]
    assert r['n_clashes'][0].tolist() == [0, 2, 3, 15, 21]                       # the real ligand is clash-free, its jittered copies are not
    assert not r['n_crowded'].any() and not r['n_degenerate'].any() and r['atom_clash'][0, :25].tolist() == [0] * 25
    m = GR.molecule(q['pos'][0, :25], q['v'][0, :25], CLASS_Z, AROMATIC, TABLE)
    ring6 = np.asarray([all(m['atom_ring'][a] == 6 for a in t) for t in m['ang']])
    deg = np.degrees(np.arccos(m['ang_cos']))
    assert ring6.sum() >= 6 and (np.abs(deg[ring6] - 120.0) < 5.0).all()         # the angles inside the six-ring
    assert (np.abs(deg[deg < 90] - 60.0) < 1.0).all() and (deg < 90).sum() == 3  # and the three of its three-ring
    # in degrees, through the default profiles: two-degree bins, by ascending angle
    prof = quality.default_geometry_profiles()
    assert [quality.geometry_profile_name(p) for p in prof] == ['CCC', 'CCN', 'CCO', 'CNC', 'COC', 'NCN', 'CCCC|chain', 'CCCC|ring', 'CCCN',
                                                                 'CCCO', 'CCNC', 'CCOC|chain']
    assert len(prof[0][4]) == 89 and len(prof[6][4]) == 35


def test_library_entry_point_and_its_checks():
    lib = capi.load_library()
    assert hasattr(lib, 'td_geometry_report') and len(capi.SIGNATURES['td_geometry_report'][1]) == 24
    assert lib.td_abi_version() == capi.ABI_VERSION == 5
    header = open(os.path.join(ROOT, 'include', 'targetdiff_hip.h')).read()
    assert 'int td_geometry_report(' in header and '#define TD_ABI_VERSION 5' in header
    decl = header[header.index('int td_geometry_report('):]
    assert decl[:decl.index(';')].count(',') == 23
    assert ctypes.sizeof(capi.TdGeometryProfile) == 40
    cz = (ctypes.c_int32 * 13)(*CLASS_Z)
    some = ctypes.c_void_p(8)                                                   # never dereferenced: every call below is refused first
    table = (ctypes.c_double * 64)(*TABLE.reshape(-1))

    def profiles(*rows):
        arr = (capi.TdGeometryProfile * len(rows))()
        for k, (kind, z, cat, ring, n_edges, edges) in enumerate(rows):
            arr[k] = capi.TdGeometryProfile(kind, (ctypes.c_int32 * 4)(*z), cat, ring, n_edges, edges)
        return ctypes.cast(arr, ctypes.c_void_p)

    def call(S=1, B=1, K=13, classes=cz, prof=None, P=0, bond_ptr=None, nb=0, bond_ring=None, clash=None, counts=None, hist=None):
        return lib.td_geometry_report(None, None, None, S, 0, B, classes, K, None, None, prof, P, bond_ptr, nb, bond_ring, clash, counts, counts,
                                      counts, counts, None, None, hist, None)

    assert call(S=-1) == -1 and b'bad argument' in lib.td_last_error()
    assert call(B=-1) == -1 and call(S=1 << 20, B=1 << 20) == -1
    assert call(nb=-1) == -1 and b'n_bonds' in lib.td_last_error()
    assert call(K=0) == -1 and call(K=65) == -1 and b'class table' in lib.td_last_error()
    assert call(classes=None) == -1
    bad = (ctypes.c_int32 * 13)(*([6] * 12 + [35]))
    assert call(classes=bad) == -1 and b'atomic number 35' in lib.td_last_error()
    assert call(P=-1) == -1 and call(P=17, prof=some) == -1 and call(P=1) == -1 and b'geometry profiles' in lib.td_last_error()
    angle = (1, (6, 6, 6, 0), 0, 0, 5, 8)
    torsion = (2, (6, 6, 6, 6), 0, 0, 5, 8)
    refused = lambda row, **kw: call(S=0, prof=profiles(row), P=1, **kw) == -1
    assert call(S=0, prof=profiles(angle, torsion), P=2) == 0                   # no work: nothing is touched
    assert refused((0,) + angle[1:]) and refused((3,) + angle[1:]) and b'kind' in lib.td_last_error()
    assert refused((1, (6, 6, 6, 6), 0, 0, 5, 8)) and b'z[3]' in lib.td_last_error()
    assert refused((1, (6, 6, 6, 0), 1, 0, 5, 8)) and refused((1, (6, 6, 6, 0), 0, 2, 5, 8, ), bond_ptr=some, bond_ring=some)
    assert refused((2, (6, 35, 6, 6), 0, 0, 5, 8)) and b'atomic number' in lib.td_last_error()
    assert refused((2, (6, 6, 6, 6), 5, 0, 5, 8)) and refused((2, (6, 6, 6, 6), 0, 3, 5, 8)) and refused((2, (6, 6, 6, 6), -1, 0, 5, 8))
    assert refused((2, (6, 6, 6, 6), 0, 1, 5, 8)) and b'd_bond_ring' in lib.td_last_error()
    assert refused((2, (6, 6, 6, 6), 0, 2, 5, 8), bond_ptr=some) and refused((2, (6, 6, 6, 6), 0, 2, 5, 8), bond_ring=some)
    assert call(S=0, prof=profiles((2, (6, 6, 6, 6), 0, 2, 5, 8)), P=1, bond_ptr=some, bond_ring=some) == 0
    assert refused(torsion[:4] + (0, 8)) and refused(torsion[:4] + (128, 8)) and refused(torsion[:4] + (5, None)) and b'edges' in lib.td_last_error()
    assert call(S=0, prof=profiles(torsion[:4] + (127, 8)), P=1) == 0
    assert call() == -1 and b'null pointer' in lib.td_last_error()              # S = B = 1 without a ligand_ptr
    assert call(S=1, B=0, prof=profiles(angle), P=1) == -1 and b'null pointer' in lib.td_last_error()      # frames and profiles need d_hist
    assert call(S=1, B=0) == 0 and call(S=0, B=5, clash=table) == 0 and call(S=0) == 0


def test_binding_refusals_before_any_device_work():
    pos = torch.zeros(2, 5, 3)
    v = torch.zeros(2, 5, dtype=torch.int64)
    ptr = torch.tensor([0, 2, 5], dtype=torch.int32)
    e = np.array([-0.5, 0.0, 0.5])
    with pytest.raises(ValueError, match='513 atoms'):
        capi.geometry_report(torch.zeros(1, 513, 3), torch.zeros(1, 513, dtype=torch.int64), torch.tensor([0, 513], dtype=torch.int32), CLASS_Z, AROMATIC)
    for bad, match in (((('bend', (6, 6, 6), 0, 0, e),), 'kind'), ((('angle', (6, 6, 6, 6), 0, 0, e),), '3 elements'),
                       ((('torsion', (6, 6, 6), 0, 0, e),), '3 elements'), ((('angle', (6, 35, 6), 0, 0, e),), 'elements of'),
                       ((('angle', (6, 6, 6), 1, 0, e),), 'no category'), ((('angle', (6, 6, 6), 0, 'ring', e),), 'no category'),
                       ((('torsion', (6, 6, 6, 6), 5, 0, e),), 'category'), ((('torsion', (6, 6, 6, 6), 0, 3, e),), 'category'),
                       ((('torsion', (6, 6, 6, 6), 0, 0, e[::-1]),), 'ascending'), ((('torsion', (6, 6, 6, 6), 0, 0, np.zeros(128)),), 'edges'),
                       ((('torsion', (6, 6, 6, 6), 0, 0, []),), 'edges'), ((('torsion', (6, 6, 6, 6), 0, 'ring', e),), 'ring filter needs'),
                       ([('angle', (6, 6, 6), 0, 0, e)] * 17, 'at most 16')):
        with pytest.raises(ValueError, match=match):
            capi.geometry_report(pos, v, ptr, CLASS_Z, AROMATIC, bad)
    with pytest.raises(ValueError, match='bond_ptr'):
        capi.geometry_report(pos, v, ptr, CLASS_Z, AROMATIC, bond_ptr=torch.zeros(4, dtype=torch.int64), bond_ring=torch.zeros(0, dtype=torch.int16))
    with pytest.raises(ValueError, match='bond_ring'):
        capi.geometry_report(pos, v, ptr, CLASS_Z, AROMATIC, bond_ptr=torch.zeros(5, dtype=torch.int64), bond_ring=torch.zeros(0, dtype=torch.int32))
    with pytest.raises(ValueError, match='clash_threshold'):
        capi.geometry_report(pos, v, ptr, CLASS_Z, AROMATIC, clash_threshold=np.zeros(63))
    with pytest.raises(ValueError, match='one flag per class'):
        capi.geometry_report(pos, v, ptr, CLASS_Z, [True])
    with pytest.raises(ValueError):
        capi.geometry_report(pos, v, ptr, CLASS_Z, AROMATIC, include=torch.ones(2, 3, dtype=torch.bool))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU path'):
            capi.geometry_report(pos, v, ptr, CLASS_Z, AROMATIC)
    res = ([], [], [np.zeros((1, 2, 3))], [np.zeros((1, 2), np.int64)], [], [], [])
    with pytest.raises(ValueError, match="'complete'"):
        quality.sample_geometry(res, include='stable', device='cpu')
    with pytest.raises(ValueError, match='degrees'):
        quality.sample_geometry(res, profiles=(('angle', (6, 6, 6), 0, 'any', [10.0, 190.0]),), device='cpu')
    with pytest.raises(ValueError, match='degrees'):
        quality.sample_geometry(res, profiles=(('angle', (6, 6, 6), 0, 'any', [30.0, 30.0]),), device='cpu')
    with pytest.raises(ValueError, match='radii'):
        quality.clash_thresholds(radii={35: 1.85})
    with pytest.raises(ValueError, match='clash_scale'):
        quality.clash_thresholds(-1.0)
    np.testing.assert_array_equal(quality.clash_thresholds(), TABLE)
    assert quality.clash_thresholds(0.5, {6: 2.0})[1, 1] == 2.0 and quality.clash_thresholds(0.5, {6: 2.0})[0, 0] == 1.2


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
    monkeypatch.setattr(capi, 'geometry_report', patched('geometry_report', GR.torch_geometry_report))
    return calls


def degree_histograms(pos, v, ptr, profiles, include=None):
    """[S, P, 128] by ascending angle, from the restatement's cosines through arccos: numpy.searchsorted(edges, degrees, 'right')"""
    S, B = pos.shape[0], len(ptr) - 1
    out = np.zeros((S, len(profiles), 128), np.int64)
    for s in range(S):
        for g in range(B):
            if include is not None and not include[s, g]:
                continue
            m = GR.molecule(pos[s, ptr[g]:ptr[g + 1]], v[s, ptr[g]:ptr[g + 1]], CLASS_Z, AROMATIC)
            for p, prof in enumerate(profiles):
                theta = np.degrees(np.arccos(np.clip(GR.matching(m, prof), -1.0, 1.0)))
                np.add.at(out[s, p], np.searchsorted(np.asarray(prof[4], np.float64), theta, 'right'), 1)
    return out


def test_sample_geometry_packs_a_ragged_result_and_flips_the_edges(numpy_binding):
    sizes, T = [7, 3, 12, 1, 9, 2], 4
    res = ringed_result(3, sizes, T)
    prof = quality.default_geometry_profiles() + (('angle', (0, 0, 0), 0, 'any', [60.0, 90.0, 120.0]), ('torsion', (0, 0, 0, 0), 0, 'ring', [90.0]),
                                                  ('torsion', (0, 6, 7, 0), 1, 'any', np.arange(10.0, 180.0, 10.0)))
    cosp = quality._cosine_profiles(prof)
    for p, q in zip(prof, cosp):
        np.testing.assert_array_equal(q[4], np.cos(np.radians(np.asarray(p[4], np.float64)))[::-1])
        assert (np.diff(q[4]) > 0).all()
    for eval_step, frames in ((-1, slice(T - 1, T)), (1, slice(1, 2)), ('all', slice(0, T))):
        pos, v, ptr = packed(res, frames)
        want = GR.geometry_report(pos, v, ptr, CLASS_Z, AROMATIC, cosp, None, TABLE)
        del numpy_binding[:]
        rep = quality.sample_geometry(res, eval_step, profiles=prof, device='cpu')
        assert numpy_binding == ['bond_graph', 'ring_report', 'geometry_report']
        assert rep.num_frames == (T if eval_step == 'all' else 1) and rep.n_samples == 6 and rep.n_included.tolist() == [6] * rep.num_frames
        np.testing.assert_array_equal(rep.hist, degree_histograms(pos, v, ptr, prof))
        for p, q in enumerate(cosp):
            m = len(q[4])
            np.testing.assert_array_equal(rep.hist[:, p, :m + 1], want['hist'][:, p, :m + 1][:, ::-1])
        np.testing.assert_array_equal(rep.sum_clashes, want['n_clashes'].sum(1))
        np.testing.assert_array_equal(rep.n_clash_free, (want['n_clashes'] == 0).sum(1))
        np.testing.assert_array_equal(rep.n_crowded, want['n_crowded'].sum(1))
        np.testing.assert_array_equal(rep.n_angles, want['n_angles'].sum(1))
        np.testing.assert_array_equal(rep.n_torsions, want['n_torsions'].sum(1))
        for s in range(rep.num_frames):
            assert rep.clash_free(s) == (want['n_clashes'][s] == 0).sum() / 6 and rep.mean_clashes(s) == want['n_clashes'][s].sum() / 6
            assert set(rep.summary(s)) == {'clash_free', 'mean_clashes', 'crowded_atoms', 'degenerate', 'angles', 'torsions'} | set(rep.names)
            assert len(rep.lines(s)) == 6 + len(prof)
        # include='complete': the bond graph's flags are the mask
        mask = BR.bond_graph(pos, v, ptr, CLASS_Z, AROMATIC)['n_fragments'] == 1
        rep2 = quality.sample_geometry(res, eval_step, include='complete', profiles=prof, device='cpu')
        np.testing.assert_array_equal(rep2.hist, degree_histograms(pos, v, ptr, prof, mask))
        np.testing.assert_array_equal(rep2.n_included, mask.sum(1))
        np.testing.assert_array_equal(rep2.sum_clashes, np.where(mask, want['n_clashes'], 0).sum(1))
        np.testing.assert_array_equal(rep2.hist, quality.sample_geometry(res, eval_step, include=mask, profiles=prof, device='cpu').hist)
        both = quality.GeometryReport.merged([rep, rep2])
        np.testing.assert_array_equal(both.hist, rep.hist + rep2.hist)
        assert both.n_samples == 12 and both.n_included.tolist() == (6 + mask.sum(1)).tolist()
    assert 0 < mask.sum() < mask.size and rep.hist[:, 12].sum() > 50 and rep.hist[:, 13].sum() > 0 and want['n_clashes'].sum() > 0
    with pytest.raises(ValueError):
        quality.GeometryReport.merged([rep, quality.sample_geometry(res, -1, profiles=prof, device='cpu')])
    # without a ring filter: one launch
    del numpy_binding[:]
    quality.sample_geometry(res, -1, profiles=prof[:6], device='cpu')
    assert numpy_binding == ['geometry_report']
    # the mean angle from the bin centres, the counts, no distance without a reference
    name = rep.names[12]
    h = rep.counts(name, -1)
    assert name == '***' and rep.count(name, -1) == h.sum() and rep.bin_centres(name).tolist() == [30.0, 75.0, 105.0, 150.0]
    assert rep.mean_angle(name, -1) == float((h * np.array([30.0, 75.0, 105.0, 150.0])).sum() / h.sum())
    assert all(x is None for x in rep.js(-1).values())


def test_an_angle_on_an_edge_lands_in_the_bin_that_starts_there(numpy_binding):
    """cos(radians(0)) == 1 and cos(radians(180)) == -1 exactly: a cis torsion and a straight angle sit on those edges"""
    pos = np.array([[-0.5, 1.25, 0], [0, 0, 0], [1.5, 0, 0], [2.0, 1.25, 0], [10, 0, 0], [11.5, 0, 0], [13, 0, 0]], np.float32)
    v = np.ones(7, np.int64)
    prof = (('torsion', (0, 0, 0, 0), 0, 'any', [0.0, 90.0]), ('angle', (0, 0, 0), 0, 'any', [90.0, 180.0]))
    g = quality.geometry(pos, v, ligand_ptr=[0, 4, 7], profiles=prof, device='cpu')
    assert g.hist[0, 0, :3].tolist() == [0, 1, 0] and g.hist[0, 1, :3].tolist() == [0, 2, 1]
    assert g.n_angles[0].tolist() == [2, 1] and g.n_torsions[0].tolist() == [1, 0] and g.clash_free[0].tolist() == [True, True]
    assert g.names == ('****', '***') and g.atom_clash.shape == (1, 7)


def test_geometry_reference_and_the_tools(numpy_binding, tmp_path, capsys, monkeypatch):
    import _quality_ref as QR
    monkeypatch.setattr(capi, 'quality_report', QR.torch_binding)
    results = {10: ringed_result(5, [6, 9], 3), 2: ringed_result(6, [4, 11, 5], 3)}
    save_results(tmp_path, results)
    prof = quality.default_geometry_profiles()
    cosp = quality._cosine_profiles(prof)
    # a reference from molecules given as (pos, v) and as records of an SD file: the same kernel, the same bond rule
    known = ringed_result(8, [10, 12, 8], 1)
    mols = [(p[-1].astype(np.float32), c[-1]) for p, c in zip(known[2], known[3])]
    ref = quality.geometry_reference(mols, device='cpu')
    kpos, kv, kptr = packed(known, slice(0, 1))
    w = GR.geometry_report(kpos, kv, kptr, CLASS_Z, AROMATIC, cosp, None, None)
    assert list(ref) == [quality.geometry_profile_name(p) for p in prof]
    for p, (name, h) in enumerate(ref.items()):
        np.testing.assert_array_equal(h, w['hist'][0, p, :len(prof[p][4]) + 1][::-1])
    assert sum(int(h.sum()) for h in ref.values()) > 0
    g = quality.bond_graph(kpos, kv, ligand_ptr=kptr, return_fragments=True, return_bonds=True, device='cpu')
    sdf = tmp_path / 'known.sdf'
    molfile.write_sdf(sdf, molfile.molecules_from_graph(g, kpos, kv))
    ref2 = quality.geometry_reference(molfile.read_sdf(sdf), device='cpu')
    assert ref2.keys() == ref.keys() and sum(int(h.sum()) for h in ref2.values()) > 0      # coordinates rounded to the file's four decimals
    with pytest.raises(ValueError, match='at least one'):
        quality.geometry_reference([], device='cpu')

    tool = load_tool('evaluate_samples')
    capsys.readouterr()
    del numpy_binding[:]
    base = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu'])
    assert 'geometry' not in base and 'clash_free' not in capsys.readouterr().out and 'geometry_report' not in numpy_binding
    out = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--geometry', '--eval_step', 'all', '--reference_sdf', str(sdf)])
    text = capsys.readouterr().out
    want = [GR.geometry_report(*packed(results[i], slice(0, 3)), CLASS_Z, AROMATIC, cosp, None, TABLE) for i in (2, 10)]
    clashes = np.concatenate([x['n_clashes'] for x in want], axis=1)
    hist = sum(x['hist'] for x in want)
    geo = out['geometry']
    assert geo['clash_free'] == (clashes[-1] == 0).sum() / 5 and geo['mean_clashes'] == clashes[-1].sum() / 5 and geo['num_included'] == 5
    assert f"clash_free:\t{geo['clash_free']:.4f}\n" in text and 'mean_clashes:\t' in text and 'crowded_atoms:\t' in text and 'degenerate:\t' in text
    assert 'angle CCC:\tcount ' in text and 'torsion CCCC|ring:\tcount ' in text
    for p, name in enumerate(ref):
        m = len(prof[p][4])
        assert geo['hist'][name] == hist[-1, p, :m + 1][::-1].tolist()
        d = hist[-1, p, :m + 1][::-1]
        if d.sum() > 0 and ref2[name].sum() > 0:
            assert geo[name]['js'] == float(quality.jensenshannon(ref2[name].astype(np.float64), d / d.sum()))
        else:
            assert geo[name]['js'] is None
    assert any(geo[name]['js'] is not None for name in ref) and hist[-1].sum() > 0
    assert [c['mean_clashes'] for c in geo['curve']] == (clashes.sum(1) / 5).tolist() and len(geo['curve']) == 3
    assert {k: base[k] for k in ('mol_stable', 'atm_stable')} == {k: out[k] for k in ('mol_stable', 'atm_stable')}
    saved = json.load(open(tmp_path / 'eval_results' / 'quality.json'))
    assert saved['geometry']['hist'] == geo['hist']
    inc = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--geometry', '--include', 'complete'])
    n_inc = n_cl = 0
    for i in (2, 10):
        pos, v, ptr = packed(results[i], slice(2, 3))
        mask = BR.bond_graph(pos, v, ptr, CLASS_Z, AROMATIC)['n_fragments'] == 1
        n_inc += int(mask.sum())
        n_cl += int(GR.geometry_report(pos, v, ptr, CLASS_Z, AROMATIC, (), None, TABLE)['n_clashes'][mask].sum())
    assert inc['geometry']['num_included'] == n_inc and (n_inc == 0 or inc['geometry']['mean_clashes'] == n_cl / n_inc)

    # export_sdf --clash-free
    tool = load_tool('export_sdf')
    del numpy_binding[:]
    plain = tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'plain'), '--device', 'cpu'])
    assert 'geometry_report' not in numpy_binding and 'clash_free' not in plain['result_2']     # without the flag: no launch, the files of before
    done = tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'free'), '--device', 'cpu', '--clash-free'])
    kept = 0
    for i, res in results.items():
        pos, v, ptr = packed(res, slice(2, 3))
        free = GR.geometry_report(pos, v, ptr, CLASS_Z, AROMATIC, (), None, TABLE)['n_clashes'][0] == 0
        every = parse_sdf(open(tmp_path / 'plain' / f'result_{i}.sdf').read())
        recs = parse_sdf(open(tmp_path / 'free' / f'result_{i}.sdf').read())
        assert recs == [r for r, f in zip(every, free) if f]
        assert done[f'result_{i}']['written'] == done[f'result_{i}']['clash_free'] == int(free.sum())
        kept += int(free.sum())
    assert 0 < kept < 5
