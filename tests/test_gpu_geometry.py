"""td_geometry_report on the GPU (csrc/geometry.hip) against tests/_geometry_ref.py, array_equal on every output (the restatement is
pinned to networkx, to arccos / arctan2 and to brute-force enumeration on the host, tests/test_geometry_host.py).

  1. the fixture packs: the docked ligand and its jittered copies, every frame of the sizes pack (both instantiations, a 600-atom
     molecule that is answered with -1) and the 1000-frame trajectory, under profiles that use every filter, with and without include.
  2. a size pack cut from a jittered lattice around the instantiation boundary and the limit: 127 / 128 / 129 and 511 / 512 atoms.
  3. a planted pack of tiny molecules with exact fp32 coordinates: cosines that sit on an edge, degenerate cases, the three-ring
     exclusion, clashes by topological distance, the degree cap, an atom of no class.
  4. null optional outputs, the clash pass off, a side stream; oversize molecules.
  5. end to end: sample_geometry, geometry_reference, evaluate_samples --geometry and export_sdf --clash-free on the driver's trajectories.
"""
import types

import numpy as np
import pytest
import torch

import _bonds_ref as BR
import _geometry_ref as GR
from conftest import load_golden
from targetdiff_amd import capi, quality
from test_bonds_host import load_tool, parse_sdf, save_results

pytestmark = pytest.mark.gpu

CLASS_Z = quality.class_atomic_numbers('add_aromatic')
AROMATIC = quality.class_aromatic('add_aromatic')
H, C, C_ARO, N, O = 0, 1, 2, 3, 5                                           # classes of 'add_aromatic'
TABLE = GR.clash_table()
EA = np.cos(np.radians(np.arange(2.0, 180.0, 2.0)))[::-1].copy()            # ascending cosine edges: 2 degree and 5 degree bins
ET = np.cos(np.radians(np.arange(5.0, 180.0, 5.0)))[::-1].copy()
# every filter: any element, ends in either order, reversed torsions, every category, both ring modes
PROFILES = (('angle', (6, 6, 6), 0, 0, EA), ('angle', (0, 0, 0), 0, 0, EA), ('angle', (7, 6, 8), 0, 0, EA), ('angle', (0, 7, 6), 0, 0, EA),
            ('angle', (6, 0, 0), 0, 0, ET), ('torsion', (6, 6, 6, 6), 0, 'chain', ET), ('torsion', (6, 6, 6, 6), 0, 'ring', ET),
            ('torsion', (7, 6, 6, 6), 0, 'any', ET), ('torsion', (0, 0, 0, 0), 0, 0, ET), ('torsion', (0, 6, 7, 0), 1, 0, ET),
            ('torsion', (0, 0, 0, 0), 2, 'ring', EA), ('torsion', (0, 0, 0, 0), 4, 0, ET), ('torsion', (0, 0, 0, 0), 3, 'chain', ET),
            ('torsion', (8, 0, 0, 0), 0, 0, ET), ('torsion', (0, 0, 0, 0), 0, 'ring', ET), ('torsion', (0, 0, 0, 0), 0, 'chain', ET))
NO_RING = tuple(p for p in PROFILES if p[3] in (0, 'any'))


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


def geom(pos, v, ptr, profiles=PROFILES, include=None, table=TABLE, atom_clash=True, check=False):
    """capi.geometry_report of numpy inputs, as numpy; capi.bond_graph and capi.ring_report first when a profile filters on the ring"""
    dev = _dev()
    inc = None if include is None else torch.as_tensor(np.ascontiguousarray(include), dtype=torch.bool, device=dev)
    p, c = torch.as_tensor(np.ascontiguousarray(pos), device=dev), torch.as_tensor(np.ascontiguousarray(v), dtype=torch.int64, device=dev)
    lp = torch.as_tensor(np.asarray(ptr), dtype=torch.int32, device=dev)
    bond_ptr = bond_ring = None
    if any(q[3] not in (0, 'any') for q in profiles):
        bond_ptr = capi.bond_graph(p, c, lp, CLASS_Z, AROMATIC, (), None, False, True, check=check)['bond_ptr']
        bond_ring = capi.ring_report(p, c, lp, CLASS_Z, AROMATIC, None, bond_ptr, False, check=check)['bond_ring']
    out = capi.geometry_report(p, c, lp, CLASS_Z, AROMATIC, profiles, inc, table, bond_ptr, bond_ring, atom_clash, check=check)
    out = {k: (None if t is None else t.cpu().numpy()) for k, t in out.items()}
    if out['atom_clash'] is not None:
        for g in np.nonzero(np.diff(np.asarray(ptr)) > GR.MAX_ATOMS)[0]:        # the atoms of a refused molecule are not written
            out['atom_clash'][:, ptr[g]:ptr[g + 1]] = 0
    return out


def same(a, b, what, keys=GR.KEYS):
    for k in keys:
        if b[k] is None:
            assert a[k] is None, f'{what}: {k}'
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f'{what}: {k}')


def against_restatement(pos, v, ptr, profiles=PROFILES, include=None, what=''):
    r = geom(pos, v, ptr, profiles, include)
    want = GR.geometry_report(pos, v, ptr, CLASS_Z, AROMATIC, profiles, include, TABLE)
    same(r, want, what)
    return r


_CACHE = {}


def sizes_geometry():
    """the sizes pack through the kernel and the restatement, once: shared by the tests that need a baseline"""
    if 'sizes' not in _CACHE:
        q = load_golden('quality_sizes.npz')
        _CACHE['sizes'] = (q, geom(q['pos'], q['v'], q['ptr'], PROFILES, q['include']),
                           GR.geometry_report(q['pos'], q['v'], q['ptr'], CLASS_Z, AROMATIC, PROFILES, q['include'], TABLE))
    return _CACHE['sizes']


def test_fixture_docked():
    q = load_golden('quality_docked.npz')
    r = against_restatement(q['pos'], q['v'], q['ptr'], what='docked')
    for k in GR.COUNT_KEYS + GR.CLASH_KEYS:
        assert r[k].dtype == np.int32, k
    assert r['hist'].dtype == np.int64 and r['hist'].shape == (1, 16, 128)
    assert r['n_angles'][0].tolist() == [36, 29, 29, 13, 9] and r['n_torsions'][0].tolist() == [42, 34, 31, 8, 2]
    assert r['n_clashes'][0].tolist() == [0, 2, 3, 15, 21] and not r['n_crowded'].any() and not r['n_degenerate'].any()
    assert r['atom_clash'][0].sum() == 2 * r['n_clashes'][0].sum()
    inc = np.array([[True, False, True, True, False]])
    r2 = against_restatement(q['pos'], q['v'], q['ptr'], include=inc, what='docked, include')
    same(r2, r, 'include changes the histograms only', GR.COUNT_KEYS + GR.CLASH_KEYS)
    assert 0 < r2['hist'].sum() < r['hist'].sum()


def test_fixture_sizes_every_frame_with_an_oversize_molecule_and_include():
    q, r, want = sizes_geometry()
    assert np.diff(q['ptr']).tolist() == [0, 1, 2, 63, 64, 65, 130, 300, 600] and not q['include'].all() and q['pos'].shape[0] > 1
    same(r, want, 'sizes')
    for k in GR.COUNT_KEYS + ('n_clashes',):
        assert (r[k][:, 8] == -1).all() and (r[k][:, :8] >= 0).all(), k
    assert r['n_angles'].sum() > 0 and r['n_torsions'].sum() > 0 and r['n_clashes'][:, :8].sum() > 0
    assert (r['hist'].sum((0, 2)) > 0).sum() >= 6                                 # sparse clouds: the lattice pack below fills every profile
    # without include every molecule enters; the frames are histogrammed apart
    every = against_restatement(q['pos'], q['v'], q['ptr'], what='sizes, include=None')
    same(every, r, 'include=None', GR.COUNT_KEYS + ('n_clashes',))
    assert (every['hist'] >= r['hist']).all() and (every['hist'] != r['hist']).any()
    for s in range(q['pos'].shape[0]):
        one = geom(q['pos'][s:s + 1], q['v'][s:s + 1], q['ptr'], PROFILES, q['include'][s:s + 1])
        same(one, {k: want[k][s:s + 1] for k in GR.KEYS if k != 'atom_clash'}, f'frame {s} alone', tuple(k for k in GR.KEYS if k != 'atom_clash'))


def test_trajectory_1000_frames():
    """the 1000-frame trajectory of sample_small_1000 in one call; the restatement on every ninth frame and the last"""
    t = load_golden('sample_small_1000.npz')
    ptr = load_golden('quality_traj.npz')['ptr']
    v = t['v_traj'].astype(np.int64)
    r = geom(t['pos_traj'], v, ptr)
    pick = sorted(set(range(0, 1000, 9)) | {999})
    want = GR.geometry_report(t['pos_traj'][pick], v[pick], ptr, CLASS_Z, AROMATIC, PROFILES, None, TABLE)
    same({k: r[k][pick] for k in GR.KEYS}, want, 'picked frames')
    assert r['n_angles'].sum() > 0 and r['n_torsions'].sum() > 0 and r['n_clashes'].sum() > 0


def lattice_molecule(n, seed):
    """n atoms of a jittered cubic lattice (1.5 A, 70 % of the sites nearest the centre) in random order, C / N / O of both kinds"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil((n / 0.7) ** (1.0 / 3.0))) + 2
    sites = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing='ij'), -1).reshape(-1, 3).astype(np.float64)
    sites = sites[np.argsort(((sites - (side - 1) / 2.0) ** 2).sum(1), kind='stable')[:int(np.ceil(n / 0.7))]]
    keep = rng.permutation(len(sites))[:n]
    return 1.5 * sites[keep] + rng.normal(0.0, 0.12, (n, 3)), rng.choice([C, C, C, C_ARO, N, O], n)


def pack(mols, apart=80.0):
    """[(pos [n, 3], classes [n] or one class)] -> pos [1, N, 3] fp32, v [1, N], ptr; the molecules `apart` A apart along z"""
    pos, v, ptr = [], [], [0]
    for k, (p, c) in enumerate(mols):
        p = np.asarray(p, np.float64).reshape(-1, 3)
        pos.append(p + np.array([0.0, 0.0, apart * k]))
        v.append(np.full(len(p), c, np.int64) if np.isscalar(c) else np.asarray(c, np.int64))
        ptr.append(ptr[-1] + len(p))
    return np.concatenate(pos).astype(np.float32)[None], np.concatenate(v)[None], np.asarray(ptr)


def test_sizes_around_the_instantiation_boundary_and_the_limit_under_every_filter():
    """two frames, so that the histograms of the frames are kept apart; every one of the 16 profiles is populated"""
    sizes = (127, 128, 129, 511, 512)
    frames = [pack([lattice_molecule(n, n + 1000 * s) for n in sizes]) for s in range(2)]
    pos, v, ptr = np.concatenate([f[0] for f in frames]), np.concatenate([f[1] for f in frames]), frames[0][2]
    r = against_restatement(pos, v, ptr, what='lattice')
    assert (r['n_angles'] > np.asarray(sizes)).all() and (r['n_torsions'] > np.asarray(sizes)).all() and (r['n_clashes'] > 0).all()
    assert (r['hist'].sum(2) > 0).all() and (r['hist'][0] != r['hist'][1]).any()
    inc = np.array([[True, False, True, True, False], [False, True, True, False, True]])
    r2 = against_restatement(pos, v, ptr, include=inc, what='lattice, include')
    same(r2, r, 'include changes the histograms only', GR.COUNT_KEYS + GR.CLASH_KEYS)
    assert (r2['hist'].sum(2) > 0).all() and (r2['hist'] <= r['hist']).all() and r2['hist'].sum() < r['hist'].sum()


def planted():
    """name -> (pos, classes): exact fp32 coordinates, carbons unless said otherwise (C-C: bonded below 1.64 A)"""
    ring8 = [(0.25, 1.0 * np.cos(a), 1.0 * np.sin(a)) for a in np.pi / 2 * np.arange(4)] + \
            [(-0.625, 0.75 * np.cos(a), 0.75 * np.sin(a)) for a in np.pi / 4 + np.pi / 2 * np.arange(4)]
    tail = [(0.0, 0.0, 0.0), (1.5, 0.0, 0.0), (2.25, 1.25, 0.0), (3.75, 1.25, 0.0)]      # the hub, then a chain of three carbons
    return dict(
        right=([(1.5, 0, 0), (0, 0, 0), (0, 1.5, 0)], C),
        straight=([(-1.5, 0, 0), (0, 0, 0), (1.5, 0, 0)], C),
        cis=([(-0.5, 1.25, 0), (0, 0, 0), (1.5, 0, 0), (2.0, 1.25, 0)], C),
        trans=([(-0.5, 1.25, 0), (0, 0, 0), (1.5, 0, 0), (2.0, -1.25, 0)], C),
        collinear=([(0, 0, 0), (1.5, 0, 0), (3.0, 0, 0), (4.5, 0, 0)], C),
        coincident=([(0, 0, 0), (0, 0, 0), (1.5, 0, 0)], C),
        three_ring=([(0, 0, 0), (1.5, 0, 0), (0.75, 1.25, 0), (-0.5, -1.25, 0)], C),
        folded=([(-0.5, 0, 0.5), (0, 0, 0), (1.5, 0, 0), (1.5, 1.5, 0), (0.5, 1.5, 1.0)], C),
        two_fragments=([(0, 0, 0), (1.5, 0, 0), (0, 2.0, 0), (1.5, 2.0, 0)], C),
        hub8=(tail + ring8[:7], [C] * 4 + [H] * 7),
        hub9=(tail + ring8, [C] * 4 + [H] * 8),
        no_class=([(0, 0, 0), (1.5, 0, 0), (3.0, 0, 0), (4.5, 0, 0), (6.0, 0, 0)], [C, C, 13, C, C]),
        no_class_negative=([(0, 0, 0), (1.5, 0, 0), (3.0, 0, 0)], [C, -1, C]))


def test_planted_molecules():
    mols = planted()
    names = list(mols)
    pos, v, ptr = pack([mols[k] for k in names])
    edges = np.array([-1.0, -0.5, 0.0, 0.5, 1.0])
    prof = (('angle', (0, 0, 0), 0, 0, edges), ('torsion', (0, 0, 0, 0), 0, 0, edges))
    r = against_restatement(pos, v, ptr, prof, what='planted')
    got = {k: tuple(int(r[q][0, g]) for q in GR.COUNT_KEYS + ('n_clashes',)) for g, k in enumerate(names)}
    one = lambda g: geom(pos[:, ptr[g]:ptr[g + 1]], v[:, ptr[g]:ptr[g + 1]], [0, ptr[g + 1] - ptr[g]], prof)
    hist = {k: one(g)['hist'][0] for g, k in enumerate(names)}
    bins = lambda h: {int(b): int(h[b]) for b in np.nonzero(h)[0]}
    # (angles, torsions, degenerate, crowded, clashes); a value equal to an edge lands in the bin that ends at it (searchsorted 'left')
    assert got['right'] == (1, 0, 0, 0, 0) and bins(hist['right'][0]) == {2: 1}                  # c == 0 == edges[2]
    assert got['straight'] == (1, 0, 0, 0, 0) and bins(hist['straight'][0]) == {0: 1}            # c == -1 == edges[0]
    assert got['cis'] == (2, 1, 0, 0, 0) and bins(hist['cis'][1]) == {4: 1}                      # c == +1 == edges[4]
    assert got['trans'] == (2, 1, 0, 0, 0) and bins(hist['trans'][1]) == {0: 1}                  # c == -1
    assert got['collinear'] == (2, 0, 1, 0, 0) and bins(hist['collinear'][0]) == {0: 2}          # the ends, 3 A apart, are 3 bonds apart
    assert got['coincident'] == (1, 0, 2, 0, 0) and bins(hist['coincident'][0]) == {4: 1}        # the angle at the third atom: c == 1
    assert got['three_ring'] == (5, 2, 0, 0, 0)                                                  # no (i, j, k, i)
    assert got['folded'] == (3, 2, 0, 0, 1) and r['atom_clash'][0, ptr[names.index('folded')]:ptr[names.index('folded') + 1]].tolist() == [1, 0, 0, 0, 1]
    assert got['two_fragments'] == (0, 0, 0, 0, 2)
    assert got['hub8'][:4] == (28 + 2, 7 + 1, 0, 0) and got['hub9'][:4] == (2, 1, 0, 1)          # the cap: on the centre and the central bond only
    assert got['no_class'] == (0, 0, 0, 0, 0) and got['no_class_negative'] == (0, 0, 0, 0, 0)
    # the 1-4 pair of the folded chain is exactly as far apart as its clashing 1-5 pair
    f = pos[0, ptr[names.index('folded')]:ptr[names.index('folded') + 1]].astype(np.float64)
    assert ((f[0] - f[4]) ** 2).sum() == ((f[1] - f[4]) ** 2).sum() == 3.5


def test_null_outputs_clash_pass_off_and_a_side_stream():
    dev = _dev()
    q, base, _ = sizes_geometry()
    args = (q['pos'], q['v'], q['ptr'], PROFILES, q['include'])
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        side = geom(*args)
        bare = geom(*args, atom_clash=False)
        off = geom(*args, table=None)
    torch.cuda.current_stream(dev).wait_stream(st)
    same(side, base, 'side stream')
    assert bare['atom_clash'] is None and off['atom_clash'] is None and off['n_clashes'] is None
    same(bare, base, 'atom_clash == NULL', tuple(k for k in GR.KEYS if k != 'atom_clash'))
    same(off, base, 'no clash pass', GR.COUNT_KEYS + ('hist',))
    # no profiles at all, and profiles without a ring filter and without bond_ptr / bond_ring
    none = geom(q['pos'], q['v'], q['ptr'], (), q['include'])
    same(none, base, 'P = 0', GR.COUNT_KEYS + GR.CLASH_KEYS)
    assert none['hist'].shape == (q['pos'].shape[0], 0, 128)
    keep = [k for k, p in enumerate(PROFILES) if p[3] in (0, 'any')]
    plain = geom(q['pos'], q['v'], q['ptr'], NO_RING, q['include'])
    np.testing.assert_array_equal(plain['hist'], base['hist'][:, keep])
    # an asymmetric table is read as the pair's lower atom first: with the lower triangle zeroed some clashes go
    n8 = q['ptr'][8]
    sub = (q['pos'][:, :n8], q['v'][:, :n8], q['ptr'][:9])
    lop = np.triu(TABLE)
    r = geom(*sub, (), None, lop)
    same(r, GR.geometry_report(*sub, CLASS_Z, AROMATIC, (), None, lop), 'asymmetric table')
    assert 0 < r['n_clashes'].sum() < base['n_clashes'][:, :8].sum()


def test_ring_filter_reads_the_ring_report_and_nothing_beyond_it():
    """the two ring modes split every torsion profile; a bond_ring of zeros or ones moves everything to one side; a short n_bonds
    matches neither"""
    dev = _dev()
    q, base, _ = sizes_geometry()
    names = [p[3] for p in PROFILES]
    any_p, ring_p, chain_p = 8, 14, 15
    assert (names[any_p], names[ring_p], names[chain_p]) == (0, 'ring', 'chain')
    np.testing.assert_array_equal(base['hist'][:, ring_p] + base['hist'][:, chain_p], base['hist'][:, any_p])
    assert base['hist'][:, ring_p].sum() > 0 and base['hist'][:, chain_p].sum() > 0
    n8 = q['ptr'][8]                                                             # without the oversize molecule
    p = torch.as_tensor(np.ascontiguousarray(q['pos'][:, :n8]), device=dev)
    c = torch.as_tensor(np.ascontiguousarray(q['v'][:, :n8]), dtype=torch.int64, device=dev)
    lp = torch.as_tensor(q['ptr'][:9], dtype=torch.int32, device=dev)
    inc = torch.as_tensor(q['include'][:, :8].copy(), dtype=torch.bool, device=dev)
    bp = capi.bond_graph(p, c, lp, CLASS_Z, AROMATIC, (), None, False, True)['bond_ptr']
    ring = capi.ring_report(p, c, lp, CLASS_Z, AROMATIC, None, bp, False)['bond_ring']
    prof = (PROFILES[any_p], PROFILES[ring_p], PROFILES[chain_p])
    call = lambda br: capi.geometry_report(p, c, lp, CLASS_Z, AROMATIC, prof, inc, None, bp, br, check=False)['hist'].cpu().numpy()
    real, zeros, ones = call(ring), call(torch.zeros_like(ring)), call(torch.ones_like(ring))
    np.testing.assert_array_equal(real, base['hist'][:, [any_p, ring_p, chain_p]])
    np.testing.assert_array_equal(zeros[:, 2], real[:, 0])
    np.testing.assert_array_equal(ones[:, 1], real[:, 0])
    assert not zeros[:, 1].any() and not ones[:, 2].any()
    short = call(ring[:7].contiguous())                                         # n_bonds = 7: a bond at or beyond it matches neither mode
    np.testing.assert_array_equal(short[:, 0], real[:, 0])
    assert (short[:, 1:] <= real[:, 1:]).all() and short[:, 1:].sum() < real[:, 1:].sum()


def test_oversize_molecules():
    n = 513
    line = np.stack([1.5 * np.arange(n), np.zeros(n), np.zeros(n)], 1)
    pos, v, ptr = pack([(line[:4], C), (line, C), (line[:3], C)], apart=5.0)
    r = against_restatement(pos, v, ptr, what='oversize')
    assert r['n_angles'][0].tolist() == [2, -1, 1] and r['n_degenerate'][0].tolist() == [1, -1, 0] and r['n_clashes'][0].tolist() == [0, -1, 0]
    dev = _dev()
    with pytest.raises(ValueError, match='513 atoms'):
        quality.geometry(pos[0], v[0], ligand_ptr=ptr)
    with pytest.raises(ValueError, match='513 atoms'):
        capi.geometry_report(torch.as_tensor(pos, device=dev), torch.as_tensor(v, device=dev), torch.as_tensor(ptr, dtype=torch.int32, device=dev),
                             CLASS_Z, AROMATIC)


def test_geometry_of_a_sampled_trajectory(tmp_path, capsys):
    """4 samples x 20 steps on a small pocket with seeded random weights, the run of test_gpu_bonds.py: the reports equal the restatement"""
    from oracle import draws
    from targetdiff_amd import sampling, workloads
    from test_gpu_bonds import _model
    dev = _dev()
    pk = workloads.synthetic_pocket(301, 70, 3.0, 9.0)
    data = types.SimpleNamespace(protein_pos=torch.from_numpy(pk.pos), protein_atom_feature=torch.from_numpy(pk.feat))
    src = draws.Source(9900, dev)
    sizes = [6, 9, 4, 11]
    res = sampling.sample_diffusion_ligand(_model(), data, 4, batch_size=4, device=dev, ligand_num_atoms=sizes, num_steps=20,
                                           noise_source=lambda b, st, name, like: src(st + 1, name, like))
    pos = np.concatenate([p.astype(np.float32) for p in res[2]], axis=1)
    v = np.concatenate(res[3], axis=1)
    ptr = np.cumsum([0] + sizes)
    deg = quality.default_geometry_profiles()
    cosp = quality._cosine_profiles(deg)
    want = GR.geometry_report(pos, v, ptr, CLASS_Z, AROMATIC, cosp, None, TABLE)
    rep = quality.sample_geometry(res, 'all')
    assert rep.num_frames == 20 and rep.n_samples == 4 and rep.n_included.tolist() == [4] * 20
    for p, prof in enumerate(deg):
        m = len(prof[4])
        np.testing.assert_array_equal(rep.hist[:, p, :m + 1], want['hist'][:, p, :m + 1][:, ::-1], err_msg=rep.names[p])
        assert not rep.hist[:, p, m + 1:].any()
    np.testing.assert_array_equal(rep.sum_clashes, want['n_clashes'].sum(1))
    np.testing.assert_array_equal(rep.n_clash_free, (want['n_clashes'] == 0).sum(1))
    for k, x in (('n_angles', rep.n_angles), ('n_torsions', rep.n_torsions), ('n_crowded', rep.n_crowded), ('n_degenerate', rep.n_degenerate)):
        np.testing.assert_array_equal(x, want[k].sum(1), err_msg=k)
    assert rep.hist.sum() > 0 and want['n_angles'].sum() > 0
    # the histograms of all frames together are the sum of the frames' own
    g = quality.geometry(pos, v, ligand_ptr=ptr)
    np.testing.assert_array_equal(g.hist.cpu().numpy().sum(0), rep.hist.sum(0))
    np.testing.assert_array_equal(g.atom_clash.cpu().numpy(), want['atom_clash'])
    np.testing.assert_array_equal(g.clash_free.cpu().numpy(), want['n_clashes'] == 0)
    mask = BR.bond_graph(pos[-1:], v[-1:], ptr, CLASS_Z, AROMATIC)['n_fragments'] == 1
    last = quality.sample_geometry(res, -1, include='complete')
    w = GR.geometry_report(pos[-1:], v[-1:], ptr, CLASS_Z, AROMATIC, cosp, mask, TABLE)
    assert last.n_included.tolist() == [int(mask.sum())] and last.sum_clashes.tolist() == [int(w['n_clashes'][mask].sum())]
    np.testing.assert_array_equal(last.hist[0, :, :91].sum(1), w['hist'][0, :, :91].sum(1))
    # a reference through the same kernel; the tool; the SD files
    mols = [(pos[-1, a:b], v[-1, a:b]) for a, b in zip(ptr[:-1], ptr[1:])]
    ref = quality.geometry_reference(mols)
    for p, name in enumerate(rep.names):
        np.testing.assert_array_equal(ref[name], rep.counts(name, -1))
    with_ref = quality.sample_geometry(res, -1, reference=ref)
    assert all(x is None or x == 0.0 for x in with_ref.js(-1).values())
    save_results(tmp_path, {0: res})
    out = load_tool('evaluate_samples').main(['--sample_path', str(tmp_path), '--geometry', '--eval_step', 'all'])
    text = capsys.readouterr().out
    assert out['geometry']['clash_free'] == rep.clash_free(-1) and out['geometry']['mean_clashes'] == want['n_clashes'][-1].sum() / 4
    assert f'clash_free:\t{rep.clash_free(-1):.4f}' in text and len(out['geometry']['curve']) == 20
    assert out['geometry']['hist']['CCC'] == rep.counts('CCC', -1).tolist()
    tool = load_tool('export_sdf')
    done = tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'free'), '--clash-free'])
    free = want['n_clashes'][-1] == 0
    assert done['result_0']['written'] == done['result_0']['clash_free'] == int(free.sum())
    recs = parse_sdf(open(tmp_path / 'free' / 'result_0.sdf').read())
    assert [len(a) for _, a, _, _ in recs] == [n for n, f in zip(sizes, free) if f]
