"""td_ring_report on the GPU (csrc/rings.hip) against tests/_rings_ref.py, array_equal throughout (the restatement is pinned to
networkx and to known answers on the host, tests/test_rings_host.py).

  1. the fixture packs: the docked ligand and its jittered copies, the sizes pack (both instantiations, a 600-atom molecule that is
     refused with -1) and the 1000-frame trajectory.
  2. constructed molecules of class-1 carbons: regular n-gons as rings up to the instantiation boundary 128 | 129, a 40-ring that
     saturates bit 31, a 512-ring stored in random order, a cube, fused and spiro rings, two aromatic rings joined by one bond, chains,
     a single atom, an empty molecule, two fragments, a ring opened by an atom of no class, collapsed clouds (complete graphs).
  3. a molecule's result depends on that molecule alone: frames one by one, molecules reversed, an unrelated pack in front, a side
     stream, null optional outputs; include changes ring_hist only.
  4. the per-bond outputs are aligned with td_bond_list's; oversize molecules.
  5. end to end: sample_rings and tools/export_sdf.py --ring-aromatic on the driver's trajectories.
"""
import types

import numpy as np
import pytest
import torch

import _bonds_ref as BR
import _rings_ref as RR
from conftest import load_golden
from targetdiff_amd import capi, quality
from test_bonds_host import load_tool, parse_sdf, save_results

pytestmark = pytest.mark.gpu

CLASS_Z = quality.class_atomic_numbers('add_aromatic')
AROMATIC = quality.class_aromatic('add_aromatic')
KEYS = RR.GRAPH_KEYS + RR.LIST_KEYS
C, C_ARO = 1, 2                                                             # classes of 'add_aromatic'
SIDE = 1.45                                                                 # a C-C single bond: 1.39 <= d < 1.64


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


def rings(pos, v, ptr, include=None, atom_ring=True, bonds=True, check=False):
    """capi.bond_graph + capi.bond_list + capi.ring_report of numpy inputs, as numpy; class_category: td_bond_list's category"""
    dev = _dev()
    inc = None if include is None else torch.as_tensor(np.ascontiguousarray(include), dtype=torch.bool, device=dev)
    p, c = torch.as_tensor(np.ascontiguousarray(pos), device=dev), torch.as_tensor(np.ascontiguousarray(v), dtype=torch.int64, device=dev)
    lp = torch.as_tensor(np.asarray(ptr), dtype=torch.int32, device=dev)
    out = {}
    bond_ptr = None
    if bonds:
        g = capi.bond_graph(p, c, lp, CLASS_Z, AROMATIC, (), None, False, True, check=check)
        lst = capi.bond_list(p, c, lp, CLASS_Z, AROMATIC, g['bond_ptr'], check=check)
        bond_ptr = g['bond_ptr']
        out.update(bond_ptr=bond_ptr, bond_atoms=lst['bond_atoms'], class_category=lst['bond_category'], bond_order=lst['bond_order'])
    out.update(capi.ring_report(p, c, lp, CLASS_Z, AROMATIC, inc, bond_ptr, atom_ring, check=check))
    return {k: (None if t is None else t.cpu().numpy()) for k, t in out.items()}


def same(a, b, what, keys=KEYS):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f'{what}: {k}')


def against_restatement(pos, v, ptr, include=None, what=''):
    r = rings(pos, v, ptr, include)
    want = RR.ring_report(pos, v, ptr, CLASS_Z, AROMATIC, include)
    for g in np.nonzero(np.diff(ptr) > RR.MAX_ATOMS)[0]:                        # the atoms of a refused molecule are not written
        r['atom_ring'][:, ptr[g]:ptr[g + 1]] = 0
    same(r, want, what, KEYS + ('bond_ptr', 'bond_atoms', 'class_category'))
    return r


_CACHE = {}


def sizes_rings():
    """the sizes pack of the bond fixtures through the kernels, once: the baseline of the independence tests"""
    if 'sizes' not in _CACHE:
        g = load_golden('bonds_sizes.npz')
        _CACHE['sizes'] = (g, rings(g['pos'], g['v'], g['ptr'], g['include']))
    return _CACHE['sizes']


def test_fixture_docked():
    q = load_golden('quality_docked.npz')
    r = against_restatement(q['pos'], q['v'], q['ptr'], what='docked')
    assert r['ring_mask'].dtype == np.int64 and r['n_ring_bonds'].dtype == np.int32 and r['atom_ring'].dtype == np.int32
    assert r['ring_hist'].dtype == np.int64 and r['ring_hist'].shape == (1, 32) and r['bond_ring'].dtype == np.int16
    assert r['bond_category'].dtype == np.uint8
    assert r['ring_mask'][0].tolist() == [72, 64, 72, 0, 8] and r['n_ring_bonds'][0].tolist() == [15, 12, 9, 0, 6]
    ring_aro = [int((r['bond_category'][a:b] == 4).sum()) for a, b in zip(r['bond_ptr'][:-1], r['bond_ptr'][1:])]
    class_aro = [int((r['class_category'][a:b] == 4).sum()) for a, b in zip(r['bond_ptr'][:-1], r['bond_ptr'][1:])]
    assert ring_aro == [1, 1, 1, 0, 0] and class_aro == [1, 1, 1, 1, 0]


def test_fixture_sizes_with_an_oversize_molecule_and_include():
    q = load_golden('quality_sizes.npz')
    assert np.diff(q['ptr']).tolist() == [0, 1, 2, 63, 64, 65, 130, 300, 600] and not q['include'].all()
    r = against_restatement(q['pos'], q['v'], q['ptr'], q['include'], what='sizes')
    assert (r['n_ring_bonds'][:, 8] == -1).all() and (r['n_ring_atoms'][:, 8] == -1).all() and not r['ring_mask'][:, 8].any()
    assert r['ring_hist'][:, 3:].sum() > 0 and r['ring_hist'][:, 0].sum() > 0


def test_trajectory_1000_frames():
    """the 1000-frame trajectory of sample_small_1000 in one call; the restatement on every ninth frame and the last"""
    t = load_golden('sample_small_1000.npz')
    ptr = load_golden('quality_traj.npz')['ptr']
    B = len(ptr) - 1
    v = t['v_traj'].astype(np.int64)
    r = rings(t['pos_traj'], v, ptr)
    pick = sorted(set(range(0, 1000, 9)) | {999})
    want = RR.ring_report(t['pos_traj'][pick], v[pick], ptr, CLASS_Z, AROMATIC)
    for k in RR.GRAPH_KEYS:
        np.testing.assert_array_equal(r[k][pick], want[k], err_msg=k)
    rows = np.concatenate([np.arange(r['bond_ptr'][s * B], r['bond_ptr'][(s + 1) * B]) for s in pick])
    same({k: r[k][rows] for k in RR.LIST_KEYS}, want, 'picked frames', RR.LIST_KEYS)
    bits = (r['ring_mask'][:, :, None] >> np.arange(32)) & 1
    bits[:, :, 0] = r['ring_mask'] == 0
    np.testing.assert_array_equal(r['ring_hist'], bits.sum(1))
    assert r['ring_hist'][:, 3:].sum() > 0


def ngon(n, centre=(0.0, 0.0, 0.0), side=SIDE, start=0.0):
    """n atoms on a regular polygon of side `side` in the xy plane"""
    R = side / (2.0 * np.sin(np.pi / n))
    a = start + 2.0 * np.pi * np.arange(n) / n
    return np.stack([centre[0] + R * np.cos(a), centre[1] + R * np.sin(a), centre[2] + np.zeros(n)], 1)


def polygon_on_edge(p0, p1, m, inside):
    """the m - 2 further corners of the regular m-gon (in the xy plane) on the edge p0 -> p1, on the side away from `inside`"""
    mid, side = (p0 + p1) / 2.0, np.linalg.norm(p1 - p0)
    normal = np.array([-(p1 - p0)[1], (p1 - p0)[0], 0.0]) / side
    if np.dot(normal, mid - inside) < 0:
        normal = -normal
    c = mid + normal * side / (2.0 * np.tan(np.pi / m))
    for sign in (1.0, -1.0):
        t = sign * 2.0 * np.pi / m * np.arange(m)
        d = p0 - c
        pts = c + np.stack([np.cos(t) * d[0] - np.sin(t) * d[1], np.sin(t) * d[0] + np.cos(t) * d[1], np.zeros(m)], 1)
        if np.linalg.norm(pts[1] - p1) < 1e-9:
            return pts[2:]
    raise AssertionError('no orientation closes the polygon')


def pack(mols):
    """[(pos [n, 3], classes [n] or one class)] -> pos [1, N, 3] fp32, v [1, N], ptr; the molecules 40 A apart along z"""
    pos, v, ptr = [], [], [0]
    for k, (p, c) in enumerate(mols):
        p = np.asarray(p, np.float64).reshape(-1, 3)
        pos.append(p + np.array([0.0, 0.0, 40.0 * k]))
        v.append(np.full(len(p), c, np.int64) if np.isscalar(c) else np.asarray(c, np.int64))
        ptr.append(ptr[-1] + len(p))
    return np.concatenate(pos).astype(np.float32)[None], np.concatenate(v)[None], np.asarray(ptr)


def molecule_of(r, ptr, g):
    """(bond ring sizes, ring-aware categories, atom ring sizes) of molecule g of a one-frame result"""
    a, b = r['bond_ptr'][g], r['bond_ptr'][g + 1]
    return r['bond_ring'][a:b].tolist(), r['bond_category'][a:b].tolist(), r['atom_ring'][0, ptr[g]:ptr[g + 1]].tolist()


def test_regular_polygons_are_rings_of_their_size():
    sizes = (3, 4, 5, 6, 7, 12, 40, 128, 129)
    rng = np.random.default_rng(5)
    mols = [(ngon(n)[rng.permutation(n)], C) for n in sizes]
    pos, v, ptr = pack(mols)
    r = against_restatement(pos, v, ptr, what='polygons')
    for g, n in enumerate(sizes):
        ring, cat, atoms = molecule_of(r, ptr, g)
        assert ring == [n] * n and cat == [1] * n and atoms == [n] * n, n
        assert r['ring_mask'][0, g] == 1 << min(n, 31) and r['n_ring_bonds'][0, g] == n and r['n_ring_atoms'][0, g] == n
    want = np.zeros(32, np.int64)
    want[[3, 4, 5, 6, 7, 12]] = 1
    want[31] = 3                                                                # 40, 128 and 129 saturate the last bit
    assert r['ring_hist'][0].tolist() == want.tolist()


def test_ring_of_512_atoms_in_random_order():
    n = 512
    place = np.random.default_rng(11).permutation(n)
    pos, v, ptr = pack([(ngon(n)[place], C), (ngon(130)[::-1], C)])
    r = against_restatement(pos, v, ptr, what='512-ring')
    assert molecule_of(r, ptr, 0) == ([n] * n, [1] * n, [n] * n) and molecule_of(r, ptr, 1) == ([130] * 130, [1] * 130, [130] * 130)
    assert r['ring_mask'][0].tolist() == [1 << 31] * 2 and r['ring_hist'][0, 31] == 2 and r['ring_hist'][0, :31].sum() == 0
    # cut open, it is a chain of bridges
    pos2 = pos.copy()
    pos2[0, 7] += np.float32(5.0)
    r = against_restatement(pos2, v, ptr, what='512-chain')
    assert r['n_ring_bonds'][0].tolist() == [0, 130] and set(molecule_of(r, ptr, 0)[0]) == {0} and r['ring_hist'][0, 0] == 1


def constructed():
    """the small constructed molecules: name -> (pos, classes)"""
    cube = np.array([[x, y, z] for x in (0.0, 1.5) for y in (0.0, 1.5) for z in (0.0, 1.5)])
    six = ngon(6)
    inside = six.mean(0)
    two_six = np.concatenate([six, polygon_on_edge(six[0], six[1], 6, inside)])
    six_five = np.concatenate([six, polygon_on_edge(six[0], six[1], 5, inside)])
    # spiro: a hexagon in the xy plane and a pentagon in the xz plane that share the atom at the origin and nothing else
    hexa = ngon(6, (-SIDE, 0.0, 0.0))                                            # its corner 0 is the origin (R = side for a hexagon)
    penta = ngon(5, (SIDE / (2.0 * np.sin(np.pi / 5)), 0.0, 0.0), start=np.pi)[:, [0, 2, 1]]
    spiro = np.concatenate([hexa, penta[1:]])
    left, right = ngon(6), ngon(6, (2 * SIDE + 1.48, 0.0, 0.0), start=np.pi)     # corner 0 of each faces the other ring
    chain = np.stack([1.5 * np.arange(9), np.zeros(9), np.zeros(9)], 1)
    two_fragments = np.concatenate([ngon(3), ngon(4, (10.0, 0.0, 0.0))])
    return dict(cube=(cube, C), two_six=(two_six, C), six_five=(six_five, C), spiro=(spiro, C),
                biphenyl=(np.concatenate([left, right]), C_ARO), chain=(chain, C), atom=(np.zeros((1, 3)), C), empty=(np.zeros((0, 3)), C),
                two_fragments=(two_fragments, C), opened=(six, [C, C, 13, C, C, C]), opened_negative=(six, [C, C, C, C, -1, C]),
                aromatic_triangle=(ngon(3), C_ARO))


def test_constructed_molecules():
    mols = constructed()
    names = list(mols)
    pos, v, ptr = pack([mols[k] for k in names])
    r = against_restatement(pos, v, ptr, what='constructed')
    got = {k: molecule_of(r, ptr, g) for g, k in enumerate(names)}
    mask = dict(zip(names, r['ring_mask'][0].tolist()))
    assert got['cube'] == ([4] * 12, [1] * 12, [4] * 8) and mask['cube'] == 1 << 4
    ring, cat, atoms = got['two_six']
    assert ring == [6] * 11 and atoms == [6] * 10 and mask['two_six'] == 1 << 6
    ring, cat, atoms = got['six_five']                                          # atoms 0, 1: the shared edge; 6 .. 8: the pentagon's own
    assert sorted(ring) == [5] * 5 + [6] * 5 and ring[0] == 5 and atoms == [5, 5, 6, 6, 6, 6, 5, 5, 5] and mask['six_five'] == (1 << 5 | 1 << 6)
    ring, cat, atoms = got['spiro']                                             # atom 0 is shared: it reads the smaller ring
    assert sorted(ring) == [5] * 5 + [6] * 6 and atoms == [5] + [6] * 5 + [5] * 4
    ring, cat, atoms = got['biphenyl']                                          # atoms 0 and 6 carry the link
    assert sorted(ring) == [0] + [6] * 12 and sorted(cat) == [1] + [4] * 12 and [c for x, c in zip(ring, cat) if x == 0] == [1]
    assert atoms == [6] * 12 and r['n_ring_bonds'][0, names.index('biphenyl')] == 12
    a, b = r['bond_ptr'][names.index('biphenyl')], r['bond_ptr'][names.index('biphenyl') + 1]
    assert r['class_category'][a:b].tolist() == [4] * 13                        # td_bond_list's own category stays as it is
    assert got['chain'] == ([0] * 8, [1] * 8, [0] * 9) and got['atom'] == ([], [], [0]) and got['empty'] == ([], [], [])
    assert got['two_fragments'] == ([3] * 3 + [4] * 4, [1] * 7, [3] * 3 + [4] * 4) and mask['two_fragments'] == (1 << 3 | 1 << 4)
    assert got['opened'] == ([0] * 4, [1] * 4, [0] * 6) and got['opened_negative'] == ([0] * 4, [1] * 4, [0] * 6)
    assert got['aromatic_triangle'] == ([3] * 3, [1] * 3, [3] * 3)              # aromatic classes in a 3-ring: not aromatic bonds
    assert r['ring_hist'][0].tolist() == [5, 0, 0, 2, 2, 2, 4] + [0] * 25


@pytest.mark.parametrize('n', [40, 130])
def test_collapsed_cloud_is_a_complete_graph(n):
    pos = (np.random.default_rng(n).uniform(-0.15, 0.15, (1, n, 3))).astype(np.float32)     # within 0.3 A of one point
    v = np.full((1, n), C, np.int64)
    r = against_restatement(pos, v, [0, n], what='cloud')
    nb = n * (n - 1) // 2
    assert r['bond_ptr'].tolist() == [0, nb] and (r['bond_ring'] == 3).all() and (r['atom_ring'] == 3).all()
    assert (r['n_ring_bonds'][0, 0], r['n_ring_atoms'][0, 0], r['ring_mask'][0, 0]) == (nb, n, 8)


def test_frames_one_by_one_reversed_and_behind_another_pack():
    g, base = sizes_rings()
    pos, v, ptr, inc = g['pos'], g['v'], g['ptr'], g['include']
    S, B = inc.shape
    assert np.diff(ptr).tolist() == [0, 1, 2, 63, 64, 65, 130, 300] and base['ring_hist'][:, 3:].sum() > 0
    same(base, RR.ring_report(pos, v, ptr, CLASS_Z, AROMATIC, inc), 'sizes')
    for s in range(S):
        one = rings(pos[s:s + 1], v[s:s + 1], ptr, inc[s:s + 1])
        same(one, {k: base[k][s:s + 1] for k in RR.GRAPH_KEYS}, f'frame {s} alone', RR.GRAPH_KEYS)
        a, b = base['bond_ptr'][s * B], base['bond_ptr'][(s + 1) * B]
        same(one, {k: base[k][a:b] for k in RR.LIST_KEYS}, f'frame {s} alone', RR.LIST_KEYS)
    # the molecules in reversed order
    order = np.concatenate([np.arange(ptr[b], ptr[b + 1]) for b in reversed(range(B))]).astype(np.int64)
    rptr = np.concatenate([[0], np.cumsum(np.diff(ptr)[::-1])])
    rev = rings(pos[:, order], v[:, order], rptr, inc[:, ::-1])
    np.testing.assert_array_equal(rev['atom_ring'], base['atom_ring'][:, order])
    for k in ('ring_mask', 'n_ring_bonds', 'n_ring_atoms'):
        np.testing.assert_array_equal(rev[k], base[k][:, ::-1], err_msg=k)
    np.testing.assert_array_equal(rev['ring_hist'], base['ring_hist'])
    for s in range(S):
        for b in range(B):
            k0, k1 = base['bond_ptr'][s * B + b], base['bond_ptr'][s * B + b + 1]
            q0, q1 = rev['bond_ptr'][s * B + B - 1 - b], rev['bond_ptr'][s * B + B - b]
            same({k: rev[k][q0:q1] for k in RR.LIST_KEYS}, {k: base[k][k0:k1] for k in RR.LIST_KEYS}, f'reversed {s} {b}', RR.LIST_KEYS)
    # an unrelated pack in front, kept out of the histogram by the mask
    d = load_golden('quality_docked.npz')
    n0 = d['pos'].shape[1]
    fpos = np.concatenate([np.repeat(d['pos'], S, 0) + np.float32(3.0), pos], axis=1)
    fv = np.concatenate([np.repeat(d['v'], S, 0), v], axis=1)
    fptr = np.concatenate([d['ptr'][:-1], ptr + n0])
    finc = np.concatenate([np.zeros((S, 5), bool), inc], axis=1)
    front = rings(fpos, fv, fptr, finc)
    np.testing.assert_array_equal(front['atom_ring'][:, n0:], base['atom_ring'])
    for k in ('ring_mask', 'n_ring_bonds', 'n_ring_atoms'):
        np.testing.assert_array_equal(front[k][:, 5:], base[k], err_msg=k)
    np.testing.assert_array_equal(front['ring_hist'], base['ring_hist'])
    mine = front['bond_atoms'][:, 0] >= n0
    same({k: front[k][mine] for k in RR.LIST_KEYS}, base, 'behind another pack', RR.LIST_KEYS)


def test_side_stream_null_outputs_and_include():
    dev = _dev()
    g, base = sizes_rings()
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        side = rings(g['pos'], g['v'], g['ptr'], g['include'])
        bare = rings(g['pos'], g['v'], g['ptr'], g['include'], atom_ring=False, bonds=False)
    torch.cuda.current_stream(dev).wait_stream(st)
    same(side, base, 'side stream')
    assert bare['atom_ring'] is None and bare['bond_ring'] is None and bare['bond_category'] is None
    same(bare, base, 'null optional outputs', ('ring_mask', 'n_ring_bonds', 'n_ring_atoms', 'ring_hist'))
    # include changes ring_hist and nothing else; ring_hist is the column sums of the mask bits over the included molecules
    every = rings(g['pos'], g['v'], g['ptr'], None)
    same(every, base, 'include=None', tuple(k for k in KEYS if k != 'ring_hist'))
    assert (every['ring_hist'] != base['ring_hist']).any()
    for r, inc in ((every, np.ones_like(g['include'])), (base, g['include'])):
        bits = (r['ring_mask'][:, :, None] >> np.arange(32)) & 1
        bits[:, :, 0] = r['ring_mask'] == 0
        np.testing.assert_array_equal(r['ring_hist'], (bits * inc[:, :, None]).sum(1))
    # one per-bond output without the other
    p, c = torch.as_tensor(g['pos'], device=dev), torch.as_tensor(g['v'], dtype=torch.int64, device=dev)
    lp, bp = torch.as_tensor(g['ptr'], dtype=torch.int32, device=dev), torch.as_tensor(base['bond_ptr'], device=dev)
    nb = int(base['bond_ptr'][-1])
    lib = capi.load_library()
    cz = np.asarray(CLASS_Z, np.int32)
    aro = np.asarray(AROMATIC, np.uint8)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    for which in ('ring', 'category'):
        mask, nrb, nra, hist = i32(3, 8), i32(3, 8), i32(3, 8), torch.empty(3, 32, dtype=torch.int64, device=dev)
        ring = torch.full((nb + 8,), -7, dtype=torch.int16, device=dev)
        cat = torch.full((nb + 8,), 77, dtype=torch.uint8, device=dev)
        rc = lib.td_ring_report(p.data_ptr(), c.data_ptr(), lp.data_ptr(), 3, p.shape[1], 8, cz.ctypes.data_as(capi.POINTER(capi.c_int32)), 13, None,
                                aro.ctypes.data_as(capi.POINTER(capi.ctypes.c_uint8)), bp.data_ptr(), nb, mask.data_ptr(), nrb.data_ptr(),
                                nra.data_ptr(), None, hist.data_ptr(), ring.data_ptr() if which == 'ring' else None,
                                cat.data_ptr() if which == 'category' else None, capi._stream(dev))
        assert rc == 0
        torch.cuda.synchronize(dev)
        if which == 'ring':
            np.testing.assert_array_equal(ring[:nb].cpu().numpy(), base['bond_ring'])
        else:
            np.testing.assert_array_equal(cat[:nb].cpu().numpy(), base['bond_category'])
        assert (ring[nb:] == -7).all() and (cat[nb:] == 77).all() and ((ring == -7).all() or (cat == 77).all())
        np.testing.assert_array_equal(hist.cpu().numpy(), every['ring_hist'])
    # a capacity below the pack's own number of bonds: nothing at or beyond it is written
    short = nb // 2
    ring = torch.full((nb,), -7, dtype=torch.int16, device=dev)
    rc = lib.td_ring_report(p.data_ptr(), c.data_ptr(), lp.data_ptr(), 3, p.shape[1], 8, cz.ctypes.data_as(capi.POINTER(capi.c_int32)), 13, None,
                            None, bp.data_ptr(), short, mask.data_ptr(), nrb.data_ptr(), nra.data_ptr(), None, hist.data_ptr(), ring.data_ptr(),
                            None, capi._stream(dev))
    assert rc == 0
    torch.cuda.synchronize(dev)
    np.testing.assert_array_equal(ring[:short].cpu().numpy(), base['bond_ring'][:short])
    assert (ring[short:] == -7).all()


def test_bond_outputs_are_aligned_with_the_bond_list():
    g, base = sizes_rings()
    S, B = g['include'].shape
    ptr = g['ptr']
    assert base['bond_ptr'][-1] == len(base['bond_ring']) == len(base['bond_category']) == len(base['bond_atoms'])
    for s in range(S):
        for b in range(B):
            k0, k1 = base['bond_ptr'][s * B + b], base['bond_ptr'][s * B + b + 1]
            atoms = base['bond_atoms'][k0:k1] - ptr[b]
            np.testing.assert_array_equal(base['bond_ring'][k0:k1], RR.bond_ring_sizes(ptr[b + 1] - ptr[b], atoms[:, 0], atoms[:, 1]))
    keep = base['class_category'] != 4
    np.testing.assert_array_equal(base['bond_category'][keep], base['class_category'][keep])
    aro = ~keep
    assert aro.any() and set(base['bond_category'][aro & np.isin(base['bond_ring'], (5, 6))].tolist()) <= {4}
    np.testing.assert_array_equal(base['bond_category'][aro & ~np.isin(base['bond_ring'], (5, 6))],
                                  base['bond_order'][aro & ~np.isin(base['bond_ring'], (5, 6))])
    # the public function
    bg = quality.bond_graph(g['pos'], g['v'], ligand_ptr=ptr, include=g['include'], return_bonds=True, rings=True)
    assert bg.ring_mask.is_cuda and bg.bond_ring.is_cuda
    for k, t in (('ring_mask', bg.ring_mask), ('n_ring_bonds', bg.n_ring_bonds), ('n_ring_atoms', bg.n_ring_atoms), ('atom_ring', bg.atom_ring),
                 ('bond_ring', bg.bond_ring), ('bond_category', bg.ring_category), ('class_category', bg.bond_category)):
        np.testing.assert_array_equal(t.cpu().numpy(), base[k], err_msg=k)
    a, o, c, d, ring, ring_cat = bg.molecule_bonds(1, 7)
    k0, k1 = base['bond_ptr'][1 * B + 7], base['bond_ptr'][1 * B + 8]
    np.testing.assert_array_equal(ring, base['bond_ring'][k0:k1])
    np.testing.assert_array_equal(ring_cat, base['bond_category'][k0:k1])
    plain = quality.bond_graph(g['pos'], g['v'], ligand_ptr=ptr, return_bonds=True)
    assert plain.bond_ring is None and plain.ring_mask is None and len(plain.molecule_bonds(1, 7)) == 4


def test_oversize_molecules():
    n = 513
    pos, v, ptr = pack([(ngon(6), C), (ngon(n), C), (ngon(5), C)])
    r = against_restatement(pos, v, ptr, what='oversize')
    assert r['n_ring_bonds'][0].tolist() == [6, -1, 5] and r['n_ring_atoms'][0].tolist() == [6, -1, 5]
    assert r['ring_mask'][0].tolist() == [1 << 6, 0, 1 << 5] and r['ring_hist'][0].sum() == 2 and r['ring_hist'][0, 0] == 0
    assert r['bond_ring'].tolist() == [6] * 6 + [5] * 5 and r['bond_ptr'].tolist() == [0, 6, 6, 11]
    with pytest.raises(ValueError, match='513 atoms'):
        quality.bond_graph(pos[0], v[0], ligand_ptr=ptr, rings=True)
    with pytest.raises(ValueError, match='513 atoms'):
        capi.ring_report(torch.as_tensor(pos, device=_dev()), torch.as_tensor(v, device=_dev()),
                         torch.as_tensor(ptr, dtype=torch.int32, device=_dev()), CLASS_Z, AROMATIC)
    big = ngon(n).astype(np.float32).astype(np.float64)
    with pytest.raises(ValueError, match='513 atoms'):
        quality.sample_rings(([], [], [big[None]], [np.ones((1, n), np.int64)], [], [], []))


def test_rings_of_a_sampled_trajectory(tmp_path):
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
    n = np.asarray(sizes, np.float64)
    want = RR.ring_report(pos, v, ptr, CLASS_Z, AROMATIC)
    rep = quality.sample_rings(res, 'all')
    assert rep.num_frames == 20 and rep.n_samples == 4 and rep.n_included.tolist() == [4] * 20
    np.testing.assert_array_equal(rep.ring_hist, want['ring_hist'])
    for s in range(20):
        assert rep.ring_ratio(s) == {k: want['ring_hist'][s, k] / 4 for k in range(3, 10)}
        assert rep.no_ring(s) == (want['ring_mask'][s] == 0).sum() / 4 and rep.large_ring(s) == (want['ring_mask'][s] >= 1024).sum() / 4
        assert rep.ring_atom_share(s) == (want['n_ring_atoms'][s] / n).sum() / 4
    mask = BR.bond_graph(pos[-1:], v[-1:], ptr, CLASS_Z, AROMATIC)['n_fragments'] == 1
    last = quality.sample_rings(res, -1, include='complete')
    np.testing.assert_array_equal(last.ring_hist, RR.ring_report(pos[-1:], v[-1:], ptr, CLASS_Z, AROMATIC, mask)['ring_hist'])
    assert last.n_included.tolist() == [int(mask.sum())] and last.num_frames == 1
    # the SD files: with the flag the ring-aware categories, without it the files of before
    save_results(tmp_path, {0: res})
    tool = load_tool('export_sdf')
    tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'plain')])
    tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'ring'), '--ring-aromatic'])
    w = RR.ring_report(pos[-1:], v[-1:], ptr, CLASS_Z, AROMATIC)
    for name, key in (('plain', 'class_category'), ('ring', 'bond_category')):
        recs = parse_sdf(open(tmp_path / name / 'result_0.sdf').read())
        assert len(recs) == 4
        for g, (_, atoms, bonds, _p) in enumerate(recs):
            k0, k1 = w['bond_ptr'][g], w['bond_ptr'][g + 1]
            assert bonds == [(int(i - ptr[g]), int(j - ptr[g]), int(c)) for (i, j), c in zip(w['bond_atoms'][k0:k1], w[key][k0:k1])]
    g = quality.bond_graph(pos[-1], v[-1], ligand_ptr=ptr, bond_profiles=(), return_fragments=True, return_bonds=True)
    from targetdiff_amd import molfile
    molfile.write_sdf(tmp_path / 'before.sdf', molfile.molecules_from_graph(g, pos[-1], v[-1]))
    assert open(tmp_path / 'before.sdf').read() == open(tmp_path / 'plain' / 'result_0.sdf').read()
