"""td_bond_graph / td_bond_list on the GPU (csrc/bonds.hip) against the reference's own results.

  1. every fixture of tools/make_golden_bonds.py (made with the real reference: get_bond_order per pair, scipy's connected components,
     get_bond_length_profile) through the kernels, array_equal throughout; bond lengths bit for bit.  quality_thresholds holds 425
     two-atom molecules within two fp32 ulps of a threshold: the order listed there flips with any other arithmetic.
  2. shapes made to break the propagation: a 512-atom chain stored in random order, the chain cut at a threshold exactly, fused rings,
     two aromatic rings joined by one bond.
  3. a molecule's result depends on that molecule alone: frames one by one, molecules reversed, an unrelated pack in front, a side
     stream, null optional outputs; include changes bond_hist only.
  4. the bond list: ascending order, bond_ptr, and per atom the listed orders sum to td_quality_report's nr_bonds.
  5. end to end: sample_connectivity, sample_quality(include='complete') and tools/export_sdf.py on the driver's trajectories equal
     tests/_bonds_ref.py (pinned to the same fixtures on the host).
"""
import types

import numpy as np
import pytest
import torch

import _bonds_ref as BR
import _quality_ref as QR
from conftest import load_golden
from oracle import draws, weights
from targetdiff_amd import capi, quality, workloads
from targetdiff_amd.schedule import TimeProgram
from test_bonds_host import load_tool, parse_sdf, save_results

pytestmark = pytest.mark.gpu

CLASS_Z = quality.class_atomic_numbers('add_aromatic')
AROMATIC = quality.class_aromatic('add_aromatic')
PROFILES = quality.default_bond_profiles()
GRAPH_KEYS = ('n_bonds', 'n_fragments', 'largest_fragment', 'fragment', 'bond_hist', 'bond_ptr')
LIST_KEYS = ('bond_atoms', 'bond_order', 'bond_category', 'bond_length')
C, C_ARO, N_ARO = 1, 2, 4                                                  # classes of 'add_aromatic'


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


def graph(pos, v, ptr, include=None, profiles=PROFILES, aromatic=AROMATIC, fragments=True, bond_ptr=True, bonds=True):
    """capi.bond_graph (+ capi.bond_list) of numpy inputs, as numpy"""
    dev = _dev()
    inc = None if include is None else torch.as_tensor(np.ascontiguousarray(include), dtype=torch.bool, device=dev)
    p, c = torch.as_tensor(np.ascontiguousarray(pos), device=dev), torch.as_tensor(np.ascontiguousarray(v), dtype=torch.int64, device=dev)
    lp = torch.as_tensor(np.asarray(ptr), dtype=torch.int32, device=dev)
    r = capi.bond_graph(p, c, lp, CLASS_Z, aromatic, profiles, inc, fragments, bond_ptr)
    if bonds and bond_ptr:
        r.update(capi.bond_list(p, c, lp, CLASS_Z, aromatic, r['bond_ptr']))
    return {k: (None if t is None else t.cpu().numpy()) for k, t in r.items()}


def same(a, b, what, keys=GRAPH_KEYS + LIST_KEYS):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f'{what}: {k}')


_CACHE = {}


def sizes_graph():
    """the sizes fixture through the kernels, once: the baseline of the independence tests"""
    if 'sizes' not in _CACHE:
        g = load_golden('bonds_sizes.npz')
        _CACHE['sizes'] = (g, graph(g['pos'], g['v'], g['ptr'], g['include']))
    return _CACHE['sizes']


def test_fixture_docked():
    g, q = load_golden('bonds_docked.npz'), load_golden('quality_docked.npz')
    r = graph(q['pos'], q['v'], q['ptr'])
    assert r['n_bonds'].dtype == np.int32 and r['bond_hist'].dtype == np.int64 and r['bond_hist'].shape == (1, 8, 128)
    assert r['bond_length'].dtype == np.float64 and r['bond_order'].dtype == np.uint8 and r['bond_ptr'].dtype == np.int64
    BR.check_against_fixture(r, g)
    rings = r['n_bonds'] - np.diff(q['ptr'])[None] + r['n_fragments']
    assert (r['n_bonds'][0, 0], r['n_fragments'][0, 0], rings[0, 0]) == (27, 1, 3)          # the docked 1h36 ligand: 25 atoms
    assert r['n_fragments'][0, 1:].tolist() == [3, 3, 8, 16]                                # its four jittered copies


def test_fixture_thresholds():
    g, q = load_golden('bonds_thresholds.npz'), load_golden('quality_thresholds.npz')
    r = graph(q['pos'], q['v'], q['ptr'])
    BR.check_against_fixture(r, g)
    order = g['pair_order']                                                                 # one pair per molecule
    np.testing.assert_array_equal(r['n_bonds'][0], order > 0)
    np.testing.assert_array_equal(r['n_fragments'][0], np.where(order > 0, 1, 2))
    np.testing.assert_array_equal(r['bond_order'], order[order > 0])
    assert set(r['n_fragments'][0].tolist()) == {1, 2} and set(r['bond_order'].tolist()) == {1, 2, 3}


def test_fixture_sizes_and_include_mask():
    g, r = sizes_graph()
    assert np.diff(g['ptr']).tolist() == [0, 1, 2, 63, 64, 65, 130, 300]                    # both instantiations, and their boundary below
    BR.check_against_fixture(r, g)
    assert r['n_fragments'][:, :3].tolist() == [[0, 1, 2]] * 3 and not g['include'].all()


def test_trajectory_1000_frames():
    """the 1000-frame trajectory of sample_small_1000 in one call; the restatement on every ninth frame and the last"""
    t = load_golden('sample_small_1000.npz')
    ptr = load_golden('quality_traj.npz')['ptr']
    B = len(ptr) - 1
    r = graph(t['pos_traj'], t['v_traj'], ptr)
    pick = sorted(set(range(0, 1000, 9)) | {999})
    want = BR.bond_graph(t['pos_traj'][pick], t['v_traj'][pick].astype(np.int64), ptr, CLASS_Z, AROMATIC, PROFILES)
    for k in ('n_bonds', 'n_fragments', 'largest_fragment', 'fragment', 'bond_hist'):
        np.testing.assert_array_equal(r[k][pick], want[k], err_msg=k)
    assert r['bond_ptr'][-1] == len(r['bond_order']) == r['n_bonds'].sum()
    rows = np.concatenate([np.arange(r['bond_ptr'][s * B], r['bond_ptr'][(s + 1) * B]) for s in pick])
    same({k: r[k][rows] for k in LIST_KEYS}, want, 'picked frames', LIST_KEYS)


def chain(n, seed, aromatic=False):
    """a C-C chain of n atoms, 1.5 A apart along x, stored in a seeded random order: (pos [1, n, 3], v [1, n], place)"""
    place = np.random.default_rng(seed).permutation(n)                                       # chain position k is stored at place[k]
    pos = np.zeros((1, n, 3), np.float32)
    pos[0, place, 0] = np.float32(1.5) * np.arange(n, dtype=np.float32)
    return pos, np.full((1, n), C_ARO if aromatic else C, np.int64), place


def test_chain_of_512_atoms_in_random_order():
    n = 512
    pos, v, place = chain(n, 11)
    r = graph(pos, v, [0, n], profiles=())
    assert (r['n_bonds'][0, 0], r['n_fragments'][0, 0], r['largest_fragment'][0, 0]) == (n - 1, 1, n)
    assert r['n_bonds'][0, 0] - n + r['n_fragments'][0, 0] == 0                             # rings
    assert not r['fragment'].any()                                                          # every label: the atom stored first
    assert set(r['bond_order'].tolist()) == {1} and r['bond_ptr'].tolist() == [0, n - 1]
    want = BR.bond_graph(pos, v, [0, n], CLASS_Z, AROMATIC)
    same(r, want, 'chain', ('fragment',) + LIST_KEYS)
    # two such chains and a 129-atom one in one pack, far apart: labels are molecule-local
    pos2, v2, _ = chain(n, 12)
    pos3, v3, _ = chain(129, 13)
    pack = np.concatenate([pos, pos2 + np.float32(50.0), pos3], axis=1)
    r = graph(pack, np.concatenate([v, v2, v3], axis=1), [0, n, 2 * n, 2 * n + 129], profiles=())
    assert r['n_fragments'].tolist() == [[1, 1, 1]] and r['n_bonds'].tolist() == [[n - 1, n - 1, 128]] and not r['fragment'].any()
    assert r['bond_ptr'].tolist() == [0, n - 1, 2 * n - 2, 2 * n + 126]


def test_chain_cut_at_the_threshold_exactly():
    """C-C: b1 + margin = 164 pm.  The atom at chain position 256 moves away from 255 (and towards 257, to which it stays bonded) to
    the first fp32 coordinate at which D = 100 d reaches 164 -- no bond: the rule is D < 164 -- and to the fp32 value just below"""
    n = 512
    pos, v, place = chain(n, 21)
    x255 = pos[0, place[255], 0]
    bonded = lambda x: 100.0 * np.sqrt((np.float64(x) - np.float64(x255)) ** 2) < 164.0     # the rule in float64; dy = dz = 0
    x = np.float32(x255 + np.float32(1.64))
    while not bonded(x):
        x = np.nextafter(x, np.float32(-np.inf))
    while bonded(np.nextafter(x, np.float32(np.inf))):
        x = np.nextafter(x, np.float32(np.inf))
    below, cut = x, np.nextafter(x, np.float32(np.inf))                                     # the last bonded coordinate, the first unbonded one
    assert bonded(below) and not bonded(cut)
    out = {}
    for name, xc in (('cut', cut), ('below', below)):
        p = pos.copy()
        p[0, place[256], 0] = xc
        out[name] = graph(p, v, [0, n], profiles=())
        want = BR.bond_graph(p, v, [0, n], CLASS_Z, AROMATIC)
        same(out[name], want, name, ('n_bonds', 'n_fragments', 'largest_fragment', 'fragment', 'bond_atoms', 'bond_order', 'bond_length'))
    assert (out['cut']['n_fragments'][0, 0], out['cut']['n_bonds'][0, 0], out['cut']['largest_fragment'][0, 0]) == (2, n - 2, 256)
    assert (out['below']['n_fragments'][0, 0], out['below']['n_bonds'][0, 0]) == (1, n - 1)
    lab = out['cut']['fragment'][0]
    assert set(lab[place[:256]].tolist()) == {int(place[:256].min())} and set(lab[place[256:]].tolist()) == {int(place[256:].min())}


def ring(k, centre, start_angle=0.0, bond=1.4):
    """k atoms on a regular polygon of side `bond` in the xy plane"""
    R = bond / (2.0 * np.sin(np.pi / k))
    a = start_angle + 2.0 * np.pi * np.arange(k) / k
    return np.stack([centre[0] + R * np.cos(a), centre[1] + R * np.sin(a), np.zeros(k)], 1)


def test_fused_rings_and_joined_aromatic_rings():
    # a 6-ring fused to a 5-ring along one edge (indane's skeleton): 9 atoms, 10 bonds, rings 2
    six = ring(6, (0.0, 0.0))
    a, b = six[0], six[1]                                                                   # the shared edge
    mid = (a + b) / 2.0
    c5 = mid + mid / np.linalg.norm(mid) * (1.4 / (2.0 * np.tan(np.pi / 5)))                # the pentagon's centre, outside the hexagon
    for sign in (1.0, -1.0):                                                                # turn a about c5 by 72 degrees, towards b
        t = sign * 2.0 * np.pi / 5 * np.arange(5)
        five = c5 + np.stack([np.cos(t) * (a - c5)[0] - np.sin(t) * (a - c5)[1], np.sin(t) * (a - c5)[0] + np.cos(t) * (a - c5)[1], np.zeros(5)], 1)
        if np.linalg.norm(five[1] - b) < 1e-9:
            break
    assert np.linalg.norm(five[1] - b) < 1e-9
    extra = five[2:]
    fused = np.concatenate([six, extra]).astype(np.float32)
    # two aromatic 6-rings joined by one 1.48 A bond (biphenyl's skeleton), classes C-aromatic with one N-aromatic: 12 atoms, 13 bonds
    R = 1.4
    left, right = ring(6, (0.0, 0.0)), ring(6, (2 * R + 1.48, 0.0), np.pi)
    joined = np.concatenate([left, right]).astype(np.float32) + np.float32(30.0)
    pos = np.concatenate([fused, joined])[None]
    v = np.array([[C] * 9 + [C_ARO] * 11 + [N_ARO]], np.int64)
    r = graph(pos, v, [0, 9, 21])
    want = BR.bond_graph(pos, v, [0, 9, 21], CLASS_Z, AROMATIC, PROFILES)
    same(r, want, 'rings')
    rings = r['n_bonds'] - np.array([[9, 12]]) + r['n_fragments']
    assert r['n_bonds'].tolist() == [[10, 13]] and r['n_fragments'].tolist() == [[1, 1]] and rings.tolist() == [[2, 1 + 1]]
    cat = r['bond_category'][r['bond_ptr'][1]:]
    assert cat.tolist() == [4] * 13                                                         # the joining single bond too, as the rule states
    join = [k for k, (i, j) in enumerate(r['bond_atoms'][10:]) if (i < 15) != (j < 15)]
    assert len(join) == 1 and r['bond_order'][10 + join[0]] == 1 and abs(r['bond_length'][10 + join[0]] - 1.48) < 1e-5
    assert set(r['bond_category'][:10].tolist()) <= {1, 2} and r['bond_hist'][0, 2].sum() + r['bond_hist'][0, 5].sum() == 13
    # the same atoms without aromatic flags: the category is the order
    plain = graph(pos, v, [0, 9, 21], aromatic=None)
    np.testing.assert_array_equal(plain['bond_category'], plain['bond_order'])
    np.testing.assert_array_equal(plain['bond_order'], r['bond_order'])


def test_frames_one_by_one_reversed_and_behind_another_pack():
    g, base = sizes_graph()
    pos, v, ptr, inc = g['pos'], g['v'], g['ptr'], g['include']
    S, B = inc.shape
    per_frame = lambda r, s: {k: r[k][s:s + 1] for k in ('n_bonds', 'n_fragments', 'largest_fragment', 'fragment', 'bond_hist')}
    for s in range(S):
        one = graph(pos[s:s + 1], v[s:s + 1], ptr, inc[s:s + 1])
        same(one, per_frame(base, s), f'frame {s} alone', ('n_bonds', 'n_fragments', 'largest_fragment', 'fragment', 'bond_hist'))
        a, b = base['bond_ptr'][s * B], base['bond_ptr'][(s + 1) * B]
        np.testing.assert_array_equal(one['bond_ptr'], base['bond_ptr'][s * B:(s + 1) * B + 1] - a)
        same(one, {k: base[k][a:b] for k in LIST_KEYS}, f'frame {s} alone', LIST_KEYS)
    # the molecules in reversed order
    order = np.concatenate([np.arange(ptr[b], ptr[b + 1]) for b in reversed(range(B))]).astype(np.int64)
    rptr = np.concatenate([[0], np.cumsum(np.diff(ptr)[::-1])])
    rev = graph(pos[:, order], v[:, order], rptr, inc[:, ::-1])
    np.testing.assert_array_equal(rev['fragment'], base['fragment'][:, order])
    for k in ('n_bonds', 'n_fragments', 'largest_fragment'):
        np.testing.assert_array_equal(rev[k], base[k][:, ::-1], err_msg=k)
    np.testing.assert_array_equal(rev['bond_hist'], base['bond_hist'])
    np.testing.assert_array_equal(np.sort(rev['bond_length']), np.sort(base['bond_length']))
    # an unrelated pack in front, kept out of the histograms by the mask
    d = load_golden('quality_docked.npz')
    n0 = d['pos'].shape[1]
    fpos = np.concatenate([np.repeat(d['pos'], S, 0) + np.float32(3.0), pos], axis=1)
    fv = np.concatenate([np.repeat(d['v'], S, 0), v], axis=1)
    fptr = np.concatenate([d['ptr'][:-1], ptr + n0])
    finc = np.concatenate([np.zeros((S, 5), bool), inc], axis=1)
    front = graph(fpos, fv, fptr, finc)
    np.testing.assert_array_equal(front['fragment'][:, n0:], base['fragment'])
    for k in ('n_bonds', 'n_fragments', 'largest_fragment'):
        np.testing.assert_array_equal(front[k][:, 5:], base[k], err_msg=k)
    np.testing.assert_array_equal(front['bond_hist'], base['bond_hist'])
    mine = front['bond_atoms'][:, 0] >= n0
    np.testing.assert_array_equal(front['bond_atoms'][mine] - n0, base['bond_atoms'])
    np.testing.assert_array_equal(front['bond_length'][mine], base['bond_length'])


def test_side_stream_null_outputs_and_include():
    dev = _dev()
    g, base = sizes_graph()
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        side = graph(g['pos'], g['v'], g['ptr'], g['include'])
        bare = graph(g['pos'], g['v'], g['ptr'], g['include'], fragments=False, bond_ptr=False)
    torch.cuda.current_stream(dev).wait_stream(st)
    same(side, base, 'side stream')
    assert bare['fragment'] is None and bare['bond_ptr'] is None
    same(bare, base, 'null fragment and bond_ptr', ('n_bonds', 'n_fragments', 'largest_fragment', 'bond_hist'))
    # include changes bond_hist and nothing else
    every = graph(g['pos'], g['v'], g['ptr'], None)
    same(every, base, 'include=None', ('n_bonds', 'n_fragments', 'largest_fragment', 'fragment', 'bond_ptr') + LIST_KEYS)
    want = BR.bond_graph(g['pos'], g['v'], g['ptr'], CLASS_Z, AROMATIC, PROFILES)
    np.testing.assert_array_equal(every['bond_hist'], want['bond_hist'])
    assert (every['bond_hist'] != base['bond_hist']).any()
    # no profile; sixteen of them: any element, any category, a single edge, 127 edges, element pairs in either order
    none = graph(g['pos'], g['v'], g['ptr'], g['include'], profiles=())
    assert none['bond_hist'].shape == (3, 0, 128)
    same(none, base, 'no profile', ('n_bonds', 'n_fragments', 'fragment', 'bond_ptr'))
    many = ((0, 0, 0, [1.5]), (8, 7, 0, np.linspace(1.0, 2.2, 127)), (7, 8, 0, np.linspace(1.0, 2.2, 127)), (6, 0, 1, [1.2, 1.4, 1.6]),
            (0, 0, 4, [1.3, 1.5]), (0, 0, 3, [1.0, 1.1, 1.2])) + PROFILES + ((6, 6, 0, [1.4]), (16, 15, 0, [2.0]))
    assert len(many) == 16
    r16 = graph(g['pos'], g['v'], g['ptr'], g['include'], profiles=many)
    want = BR.bond_graph(g['pos'], g['v'], g['ptr'], CLASS_Z, AROMATIC, many, g['include'])
    np.testing.assert_array_equal(r16['bond_hist'], want['bond_hist'])
    np.testing.assert_array_equal(r16['bond_hist'][:, 1], r16['bond_hist'][:, 2])
    np.testing.assert_array_equal(r16['bond_hist'][:, 6:14], base['bond_hist'])
    inc_bonds = sum(int(base['n_bonds'][s, b]) for s in range(3) for b in range(8) if g['include'][s, b])
    assert r16['bond_hist'][:, 0].sum() == inc_bonds and r16['bond_hist'][:, 1].sum() > 0 and r16['bond_hist'][:, 4].sum() > 0


def test_bond_list_order_and_quality_report_nr_bonds():
    g, base = sizes_graph()
    dev = _dev()
    S, B = g['include'].shape
    N = g['pos'].shape[1]
    atoms, ptr = base['bond_atoms'].astype(np.int64), base['bond_ptr']
    assert ptr[0] == 0 and ptr[-1] == len(atoms) == base['n_bonds'].sum() and (np.diff(ptr) == base['n_bonds'].reshape(-1)).all()
    frame = np.repeat(np.arange(S), np.diff(ptr).reshape(S, B).sum(1))
    mol = np.repeat(np.tile(np.arange(B), S), np.diff(ptr))
    key = ((frame * B + mol) * N + atoms[:, 0]) * N + atoms[:, 1]
    assert (np.diff(key) > 0).all() and (atoms[:, 0] < atoms[:, 1]).all()                    # ascending (frame, molecule, i, j)
    assert (g['ptr'][mol] <= atoms[:, 0]).all() and (atoms[:, 1] < g['ptr'][mol + 1]).all()
    np.testing.assert_array_equal(base['bond_length'], g['bond_length'])                     # float64, bit for bit
    nr = np.zeros((S, N), np.int64)
    np.add.at(nr, (frame, atoms[:, 0]), base['bond_order'])
    np.add.at(nr, (frame, atoms[:, 1]), base['bond_order'])
    q = capi.quality_report(torch.as_tensor(g['pos'], device=dev), torch.as_tensor(g['v'], dtype=torch.int64, device=dev),
                            torch.as_tensor(g['ptr'], dtype=torch.int32, device=dev), CLASS_Z)
    np.testing.assert_array_equal(nr, q['nr_bonds'].cpu().numpy())
    # the public function: device tensors, rings, one molecule's bonds
    bg = quality.bond_graph(g['pos'], g['v'], ligand_ptr=g['ptr'], include=g['include'], return_fragments=True, return_bonds=True)
    assert bg.n_bonds.is_cuda and bg.complete.dtype == torch.bool
    np.testing.assert_array_equal(bg.rings.cpu().numpy(), base['n_bonds'] - np.diff(g['ptr'])[None] + base['n_fragments'])
    np.testing.assert_array_equal(bg.bond_hist.cpu().numpy(), base['bond_hist'])
    a, o, c, d = bg.molecule_bonds(1, 7)
    k0, k1 = ptr[1 * B + 7], ptr[1 * B + 8]
    np.testing.assert_array_equal(a, atoms[k0:k1] - g['ptr'][7])
    np.testing.assert_array_equal(d, base['bond_length'][k0:k1])
    with pytest.raises(ValueError, match='513 atoms'):
        quality.bond_graph(np.zeros((513, 3), np.float32), np.ones(513, np.int64), ligand_ptr=[0, 513])


def _model():
    if 'model' not in _CACHE:
        from targetdiff_amd.models import ScorePosNet3D
        m = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG), 27, 13)
        assert not m.load_state_dict(weights.make_state_dict(2021), strict=False).unexpected_keys
        _CACHE['model'] = m.to(_dev()).eval()
    return _CACHE['model']


@pytest.mark.parametrize('mode', ['num_steps', 'strided'])
def test_connectivity_of_a_sampled_trajectory(mode, tmp_path):
    """4 samples x 20 steps on a small pocket with seeded random weights: the whole-trajectory reports equal the restatement"""
    from targetdiff_amd import sampling
    dev = _dev()
    pk = workloads.synthetic_pocket(301, 70, 3.0, 9.0)
    data = types.SimpleNamespace(protein_pos=torch.from_numpy(pk.pos), protein_atom_feature=torch.from_numpy(pk.feat))
    src = draws.Source(9900, dev)
    sizes = [6, 9, 4, 11]
    steps = dict(num_steps=20) if mode == 'num_steps' else dict(time_program=TimeProgram.strided(1000, 5))
    frames = 20 if mode == 'num_steps' else len(steps['time_program'])
    res = sampling.sample_diffusion_ligand(_model(), data, 4, batch_size=4, device=dev, ligand_num_atoms=sizes,
                                           noise_source=lambda b, st, name, like: src(st + 1, name, like), **steps)
    pos = np.concatenate([p.astype(np.float32) for p in res[2]], axis=1)
    v = np.concatenate(res[3], axis=1)
    ptr = np.cumsum([0] + sizes)
    want = BR.bond_graph(pos, v, ptr, CLASS_Z, AROMATIC, PROFILES)
    con = quality.sample_connectivity(res, 'all', reference={})
    assert con.num_frames == frames and con.n_samples == 4
    np.testing.assert_array_equal(con.bond_hist, want['bond_hist'])
    np.testing.assert_array_equal(con.n_complete, (want['n_fragments'] == 1).sum(1))
    np.testing.assert_array_equal(con.sum_fragments, want['n_fragments'].sum(1))
    np.testing.assert_array_equal(con.mean_largest_share, (want['largest_fragment'] / np.asarray(sizes, np.float64)[None]).sum(1) / 4.0)
    last = quality.sample_connectivity(res, reference={})
    np.testing.assert_array_equal(last.bond_hist[0], want['bond_hist'][-1])
    assert all(x is None for x in last.js().values())
    mask = want['n_fragments'] == 1
    rep = quality.sample_quality(res, 'all', include='complete', reference={})
    wq = QR.quality_report(pos, v, ptr, CLASS_Z, quality.default_profiles(), mask)
    np.testing.assert_array_equal(rep.hist, wq['hist'])
    np.testing.assert_array_equal(rep.counts, wq['counts'])
    np.testing.assert_array_equal(rep.stable_atoms, wq['stable_atoms'].sum(1))
    con2 = quality.sample_connectivity(res, 'all', include='complete', reference={})
    np.testing.assert_array_equal(con2.bond_hist, BR.bond_graph(pos, v, ptr, CLASS_Z, AROMATIC, PROFILES, mask)['bond_hist'])
    if mode == 'num_steps':
        save_results(tmp_path, {0: res})
        out = load_tool('export_sdf').main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'sdf')])
        recs = parse_sdf(open(tmp_path / 'sdf' / 'result_0.sdf').read())
        assert out['result_0']['written'] == len(recs) == 4 and [len(r[1]) for r in recs] == sizes            # one record per sample
        k = want['bond_ptr'][(frames - 1) * 4:]
        assert [len(r[2]) for r in recs] == np.diff(k).tolist()
        for g, (_, atoms, bonds, _p) in enumerate(recs):
            np.testing.assert_array_equal(np.array([xyz for _, *xyz in atoms]), np.round(pos[-1, ptr[g]:ptr[g + 1]].astype(np.float64), 4))
            assert [(i + ptr[g], j + ptr[g]) for i, j, _ in bonds] == [tuple(x) for x in want['bond_atoms'][k[g]:k[g + 1]].tolist()]
