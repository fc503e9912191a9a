"""td_fingerprint and td_fingerprint_similarity on the GPU (csrc/fingerprint.hip) against tests/_fingerprint_ref.py, array_equal
throughout, the float64 outputs included (the restatement is pinned to networkx, to known answers and to recorded values on the host,
tests/test_fingerprint_host.py).

  1. the fixture packs: the docked ligand and its jittered copies (also against the recorded values), the sizes pack (both
     instantiations, a 600-atom molecule that is refused with -1) and the 1000-frame trajectory.
  2. constructed molecules of class-1 carbons with side 1.45 A: a molecule, its atom-permuted and its rotated copy; n-gons at the
     instantiation boundary 128 | 129; a 512-ring stored in random order; a chain, a single atom, an empty molecule, an atom of no
     class, a collapsed cloud (the complete graph of 130 atoms: the worst case of the neighbour loop), dense clouds with bonds of
     every category and more than 32 per atom; radius 0 and 4, key_rounds =
     radius and 16; decalin and bicyclopentyl (equal keys: the documented limit), naphthalene and biphenyl (different keys).
  3. similarity: a pack of 12 molecules that holds one molecule three times, include masks, a query set, B = 1, B = 0, and a pack of
     130 molecules so that the ascending sum crosses the 64-partner chunks.
  4. a molecule's fingerprint depends on that molecule alone: frames one by one, molecules reversed, an unrelated pack in front, a side
     stream, null optional outputs; include changes the similarity outputs only.
  5. end to end: sample_diversity, tools/evaluate_samples.py --diversity and tools/export_sdf.py --unique on the driver's trajectories.
"""
import types

import numpy as np
import pytest
import torch

import _fingerprint_ref as FR
from conftest import load_golden
from targetdiff_amd import capi, quality
from test_bonds_host import load_tool, parse_sdf, save_results
from test_fingerprint_host import (C, C_ARO, DOUBLE, TRIPLE, chain, duplicates_pack, fused_hexagons, linked_polygons, ngon, pack, rotated,
                                   same_report, want_report)

pytestmark = pytest.mark.gpu

CLASS_Z = quality.class_atomic_numbers('add_aromatic')
AROMATIC = quality.class_aromatic('add_aromatic')


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


def fingerprint(pos, v, ptr, radius=2, key_rounds=8, atom_keys=True, check=False):
    """capi.fingerprint of numpy inputs, as numpy"""
    dev = _dev()
    p, c = torch.as_tensor(np.ascontiguousarray(pos), device=dev), torch.as_tensor(np.ascontiguousarray(v), dtype=torch.int64, device=dev)
    lp = torch.as_tensor(np.asarray(ptr), dtype=torch.int32, device=dev)
    r = capi.fingerprint(p, c, lp, CLASS_Z, AROMATIC, radius, key_rounds, atom_keys, check=check)
    return {k: (None if t is None else t.cpu().numpy()) for k, t in r.items()}


def similarity(fp, include=None, query=None, common=True):
    """capi.fingerprint_similarity of a fingerprint() result (numpy), as numpy; query: (q_words [Q, 32], q_bits [Q])"""
    dev = _dev()
    t = lambda a, dtype=None: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)
    inc = None if include is None else t(include, torch.bool)
    qw, qb = (None, None) if query is None else (t(query[0]), t(query[1], torch.int32))
    r = capi.fingerprint_similarity(t(fp['fp_words']), t(fp['n_bits']), t(fp['key']), inc, qw, qb, common)
    return {k: (None if x is None else x.cpu().numpy()) for k, x in r.items()}


def same(a, b, what, keys):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f'{what}: {k}')
        assert a[k].dtype == b[k].dtype, (what, k)


def against_restatement(pos, v, ptr, radius=2, key_rounds=8, include=None, what=''):
    """both kernels against the restatement on one pack; returns (fingerprints, similarity) of the kernels"""
    r = fingerprint(pos, v, ptr, radius, key_rounds)
    want = FR.fingerprints(pos, v, ptr, CLASS_Z, AROMATIC, radius, key_rounds)
    same(r, want, what, FR.FP_KEYS)
    s = similarity(r, include)
    same(s, FR.similarity(want['fp_words'], want['n_bits'], want['key'], include), what, FR.SIM_KEYS)
    return r, s


_CACHE = {}


def sizes_pack():
    """the sizes pack of the bond fixtures through the kernels, once: the baseline of the independence tests"""
    if 'sizes' not in _CACHE:
        g = load_golden('bonds_sizes.npz')
        fp = fingerprint(g['pos'], g['v'], g['ptr'])
        _CACHE['sizes'] = (g, fp, similarity(fp, g['include']))
    return _CACHE['sizes']


def test_fixture_docked_and_the_recorded_values():
    q, g = load_golden('quality_docked.npz'), load_golden('fingerprint_known.npz')
    r, s = against_restatement(q['pos'], q['v'], q['ptr'], what='docked')
    assert r['fp_words'].dtype == np.int64 and r['fp_words'].shape == (1, 5, 32) and r['n_bits'].dtype == np.int32
    assert r['key'].dtype == np.int64 and r['atom_key'].dtype == np.int64 and r['atom_key'].shape == q['v'].shape
    assert s['sim_sum'].dtype == np.float64 and s['sim_max'].dtype == np.float64 and s['first_equal'].dtype == np.int32
    assert s['common'].dtype == np.int32 and s['common'].shape == (1, 5, 5)
    for k in FR.FP_KEYS:
        np.testing.assert_array_equal(r[k], g[k], err_msg=k)
    r0 = fingerprint(q['pos'], q['v'], q['ptr'], 0, 0)
    np.testing.assert_array_equal(r0['key'], g['key_r0'])
    np.testing.assert_array_equal(r0['n_bits'], g['n_bits_r0'])
    assert r['n_bits'][0].tolist() == [54, 61, 64, 63, 45] and s['first_equal'][0].tolist() == [0, 1, 2, 3, 4]
    assert np.diagonal(s['common'][0]).tolist() == r['n_bits'][0].tolist() and (s['sim_max'] < 1.0).all() and (s['sim_max'] > 0.0).all()


def test_fixture_sizes_with_an_oversize_molecule_and_include():
    q = load_golden('quality_sizes.npz')
    assert np.diff(q['ptr']).tolist() == [0, 1, 2, 63, 64, 65, 130, 300, 600] and not q['include'].all()
    r, s = against_restatement(q['pos'], q['v'], q['ptr'], include=q['include'], what='sizes')
    assert (r['n_bits'][:, 8] == -1).all() and not r['fp_words'][:, 8].any() and not r['key'][:, 8].any()
    assert not r['atom_key'][:, q['ptr'][8]:].any() and (r['n_bits'][:, :8] >= 0).all() and r['n_bits'].max() > 200
    # the refused molecule is never included, whatever the mask says: no partner of anybody, -1 for itself
    every = similarity(r)
    assert (every['first_equal'][:, 8] == -1).all() and not every['sim_sum'][:, 8].any() and (every['first_equal'][:, :8] >= 0).all()
    same(every, FR.similarity(r['fp_words'], r['n_bits'], r['key']), 'sizes, no mask', FR.SIM_KEYS)
    assert (s['first_equal'][~q['include']] == -1).all() and not s['sim_sum'][~q['include']].any()


def test_trajectory_1000_frames():
    """the 1000-frame trajectory of sample_small_1000 in one call; the restatement on every ninth frame and the last"""
    t = load_golden('sample_small_1000.npz')
    ptr = load_golden('quality_traj.npz')['ptr']
    v = t['v_traj'].astype(np.int64)
    r = fingerprint(t['pos_traj'], v, ptr)
    s = similarity(r)
    pick = sorted(set(range(0, 1000, 9)) | {999})
    want = FR.fingerprints(t['pos_traj'][pick], v[pick], ptr, CLASS_Z, AROMATIC)
    same({k: r[k][pick] for k in FR.FP_KEYS}, want, 'picked frames', FR.FP_KEYS)
    same({k: s[k][pick] for k in FR.SIM_KEYS}, FR.similarity(want['fp_words'], want['n_bits'], want['key']), 'picked frames', FR.SIM_KEYS)
    pop = np.array([[sum(bin(int(w) & FR.M64).count('1') for w in row) for row in frame] for frame in r['fp_words'][::50]])
    np.testing.assert_array_equal(pop, r['n_bits'][::50])
    assert r['n_bits'].min() > 0 and len(np.unique(r['key'])) > 100


def test_permuted_and_rotated_copies():
    rng = np.random.default_rng(2)
    two = fused_hexagons()
    place = rng.permutation(10)
    pos, v, ptr = pack([(two, C), (two[place], C), (rotated(two, 9), C), (linked_polygons(6), C_ARO)])
    r, s = against_restatement(pos, v, ptr, what='copies')
    atoms = [r['atom_key'][0, a:b] for a, b in zip(ptr[:-1], ptr[1:])]
    for g in (1, 2):
        np.testing.assert_array_equal(r['fp_words'][0, g], r['fp_words'][0, 0])
        assert r['key'][0, g] == r['key'][0, 0] and sorted(atoms[g].tolist()) == sorted(atoms[0].tolist())
    np.testing.assert_array_equal(atoms[1], atoms[0][place])
    assert sorted(np.unique(atoms[0], return_counts=True)[1].tolist()) == [2, 4, 4]
    assert s['first_equal'][0].tolist() == [0, 0, 0, 3] and s['sim_max'][0, :3].tolist() == [1.0] * 3 and s['sim_max'][0, 3] < 1.0
    assert s['common'][0, 0, 1] == r['n_bits'][0, 0]


def test_polygons_at_the_instantiation_boundary_and_a_512_ring():
    rng = np.random.default_rng(5)
    big = ngon(512)
    pos, v, ptr = pack([(ngon(128)[rng.permutation(128)], C), (ngon(129)[rng.permutation(129)], C), (big[rng.permutation(512)], C), (big, C),
                        (ngon(6), C)])
    r, _ = against_restatement(pos, v, ptr, what='polygons')
    # every atom of a ring of one element is alike: one id per round, radius + 1 bits, whatever the size; the key tells the sizes apart
    assert r['n_bits'][0].tolist() == [3] * 5 and len(set(r['key'][0].tolist())) == 4 and r['key'][0, 2] == r['key'][0, 3]
    np.testing.assert_array_equal(r['fp_words'][0, 2], r['fp_words'][0, 3])
    np.testing.assert_array_equal(r['fp_words'][0, 0], r['fp_words'][0, 4])
    for a, b in zip(ptr[:-1], ptr[1:]):
        assert len(set(r['atom_key'][0, a:b].tolist())) == 1
    # cut open, the 512-ring is a chain: its ends are told apart from the middle, round by round
    pos2 = pos.copy()
    pos2[0, ptr[3] + 7] += np.float32(5.0)
    r2, _ = against_restatement(pos2, v, ptr, what='512-chain')
    assert r2['key'][0, 3] != r['key'][0, 3] and r2['n_bits'][0, 3] > 3 and r2['key'][0, 2] == r['key'][0, 2]


def constructed():
    """the small constructed molecules: name -> (pos, classes)"""
    return dict(chain=(chain(9), C), atom=(np.zeros((1, 3)), C), empty=(np.zeros((0, 3)), C), no_class=(ngon(6), [C, C, 13, C, C, C]),
                negative_class=(ngon(6), [C, C, -1, C, C, C]), chain5=(chain(5), C), ethane=(chain(2), C), ethene=(chain(2, DOUBLE), C),
                ethyne=(chain(2, TRIPLE), C), hexagon=(ngon(6), C), aromatic_hexagon=(ngon(6), C_ARO), decalin=(fused_hexagons(), C),
                bicyclopentyl=(linked_polygons(5), C), naphthalene=(fused_hexagons(), C_ARO), biphenyl=(linked_polygons(6), C_ARO),
                only_no_class=(chain(3), [13, 13, -5]))


@pytest.mark.parametrize('radius,key_rounds', [(2, 8), (0, 0), (0, 16), (4, 4), (4, 16), (1, 3)])
def test_constructed_molecules(radius, key_rounds):
    mols = constructed()
    names = list(mols)
    pos, v, ptr = pack([mols[k] for k in names])
    r, s = against_restatement(pos, v, ptr, radius, key_rounds, what=f'constructed {radius} {key_rounds}')
    key, bits = dict(zip(names, r['key'][0].tolist())), dict(zip(names, r['n_bits'][0].tolist()))
    atoms = {k: r['atom_key'][0, a:b].tolist() for k, a, b in zip(names, ptr[:-1], ptr[1:])}
    assert 1 <= bits['atom'] <= radius + 1 and bits['empty'] == 0 and bits['only_no_class'] == 0 and key['empty'] == key['only_no_class']
    assert atoms['only_no_class'] == [0, 0, 0] and atoms['no_class'][2] == 0 and atoms['negative_class'][2] == 0
    assert key['no_class'] == key['negative_class'] == key['chain5'] and bits['no_class'] == bits['chain5']
    assert sorted(atoms['no_class'][:2] + atoms['no_class'][3:]) == sorted(atoms['chain5'])
    assert len({key['ethane'], key['ethene'], key['ethyne']}) == 3 and atoms['ethane'][0] == atoms['ethane'][1]
    assert key['decalin'] == key['bicyclopentyl']                               # the documented limit of colour refinement
    assert sorted(atoms['decalin']) == sorted(atoms['bicyclopentyl'])
    assert key['naphthalene'] != key['biphenyl'] and key['naphthalene'] != key['decalin']
    if key_rounds >= 1:
        assert key['hexagon'] != key['aromatic_hexagon']
    if radius == 0:
        assert bits['atom'] == 1 and bits['chain'] == 2 and bits['hexagon'] == 1 and bits['decalin'] == 2
    first = dict(zip(names, s['first_equal'][0].tolist()))
    assert first['bicyclopentyl'] == names.index('decalin') and first['negative_class'] == names.index('no_class')
    assert first['chain5'] == names.index('no_class') and first['only_no_class'] == names.index('empty')


def test_collapsed_cloud_is_a_complete_graph():
    n = 130
    pos = (np.random.default_rng(n).uniform(-0.15, 0.15, (1, n, 3))).astype(np.float32)     # within 0.3 A of one point: all triple bonds
    v = np.full((1, n), C, np.int64)
    r, _ = against_restatement(pos, v, [0, n], 4, 16, what='cloud')
    assert r['n_bits'][0, 0] <= 5 and len(set(r['atom_key'][0].tolist())) == 1
    m = FR.molecule(pos[0], v[0], CLASS_Z, AROMATIC, 4, 16)
    assert m['inv'] == [(6, 0, n - 1, 3 * (n - 1))] * n and len(m['o']) == n * (n - 1) // 2


@pytest.mark.parametrize('n,half', [(60, 1.2), (140, 1.7)])
def test_dense_cloud_with_mixed_orders(n, half):
    """atoms of four classes, two of them aromatic, in a small box: bonds of every order and category, per atom fewer and more than
    the 32 bonds whose category a lane keeps, in both instantiations"""
    rng = np.random.default_rng(n)
    pos = rng.uniform(-half, half, (2, n, 3)).astype(np.float32)
    v = rng.integers(1, 5, (2, n))
    r, _ = against_restatement(pos, v, [0, n], 2, 8, what='dense cloud')
    m = FR.molecule(pos[0], v[0], CLASS_Z, AROMATIC)
    degree = np.array([x[2] for x in m['inv']])
    assert degree.min() < 31 and {32, 33} <= set(degree.tolist()) and set(m['cat'].tolist()) == {1, 2, 3, 4} and r['n_bits'].min() > 2 * n


def test_similarity_of_a_pack_with_duplicates():
    names, pos, v, ptr = duplicates_pack()
    assert len(names) == 12
    r, s = against_restatement(pos, v, ptr, what='duplicates')
    fused = [names.index(k) for k in ('fused', 'fused_permuted', 'fused_rotated')]
    want_first = list(range(12))
    want_first[fused[1]] = want_first[fused[2]] = fused[0]
    assert s['first_equal'][0].tolist() == want_first and (s['first_equal'][0] == np.arange(12)).sum() == 10
    assert s['sim_max'][0, fused].tolist() == [1.0] * 3 and (s['common'][0] == s['common'][0].T).all()
    # include masks drop rows and partners: without the first copy the second is the first of its key, and the third's partner
    inc = np.ones((1, 12), bool)
    inc[0, [fused[0], 0]] = False
    s2 = similarity(r, inc)
    want2 = FR.similarity(r['fp_words'], r['n_bits'], r['key'], inc)
    same(s2, want2, 'masked', FR.SIM_KEYS)
    assert s2['first_equal'][0, fused].tolist() == [-1, fused[1], fused[1]] and s2['sim_sum'][0, fused[0]] == 0.0 and s2['sim_max'][0, 0] == 0.0
    np.testing.assert_array_equal(s2['common'], s['common'])                    # the pair matrix does not look at the mask
    assert (s2['sim_sum'][0, 1:][inc[0, 1:]] < s['sim_sum'][0, 1:][inc[0, 1:]]).any()
    only = np.zeros((1, 12), bool)
    only[0, 5] = True
    s3 = similarity(r, only)
    same(s3, FR.similarity(r['fp_words'], r['n_bits'], r['key'], only), 'one included', FR.SIM_KEYS)
    assert s3['first_equal'][0, 5] == 5 and not s3['sim_sum'].any() and not s3['sim_max'].any()
    # a query set: three of the pack's own fingerprints and an empty one
    q_words = np.concatenate([r['fp_words'][0, [fused[0], 0, 10]], np.zeros((1, 32), np.int64)])
    q_bits = np.concatenate([r['n_bits'][0, [fused[0], 0, 10]], [0]]).astype(np.int32)
    s4 = similarity(r, inc, (q_words, q_bits), common=False)
    want4 = FR.similarity(r['fp_words'], r['n_bits'], r['key'], inc, q_words)
    same(s4, want4, 'query', ('sim_sum', 'sim_max', 'first_equal', 'query_common'))
    assert s4['common'] is None and s4['query_common'].shape == (1, 12, 4) and s4['query_sim'].dtype == np.float64
    np.testing.assert_array_equal(s4['query_common'][0, :, :3], s['common'][0][:, [fused[0], 0, 10]])
    want_sim = np.array([[[FR.tanimoto(int(want4['query_common'][0, a, q]), int(r['n_bits'][0, a]), int(q_bits[q])) for q in range(4)]
                          for a in range(12)]])
    np.testing.assert_array_equal(s4['query_sim'], want_sim)
    assert s4['query_sim'][0, fused, 0].tolist() == [1.0] * 3 and not s4['query_sim'][0, :, 3].any()


def test_similarity_of_one_molecule_of_none_and_across_chunks():
    pos, v, ptr = pack([(fused_hexagons(), C)])
    r, s = against_restatement(pos, v, ptr, what='B = 1')
    assert s['sim_sum'].tolist() == [[0.0]] and s['sim_max'].tolist() == [[0.0]] and s['first_equal'].tolist() == [[0]]
    assert s['common'].tolist() == [[[int(r['n_bits'][0, 0])]]]
    empty = fingerprint(np.zeros((2, 0, 3), np.float32), np.zeros((2, 0), np.int64), [0])
    assert empty['fp_words'].shape == (2, 0, 32) and empty['key'].shape == (2, 0)
    s0 = similarity(empty, query=(r['fp_words'][0], r['n_bits'][0]))
    assert s0['sim_sum'].shape == (2, 0) and s0['common'].shape == (2, 0, 0) and s0['query_common'].shape == (2, 0, 1)
    none = fingerprint(np.zeros((0, 4, 3), np.float32), np.zeros((0, 4), np.int64), [0, 1, 4])
    assert none['n_bits'].shape == (0, 2) and similarity(none)['first_equal'].shape == (0, 2)
    # 130 small molecules in two frames: partners in three chunks of 64, the sum in ascending order over all of them
    rng = np.random.default_rng(31)
    sizes = rng.integers(2, 9, 130)
    sizes[[70, 100]] = 10                                                       # a first copy beyond the first chunk of partners
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    pos = np.concatenate([rng.normal(0, 0.9, (2, n, 3)) for n in sizes], axis=1).astype(np.float32)
    v = rng.integers(1, 5, (2, ptr[-1]))
    pos[:, ptr[70]:ptr[71]], pos[:, ptr[100]:ptr[101]] = fused_hexagons().astype(np.float32), fused_hexagons()[::-1].astype(np.float32)
    v[:, ptr[70]:ptr[71]] = v[:, ptr[100]:ptr[101]] = C
    inc = rng.random((2, 130)) < 0.8
    inc[0, 64] = inc[1, 128] = False
    inc[:, [70, 100]] = True
    r, s = against_restatement(pos, v, ptr, include=inc, what='130 molecules')
    assert (s['first_equal'][inc] != np.broadcast_to(np.arange(130), (2, 130))[inc]).any()      # small clouds repeat
    assert s['first_equal'][:, 100].tolist() == [70, 70] and s['first_equal'][:, 70].tolist() == [70, 70]
    back = np.zeros_like(s['sim_sum'])
    for f in range(2):
        for a in np.nonzero(inc[f])[0]:
            for b in reversed(np.nonzero(inc[f])[0]):
                if b != a:
                    back[f, a] += FR.tanimoto(int(s['common'][f, a, b]), int(r['n_bits'][f, a]), int(r['n_bits'][f, b]))
    assert (back != s['sim_sum']).any() and np.allclose(back, s['sim_sum'], rtol=1e-13)           # the order of the adds is the ascending one


def test_frames_one_by_one_reversed_and_behind_another_pack():
    g, base, base_sim = sizes_pack()
    pos, v, ptr, inc = g['pos'], g['v'], g['ptr'], g['include']
    S, B = inc.shape
    assert np.diff(ptr).tolist() == [0, 1, 2, 63, 64, 65, 130, 300]
    same(base, FR.fingerprints(pos, v, ptr, CLASS_Z, AROMATIC), 'sizes', FR.FP_KEYS)
    same(base_sim, FR.similarity(base['fp_words'], base['n_bits'], base['key'], inc), 'sizes', FR.SIM_KEYS)
    for s in range(S):
        one = fingerprint(pos[s:s + 1], v[s:s + 1], ptr)
        same(one, {k: base[k][s:s + 1] for k in FR.FP_KEYS}, f'frame {s} alone', FR.FP_KEYS)
        same(similarity(one, inc[s:s + 1]), {k: base_sim[k][s:s + 1] for k in FR.SIM_KEYS}, f'frame {s} alone', FR.SIM_KEYS)
    # the molecules in reversed order
    order = np.concatenate([np.arange(ptr[b], ptr[b + 1]) for b in reversed(range(B))]).astype(np.int64)
    rptr = np.concatenate([[0], np.cumsum(np.diff(ptr)[::-1])])
    rev = fingerprint(pos[:, order], v[:, order], rptr)
    np.testing.assert_array_equal(rev['atom_key'], base['atom_key'][:, order])
    for k in ('fp_words', 'n_bits', 'key'):
        np.testing.assert_array_equal(rev[k], base[k][:, ::-1], err_msg=k)
    rev_sim = similarity(rev, inc[:, ::-1])
    np.testing.assert_array_equal(rev_sim['sim_max'], base_sim['sim_max'][:, ::-1])
    np.testing.assert_array_equal(rev_sim['common'], base_sim['common'][:, ::-1, ::-1])
    same(rev_sim, FR.similarity(rev['fp_words'], rev['n_bits'], rev['key'], inc[:, ::-1]), 'reversed', FR.SIM_KEYS)
    # an unrelated pack in front, kept out of the comparison by the mask
    d = load_golden('quality_docked.npz')
    n0 = d['pos'].shape[1]
    fpos = np.concatenate([np.repeat(d['pos'], S, 0) + np.float32(3.0), pos], axis=1)
    fv = np.concatenate([np.repeat(d['v'], S, 0), v], axis=1)
    fptr = np.concatenate([d['ptr'][:-1], ptr + n0])
    finc = np.concatenate([np.zeros((S, 5), bool), inc], axis=1)
    front = fingerprint(fpos, fv, fptr)
    np.testing.assert_array_equal(front['atom_key'][:, n0:], base['atom_key'])
    for k in ('fp_words', 'n_bits', 'key'):
        np.testing.assert_array_equal(front[k][:, 5:], base[k], err_msg=k)
    front_sim = similarity(front, finc)
    for k in ('sim_sum', 'sim_max'):
        np.testing.assert_array_equal(front_sim[k][:, 5:], base_sim[k], err_msg=k)
    np.testing.assert_array_equal(front_sim['first_equal'][:, 5:], np.where(base_sim['first_equal'] >= 0, base_sim['first_equal'] + 5, -1))
    np.testing.assert_array_equal(front_sim['common'][:, 5:, 5:], base_sim['common'])
    assert (front_sim['first_equal'][:, :5] == -1).all() and not front_sim['sim_sum'][:, :5].any()


def test_side_stream_null_outputs_and_include():
    dev = _dev()
    g, base, base_sim = sizes_pack()
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        side = fingerprint(g['pos'], g['v'], g['ptr'])
        side_sim = similarity(side, g['include'])
        bare = fingerprint(g['pos'], g['v'], g['ptr'], atom_keys=False)
        bare_sim = similarity(bare, g['include'], common=False)
    torch.cuda.current_stream(dev).wait_stream(st)
    same(side, base, 'side stream', FR.FP_KEYS)
    same(side_sim, base_sim, 'side stream', FR.SIM_KEYS)
    assert bare['atom_key'] is None and bare_sim['common'] is None and bare_sim['query_common'] is None and bare_sim['query_sim'] is None
    same(bare, base, 'null optional outputs', ('fp_words', 'n_bits', 'key'))
    same(bare_sim, base_sim, 'null optional outputs', ('sim_sum', 'sim_max', 'first_equal'))
    # include changes the similarity outputs and nothing of the fingerprints (which do not take it); the pair matrix stays
    every = similarity(base)
    np.testing.assert_array_equal(every['common'], base_sim['common'])
    assert (every['sim_sum'] != base_sim['sim_sum']).any() and (every['first_equal'] != base_sim['first_equal']).any()
    same(every, FR.similarity(base['fp_words'], base['n_bits'], base['key']), 'include=None', FR.SIM_KEYS)
    # the public functions give the same tensors
    fp = quality.fingerprints(g['pos'], g['v'], ligand_ptr=g['ptr'], return_atom_keys=True)
    assert fp.fp_words.is_cuda and fp.key.is_cuda
    for k, t in (('fp_words', fp.fp_words), ('n_bits', fp.n_bits), ('key', fp.key), ('atom_key', fp.atom_key)):
        np.testing.assert_array_equal(t.cpu().numpy(), base[k], err_msg=k)
    r = fp.similarity(g['include'], return_common=True)
    for k in FR.SIM_KEYS:
        np.testing.assert_array_equal(r[k].cpu().numpy(), base_sim[k], err_msg=k)
    one = quality.fingerprints(g['pos'][1], g['v'][1], ligand_ptr=g['ptr'])
    np.testing.assert_array_equal(one.key.cpu().numpy(), base['key'][1:2])
    assert one.atom_key is None


def test_oversize_molecules_are_refused_by_the_binding():
    n = 513
    pos, v, ptr = pack([(ngon(6), C), (ngon(n), C), (ngon(5), C)])
    r, s = against_restatement(pos, v, ptr, what='oversize')
    assert r['n_bits'][0].tolist() == [3, -1, 3] and s['first_equal'][0].tolist() == [0, -1, 2] and s['sim_sum'][0, 1] == 0.0
    # offsets that are not this pack's own (past N_l; negative): the molecule is refused, nothing of it is read or written
    pos, v, _ = pack([(ngon(6), C), (ngon(5), C)])
    for foreign, want_bits in (([0, 6, 20], [3, -1]), ([0, -3, 6], [0, -1])):
        f = fingerprint(pos, v, foreign)
        assert f['n_bits'][0].tolist() == want_bits and not f['fp_words'][0, 1].any() and f['key'][0, 1] == 0
        assert not f['atom_key'][0, 6:].any() and similarity(f)['first_equal'][0].tolist() == [0, -1]
    pos, v, ptr = pack([(ngon(6), C), (ngon(n), C), (ngon(5), C)])
    with pytest.raises(ValueError, match='513 atoms'):
        quality.fingerprints(pos[0], v[0], ligand_ptr=ptr)
    big = ngon(n).astype(np.float32).astype(np.float64)
    with pytest.raises(ValueError, match='513 atoms'):
        quality.sample_diversity(([], [], [big[None]], [np.ones((1, n), np.int64)], [], [], []))


def with_copies(res, which):
    """the driver's 7-tuple with the samples `which` once more at the end, their atoms in reversed order"""
    pos, v, pos_traj, v_traj = (list(x) for x in res[:4])
    for k in which:
        pos.append(res[0][k][::-1].copy())
        v.append(res[1][k][::-1].copy())
        pos_traj.append(res[2][k][:, ::-1].copy())
        v_traj.append(res[3][k][:, ::-1].copy())
    return (pos, v, pos_traj, v_traj) + tuple(res[4:])


def test_diversity_of_a_sampled_trajectory(tmp_path, capsys):
    """4 samples x 20 steps on a small pocket with seeded random weights, the run of test_gpu_bonds.py and two copies of it as further
    samples: the reports equal the restatement's, and so do the tools"""
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
    ref = (res[2][1][-1].astype(np.float32), res[3][1][-1])                    # sample 1's final pose as the known ligand
    want, _, _ = want_report(res, slice(0, 20), None, ref)
    rep = quality.sample_diversity(res, 'all', reference_ligand=ref)
    assert rep.num_frames == 20 and rep.n_samples == 4 and rep.n_included.tolist() == [4] * 20
    same_report(rep, want)
    assert rep.reference_similarity(-1)['ref_sim_max'] == 1.0
    last = quality.sample_diversity(res, -1, include='complete', radius=1, key_rounds=4)
    same_report(last, want_report(res, slice(19, 20), 'complete', None, 1, 4)[0])
    # samples 0 and 2 once more, atoms reversed: six samples of which four are distinct
    twice = with_copies(res, (0, 2))
    rep2 = quality.sample_diversity(twice, -1)
    same_report(rep2, want_report(twice, slice(19, 20))[0])
    assert rep2.n_included.tolist() == [6] and rep2.n_distinct.tolist() == [4] and rep2.uniqueness(-1) == 4 / 6
    save_results(tmp_path, {0: twice})
    out = load_tool('evaluate_samples').main(['--sample_path', str(tmp_path), '--diversity'])
    assert out['diversity'] == dict({k: (None if x != x else x) for k, x in rep2.summary(-1).items()}, num_included=6, num_distinct=4)
    assert f"uniqueness:\t{4 / 6:.4f}\n" in capsys.readouterr().out
    tool = load_tool('export_sdf')
    assert tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'all')])['result_0']['written'] == 6
    assert tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'unique'), '--unique'])['result_0']['written'] == 4
    recs = parse_sdf(open(tmp_path / 'unique' / 'result_0.sdf').read())
    before = parse_sdf(open(tmp_path / 'all' / 'result_0.sdf').read())
    assert [r[0] for r in recs] == ['sample_0', 'sample_1', 'sample_2', 'sample_3'] and recs == before[:4]
