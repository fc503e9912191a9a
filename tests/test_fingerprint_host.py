"""CPU-only checks of the fingerprints (targetdiff_amd.quality.fingerprints / sample_diversity, the host side of td_fingerprint and
td_fingerprint_similarity).

  1. tests/_fingerprint_ref.py -- the pure-Python restatement the GPU tests compare the kernels with -- against an independent party,
     networkx.weisfeiler_lehman_graph_hash: equal key <=> equal hash, on the fixture packs and on a constructed pack that has duplicates;
     against answers known by hand; against the recorded values of tests/golden/fingerprint_known.npz.
  2. the ABI surface and the refusals of the library and of the binding; TD_ABI_VERSION stays 5.
  3. DiversityReport's arithmetic and merged; sample_diversity, tools/evaluate_samples.py --diversity and tools/export_sdf.py --unique
     with the bindings patched by the restatements; the SD-file reader against write_sdf.
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import _bonds_ref as BR
import _fingerprint_ref as FR
import _quality_ref as QR
from conftest import ROOT, load_golden
from targetdiff_amd import capi, molfile, quality
from test_bonds_host import load_tool, packed, parse_sdf, ragged_result, save_results

CLASS_Z = quality.class_atomic_numbers('add_aromatic')
AROMATIC = quality.class_aromatic('add_aromatic')
C, C_ARO, N_, O_ = 1, 2, 3, 5                                               # classes of 'add_aromatic'
SIDE = 1.45                                                                 # a C-C single bond: 1.39 <= d < 1.64
DOUBLE, TRIPLE = 1.30, 1.15                                                 # C-C: 1.23 <= d < 1.39 double, d < 1.23 triple


# ---- constructed molecules (also used by tests/test_gpu_fingerprint.py): class-1 carbons unless said otherwise, every bond length at
# least 0.02 A from a threshold of the table
def ngon(n, centre=(0.0, 0.0, 0.0), side=SIDE, start=0.0):
    """n atoms on a regular polygon of side `side` in the xy plane"""
    R = side / (2.0 * np.sin(np.pi / n))
    a = start + 2.0 * np.pi * np.arange(n) / n
    return np.stack([centre[0] + R * np.cos(a), centre[1] + R * np.sin(a), centre[2] + np.zeros(n)], 1)


def chain(n, step=SIDE):
    return np.stack([step * np.arange(n), np.zeros(n), np.zeros(n)], 1)


def fused_hexagons():
    """the skeleton of decalin / naphthalene: two regular hexagons that share the edge 0 - 1 (10 atoms, 11 bonds)"""
    six = ngon(6)
    mirror = six[2:] - 2.0 * ((six[2:] - six[0]) @ _normal(six[0], six[1]))[:, None] * _normal(six[0], six[1])[None]
    return np.concatenate([six, mirror])


def _normal(p0, p1):
    d = (p1 - p0) / np.linalg.norm(p1 - p0)
    return np.array([-d[1], d[0], 0.0])


def linked_polygons(n, link=1.48):
    """two regular n-gons joined by one bond between their corners 0 (bicyclopentyl for n = 5, biphenyl for n = 6)"""
    R = SIDE / (2.0 * np.sin(np.pi / n))
    return np.concatenate([ngon(n), ngon(n, (2.0 * R + link, 0.0, 0.0), start=np.pi)])


def rotated(pos, seed):
    """the molecule turned by a random rotation and moved"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return np.asarray(pos) @ q.T + rng.uniform(-3.0, 3.0, 3)


def pack(mols):
    """[(pos [n, 3], classes [n] or one class)] -> pos [1, N, 3] fp32, v [1, N], ptr; the molecules are separate by the offsets alone"""
    pos, v, ptr = [], [], [0]
    for p, c in mols:
        p = np.asarray(p, np.float64).reshape(-1, 3)
        pos.append(p)
        v.append(np.full(len(p), c, np.int64) if np.isscalar(c) else np.asarray(c, np.int64))
        ptr.append(ptr[-1] + len(p))
    return np.concatenate(pos).astype(np.float32)[None], np.concatenate(v)[None], np.asarray(ptr)


def duplicates_pack():
    """12 molecules: a fused pair of hexagons three times (as built, atom-permuted, rotated) among nine distinct ones.  Returns
    (names, pos, v, ptr)."""
    rng = np.random.default_rng(17)
    two = fused_hexagons()
    mols = [('hexagon', ngon(6), C), ('fused', two, C), ('pentagon', ngon(5), C), ('chain5', chain(5), C),
            ('fused_permuted', two[rng.permutation(10)], C), ('aromatic_hexagon', ngon(6), C_ARO), ('ethane', chain(2), C),
            ('ethene', chain(2, DOUBLE), C), ('fused_rotated', rotated(two, 3), C), ('pyridine_like', ngon(6), [N_, C, C, C, C, C]),
            ('atom', np.zeros((1, 3)), C), ('chain6', chain(6), C)]
    pos, v, ptr = pack([(p, c) for _, p, c in mols])
    return [k for k, _, _ in mols], pos, v, ptr


def one(pos, cls=C, radius=2, key_rounds=8):
    p = np.asarray(pos, np.float64).astype(np.float32)
    return FR.molecule(p, np.full(len(p), cls, np.int64) if np.isscalar(cls) else np.asarray(cls, np.int64), CLASS_Z, AROMATIC, radius, key_rounds)


def fixture_molecules():
    """(name, pos [n, 3], v [n]) of the docked pack and of frames 0 and 2 of the sizes pack of the bond fixtures"""
    q = load_golden('quality_docked.npz')
    for g, (a, b) in enumerate(zip(q['ptr'][:-1], q['ptr'][1:])):
        yield f'docked[{g}]', q['pos'][0, a:b], q['v'][0, a:b]
    q = load_golden('bonds_sizes.npz')
    for s in (0, 2):
        for g, (a, b) in enumerate(zip(q['ptr'][:-1], q['ptr'][1:])):
            yield f'sizes[{s},{g}]', q['pos'][s, a:b], q['v'][s, a:b]


def nx_hash(nx, m, iterations=8):
    """networkx's refinement hash of a restatement molecule: the invariant as node attribute, the category as edge attribute; the atoms
    of no class are not part of the graph"""
    G = nx.Graph()
    for a, inv in enumerate(m['inv']):
        if inv is not None:
            G.add_node(a, inv='%d.%d.%d.%d' % inv)
    for i, j, c in zip(m['i'].tolist(), m['j'].tolist(), m['cat'].tolist()):
        G.add_edge(i, j, cat=str(c))
    return nx.weisfeiler_lehman_graph_hash(G, node_attr='inv', edge_attr='cat', iterations=iterations)


def test_restatement_matches_networkx():
    nx = pytest.importorskip('networkx')
    mols = [(name, FR.molecule(pos, v, CLASS_Z, AROMATIC)) for name, pos, v in fixture_molecules()]
    keys = [m['key'] for _, m in mols if len(m['inv'])]
    assert len(set(keys)) == len(keys) == 19                                # 5 docked, 7 non-empty x 2 frames: all distinct
    bits = [m['n_bits'] for name, m in mols]
    assert (min(bits[:5]), max(bits[:5])) == (45, 64) and (min(b for b in bits[5:] if b), max(bits[5:])) == (3, 226)
    names, pos, v, ptr = duplicates_pack()
    mols += [(k, FR.molecule(pos[0, a:b], v[0, a:b], CLASS_Z, AROMATIC)) for k, a, b in zip(names, ptr[:-1], ptr[1:])]
    # decalin and bicyclopentyl: refinement separates them no more than the key does
    mols += [('decalin', one(fused_hexagons())), ('bicyclopentyl', one(linked_polygons(5)))]
    hashes = [nx_hash(nx, m) for _, m in mols]
    equal = 0
    for x in range(len(mols)):
        for y in range(x):
            same_key, same_hash = mols[x][1]['key'] == mols[y][1]['key'], hashes[x] == hashes[y]
            assert same_key == same_hash, (mols[x][0], mols[y][0])
            equal += same_key
    # the three fused pairs and decalin (4 molecules: 6 pairs) + bicyclopentyl with each of them (4) + the two empty molecules (1)
    assert equal == 11
    # fewer rounds: the partition of the key follows the number of rounds, as networkx's does
    for rounds in (0, 1, 3):
        few = [FR.molecule(pos[0, a:b], v[0, a:b], CLASS_Z, AROMATIC, 0, rounds) for a, b in zip(ptr[:-1], ptr[1:])]
        if rounds == 0:                                                     # no round: the key is the multiset of invariants and the bond count
            hs = [(sorted(m['inv']), len(m['o'])) for m in few]
        else:
            hs = [nx_hash(nx, m, rounds) for m in few]
        for x in range(len(few)):
            for y in range(x):
                assert (few[x]['key'] == few[y]['key']) == (hs[x] == hs[y]), (rounds, names[x], names[y])


def test_known_answers_by_hand():
    # a single carbon: one id per round, so at most radius + 1 bits; exactly one at radius 0
    for radius in range(5):
        m = one(np.zeros((1, 3)), radius=radius)
        assert 1 <= m['n_bits'] <= radius + 1 and len({ids[0] for ids in m['ids'][:radius + 1]}) == m['n_bits']
    atom = one(np.zeros((1, 3)), radius=0, key_rounds=0)
    assert atom['n_bits'] == 1 and atom['inv'] == [(6, 0, 0, 0)] and atom['bits'] == {FR.mix(6) % 2048}
    # ethane: both atoms share every id of every round
    ethane, ethene, ethyne = one(chain(2)), one(chain(2, DOUBLE)), one(chain(2, TRIPLE))
    assert ethane['inv'] == [(6, 0, 1, 1)] * 2 and ethene['inv'] == [(6, 0, 1, 2)] * 2 and ethyne['inv'] == [(6, 0, 1, 3)] * 2
    assert all(ids[0] == ids[1] for ids in ethane['ids']) and ethane['n_bits'] == 3 and len(ethane['ids']) == 9
    assert ethane['cat'].tolist() == [1] and ethene['cat'].tolist() == [2] and ethyne['cat'].tolist() == [3]
    assert len({ethane['key'], ethene['key'], ethyne['key']}) == 3
    assert not (ethane['bits'] & ethene['bits']) and not (ethane['bits'] & ethyne['bits']) and not (ethene['bits'] & ethyne['bits'])
    # equal invariants, different bond category: aromatic-class carbons against plain ones on the same hexagon
    plain, aromatic = one(ngon(6)), one(ngon(6), C_ARO)
    assert plain['cat'].tolist() == [1] * 6 and aromatic['cat'].tolist() == [4] * 6
    assert plain['inv'] == [(6, 0, 2, 2)] * 6 and aromatic['inv'] == [(6, 1, 2, 2)] * 6
    assert plain['key'] != aromatic['key'] and plain['n_bits'] == aromatic['n_bits'] == 3 and not (plain['bits'] & aromatic['bits'])
    # the category alone: a pack without aromatic flags sees the same invariants on both and only then equal keys
    no_flags = FR.molecule(ngon(6).astype(np.float32), np.full(6, C_ARO), CLASS_Z, None)
    assert no_flags['key'] == plain['key'] and no_flags['bits'] == plain['bits']
    # an atom of no class takes no part: the hexagon it opens is a chain of five
    opened = one(ngon(6), [C, C, 13, C, C, C])
    assert opened['inv'][2] is None and opened['atom_key'][2] == 0 and opened['key'] == one(chain(5))['key']
    assert opened['bits'] == one(chain(5))['bits'] and one(ngon(6), [C, C, -1, C, C, C])['key'] == opened['key']
    # T(a, a) = 1; propane against ethane at radius 0 by hand: ethane has the bit of (C, degree 1, valence 1), propane that one and
    # the bit of (C, degree 2, valence 2): c = 1, T = 1 / (1 + 2 - 1)
    e0, p0 = one(chain(2), radius=0), one(chain(3), radius=0)
    assert (e0['n_bits'], p0['n_bits']) == (1, 2) and e0['bits'] < p0['bits']
    words = np.array([[[FR.signed(w) for w in m['words']] for m in (e0, p0)]], np.int64)
    sim = FR.similarity(words, np.array([[1, 2]], np.int32), np.array([[FR.signed(e0['key']), FR.signed(p0['key'])]], np.int64))
    assert sim['common'][0].tolist() == [[1, 1], [1, 2]] and sim['sim_sum'][0].tolist() == [0.5, 0.5] and sim['sim_max'][0].tolist() == [0.5, 0.5]
    assert sim['first_equal'][0].tolist() == [0, 1]
    assert FR.tanimoto(2, 2, 2) == 1.0 and FR.tanimoto(0, 0, 0) == 0.0 and FR.tanimoto(1, 1, 2) == 0.5
    # the documented limit: colour refinement cannot tell the skeletons of decalin and bicyclopentyl apart; it does tell apart pairs
    # that differ in their degree sequence
    decalin, bicyclopentyl = one(fused_hexagons()), one(linked_polygons(5))
    assert len(decalin['o']) == len(bicyclopentyl['o']) == 11 and sorted(decalin['inv']) == sorted(bicyclopentyl['inv'])
    assert decalin['key'] == bicyclopentyl['key'] and sorted(decalin['atom_key']) == sorted(bicyclopentyl['atom_key'])
    naphthalene, biphenyl = one(fused_hexagons(), C_ARO), one(linked_polygons(6), C_ARO)
    assert set(naphthalene['cat'].tolist()) == {4} and len(biphenyl['o']) == 13 and naphthalene['key'] != biphenyl['key']
    assert naphthalene['key'] != decalin['key']


def test_order_rotation_and_rounds_do_not_matter_where_they_should_not():
    rng = np.random.default_rng(2)
    two = fused_hexagons()
    base = one(two)
    place = rng.permutation(10)
    perm, turned = one(two[place]), one(rotated(two, 9))
    for m in (perm, turned):
        assert m['key'] == base['key'] and m['bits'] == base['bits'] and sorted(m['atom_key']) == sorted(base['atom_key'])
    assert perm['atom_key'] == [base['atom_key'][k] for k in place]
    # symmetry classes of the fused pair: the two shared atoms, their four neighbours, the four outer atoms
    assert sorted(np.unique(base['atom_key'], return_counts=True)[1].tolist()) == [2, 4, 4]
    # the bits of a smaller radius are a subset; the key does not depend on the radius, the bits not on key_rounds
    for radius in range(4):
        assert one(two, radius=radius)['bits'] <= one(two, radius=radius + 1)['bits']
        assert one(two, radius=radius, key_rounds=8)['key'] == base['key']
    assert one(two, radius=2, key_rounds=16)['bits'] == base['bits'] and one(two, radius=2, key_rounds=2)['key'] != base['key']


def test_recorded_values():
    """tests/golden/fingerprint_known.npz (tools/make_golden_fingerprints.py) pins the hash definition against silent change"""
    g, q = load_golden('fingerprint_known.npz'), load_golden('quality_docked.npz')
    r = FR.fingerprints(q['pos'], q['v'], q['ptr'], CLASS_Z, AROMATIC)
    for k in FR.FP_KEYS:
        np.testing.assert_array_equal(r[k], g[k], err_msg=k)
        assert r[k].dtype == g[k].dtype
    r0 = FR.fingerprints(q['pos'], q['v'], q['ptr'], CLASS_Z, AROMATIC, 0, 0)
    np.testing.assert_array_equal(r0['key'], g['key_r0'])
    np.testing.assert_array_equal(r0['n_bits'], g['n_bits_r0'])
    assert g['n_bits'][0].tolist() == [54, 61, 64, 63, 45] and g['fp_words'].shape == (1, 5, 32)
    pop = [[sum(bin(int(w) & FR.M64).count('1') for w in row) for row in frame] for frame in g['fp_words']]
    assert pop == g['n_bits'].tolist()
    assert FR.mix(0) == 0xE220A8397B1DCDAF                                  # splitmix64's first output for the seed 0


def test_library_entry_points_and_their_checks():
    lib = capi.load_library()
    assert hasattr(lib, 'td_fingerprint') and len(capi.SIGNATURES['td_fingerprint'][1]) == 16
    assert hasattr(lib, 'td_fingerprint_similarity') and len(capi.SIGNATURES['td_fingerprint_similarity'][1]) == 14
    assert lib.td_abi_version() == capi.ABI_VERSION == 5
    header = open(os.path.join(ROOT, 'include', 'targetdiff_hip.h')).read()
    assert '#define TD_ABI_VERSION 5' in header
    for name, commas in (('int td_fingerprint(', 15), ('int td_fingerprint_similarity(', 13)):
        decl = header[header.index(name):]
        assert decl[:decl.index(';')].count(',') == commas
    assert "not RDKit's RDKFingerprint" in header and 'not a canonical form' in header
    assert (capi.FP_BITS, capi.FP_WORDS, capi.FP_MAX_RADIUS, capi.FP_MAX_ROUNDS) == (2048, 32, 4, 16)
    cz = (ctypes.c_int32 * 13)(*CLASS_Z)
    some = ctypes.c_void_p(8)                                                   # never dereferenced: every call below is refused first
    call = lambda S=1, B=1, K=13, radius=2, rounds=8, table=cz, words=None: lib.td_fingerprint(
        None, None, None, S, 0, B, table, K, None, radius, rounds, words, None, None, None, None)
    assert call(S=-1) == -1 and b'bad argument' in lib.td_last_error()
    assert call(B=-1) == -1 and call(S=1 << 20, B=1 << 20) == -1
    assert call(radius=-1) == -1 and b'radius' in lib.td_last_error()
    assert call(radius=5) == -1 and call(radius=3, rounds=2) == -1 and call(rounds=17) == -1 and b'key_rounds' in lib.td_last_error()
    assert call(K=0) == -1 and call(K=65) == -1 and b'class table' in lib.td_last_error()
    assert call(table=None) == -1
    bad = (ctypes.c_int32 * 13)(*([6] * 12 + [35]))
    assert call(table=bad) == -1 and b'atomic number 35' in lib.td_last_error()
    assert call() == -1 and b'null pointer' in lib.td_last_error()              # S = B = 1 without a ligand_ptr
    assert call(S=0) == 0 and call(S=0, B=5, radius=0, rounds=0) == 0 and call(S=3, B=0, radius=4, rounds=16) == 0
    sim = lambda S=1, B=1, Q=0, q_words=None, q_common=None: lib.td_fingerprint_similarity(
        None, None, None, S, B, None, q_words, Q, None, None, None, None, q_common, None)
    assert sim(S=-1) == -1 and b'bad argument' in lib.td_last_error()
    assert sim(B=-1) == -1 and sim(Q=-1) == -1 and sim(S=1 << 20, B=1 << 20) == -1
    assert sim(S=0, Q=1) == -1 and b'query set' in lib.td_last_error()
    assert sim(S=0, Q=1, q_common=some) == -1 and sim(Q=1, q_words=some) == -1 and b'query set' in lib.td_last_error()
    assert sim(S=0, Q=1, q_words=some) == 0                                     # an empty pack has no query_common to write
    assert sim() == -1 and b'null pointer' in lib.td_last_error()
    assert sim(S=0) == 0 and sim(S=4, B=0) == 0 and sim(S=0, B=3, Q=2, q_words=some, q_common=some) == 0     # no work: nothing is touched


def test_binding_refusals_before_any_device_work():
    pos = torch.zeros(2, 5, 3)
    v = torch.zeros(2, 5, dtype=torch.int64)
    ptr = torch.tensor([0, 2, 5], dtype=torch.int32)
    for radius, rounds in ((-1, 8), (5, 8), (3, 2), (2, 17)):
        with pytest.raises(ValueError, match='key_rounds'):
            capi.fingerprint(pos, v, ptr, CLASS_Z, AROMATIC, radius, rounds)
    with pytest.raises(ValueError, match='513 atoms'):
        capi.fingerprint(torch.zeros(1, 513, 3), torch.zeros(1, 513, dtype=torch.int64), torch.tensor([0, 513], dtype=torch.int32), CLASS_Z, AROMATIC)
    with pytest.raises(ValueError, match='prefix offsets'):
        capi.fingerprint(pos, v, torch.tensor([0, 3, 2], dtype=torch.int32), CLASS_Z, AROMATIC)
    with pytest.raises(ValueError, match='one flag per class'):
        capi.fingerprint(pos, v, ptr, CLASS_Z, [True])
    with pytest.raises(ValueError, match='v must be in'):
        capi.fingerprint(pos, v + 13, ptr, CLASS_Z, AROMATIC)
    words, bits, key = torch.zeros(2, 3, 32, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match='fp_words'):
        capi.fingerprint_similarity(words[:, :, :31], bits, key)
    with pytest.raises(ValueError, match='fp_words'):
        capi.fingerprint_similarity(words.to(torch.int32), bits, key)
    with pytest.raises(ValueError, match='n_bits / key'):
        capi.fingerprint_similarity(words, bits.to(torch.int64), key)
    with pytest.raises(ValueError, match='n_bits / key'):
        capi.fingerprint_similarity(words, bits, key[:1])
    with pytest.raises(ValueError, match='include'):
        capi.fingerprint_similarity(words, bits, key, include=torch.ones(2, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match='together'):
        capi.fingerprint_similarity(words, bits, key, q_words=words[0])
    with pytest.raises(ValueError, match='q_words'):
        capi.fingerprint_similarity(words, bits, key, q_words=words, q_bits=bits[0])
    with pytest.raises(ValueError, match='q_bits'):
        capi.fingerprint_similarity(words, bits, key, q_words=words[0], q_bits=bits[0, :2])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU path'):
            capi.fingerprint(pos, v, ptr, CLASS_Z, AROMATIC)
        with pytest.raises(RuntimeError, match='no CPU path'):
            capi.fingerprint_similarity(words, bits, key)
    with pytest.raises(ValueError, match="'complete'"):
        quality.sample_diversity(([], [], [np.zeros((1, 2, 3))], [np.zeros((1, 2), np.int64)], [], [], []), include='stable', device='cpu')


def test_diversity_report_arithmetic_and_merged():
    # one pocket, three frames: m = 4, 1, 0
    rep = quality.DiversityReport.from_frames([4, 1, 0], [3.0, 0.0, 0.0], [3, 1, 0], [2.0, 0.0, 0.0], 5)
    assert rep.num_frames == 3 and rep.n_samples == 5
    assert rep.diversity(0) == 1.0 - 3.0 / 12.0 and rep.uniqueness(0) == 0.75 and rep.mean_nearest(0) == 0.5
    assert math.isnan(rep.diversity(1)) and rep.uniqueness(1) == 1.0 and math.isnan(rep.mean_nearest(1))
    assert math.isnan(rep.diversity(2)) and math.isnan(rep.uniqueness(2)) and rep.reference_similarity(0) == {}
    assert set(rep.summary(0)) == {'diversity', 'uniqueness', 'mean_nearest'}
    # a second pocket with a value where the first has none: the merged value is the mean over the pockets that have one
    other = quality.DiversityReport.from_frames([2, 3, 0], [1.0, 1.5, 0.0], [2, 1, 0], [1.0, 2.4, 0.0], 3)
    assert other.diversity(0) == 0.5 and other.diversity(1) == 0.75 and other.uniqueness(1) == 1.0 / 3.0
    both = quality.DiversityReport.merged([rep, other])
    assert both.diversity(0) == (0.75 + 0.5) / 2 and both.diversity(1) == 0.75 and math.isnan(both.diversity(2))
    assert both.uniqueness(0) == (0.75 + 1.0) / 2 and both.uniqueness(1) == (1.0 + 1.0 / 3.0) / 2
    assert both.mean_nearest(0) == (0.5 + 0.5) / 2 and both.mean_nearest(1) == 2.4 / 3.0
    assert both.n_samples == 8 and both.n_included.tolist() == [6, 4, 0] and both.n_distinct.tolist() == [5, 2, 0]
    assert both.n_diversity.tolist() == [2, 1, 0] and both.n_unique.tolist() == [2, 2, 0]
    assert quality.DiversityReport.merged([rep]).summary(0) == rep.summary(0)
    # with a reference ligand: mean, median and max over the included molecules
    ref_sim = np.array([[0.1, 0.9, 0.4, 0.2], [0.5, 0.7, 0.6, 0.0]])
    inc = np.array([[True, True, True, False], [False, False, True, False]])
    withref = quality.DiversityReport.from_frames(inc.sum(1), [1.0, 0.0], [3, 1], [1.0, 0.0], 4, ref_sim, inc)
    assert withref.reference_similarity(0) == dict(ref_sim_mean=(0.1 + 0.9 + 0.4) / 3, ref_sim_median=0.4, ref_sim_max=0.9)
    assert withref.reference_similarity(1) == dict(ref_sim_mean=0.6, ref_sim_median=0.6, ref_sim_max=0.6)
    twice = quality.DiversityReport.merged([withref, withref])
    assert twice.reference_similarity(0) == withref.reference_similarity(0) and twice.n_ref.tolist() == [2, 2]
    assert set(withref.summary()) == {'diversity', 'uniqueness', 'mean_nearest', 'ref_sim_mean', 'ref_sim_median', 'ref_sim_max'}
    with pytest.raises(ValueError):
        quality.DiversityReport.merged([rep, withref])
    with pytest.raises(ValueError):
        quality.DiversityReport.merged([withref, quality.DiversityReport.from_frames([1, 1], [0, 0], [1, 1], [0, 0], 1)])


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
    monkeypatch.setattr(capi, 'quality_report', patched('quality_report', QR.torch_binding))
    monkeypatch.setattr(capi, 'fingerprint', patched('fingerprint', FR.torch_fingerprint))
    monkeypatch.setattr(capi, 'fingerprint_similarity', patched('fingerprint_similarity', FR.torch_similarity))
    return calls


def repeated_result(seed, T=3):
    """a 7-tuple as sample_diffusion_ligand returns it whose final poses hold molecules twice: eight samples, of which the fused pair of
    hexagons comes three times and the pentagon twice; a jittered, spread-out copy in the frames before (fewer bonds, other duplicates)"""
    rng = np.random.default_rng(seed)
    two = fused_hexagons()
    final = [(ngon(6), C), (two, C), (ngon(5), C), (two[rng.permutation(10)], C), (chain(4), [C, N_, C, O_]), (rotated(ngon(5), seed), C),
             (rotated(two, seed + 1), C), (np.concatenate([ngon(3), ngon(4, (10.0, 0.0, 0.0))]), C)]
    pos_traj, v_traj = [], []
    for p, c in final:
        p = np.asarray(p, np.float64)
        frames = [p * (1.0 + 0.35 * (T - 1 - t)) + rng.normal(0, 0.02 * (T - 1 - t), p.shape) for t in range(T)]
        pos_traj.append(np.stack(frames).astype(np.float32).astype(np.float64))
        v_traj.append(np.tile(np.full(len(p), c, np.int64) if np.isscalar(c) else np.asarray(c, np.int64), (T, 1)))
    return ([p[-1] for p in pos_traj], [v[-1] for v in v_traj], pos_traj, v_traj, [], [], [0.0])


def want_report(res, frames, include=None, reference=None, radius=2, key_rounds=8):
    """the restatement's values for the frames of a result: FR.diversity's dict"""
    pos, v, ptr = packed(res, frames)
    fp = FR.fingerprints(pos, v, ptr, CLASS_Z, AROMATIC, radius, key_rounds)
    inc = None
    if isinstance(include, str) and include == 'complete':
        inc = BR.bond_graph(pos, v, ptr, CLASS_Z, AROMATIC)['n_fragments'] == 1
    elif include is not None:
        inc = np.asarray(include, bool)
    ref_sim = None
    q_words = None
    if reference is not None:
        q = FR.fingerprints(reference[0][None], reference[1][None], [0, len(reference[1])], CLASS_Z, AROMATIC, radius, key_rounds)
        q_words = q['fp_words'][0]
    sim = FR.similarity(fp['fp_words'], fp['n_bits'], fp['key'], inc, q_words)
    if reference is not None:
        c = sim['query_common'][:, :, 0].astype(np.int64)
        ref_sim = np.array([[FR.tanimoto(int(c[s, g]), int(fp['n_bits'][s, g]), int(q['n_bits'][0, 0])) for g in range(c.shape[1])]
                            for s in range(c.shape[0])])
    return FR.diversity(sim, fp['n_bits'], inc, ref_sim), fp, sim


def same_report(rep, want):
    for s in range(rep.num_frames):
        got = rep.summary(s)
        for k, x in got.items():
            np.testing.assert_array_equal(x, want[k][s], err_msg=f'{k} of frame {s}')
    np.testing.assert_array_equal(rep.n_included, want['n_included'])
    np.testing.assert_array_equal(rep.n_distinct, want['n_distinct'])


def test_sample_diversity_packs_a_result(numpy_binding):
    T = 3
    res = repeated_result(4, T)
    ref = (ngon(6).astype(np.float32), np.full(6, C, np.int64))
    for eval_step, frames in ((-1, slice(T - 1, T)), (0, slice(0, 1)), ('all', slice(0, T))):
        want, fp, sim = want_report(res, frames)
        rep = quality.sample_diversity(res, eval_step, device='cpu')
        assert rep.num_frames == (T if eval_step == 'all' else 1) and rep.n_samples == 8 and rep.sum_ref is None
        same_report(rep, want)
        for include in ('complete', np.arange(8 * rep.num_frames).reshape(rep.num_frames, 8) % 3 != 1):
            want2, _, _ = want_report(res, frames, include, ref)
            rep2 = quality.sample_diversity(res, eval_step, include, reference_ligand=ref, device='cpu')
            same_report(rep2, want2)
            assert set(rep2.summary()) == set(rep.summary()) | {'ref_sim_mean', 'ref_sim_median', 'ref_sim_max'}
    # the final poses: 8 samples, the fused pair three times and the pentagon twice -> 5 distinct; the last sample is two fragments
    assert rep.n_distinct[-1] == 5 and rep.uniqueness(-1) == 5 / 8 and sim['first_equal'][-1].tolist() == [0, 1, 2, 1, 4, 2, 1, 7]
    assert sim['sim_max'][-1, 1] == 1.0 and 0.0 < rep.diversity(-1) < 1.0 and rep.n_included.tolist() == [8] * T
    assert rep2.n_included[-1] < 8 and want2['ref_sim_max'][-1] == 1.0        # the hexagon itself is the reference ligand
    done = quality.sample_diversity(res, -1, 'complete', device='cpu')
    assert done.n_included.tolist() == [7] and done.n_distinct.tolist() == [4]
    del numpy_binding[:]
    quality.sample_diversity(res, -1, device='cpu')
    assert numpy_binding == ['fingerprint', 'fingerprint_similarity']
    del numpy_binding[:]
    quality.sample_diversity(res, -1, 'complete', reference_ligand=ref, device='cpu')
    assert numpy_binding == ['bond_graph', 'fingerprint', 'fingerprint', 'fingerprint_similarity']
    # other rounds reach the kernels
    same_report(quality.sample_diversity(res, -1, radius=0, key_rounds=1, device='cpu'), want_report(res, slice(T - 1, T), radius=0, key_rounds=1)[0])
    with pytest.raises(ValueError):
        quality.DiversityReport.merged([rep, done])
    # the public fingerprints object
    pos, v, ptr = packed(res, slice(T - 1, T))
    fp = quality.fingerprints(pos[0], v[0], ligand_ptr=ptr, return_atom_keys=True, device='cpu')
    want = FR.fingerprints(pos, v, ptr, CLASS_Z, AROMATIC)
    for k, t in (('fp_words', fp.fp_words), ('n_bits', fp.n_bits), ('key', fp.key), ('atom_key', fp.atom_key)):
        np.testing.assert_array_equal(t.numpy(), want[k], err_msg=k)
    assert quality.fingerprints(pos, v, ligand_ptr=ptr, device='cpu').atom_key is None
    query = quality.fingerprints(ref[0], ref[1], ligand_ptr=[0, 6], device='cpu')
    r = fp.similarity(query=query, return_common=True)
    np.testing.assert_array_equal(r['common'].numpy(), FR.similarity(want['fp_words'], want['n_bits'], want['key'])['common'])
    assert r['query_sim'][0, :, 0].tolist()[0] == 1.0 and r['query_common'].shape == (1, 8, 1)
    with pytest.raises(ValueError, match='same radius'):
        fp.similarity(query=quality.fingerprints(ref[0], ref[1], ligand_ptr=[0, 6], radius=1, device='cpu'))


def test_evaluate_samples_diversity(numpy_binding, tmp_path, capsys):
    tool = load_tool('evaluate_samples')
    results = {10: repeated_result(5), 2: repeated_result(6)}
    save_results(tmp_path, results)
    base = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu'])
    assert 'diversity' not in base and 'diversity' not in capsys.readouterr().out and 'fingerprint' not in numpy_binding
    out = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--diversity', '--eval_step', 'all'])
    text = capsys.readouterr().out
    wants = [want_report(results[i], slice(0, 3))[0] for i in (2, 10)]
    for k in ('diversity', 'uniqueness', 'mean_nearest'):
        mean = [(wants[0][k][s] + wants[1][k][s]) / 2 for s in range(3)]
        assert out['diversity'][k] == mean[-1] and [c[k] for c in out['diversity']['curve']] == mean
        assert f'{k}:\t{mean[-1]:.4f}\n' in text
    assert out['diversity']['num_included'] == 16 and out['diversity']['num_distinct'] == 10 and 'ref_sim_mean' not in out['diversity']
    assert {k: base[k] for k in ('mol_stable', 'atm_stable')} == {k: out[k] for k in ('mol_stable', 'atm_stable')}
    saved = json.load(open(tmp_path / 'eval_results' / 'quality.json'))
    assert saved['diversity']['uniqueness'] == out['diversity']['uniqueness']
    # a reference ligand from an SD file, hydrogens and an element outside the table left out; with --include complete
    ref = dict(name='known', symbols=['C'] * 6 + ['H', 'Br'], pos=np.concatenate([ngon(6), [[0.0, 0.0, 1.1], [9.0, 0.0, 0.0]]]),
               bonds=[(k, (k + 1) % 6, 1) for k in range(6)] + [(0, 6, 1)])
    molfile.write_sdf(tmp_path / 'known.sdf', [ref])
    inc = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--diversity', '--include', 'complete', '--reference_sdf',
                     str(tmp_path / 'known.sdf')])
    text = capsys.readouterr().out
    assert 'reference ligand: 1 atoms of elements outside the table left out' in text
    ligand = (ngon(6).round(4).astype(np.float32), np.full(6, C, np.int64))
    wants = [want_report(results[i], slice(2, 3), 'complete', ligand)[0] for i in (2, 10)]
    for k in ('diversity', 'uniqueness', 'ref_sim_mean', 'ref_sim_median', 'ref_sim_max'):
        assert inc['diversity'][k] == (wants[0][k][0] + wants[1][k][0]) / 2, k
    assert inc['diversity']['num_included'] == 14 and inc['diversity']['ref_sim_max'] == 1.0 and 'ref_sim_max:\t1.0000\n' in text
    # the same ligand from an npz that holds nothing else
    np.savez(tmp_path / 'ligand.npz', ligand_pos=ligand[0], ligand_v=ligand[1])
    npz = tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--diversity', '--include', 'complete', '--reference_npz',
                     str(tmp_path / 'ligand.npz')])
    assert npz['diversity'] == inc['diversity'] and npz['JSD_CC_2A'] is None


def test_export_sdf_unique(numpy_binding, tmp_path):
    tool = load_tool('export_sdf')
    res = repeated_result(8)
    save_results(tmp_path, {0: res})
    plain = tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'plain'), '--device', 'cpu'])
    assert plain['result_0']['written'] == 8 and 'fingerprint' not in numpy_binding         # without the flag: no fingerprint launch
    out = tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'unique'), '--device', 'cpu', '--unique'])
    assert out['result_0']['written'] == 5 and out['result_0']['samples'] == 8
    recs = parse_sdf(open(tmp_path / 'unique' / 'result_0.sdf').read())
    assert [r[0] for r in recs] == ['sample_0', 'sample_1', 'sample_2', 'sample_4', 'sample_7']
    before = {r[0]: r for r in parse_sdf(open(tmp_path / 'plain' / 'result_0.sdf').read())}
    assert all(before[r[0]] == r for r in recs)                                 # the records themselves are unchanged
    both = tool.main(['--sample_path', str(tmp_path), '--out', str(tmp_path / 'both'), '--device', 'cpu', '--unique', '--only-complete'])
    assert both['result_0']['written'] == 4
    assert [r[0] for r in parse_sdf(open(tmp_path / 'both' / 'result_0.sdf').read())] == ['sample_0', 'sample_1', 'sample_2', 'sample_4']
    # the keys are of the whole molecule: a pentagon and a pentagon with a far atom are both written under --largest-fragment,
    # and --only-complete decides before --unique does: an incomplete first copy does not shadow a complete second one
    lone = np.concatenate([ngon(5), [[30.0, 0.0, 0.0]]])
    mols = [(lone, C), (ngon(5), C), (rotated(ngon(5), 1), C), (lone[::-1], C)]
    pos_traj = [np.asarray(p, np.float64).astype(np.float32).astype(np.float64)[None] for p, _ in mols]
    v_traj = [np.full((1, len(p)), c, np.int64) for p, c in mols]
    other = tmp_path / 'other'
    other.mkdir()
    save_results(other, {3: ([p[-1] for p in pos_traj], [x[-1] for x in v_traj], pos_traj, v_traj, [], [], [0.0])})
    names = lambda *flags: [r[0] for r in parse_sdf(open(tool.main(['--sample_path', str(other), '--out', str(other / 'o'), '--device', 'cpu',
                                                                   *flags])['result_3']['path']).read())]
    assert names('--unique') == ['sample_0', 'sample_1']
    assert names('--unique', '--largest-fragment') == ['sample_0', 'sample_1']
    assert names('--unique', '--only-complete') == ['sample_1']
    assert names('--only-complete') == ['sample_1', 'sample_2']


def test_sdf_reader_round_trips_write_sdf(tmp_path):
    res = ragged_result(11, [7, 1, 12, 5], 2)
    pos, v, ptr = packed(res, slice(1, 2))
    g = BR.bond_graph(pos, v, ptr, CLASS_Z, AROMATIC)
    cz = np.asarray(CLASS_Z)
    mols = []
    for k, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        k0, k1 = g['bond_ptr'][k], g['bond_ptr'][k + 1]
        mols.append(dict(name=f'm{k}', symbols=[molfile.ELEMENT_SYMBOLS[int(z)] for z in cz[v[0, a:b]]], pos=pos[0, a:b],
                         bonds=[(int(i - a), int(j - a), int(c)) for (i, j), c in zip(g['bond_atoms'][k0:k1], g['bond_category'][k0:k1])],
                         properties=dict(n_atoms=int(b - a), note='x y')))
    mols.append(dict(name='', symbols=[], pos=np.zeros((0, 3)), bonds=[]))
    path = tmp_path / 'round.sdf'
    assert molfile.write_sdf(path, mols) == 5
    back = molfile.read_sdf(path)
    assert len(back) == 5 and [m['name'] for m in back] == ['m0', 'm1', 'm2', 'm3', '']
    for m, r in zip(mols, back):
        heavy = [k for k, sym in enumerate(m['symbols']) if sym != 'H']
        new = {k: n for n, k in enumerate(heavy)}
        assert r['symbols'] == [m['symbols'][k] for k in heavy]
        np.testing.assert_array_equal(r['pos'], np.asarray(m['pos'], np.float64).round(4)[heavy].reshape(-1, 3))
        assert r['bonds'] == [(new[i], new[j], t) for i, j, t in m['bonds'] if i in new and j in new]
        assert r['properties'] == {k: str(x) for k, x in (m.get('properties') or {}).items()}
    assert any('H' in m['symbols'] for m in mols) and sum(len(m['bonds']) for m in back) > 0
    # what was read writes the same file again when there was no hydrogen to drop
    no_h = [m for m in mols if 'H' not in m['symbols']]
    molfile.write_sdf(tmp_path / 'a.sdf', no_h)
    molfile.write_sdf(tmp_path / 'b.sdf', molfile.read_sdf(tmp_path / 'a.sdf'))
    # (coordinates are written with four decimals, so a second pass is exact)
    assert [parse_sdf(open(tmp_path / n).read()) for n in ('b.sdf',)] == [parse_sdf(open(tmp_path / 'a.sdf').read())]
    # classes for the fingerprint: the element and, under 'add_aromatic', a bond of type 4
    mol = dict(symbols=['C', 'C', 'N', 'O', 'Cl', 'S'], pos=np.zeros((6, 3)), bonds=[(0, 1, 1), (1, 2, 4), (3, 4, 2)])
    assert molfile.ligand_classes(mol)[1].tolist() == [1, 2, 4, 5, 12, 10] and molfile.ligand_classes(mol)[0].dtype == np.float32
    assert molfile.ligand_classes(mol, 'basic')[1].tolist() == [1, 1, 2, 3, 7, 6]
    bromo = dict(symbols=['C', 'Br', 'N'], pos=np.arange(9.0).reshape(3, 3), bonds=[(0, 1, 1)])
    with pytest.raises(ValueError, match="'Br'"):
        molfile.ligand_classes(bromo)
    p, c = molfile.ligand_classes(bromo, drop_unknown=True)
    assert c.tolist() == [1, 3] and p.tolist() == [[0.0, 1.0, 2.0], [6.0, 7.0, 8.0]]
    (tmp_path / 'v3000.sdf').write_text('x\n\n\n  0  0  0     0  0            999 V3000\nM  END\n$$$$\n')
    with pytest.raises(ValueError, match='V2000'):
        molfile.read_sdf(tmp_path / 'v3000.sdf')
