"""td_pocket_report on the GPU (csrc/pocket.hip) against tests/_pocket_ref.py: array_equal on every integer output and min_dist bit for
bit, no tolerance anywhere (the restatement is pinned to hand-counted cases on the host, tests/test_pocket_host.py).

  1. a grid of packs: pockets of 0 .. 600 atoms around the 64-atom ballot word and the 256-atom workgroup stride, ragged molecules of
     0 .. 512 atoms, one and three frames, random clouds and lattice coordinates with many equal distances; an include mask and
     reference words in every case.
  2. planted packs with exact fp32 coordinates: pairs exactly at the cutoff and at a clash threshold with their neighbours, a class
     outside the table, protein atoms that take no part, a far molecule, a pack without pairs.
  3. the size bound, include masks, null optional outputs, reference bits, batch independence, repeatability.
  4. end to end on the 1h36 pocket and its docked ligand: SamplePack.pocket and sample_pocket.
"""
import types

import numpy as np
import pytest
import torch

import _pocket_ref as PR
from conftest import load_golden
from targetdiff_amd import capi, quality

pytestmark = pytest.mark.gpu

CLASS_Z = quality.class_atomic_numbers('add_aromatic')
TABLE = PR.clash_table()
SIZES = [0, 1, 2, 63, 64, 65, 512]
INT_KEYS = tuple(k for k in PR.KEYS if k != 'min_dist')


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


def run(c, cutoff=4.0, table=TABLE, include=None, ref_bits=None, atoms=True, bits=True, n_kinds=40, check=False):
    """capi.pocket_report of a case's numpy arrays, as numpy"""
    dev = _dev()
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    inc = None if include is None else t(include, torch.bool)
    ref = None if ref_bits is None else t(ref_bits, torch.int64)
    out = capi.pocket_report(t(c['pos'], torch.float32), t(c['v'], torch.int64), t(c['ptr'], torch.int32), CLASS_Z, t(c['ppos'], torch.float32),
                             t(c['pelem'], torch.int32), t(c['pkind'], torch.int32), n_kinds, cutoff, table, inc, ref, atoms, bits, check=check)
    return {k: (None if x is None else x.cpu().numpy()) for k, x in out.items()}


def want(c, cutoff=4.0, table=TABLE, include=None, ref_bits=None, n_kinds=40):
    return PR.pocket_report(c['pos'], c['v'], c['ptr'], CLASS_Z, c['ppos'], c['pelem'], c['pkind'], n_kinds, cutoff, table, include, ref_bits)


def same(a, b, what, keys=PR.KEYS):
    for k in keys:
        if b[k] is None:
            assert a[k] is None, f'{what}: {k}'
        elif k == 'min_dist':
            assert a[k].dtype == np.float64
            np.testing.assert_array_equal(a[k].view(np.int64), b[k].view(np.int64), err_msg=f'{what}: min_dist, bit for bit')
        else:
            assert a[k].dtype == b[k].dtype, f'{what}: {k}'
            np.testing.assert_array_equal(a[k], b[k], err_msg=f'{what}: {k}')


def against_restatement(c, what, **kw):
    r = run(c, **kw)
    same(r, want(c, **{k: x for k, x in kw.items() if k in ('cutoff', 'table', 'include', 'ref_bits', 'n_kinds')}), what)
    return r


_CACHE = {}


def baseline():
    """one pack through the kernel and the restatement, once: shared by the tests that need a baseline, and left unchanged"""
    if 'base' not in _CACHE:
        c = PR.build_case(11, 300, [5, 70, 0, 31, 129, 12], S=2)
        _CACHE['base'] = (c, run(c), want(c))
    return _CACHE['base']


@pytest.mark.parametrize('lattice', [False, True], ids=['cloud', 'lattice'])
@pytest.mark.parametrize('n_p', [0, 1, 63, 64, 65, 255, 256, 257, 600])
def test_every_output_equals_the_restatement(n_p, lattice):
    S = 1 if lattice else 3
    c = PR.build_case(100 + n_p, n_p, SIZES, S, lattice)
    rng = np.random.default_rng(n_p)
    include = rng.random((S, len(SIZES))) < 0.6
    ref_bits = PR.pack_bits(rng.random(n_p) < 0.3)
    r = against_restatement(c, f'N_p = {n_p}', include=include, ref_bits=ref_bits)
    assert r['bits'].shape == (S, len(SIZES), (n_p + 63) // 64) and r['kind_hist'].shape == (S, 8, 40) and r['pocket_freq'].shape == (S, n_p)
    if n_p >= 63:
        assert r['n_contacts'][:, 3:].min() > 0 and r['n_clashes'].sum() > 0 and r['n_ref_common'].sum() > 0
        assert (r['n_pocket_atoms'][:, 6] > 0.5 * ((c['pelem'] >= 0) & (c['pkind'] >= 0)).sum()).all()     # the ballot words fill up
        assert np.isinf(r['min_dist'][:, 0]).all() and np.isfinite(r['min_dist'][:, 1:]).all()
    else:
        assert np.isinf(r['min_dist'][:, 0]).all()
    if lattice and n_p >= 255:
        d = PR.distances(c['pos'][0], c['ppos'])
        assert (d == 4.0).sum() > 0                                              # pairs exactly at the cutoff are in the pack


def planted(lig, cls, prot, pelem=None, pkind=None):
    lig, prot = np.asarray(lig, np.float32).reshape(-1, 3), np.asarray(prot, np.float32).reshape(-1, 3)
    return dict(pos=lig[None], v=np.asarray(cls, np.int64)[None], ptr=np.asarray([0, len(lig)], np.int32), ppos=prot,
                pelem=np.full(len(prot), 1, np.int32) if pelem is None else np.asarray(pelem, np.int32),
                pkind=np.zeros(len(prot), np.int32) if pkind is None else np.asarray(pkind, np.int32))


def test_pairs_exactly_at_the_cutoff_and_at_a_threshold():
    below, above = np.nextafter(np.float32(5), np.float32(0)), np.nextafter(np.float32(5), np.float32(9))
    prot = [(5, 0, 0), (0, 5, 0), (0, 0, 5), (3, 4, 0), (0, 3, 4), (4, 0, 3), (below, 0, 0), (0, below, 0), (0, 0, below),
            (above, 0, 0), (0, above, 0), (0, 0, above), (-5, 0, 0), (0, -3, -4)]
    c = planted([(0, 0, 0)], [1], prot, pkind=np.arange(14))
    d = PR.distances(c['pos'][0], c['ppos'])[0]
    assert (d == 5.0).sum() == 8 and (d < 5.0).sum() == 3 and (d > 5.0).sum() == 3
    for cutoff, n in ((5.0, 3), (float(np.nextafter(5.0, 9.0)), 11), (float(np.nextafter(5.0, 0.0)), 3), (float(below), 0),
                      (float(np.nextafter(np.float64(above), 9.0)), 14)):
        table = np.full((8, 6), cutoff)                                          # the same limits through the clash pass
        r = against_restatement(c, f'cutoff {cutoff!r}', cutoff=cutoff, table=table)
        assert r['n_contacts'][0, 0] == r['n_clashes'][0, 0] == r['n_pocket_atoms'][0, 0] == n, cutoff
        assert r['min_dist'][0, 0] == float(below)
    # a threshold per element pair: only the carbon - oxygen entry lets the pairs at exactly 5 in
    table = np.full((8, 6), 5.0)
    table[1, 3] = np.nextafter(5.0, 9.0)
    c['pelem'][:] = [3, 1, 3, 1, 3, 1, 1, 1, 1, 3, 3, 3, 3, 1]
    r = against_restatement(c, 'threshold per pair', cutoff=1.0, table=table)
    assert r['n_contacts'][0, 0] == 0 and r['n_clashes'][0, 0] == 3 + 4 and r['n_clash_atoms'][0, 0] == 1 and r['atom_clash'][0, 0] == 7


def test_atoms_that_take_no_part_a_far_molecule_and_a_pack_without_pairs():
    prot = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (2, 0, 0)]
    # ligand classes -1 and 13 are outside [0, 13); protein atom 1 has kind -1, atom 2 element -1, atom 3 both
    c = planted([(0, 0, 0), (0.5, 0, 0), (0, 0.5, 0), (0, 0, 0.5)], [1, -1, 13, 3], prot, pelem=[1, 2, -1, -1, 3], pkind=[0, -1, 5, -1, 7])
    r = against_restatement(c, 'no part')
    assert r['n_contacts'][0, 0] == 4 and r['atom_contacts'][0].tolist() == [2, 0, 0, 2] and r['n_pocket_atoms'][0, 0] == 2
    assert r['bits'][0, 0, 0] == 0b10001 and r['pocket_freq'][0].tolist() == [1, 0, 0, 0, 1] and r['min_dist'][0, 0] == 1.0
    assert r['kind_hist'][0].sum() == 4 and r['kind_hist'][0, 1, 0] == r['kind_hist'][0, 1, 7] == r['kind_hist'][0, 2, 0] == 1
    far = planted([(100, 0, 0), (101, 0, 0)], [1, 1], prot)
    r = against_restatement(far, 'far')
    for k in ('n_contacts', 'n_contact_atoms', 'n_pocket_atoms', 'n_clashes', 'n_clash_atoms', 'atom_contacts', 'kind_hist', 'pocket_freq', 'bits'):
        assert not r[k].any(), k
    assert r['min_dist'][0, 0] == 98.0
    for nothing in (planted([(0, 0, 0)], [1], prot, pkind=[-1] * 5), planted([(0, 0, 0)], [-1], prot), planted([(0, 0, 0)], [1], np.zeros((0, 3)))):
        r = against_restatement(nothing, 'no pairs')
        assert r['min_dist'][0, 0] == np.inf and r['n_contacts'][0, 0] == 0 and not r['kind_hist'].any()


def test_an_oversize_molecule_is_answered_with_minus_one_and_its_neighbours_are_not_affected():
    sizes = [20, 513, 33]
    c = PR.build_case(5, 130, sizes, S=2)
    r = run(c, include=np.ones((2, 3), bool), ref_bits=PR.pack_bits(np.ones(130, bool)))
    w = want(c, include=np.ones((2, 3), bool), ref_bits=PR.pack_bits(np.ones(130, bool)))
    same(r, w, 'oversize')
    for k in ('n_contacts', 'n_contact_atoms', 'n_pocket_atoms', 'n_clashes', 'n_clash_atoms', 'n_ref_common'):
        assert (r[k][:, 1] == -1).all() and (r[k][:, [0, 2]] > 0).all(), k
    assert np.isinf(r['min_dist'][:, 1]).all() and not r['bits'][:, 1].any() and not r['atom_contacts'][:, 20:533].any()
    # its neighbours alone give the same rows, the same histogram and the same map
    alone = dict(c, pos=np.concatenate([c['pos'][:, :20], c['pos'][:, 533:]], 1), v=np.concatenate([c['v'][:, :20], c['v'][:, 533:]], 1),
                 ptr=np.asarray([0, 20, 53], np.int32))
    a = run(alone)
    for k in PR.MOL_KEYS + PR.CLASH_KEYS + ('bits',):
        np.testing.assert_array_equal(a[k], r[k][:, [0, 2]], err_msg=k)
    same(a, r, 'the oversize molecule adds nothing', PR.SUM_KEYS)
    with pytest.raises(ValueError, match='at most 512'):
        run(c, check=True)


def test_include_masks_change_the_sums_over_molecules_only():
    c, r, w = baseline()
    same(r, w, 'baseline')
    S, B = r['n_contacts'].shape
    alternating = (np.arange(S * B).reshape(S, B) % 2).astype(bool)
    for name, mask in (('all', np.ones((S, B), bool)), ('none', np.zeros((S, B), bool)), ('alternating', alternating)):
        m = against_restatement(c, name, include=mask)
        same(m, r, f'{name}: the per-molecule outputs do not depend on the mask', tuple(k for k in PR.KEYS if k not in PR.SUM_KEYS))
    same(against_restatement(c, 'all', include=np.ones((S, B), bool)), r, 'all = None', PR.SUM_KEYS)
    none = run(c, include=np.zeros((S, B), bool))
    assert not none['kind_hist'].any() and not none['pocket_freq'].any()
    assert 0 < run(c, include=alternating)['kind_hist'].sum() < r['kind_hist'].sum() == r['n_contacts'].sum()


def test_null_optional_outputs_change_nothing_else():
    c, r, _ = baseline()
    ref = PR.pack_bits(np.arange(300) % 3 == 0)
    full = run(c, ref_bits=ref)
    same(full, r, 'reference words', tuple(k for k in PR.KEYS if k != 'n_ref_common'))
    for kw, gone in ((dict(atoms=False), PR.ATOM_KEYS), (dict(bits=False), ('bits',)), (dict(table=None), PR.CLASH_KEYS + ('atom_clash',)),
                     (dict(atoms=False, bits=False, table=None), PR.ATOM_KEYS + ('bits',) + PR.CLASH_KEYS)):
        x = run(c, **dict(dict(ref_bits=ref), **kw))
        for k in gone:
            assert x[k] is None, k
        same(x, full, str(kw), tuple(k for k in PR.KEYS if k not in gone))
    assert r['n_ref_common'] is None


def test_reference_bits():
    c, r, _ = baseline()
    B = r['bits'].shape[1]
    for s, g in ((0, 1), (1, 4)):                                               # a molecule's own words: everything it touches is common
        own = run(c, ref_bits=r['bits'][s, g])
        assert own['n_ref_common'][s, g] == r['n_pocket_atoms'][s, g] > 0
        touched = PR.unpack_bits(r['bits'], 300)
        np.testing.assert_array_equal(own['n_ref_common'], (touched & touched[s, g]).sum(-1))
    ref = PR.pack_bits(np.random.default_rng(3).random(300) < 0.5)
    against_restatement(c, 'arbitrary reference', ref_bits=ref)
    # the bits agree with the contact map summed over the molecules, and with the counts
    np.testing.assert_array_equal(PR.unpack_bits(r['bits'], 300).sum(1), r['pocket_freq'])
    np.testing.assert_array_equal(PR.unpack_bits(r['bits'], 300).sum(-1), r['n_pocket_atoms'])
    assert r['bits'].shape == (2, B, 5) and not (r['bits'][..., 4].view(np.uint64) >> np.uint64(300 - 256)).any()      # no bit past N_p


def test_a_molecule_does_not_depend_on_its_pack_and_two_calls_give_identical_bytes():
    c, r, _ = baseline()
    ptr = c['ptr']
    g = 4                                                                        # the 129-atom molecule
    mol = dict(c, pos=c['pos'][:, ptr[g]:ptr[g + 1]], v=c['v'][:, ptr[g]:ptr[g + 1]], ptr=np.asarray([0, 129], np.int32))
    other = PR.build_case(12, 300, [40, 3], S=2)
    first = dict(mol, pos=np.concatenate([mol['pos'], other['pos']], 1), v=np.concatenate([mol['v'], other['v']], 1), ptr=np.asarray([0, 129, 169, 172], np.int32))
    last = dict(mol, pos=np.concatenate([other['pos'], mol['pos']], 1), v=np.concatenate([other['v'], mol['v']], 1), ptr=np.asarray([0, 40, 43, 172], np.int32))
    for what, pack, at, lo in (('alone', mol, 0, 0), ('first', first, 0, 0), ('last', last, 2, 43)):
        x = run(pack)
        for k in PR.MOL_KEYS + PR.CLASH_KEYS + ('bits',):
            np.testing.assert_array_equal(x[k][:, at].view(np.int64 if k == 'min_dist' else x[k].dtype), r[k][:, g].view(np.int64 if k == 'min_dist' else r[k].dtype),
                                          err_msg=f'{what}: {k}')
        for k in PR.ATOM_KEYS:
            np.testing.assert_array_equal(x[k][:, lo:lo + 129], r[k][:, ptr[g]:ptr[g + 1]], err_msg=f'{what}: {k}')
    again = run(c)
    for k in PR.KEYS:
        assert (again[k] is None and r[k] is None) or again[k].tobytes() == r[k].tobytes(), k


def test_empty_packs():
    c = PR.build_case(1, 70, [4, 9], S=2)
    for S, sizes in ((0, [4, 9]), (2, [])):
        e = PR.build_case(1, 70, sizes, S=S)
        r = against_restatement(e, f'S = {S}, B = {len(sizes)}', include=np.ones((S, len(sizes)), bool), ref_bits=PR.pack_bits(np.ones(70, bool)))
        assert r['n_contacts'].shape == (S, len(sizes)) and r['kind_hist'].shape == (S, 8, 40) and not r['pocket_freq'].any()
    against_restatement(c, 'six kinds', n_kinds=6)                               # kinds 6 .. 39 of the case now take no part


def docked():
    p, l = load_golden('pocket_1h36.npz'), load_golden('ligand_1h36_docked.npz')
    cls = {'H': 0, 'C': 1, 'N': 3, 'O': 5, 'F': 7, 'P': 8, 'S': 10, 'Cl': 12, 'Br': 12}      # Br is outside the table: taken as Cl
    return p, l['pos'].astype(np.float32), np.asarray([cls[str(e)] for e in l['elements']], np.int64)


def test_sample_pocket_on_the_1h36_pocket_and_its_docked_ligand():
    dev = _dev()
    p, lpos, lv = docked()
    rng = np.random.default_rng(0)
    T = 3
    # a result of three samples: the docked pose, a jittered copy, and a copy moved 30 A away; three frames that end in those poses
    final = [lpos, (lpos + rng.normal(0, 0.5, lpos.shape)).astype(np.float32), lpos[:17] + np.float32(30)]
    pos_traj = [np.stack([(x + rng.normal(0, 0.3 * (T - 1 - t), x.shape)).astype(np.float32) for t in range(T)]).astype(np.float64) for x in final]
    v_traj = [np.stack([lv[:len(x)]] * T) for x in final]
    data = types.SimpleNamespace(protein_pos=torch.from_numpy(p['pos']), protein_atom_feature=torch.from_numpy(p['feat'].astype(np.int64)))
    result = {'data': data, 'pred_ligand_pos_traj': pos_traj, 'pred_ligand_v_traj': v_traj}
    elem, kind, names = quality.pocket_kinds(p['feat'])
    assert len(names) == 40 and (elem >= 0).all()
    for eval_step, frames in ((-1, slice(T - 1, T)), ('all', slice(0, T))):
        pack = dict(pos=np.concatenate([x[frames] for x in pos_traj], 1).astype(np.float32), v=np.concatenate([x[frames] for x in v_traj], 1),
                    ptr=np.asarray([0, 25, 50, 67], np.int32), ppos=p['pos'], pelem=elem, pkind=kind)
        ref = PR.pocket_report(lpos[None], lv[None], [0, 25], CLASS_Z, p['pos'], elem, kind, 40, 4.0)
        w = want(pack, ref_bits=ref['bits'][0, 0])
        raw = {k: w[k] for k in ('n_contacts', 'n_contact_atoms', 'n_pocket_atoms', 'n_clashes', 'min_dist', 'n_ref_common', 'kind_hist', 'pocket_freq')}
        S = w['n_contacts'].shape[0]
        expect = quality.PocketReport.from_outputs(raw, np.ones((S, 3), bool), [25, 25, 17], names, [n.endswith('.bb') for n in names],
                                                   int(ref['n_pocket_atoms'][0, 0]))
        got = quality.sample_pocket(result, eval_step, reference_ligand=(lpos, lv), device=dev)
        method = quality.SamplePack(result, eval_step, device=dev).pocket(data, reference_ligand=(lpos, lv))
        for rep in (got, method):
            assert vars(rep).keys() == vars(expect).keys()
            for k, x in vars(expect).items():
                if isinstance(x, np.ndarray):
                    np.testing.assert_array_equal(getattr(rep, k), x, err_msg=k)
            for s in range(S):
                np.testing.assert_equal(rep.summary(s), expect.summary(s))
        assert w['n_contacts'][-1, 0] > 0 and w['n_contacts'][-1, 2] == 0 and got.no_contact(-1) == 1 / 3
    # the docked ligand against itself: every contact recovered
    own = {'data': data, 'pred_ligand_pos_traj': [lpos[None].astype(np.float64)], 'pred_ligand_v_traj': [lv[None]]}
    rep = quality.sample_pocket(own, reference_ligand=(lpos, lv), device=dev)
    s = rep.summary()
    assert s['ref_recovery_mean'] == s['ref_recovery_median'] == s['ref_recovery_max'] == 1.0 and s['ref_tanimoto'] == 1.0
    assert s['mean_contacts'] > 0 and s['no_contact'] == 0.0 and 0 < s['buried_share'] <= 1.0
    freq = rep.contact_frequency()
    assert freq.shape == (572,) and set(np.unique(freq)) == {0.0, 1.0} and abs(sum(rep.contact_profile().values()) - 1.0) < 1e-12
    # the stateless function gives the kernel's raw outputs on the same pocket
    c = quality.pocket_contacts(p['pos'], p['feat'], lpos, lv, ligand_ptr=torch.tensor([0, 25], dtype=torch.int32), return_bits=True, device=dev)
    w = PR.pocket_report(lpos[None], lv[None], [0, 25], CLASS_Z, p['pos'], elem, kind, 40, 4.0, TABLE)
    same({k: (None if getattr(c, k) is None else getattr(c, k).cpu().numpy()) for k in PR.KEYS}, w, 'pocket_contacts')
    assert c.clash_free.shape == (1, 1) and c.names == names
