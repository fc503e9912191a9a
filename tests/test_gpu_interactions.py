"""td_interaction_report on the GPU (csrc/interactions.hip) against tests/_interactions_ref.py: array_equal on every output, no tolerance
anywhere -- every output is an integer (the restatement is pinned to hand-counted cases on the host, tests/test_interactions_host.py).

  1. a grid of packs: pockets of 0 .. 257 atoms around the 64-atom ballot word and the 256-atom workgroup stride and tile, ragged
     molecules of 0 .. 512 atoms in packs of five, one and three frames; an include mask, reference words, classes outside the table and
     protein atoms that take no part in every case.  The restatement's own output must show every role and every interaction type.
  2. cutoffs that differ from the defaults, include masks, null optional outputs, reference bits present and absent, the size bound,
     empty packs, repeatability.
  3. the 1h36 pocket and its docked ligand, also with a 4.5 A hydrogen-bond cutoff; SamplePack.interactions and sample_interactions.
"""
import types

import numpy as np
import pytest
import torch

import _interactions_ref as IR
import _pocket_ref as PR
from conftest import load_golden
from targetdiff_amd import capi, quality

pytestmark = pytest.mark.gpu

CLASS_Z = quality.class_atomic_numbers('add_aromatic')
PACKS = {'small-and-512': ([0, 512, 2, 63, 1], 3), 'around-64': ([64, 65, 1, 0, 2], 1)}
CUTOFFS = ('hbond_cutoff', 'hydrophobic_cutoff', 'hetero_cutoff')


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


def run(c, include=None, ref_bits=None, atoms=True, bits=True, n_kinds=40, check=False, **cutoffs):
    """capi.interaction_report of a case's numpy arrays, as numpy"""
    dev = _dev()
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    inc = None if include is None else t(include, torch.bool)
    ref = None if ref_bits is None else t(ref_bits, torch.int64)
    out = capi.interaction_report(t(c['pos'], torch.float32), t(c['v'], torch.int64), t(c['ptr'], torch.int32), CLASS_Z,
                                  t(c['ppos'], torch.float32), t(c['pelem'], torch.int32), t(c['pkind'], torch.int32),
                                  t(c['prole'], torch.int32), n_kinds, include=inc, ref_bits=ref, return_atoms=atoms, return_bits=bits,
                                  check=check, **cutoffs)
    return {k: (None if x is None else x.cpu().numpy()) for k, x in out.items()}


def want(c, include=None, ref_bits=None, n_kinds=40, **cutoffs):
    return IR.interaction_report(c['pos'], c['v'], c['ptr'], CLASS_Z, c['ppos'], c['pelem'], c['pkind'], c['prole'], n_kinds,
                                 include=include, ref_bits=ref_bits, **cutoffs)


def same(a, b, what, keys=IR.KEYS):
    assert set(a) == set(IR.KEYS)
    for k in keys:
        if b[k] is None:
            assert a[k] is None, f'{what}: {k}'
        else:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, f'{what}: {k}'
            np.testing.assert_array_equal(a[k], b[k], err_msg=f'{what}: {k}')


def against_restatement(c, what, **kw):
    r, w = run(c, **kw), want(c, **{k: x for k, x in kw.items() if k in ('include', 'ref_bits', 'n_kinds') + CUTOFFS})
    same(r, w, what)
    return r, w


def ref_words(rng, n_p):
    return np.stack([PR.pack_bits(rng.random(n_p) < 0.4) for _ in range(3)])


_CACHE = {}


def baseline():
    """one pack through the kernel and the restatement, once: shared by the tests that need a baseline, and left unchanged"""
    if 'base' not in _CACHE:
        c = IR.build_case(11, 300, [5, 70, 0, 31, 129], S=2)
        _CACHE['base'] = (c, run(c), want(c))
    return _CACHE['base']


@pytest.mark.parametrize('pack', list(PACKS))
@pytest.mark.parametrize('n_p', [0, 1, 63, 64, 65, 255, 256, 257])
def test_every_output_equals_the_restatement(n_p, pack):
    sizes, S = PACKS[pack]
    c = IR.build_case(100 + n_p, n_p, sizes, S)
    rng = np.random.default_rng(n_p)
    c['v'][:, ::37] = -1                                                         # classes outside [0, 13)
    c['v'][:, 5::41] = 13
    include = rng.random((S, len(sizes))) < 0.6
    include[:, 1], include[:, 2] = True, False                                  # a large molecule is in, a small one out, in both packs
    r, w = against_restatement(c, f'N_p = {n_p}', include=include, ref_bits=ref_words(rng, n_p))
    W = (n_p + 63) // 64
    assert r['bits'].shape == (S, 5, 3, W) and r['kind_hist'].shape == (S, 3, 40) and r['pocket_freq'].shape == (S, 3, n_p)
    assert r['n_ref_common'].shape == (S, 5, 3) and r['protein_role'].shape == (n_p,)
    # no case passes vacuously: the restatement itself shows every ligand role, the bonds that make them and, with a pocket, every
    # protein role and every interaction type
    roles = set(np.unique(w['atom_role']).tolist())
    assert roles >= {0, IR.DONOR, IR.ACCEPTOR, IR.DONOR | IR.ACCEPTOR, IR.HYDROPHOBIC}
    assert w['n_donors'].sum() > 0 and w['n_acceptors'].sum() > 0 and w['n_hydrophobic_atoms'].sum() > 0
    if n_p >= 63:
        assert set(np.unique(w['protein_role']).tolist()) == {-1, 0, 1, 2, 3, 4}
        for k in ('n_donated', 'n_accepted', 'n_hbonds', 'n_hydrophobic', 'n_hb_atoms', 'n_ref_common', 'kind_hist', 'pocket_freq'):
            assert w[k].max() > 0, k
        assert (w['n_donated'] + w['n_accepted'] - w['n_hbonds']).sum() > 0       # pairs that donate and accept at once
        assert w['kind_hist'].sum((0, 2)).min() > 0 and w['bits'].any((0, 1, 3)).all()
        carbons = (c['pelem'] == 1) & (w['protein_role'] >= 0)
        assert 0 < (w['protein_role'][carbons] == IR.HYDROPHOBIC).sum() < carbons.sum()


def test_cutoffs_that_differ_from_the_defaults():
    c, r, w = baseline()
    same(r, w, 'defaults')
    seen = []
    for kw in (dict(hbond_cutoff=2.5), dict(hbond_cutoff=5.0, hydrophobic_cutoff=3.0), dict(hydrophobic_cutoff=6.25),
               dict(hetero_cutoff=1.0), dict(hetero_cutoff=2.5), dict(hbond_cutoff=1e-3, hydrophobic_cutoff=1e-3, hetero_cutoff=1e-3),
               dict(hbond_cutoff=1e3, hydrophobic_cutoff=1e3, hetero_cutoff=1e3)):
        x, _ = against_restatement(c, str(kw), **kw)
        seen.append((int(x['n_hbonds'].sum()), int(x['n_hydrophobic'].sum()), int((x['protein_role'] == IR.HYDROPHOBIC).sum())))
    base = (int(r['n_hbonds'].sum()), int(r['n_hydrophobic'].sum()), int((r['protein_role'] == IR.HYDROPHOBIC).sum()))
    assert seen[0][0] < base[0] < seen[1][0] and seen[1][1] < base[1] < seen[2][1] and seen[4][2] < base[2] < seen[3][2]
    assert seen[5][:2] == (0, 0) and seen[6][2] == 0                            # nothing is that close; every carbon has a neighbour


def test_include_masks_change_the_sums_over_molecules_only():
    c, r, _ = baseline()
    S, B = r['n_hbonds'].shape
    alternating = (np.arange(S * B).reshape(S, B) % 2).astype(bool)
    per_molecule = tuple(k for k in IR.KEYS if k not in IR.SUM_KEYS)
    for name, mask in (('all', np.ones((S, B), bool)), ('none', np.zeros((S, B), bool)), ('alternating', alternating)):
        m, _ = against_restatement(c, name, include=mask)
        same(m, r, f'{name}: the per-molecule outputs do not depend on the mask', per_molecule)
    same(run(c, include=np.ones((S, B), bool)), r, 'all = None', IR.SUM_KEYS)
    none = run(c, include=np.zeros((S, B), bool))
    assert not none['kind_hist'].any() and not none['pocket_freq'].any()
    assert 0 < run(c, include=alternating)['kind_hist'].sum() < r['kind_hist'].sum() == (r['n_donated'] + r['n_accepted'] + r['n_hydrophobic']).sum()


def test_null_optional_outputs_and_reference_bits_change_nothing_else():
    c, r, _ = baseline()
    assert r['n_ref_common'] is None
    ref = ref_words(np.random.default_rng(3), 300)
    full, _ = against_restatement(c, 'reference words', ref_bits=ref)
    same(full, r, 'reference words', tuple(k for k in IR.KEYS if k != 'n_ref_common'))
    for kw, gone in ((dict(atoms=False), IR.ATOM_KEYS), (dict(bits=False), ('bits',)), (dict(atoms=False, bits=False), IR.ATOM_KEYS + ('bits',))):
        x = run(c, ref_bits=ref, **kw)
        for k in gone:
            assert x[k] is None, k
        same(x, full, str(kw), tuple(k for k in IR.KEYS if k not in gone))
    bare = run(c, atoms=False, bits=False)
    same(bare, r, 'nothing optional', tuple(k for k in IR.KEYS if k not in IR.ATOM_KEYS + ('bits', 'n_ref_common')))
    # a molecule's own words: everything it hits is common; the bits agree with the map and show no atom past N_p
    s, g = 1, 4
    own = run(c, ref_bits=r['bits'][s, g])
    hit = PR.unpack_bits(r['bits'], 300)
    np.testing.assert_array_equal(own['n_ref_common'], (hit & hit[s, g]).sum(-1))
    assert own['n_ref_common'][s, g].sum() > 0
    np.testing.assert_array_equal(hit.sum(1), r['pocket_freq'])
    assert not (r['bits'][..., 4].view(np.uint64) >> np.uint64(300 - 256)).any()


def test_an_oversize_molecule_is_refused_by_the_binding_and_answered_with_minus_one_by_the_kernel():
    c = IR.build_case(5, 130, [20, 513, 33], S=2)
    with pytest.raises(ValueError, match='at most 512'):
        run(c, check=True)
    ref = np.stack([PR.pack_bits(np.ones(130, bool))] * 3)
    r, _ = against_restatement(c, 'oversize', include=np.ones((2, 3), bool), ref_bits=ref)
    for k in IR.MOL_KEYS + ('n_ref_common',):
        assert (r[k][:, 1] == -1).all() and (r[k][:, [0, 2]] >= 0).all(), k
    assert not r['bits'][:, 1].any() and not any(r[k][:, 20:533].any() for k in IR.ATOM_KEYS)
    alone = dict(c, pos=np.concatenate([c['pos'][:, :20], c['pos'][:, 533:]], 1), v=np.concatenate([c['v'][:, :20], c['v'][:, 533:]], 1),
                 ptr=np.asarray([0, 20, 53], np.int32))
    a = run(alone)
    for k in IR.MOL_KEYS + ('bits',):
        np.testing.assert_array_equal(a[k], r[k][:, [0, 2]], err_msg=k)
    same(a, r, 'the oversize molecule adds nothing', IR.SUM_KEYS + ('protein_role',))


def test_empty_packs_and_two_calls_give_identical_bytes():
    for S, sizes in ((0, [4, 9]), (2, [])):
        e = IR.build_case(1, 70, sizes, S=S)
        r, w = against_restatement(e, f'S = {S}, B = {len(sizes)}', include=np.ones((S, len(sizes)), bool), ref_bits=ref_words(np.random.default_rng(0), 70))
        assert r['n_hbonds'].shape == (S, len(sizes)) and not r['pocket_freq'].any() and (w['protein_role'] == IR.HYDROPHOBIC).any()
    against_restatement(IR.build_case(1, 70, [4, 9], S=2), 'six kinds', n_kinds=6)     # kinds 6 .. 39 of the case now take no part
    c, r, _ = baseline()
    again = run(c)
    for k in IR.KEYS:
        assert (again[k] is None and r[k] is None) or again[k].tobytes() == r[k].tobytes(), k


def docked():
    p, l = load_golden('pocket_1h36.npz'), load_golden('ligand_1h36_docked.npz')
    cls = {'H': 0, 'C': 1, 'N': 3, 'O': 5, 'F': 7, 'P': 8, 'S': 10, 'Cl': 12, 'Br': 12}      # Br is outside the table: taken as Cl
    return p, l['pos'].astype(np.float32), np.asarray([cls[str(e)] for e in l['elements']], np.int64)


def test_the_1h36_pocket_and_its_docked_ligand():
    dev = _dev()
    p, lpos, lv = docked()
    elem, kind, names = quality.pocket_kinds(p['feat'])
    role = quality.pocket_roles(p['feat'])
    np.testing.assert_array_equal(role, IR.pocket_roles(p['feat']))
    c = dict(pos=lpos[None], v=lv[None], ptr=np.asarray([0, 25], np.int32), ppos=p['pos'], pelem=elem, pkind=kind, prole=role)
    r, w = against_restatement(c, '1h36')
    assert r['protein_role'].shape == (572,) and ((r['protein_role'] & IR.HYDROPHOBIC) != 0).sum() == 186 and (elem == 1).sum() == 374
    assert w['n_hbonds'][0, 0] == 0 and w['n_hydrophobic'][0, 0] > 0 and r['n_hydrophobic'][0, 0] > 0
    wide, ww = against_restatement(c, '1h36, 4.5 A hydrogen bonds', hbond_cutoff=4.5)
    assert ww['n_hbonds'][0, 0] > 0 and wide['n_hydrophobic'][0, 0] == r['n_hydrophobic'][0, 0]
    # the stateless function gives the kernel's raw outputs on the same pocket
    x = quality.pocket_interactions(p['pos'], p['feat'], lpos, lv, ligand_ptr=torch.tensor([0, 25], dtype=torch.int32), return_bits=True, device=dev)
    same({k: (None if getattr(x, k) is None else getattr(x, k).cpu().numpy()) for k in IR.KEYS}, w, 'pocket_interactions')
    assert x.names == names


def test_sample_interactions_through_a_result_dictionary():
    dev = _dev()
    p, lpos, lv = docked()
    rng = np.random.default_rng(0)
    T = 3
    # three samples: the docked pose, a jittered copy, and a part of it moved 30 A away; three frames that end in those poses
    final = [lpos, (lpos + rng.normal(0, 0.5, lpos.shape)).astype(np.float32), lpos[:17] + np.float32(30)]
    pos_traj = [np.stack([(x + rng.normal(0, 0.3 * (T - 1 - t), x.shape)).astype(np.float32) for t in range(T)]).astype(np.float64) for x in final]
    v_traj = [np.stack([lv[:len(x)]] * T) for x in final]
    data = types.SimpleNamespace(protein_pos=torch.from_numpy(p['pos']), protein_atom_feature=torch.from_numpy(p['feat'].astype(np.int64)))
    result = {'data': data, 'pred_ligand_pos_traj': pos_traj, 'pred_ligand_v_traj': v_traj}
    elem, kind, names = quality.pocket_kinds(p['feat'])
    role = IR.pocket_roles(p['feat'])
    cut = dict(hbond_cutoff=4.5)                                                # so that the known ligand has hydrogen bonds to recover
    ref = IR.interaction_report(lpos[None], lv[None], [0, 25], CLASS_Z, p['pos'], elem, kind, role, 40, **cut)
    ref_sizes = PR.unpack_bits(ref['bits'][0, 0], 572).sum(-1)
    assert (ref_sizes[[0, 1]] > 0).any() and ref_sizes[2] > 0
    for eval_step, frames in ((-1, slice(T - 1, T)), ('all', slice(0, T))):
        pack = dict(pos=np.concatenate([x[frames] for x in pos_traj], 1).astype(np.float32), v=np.concatenate([x[frames] for x in v_traj], 1),
                    ptr=np.asarray([0, 25, 50, 67], np.int32), ppos=p['pos'], pelem=elem, pkind=kind, prole=role)
        w = want(pack, ref_bits=ref['bits'][0, 0], **cut)
        S = w['n_hbonds'].shape[0]
        expect = quality.InteractionReport.from_outputs(w, np.ones((S, 3), bool), [25, 25, 17], names, ref_sizes)
        got = quality.sample_interactions(result, eval_step, reference_ligand=(lpos, lv), device=dev, **cut)
        method = quality.SamplePack(result, eval_step, device=dev).interactions(data, reference_ligand=(lpos, lv), **cut)
        for rep in (got, method):
            assert vars(rep).keys() == vars(expect).keys()
            for k, x in vars(expect).items():
                if isinstance(x, np.ndarray):
                    np.testing.assert_array_equal(getattr(rep, k), x, err_msg=k)
            for s in range(S):
                np.testing.assert_equal(rep.summary(s), expect.summary(s))
        assert w['n_hydrophobic'][-1, 0] > 0 and w['n_hydrophobic'][-1, 2] == 0 and got.num_frames == S
        s = got.summary(-1)
        assert s['ref_hydrophobic_recovery_max'] == 1.0 and s['mean_hydrophobic'] > 0 and 0 < s['ref_hydrophobic_tanimoto'] < 1
