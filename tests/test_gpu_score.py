"""td_score_report on the GPU (csrc/score.hip) against tests/_score_ref.py (pinned to hand-computed cases on the host,
tests/test_score_host.py).  Every output is an integer.  protein_role, n_pairs, n_rot and the three piecewise-linear terms (repulsion,
hydrophobic, hbond) are compared with array_equal.  The two Gaussian terms may differ by what exp's last bit can flip in the rounding
to units of 2^-24: at most one unit per pair, so |kernel - restatement| <= n_pairs units per molecule -- a cap that follows from the
definition, not a measured tolerance.  A real defect shows as differences of the order of the sums.

  1. the grid of test_gpu_interactions.py: pockets of 0 .. 257 atoms around the 64-atom wave and the 256-atom workgroup stride, ragged
     molecules of 0 .. 512 atoms in packs of five, one and three frames, classes outside the table and protein atoms that take no part
     in every case, and a planted chain so that every case has a rotatable bond.  The restatement's own output must show every term.
  2. other cutoffs and radii, the rotor inputs absent and partial, the size bound, empty packs, repeatability.
  3. the 1h36 pocket and its docked ligand; quality.pocket_score, SamplePack.score and sample_score.
A Vina-style score on this project's heuristic typing, not AutoDock Vina's number.
"""
import types

import numpy as np
import pytest
import torch

import _bonds_ref as BR
import _interactions_ref as IR
import _score_ref as SR
from conftest import load_golden
from targetdiff_amd import capi, quality

pytestmark = pytest.mark.gpu

CLASS_Z = quality.class_atomic_numbers('add_aromatic')
AROMATIC = BR.CLASS_AROMATIC
PACKS = {'small-and-512': ([0, 512, 2, 63, 1], 3), 'around-64': ([64, 65, 1, 0, 2], 1)}
RSUM = SR.radius_sums()
SEEN = dict(molecules=0, differ=0, largest=0)                                   # the exp differences of the whole module, printed per test


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


def run(c, rotors=True, rsum=RSUM, check=False, **kw):
    """capi.score_report of a case's numpy arrays, as numpy; the rotor inputs from capi.bond_graph and capi.ring_report"""
    dev = _dev()
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    pack = (t(c['pos'], torch.float32), t(c['v'], torch.int64), t(c['ptr'], torch.int32), CLASS_Z)
    bond_ptr = bond_ring = None
    if rotors:
        bond_ptr = capi.bond_graph(*pack, AROMATIC, (), None, False, True, check=False)['bond_ptr']
        bond_ring = capi.ring_report(*pack, AROMATIC, None, bond_ptr, False, check=False)['bond_ring']
    out = capi.score_report(*pack, AROMATIC, t(c['ppos'], torch.float32), t(c['pelem'], torch.int32), t(c['pkind'], torch.int32),
                            t(c['prole'], torch.int32), 40, rsum, bond_ptr=bond_ptr, bond_ring=bond_ring, check=check, **kw)
    return {k: (None if x is None else x.cpu().numpy()) for k, x in out.items()}


def want(c, rotors=True, rsum=RSUM, detail=None, **kw):
    return SR.score_report(c['pos'], c['v'], c['ptr'], CLASS_Z, AROMATIC, c['ppos'], c['pelem'], c['pkind'], c['prole'], 40, rsum,
                           with_rotors=rotors, detail=detail, **kw)


def same(r, w, what):
    """the comparison of the module's docstring; prints the exp differences seen so far"""
    assert set(r) == set(SR.KEYS)
    for k in SR.KEYS:
        if w[k] is None:
            assert r[k] is None, f'{what}: {k}'
        else:
            assert r[k].dtype == w[k].dtype and r[k].shape == w[k].shape, f'{what}: {k}'
    for k in ('protein_role', 'n_pairs', 'n_rot'):
        if w[k] is not None:
            np.testing.assert_array_equal(r[k], w[k], err_msg=f'{what}: {k}')
    np.testing.assert_array_equal(r['terms'][..., 2:], w['terms'][..., 2:], err_msg=f'{what}: the piecewise-linear terms')
    ok = w['n_pairs'] >= 0
    np.testing.assert_array_equal(r['terms'][~ok], w['terms'][~ok], err_msg=f'{what}: oversize')
    diff = np.abs(r['terms'][..., :2][ok] - w['terms'][..., :2][ok])
    SEEN['molecules'] += int(ok.sum())
    SEEN['differ'] += int((diff > 0).any(-1).sum())
    SEEN['largest'] = max(SEEN['largest'], int(diff.max()) if diff.size else 0)
    print(f'{what}: largest exp difference {int(diff.max()) if diff.size else 0} units of 2^-24; so far {SEEN["differ"]} of '
          f'{SEEN["molecules"]} molecules differ at all, the largest by {SEEN["largest"]} units')
    assert (diff <= w['n_pairs'][ok][:, None]).all(), f'{what}: the Gaussian terms differ by more than one unit per pair'


def against_restatement(c, what, **kw):
    r, w = run(c, **kw), want(c, **{k: x for k, x in kw.items() if k != 'check'})
    same(r, w, what)
    return r, w


def plant_chain(c, g):
    """the first four atoms of molecule g become a butane-like carbon chain 100 A away from everything: one rotatable bond at least"""
    a = int(c['ptr'][g])
    assert int(c['ptr'][g + 1]) - a >= 4
    chain = np.asarray([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [2.2, 1.3, 0.0], [3.7, 1.3, 0.0]], np.float32) + np.float32(100.0)
    c['pos'][:, a:a + 4] = chain
    c['v'][:, a:a + 4] = 1


_CACHE = {}


def baseline():
    """one pack through the kernel and the restatement, once: shared by the tests that need a baseline, and left unchanged"""
    if 'base' not in _CACHE:
        c = IR.build_case(11, 300, [5, 70, 0, 31, 129], S=2)
        _CACHE['base'] = (c, run(c), want(c))
    return _CACHE['base']


@pytest.mark.parametrize('pack', list(PACKS))
@pytest.mark.parametrize('n_p', [0, 1, 63, 64, 65, 255, 256, 257])
def test_every_output_against_the_restatement(n_p, pack):
    sizes, S = PACKS[pack]
    c = IR.build_case(100 + n_p, n_p, sizes, S)
    c['v'][:, ::37] = -1                                                         # classes outside [0, 13)
    c['v'][:, 5::41] = 13
    plant_chain(c, 1)
    detail = []
    r, w = run(c), want(c, detail=detail)
    same(r, w, f'N_p = {n_p}, {pack}')
    assert r['terms'].shape == (S, 5, 5) and r['n_pairs'].shape == (S, 5) and r['n_rot'].shape == (S, 5) and r['protein_role'].shape == (n_p,)
    assert (w['n_rot'][:, 1] > 0).all()                                          # the planted chain
    if n_p == 0:
        assert not r['terms'].any() and not r['n_pairs'].any()
    if n_p >= 63:                                                               # no case passes vacuously
        assert (w['terms'] > 0).any((0, 1)).all(), 'every one of the five terms is non-zero somewhere'
        d, hy = np.concatenate([x[2] for x in detail]), np.concatenate([x[3] for x in detail])
        assert (d < -0.7).any() and (hy & (d > 0.5) & (d < 1.5)).any()
        assert (c['prole'] == -1).any() and ((c['pelem'] < 0) | (c['pkind'] < 0)).any()      # protein atoms that take no part


def test_other_cutoffs_and_a_custom_radius_table():
    c, r, w = baseline()
    same(r, w, 'defaults')
    near, _ = against_restatement(c, 'cutoff 4', cutoff=4.0)
    far, _ = against_restatement(c, 'cutoff 12', cutoff=12.0)
    assert (near['n_pairs'] <= r['n_pairs']).all() and (r['n_pairs'] <= far['n_pairs']).all()
    assert near['n_pairs'].sum() < r['n_pairs'].sum() < far['n_pairs'].sum()
    # a piecewise-linear term is zero from d = 1.5 on, r < 5.6 with these radii: 12 A adds nothing to them, 4 A cuts some
    np.testing.assert_array_equal(far['terms'][..., 2:], r['terms'][..., 2:])
    assert (near['terms'][..., 2:] <= r['terms'][..., 2:]).all() and near['terms'][..., 3].sum() < r['terms'][..., 3].sum()
    rsum = SR.radius_sums((0.0, 1.0, 2.5, 1.2, 3.0, 0.7, 1.1, 2.9), (0.0, 2.2, 0.6, 3.0, 1.4, 2.6))
    other, _ = against_restatement(c, 'custom radii', rsum=rsum)
    np.testing.assert_array_equal(other['n_pairs'], r['n_pairs'])
    assert (other['terms'] != r['terms']).any()
    against_restatement(c, 'hetero cutoff 2.5', hetero_cutoff=2.5)
    bad = RSUM.copy()
    bad[3, 2] = 6.5
    with pytest.raises(ValueError, match='rsum'):
        run(c, rsum=bad)
    with pytest.raises(ValueError, match='rsum'):
        run(c, rsum=np.where(RSUM == RSUM[1, 1], np.nan, RSUM))


def test_without_the_bond_arguments_there_are_no_rotors_and_nothing_else_changes():
    c, r, _ = baseline()
    bare, _ = against_restatement(c, 'no rotor inputs', rotors=False)
    assert bare['n_rot'] is None and r['n_rot'] is not None and r['n_rot'].sum() > 0
    for k in ('protein_role', 'terms', 'n_pairs'):
        assert bare[k].tobytes() == r[k].tobytes(), k
    dev = _dev()
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    pack = (t(c['pos'], torch.float32), t(c['v'], torch.int64), t(c['ptr'], torch.int32), CLASS_Z)
    pocket = (t(c['ppos'], torch.float32), t(c['pelem'], torch.int32), t(c['pkind'], torch.int32), t(c['prole'], torch.int32), 40, RSUM)
    bond_ptr = capi.bond_graph(*pack, AROMATIC, (), None, False, True)['bond_ptr']
    bond_ring = capi.ring_report(*pack, AROMATIC, None, bond_ptr, False)['bond_ring']
    for kw in (dict(bond_ptr=bond_ptr), dict(bond_ring=bond_ring)):
        with pytest.raises(ValueError, match='come together'):
            capi.score_report(*pack, AROMATIC, *pocket, **kw)
    with pytest.raises(ValueError, match='bond_ptr'):
        capi.score_report(*pack, AROMATIC, *pocket, bond_ptr=bond_ptr[:-1].contiguous(), bond_ring=bond_ring)
    # the entry point itself refuses a part of the rotor inputs
    lib = capi.load_library()
    S, Nl, B = c['pos'].shape[0], c['pos'].shape[1], len(c['ptr']) - 1
    cz = np.asarray(CLASS_Z, np.int32)
    out = (torch.empty(300, dtype=torch.int32, device=dev), torch.empty(S, B, 5, dtype=torch.int64, device=dev),
           torch.empty(S, B, dtype=torch.int32, device=dev), torch.empty(S, B, dtype=torch.int32, device=dev))
    for ptr_arg, nb, ring_arg in ((None, 0, bond_ring), (None, 3, None), (bond_ptr, int(bond_ring.numel()), None)):
        rc = lib.td_score_report(*capi._pack_args(*pack[:3], S, Nl, B, cz), None, *(capi._ptr(x) for x in pocket[:4]), 300, 40, 8.0, 1.75,
                                 np.ascontiguousarray(RSUM.reshape(-1)).ctypes.data_as(capi.POINTER(capi.ctypes.c_double)),
                                 capi._ptr(ptr_arg), nb, capi._ptr(ring_arg), *(capi._ptr(x) for x in out), capi._stream(dev))
        assert rc == -1 and b'together' in lib.td_last_error()               # TD_EINVAL


def test_an_oversize_molecule_is_refused_by_the_binding_and_answered_by_the_kernel():
    c = IR.build_case(5, 130, [20, 513, 33], S=2)
    with pytest.raises(ValueError, match='at most 512'):
        run(c, check=True)
    r, _ = against_restatement(c, 'oversize')
    assert (r['n_pairs'][:, 1] == -1).all() and (r['n_rot'][:, 1] == -1).all() and (r['terms'][:, 1] == SR.INT64_MIN).all()
    assert (r['n_pairs'][:, [0, 2]] > 0).all() and (r['n_rot'][:, [0, 2]] >= 0).all() and (r['terms'][:, [0, 2]] >= 0).all()
    alone = dict(c, pos=np.concatenate([c['pos'][:, :20], c['pos'][:, 533:]], 1), v=np.concatenate([c['v'][:, :20], c['v'][:, 533:]], 1),
                 ptr=np.asarray([0, 20, 53], np.int32))
    a = run(alone)
    for k in ('terms', 'n_pairs', 'n_rot'):
        np.testing.assert_array_equal(a[k], r[k][:, [0, 2]], err_msg=k)
    np.testing.assert_array_equal(a['protein_role'], r['protein_role'])


def test_empty_packs_an_empty_pocket_and_two_calls_give_identical_bytes():
    for S, sizes in ((0, [4, 9]), (2, [])):
        e = IR.build_case(1, 70, sizes, S=S)
        r, w = against_restatement(e, f'S = {S}, B = {len(sizes)}')
        assert r['terms'].shape == (S, len(sizes), 5) and r['n_rot'].shape == (S, len(sizes)) and (w['protein_role'] == IR.HYDROPHOBIC).any()
    e = IR.build_case(1, 0, [4, 9], S=2)
    r, _ = against_restatement(e, 'N_p = 0')
    assert not r['terms'].any() and not r['n_pairs'].any() and r['protein_role'].shape == (0,)
    c, r, _ = baseline()
    again = run(c)
    for k in SR.KEYS:
        assert again[k].tobytes() == r[k].tobytes(), k


def docked():
    p, l = load_golden('pocket_1h36.npz'), load_golden('ligand_1h36_docked.npz')
    cls = {'H': 0, 'C': 1, 'N': 3, 'O': 5, 'F': 7, 'P': 8, 'S': 10, 'Cl': 12, 'Br': 12}      # Br is outside the table: taken as Cl
    return p, l['pos'].astype(np.float32), np.asarray([cls[str(e)] for e in l['elements']], np.int64)


def shifted_pack(lpos, lv):
    """{docked, shifted by 1.5 A, shifted by 4 A, far} as one frame of four molecules"""
    poses = [lpos, lpos + np.asarray([1.5, 0, 0], np.float32), lpos + np.asarray([4, 0, 0], np.float32), lpos + np.float32(30)]
    return np.concatenate(poses)[None].astype(np.float32), np.concatenate([lv] * 4)[None], np.arange(5, dtype=np.int32) * len(lv)


def test_the_1h36_pocket_and_its_docked_ligand():
    dev = _dev()
    p, lpos, lv = docked()
    elem, kind, names = quality.pocket_kinds(p['feat'])
    role = IR.pocket_roles(p['feat'])
    pos, v, ptr = shifted_pack(lpos, lv)
    c = dict(pos=pos, v=v, ptr=ptr, ppos=p['pos'], pelem=elem, pkind=kind, prole=role)
    r, w = against_restatement(c, '1h36')
    np.testing.assert_array_equal(r['n_pairs'][0], [2045, 2006, w['n_pairs'][0, 2], 0])
    terms, inter, score = quality.score_energies(r['terms'], r['n_rot'])
    np.testing.assert_allclose(terms[0, 0], [89.64, 1588.51, 0.405, 103.95, 0.0], atol=0.006)
    np.testing.assert_allclose(inter[0, :3], [-14.68, 7.38, 206.8], atol=0.06)
    assert inter[0, 0] < 0 < inter[0, 1] < inter[0, 2] and not r['terms'][0, 3].any() and inter[0, 3] == 0
    assert r['n_rot'][0, 0] > 0 and inter[0, 0] < score[0, 0] < 0
    # the stateless function gives the kernel's outputs on the same pocket, and the restatement's energies
    x = quality.pocket_score(p['pos'], p['feat'], pos, v, ligand_ptr=torch.from_numpy(ptr), device=dev)
    for k, a in (('raw_terms', r['terms']), ('n_pairs', r['n_pairs']), ('n_rot', r['n_rot'])):
        np.testing.assert_array_equal(getattr(x, k), a, err_msg=k)
    np.testing.assert_array_equal(x.protein_role.cpu().numpy(), w['protein_role'])
    wt, wi, ws = SR.energies(w['terms'], w['n_rot'])
    np.testing.assert_array_equal(x.terms[..., 2:], wt[..., 2:])
    np.testing.assert_array_equal(x.heavy_atoms[0], [int((lv != 0).sum())] * 4)
    for got, exp in ((x.terms, wt), (x.inter, wi), (x.score, ws), (x.efficiency, ws / x.heavy_atoms)):
        np.testing.assert_allclose(got, exp, rtol=1e-6, atol=0)
    bare = quality.pocket_score(p['pos'], p['feat'], pos, v, ligand_ptr=torch.from_numpy(ptr), rotors=False, device=dev)
    assert bare.n_rot is None
    np.testing.assert_array_equal(bare.score, bare.inter)
    np.testing.assert_array_equal(bare.inter, x.inter)


EXACT = ('n_included', 'sum_rotors', 'sum_pairs', 'n_no_pairs', 'n_efficiency', 'scored', 'n_samples', 'n_ref')


def test_sample_score_through_a_result_dictionary():
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
    pocket = (p['pos'], elem, kind, role, 40, RSUM)
    ref = SR.score_report(lpos[None], lv[None], [0, 25], CLASS_Z, AROMATIC, *pocket)
    ref_score = float(SR.energies(ref['terms'], ref['n_rot'])[2][0, 0])
    assert ref_score < 0
    for eval_step, frames in ((-1, slice(T - 1, T)), ('all', slice(0, T))):
        pos = np.concatenate([x[frames] for x in pos_traj], 1).astype(np.float32)
        v = np.concatenate([x[frames] for x in v_traj], 1)
        w = SR.score_report(pos, v, np.asarray([0, 25, 50, 67], np.int32), CLASS_Z, AROMATIC, *pocket)
        S = w['n_pairs'].shape[0]
        heavy = np.stack([[int((x[s] != 0).sum()) for x in (vt[frames] for vt in v_traj)] for s in range(S)])
        expect = quality.ScoreReport.from_outputs(w, np.ones((S, 3), bool), heavy, ref_score=ref_score)
        got = quality.sample_score(result, eval_step, reference_ligand=(lpos, lv), device=dev)
        method = quality.SamplePack(result, eval_step, device=dev).score(data, reference_ligand=(lpos, lv))
        for rep in (got, method):
            assert vars(rep).keys() == vars(expect).keys()
            for k, x in vars(expect).items():
                if k in EXACT:
                    np.testing.assert_array_equal(getattr(rep, k), x, err_msg=k)
                else:
                    np.testing.assert_allclose(getattr(rep, k), x, rtol=1e-6, atol=0, err_msg=k)
            for s in range(S):
                a, b = rep.summary(s), expect.summary(s)
                assert a.keys() == b.keys()
                for k in b:
                    np.testing.assert_allclose(a[k], b[k], rtol=1e-6, atol=0, err_msg=k)
        s = got.summary(-1)
        assert got.num_frames == S and w['n_pairs'][-1, 0] == 2045 and w['n_pairs'][-1, 2] == 0
        assert s['no_pairs'] == 1 / 3 and s['better_than_ref'] <= 1 / 3 and s['best_score'] <= s['median_score'] and s['mean_rotors'] > 0
        np.testing.assert_allclose(s['ref_score'], ref_score, rtol=1e-6)
