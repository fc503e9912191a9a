"""td_score_minimize on the GPU (csrc/relax.hip) against tests/_relax_ref.py (pinned on the host, tests/test_relax_host.py).  A local
optimisation under this project's heuristic score, not AutoDock Vina's minimize; rigid-body only: three translations and three
rotations, no torsions.

An evaluation is compared exactly: the term sums with capi.score_report's for the same coordinates (array_equal: the same arithmetic),
the three piecewise-linear terms with the restatement's (array_equal), the two Gaussians and the six gradient components within one
unit of 2^-24 per counted pair (only exp differs, and its last bit can flip one rounding).  The trajectory of the optimiser is NOT
compared with the restatement's: the 6 x 6 algebra is not specified to the bit.  What every run must satisfy instead follows from the
contract: the energy does not rise, the written terms are the score of the written coordinates under the input pose's roles, the
motion is rigid up to the fp32 rounding of the pose (each coordinate within half an ulp32, so a distance within sqrt(3) ulp32 of the
rotated one; the bound asserted is twice that), the centre stays within max_shift, the counts respect their budgets, the status is
consistent with the counts, and the transform reproduces the coordinates bit for bit.

  1. max_steps = 0 on the grids of test_gpu_score.py;  2. the defaults on the same grids;  3. the LDS list against the walk in global
  memory;  4. the size bound, empty packs, an empty pocket, repeatability;  5. the 1h36 fixture and the planted minimum;  6. quality.
"""
import types

import numpy as np
import pytest
import torch

import _bonds_ref as BR
import _interactions_ref as IR
import _relax_ref as RR
import _score_ref as SR
from conftest import load_golden
from targetdiff_amd import capi, quality

pytestmark = pytest.mark.gpu

CLASS_Z = quality.class_atomic_numbers('add_aromatic')
AROMATIC = BR.CLASS_AROMATIC
PACKS = {'small-and-512': ([0, 512, 2, 63, 1], 3), 'around-64': ([64, 65, 1, 0, 2], 1)}
N_P = [0, 1, 64, 65, 256, 257]
RSUM = SR.radius_sums()
W = SR.WEIGHTS
INT_KEYS = ('terms_in', 'terms', 'n_pairs', 'n_steps', 'n_evals', 'status', 'grad_in')


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


def tensors(c):
    dev = _dev()
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    pack = (t(c['pos'], torch.float32), t(c['v'], torch.int64), t(c['ptr'], torch.int32), CLASS_Z, AROMATIC)
    pocket = (t(c['ppos'], torch.float32), t(c['pelem'], torch.int32), t(c['pkind'], torch.int32), t(c['prole'], torch.int32), 40, RSUM)
    return pack, pocket


def run(c, check=False, **kw):
    """capi.score_minimize of a case's numpy arrays, as numpy (no rotor inputs: n_rot is None)"""
    pack, pocket = tensors(c)
    out = capi.score_minimize(*pack, *pocket, W, check=check, **kw)
    return {k: (None if x is None else x.cpu().numpy()) for k, x in out.items()}


def score(c, pos=None):
    """capi.score_report's terms and n_pairs for the case's pack, or for other coordinates of it"""
    pack, pocket = tensors(c if pos is None else dict(c, pos=pos))
    out = capi.score_report(*pack, *pocket, check=False)
    return out['terms'].cpu().numpy(), out['n_pairs'].cpu().numpy()


_CASES = {}


def grid_case(n_p, pack):
    """One case of the grid with what the restatement needs of it, computed once and left unchanged: the resolved protein roles and per
    (frame, molecule) the element indices and the roles of the input pose"""
    if (n_p, pack) not in _CASES:
        sizes, S = PACKS[pack]
        c = IR.build_case(100 + n_p, n_p, sizes, S)
        c['v'][:, ::37] = -1                                                     # classes outside [0, 13)
        c['v'][:, 5::41] = 13
        pr = IR.protein_roles(c['ppos'], c['pelem'], c['pkind'], c['prole'], 40)
        mols = {}
        for s in range(S):
            for g in range(len(sizes)):
                a, b = int(c['ptr'][g]), int(c['ptr'][g + 1])
                mols[s, g] = (a, b) + RR.molecule_inputs(c['pos'][s, a:b], c['v'][s, a:b], CLASS_Z)
        _CASES[n_p, pack] = (c, pr, mols)
    return _CASES[n_p, pack]


def evaluated(c, pr, mol, x, centre=np.zeros(3)):
    """the restatement's evaluation of the coordinates x of one molecule under the roles of its input pose"""
    a, b, lel, lrole, _ = mol
    return RR.evaluate(np.ascontiguousarray(x), lel, lrole, centre, c['ppos'], c['pelem'], pr, RSUM, 8.0, W)


def check_terms(got, want, pairs, what):
    np.testing.assert_array_equal(got[2:], want[2:], err_msg=f'{what}: the piecewise-linear terms')
    assert (np.abs(got[:2] - want[:2]) <= pairs).all(), f'{what}: the Gaussian terms differ by more than one unit per pair'


def ulp32(*arrays):
    return float(np.spacing(np.float32(max([float(np.abs(x).max()) for x in arrays if x.size] + [1e-30]))))


@pytest.mark.parametrize('pack', list(PACKS))
@pytest.mark.parametrize('n_p', N_P)
def test_zero_steps_is_one_evaluation_of_the_input_pose(n_p, pack):
    c, pr, mols = grid_case(n_p, pack)
    r = run(c, max_steps=0)
    terms, n_pairs = score(c)
    np.testing.assert_array_equal(r['terms_in'], terms)
    np.testing.assert_array_equal(r['terms'], terms)
    np.testing.assert_array_equal(r['n_pairs'], n_pairs)
    assert r['pos'].tobytes() == c['pos'].tobytes()
    np.testing.assert_array_equal(r['protein_role'], pr)
    assert not r['n_steps'].any() and (r['n_evals'] == 1).all() and (r['status'] == RR.OUT_OF_BUDGET).all() and r['n_rot'] is None
    np.testing.assert_array_equal(r['transform'], np.broadcast_to([1.0, 0, 0, 0, 0, 0, 0], r['transform'].shape))
    worst = 0
    for (s, g), mol in mols.items():
        a, b, lel, lrole, scored = mol
        x = c['pos'][s, a:b]
        w_terms, w_grad, w_pairs = evaluated(c, pr, mol, x, RR.centroid(x, scored))
        assert w_pairs == n_pairs[s, g]
        check_terms(r['terms_in'][s, g], w_terms, w_pairs, f'molecule {s, g}')
        diff = np.abs(r['grad_in'][s, g] - w_grad)
        worst = max(worst, int(diff.max()))
        assert (diff <= w_pairs).all(), f'molecule {s, g}: gradient {r["grad_in"][s, g]} against {w_grad}, {w_pairs} pairs'
    print(f'N_p = {n_p}, {pack}: largest gradient difference {worst} units of 2^-24')
    if n_p >= 64:
        assert np.abs(r['grad_in']).sum(-1).min(initial=1, where=n_pairs > 0) > 0 and (n_pairs > 0).any()


def check_run(c, pr, mols, r, max_steps, max_evals, max_shift, what):
    """what every run must satisfy (the module's docstring)"""
    for (s, g), mol in mols.items():
        a, b, lel, lrole, scored = mol
        x, y = c['pos'][s, a:b], r['pos'][s, a:b]
        tag = f'{what}, molecule {s, g}'
        steps, evals, status = int(r['n_steps'][s, g]), int(r['n_evals'][s, g]), int(r['status'][s, g])
        assert RR.energy(r['terms'][s, g], W) <= RR.energy(r['terms_in'][s, g], W), tag
        w_terms, _, w_pairs = evaluated(c, pr, mol, y)
        assert w_pairs == r['n_pairs'][s, g], tag
        check_terms(r['terms'][s, g], w_terms, w_pairs, tag)
        u = ulp32(x, y)
        if b - a > 1:
            dist = lambda z: np.sqrt(((z.astype(np.float64)[:, None] - z.astype(np.float64)[None]) ** 2).sum(-1))
            assert np.abs(dist(x) - dist(y)).max() <= 2.0 * np.sqrt(3.0) * u, tag
        t = r['transform'][s, g]
        assert abs(float((t[:4] ** 2).sum()) - 1.0) < 1e-12 and np.sqrt((t[4:] ** 2).sum()) <= max_shift, tag
        if scored.any():
            shift = y.astype(np.float64)[scored].mean(0) - x.astype(np.float64)[scored].mean(0)
            assert np.sqrt((shift ** 2).sum()) <= max_shift + 2.0 * np.sqrt(3.0) * u, tag
        assert 0 <= steps <= max_steps and 1 <= evals <= max_evals and steps < evals, tag
        assert status & 3 in (RR.CONVERGED, RR.OUT_OF_BUDGET) and not status & ~7, tag
        if status & RR.OUT_OF_BUDGET:
            assert steps == max_steps or evals == max_evals, tag
        else:
            assert steps < max_steps, tag
        if steps == 0:
            assert y.tobytes() == x.tobytes() and (r['terms'][s, g] == r['terms_in'][s, g]).all(), tag
            np.testing.assert_array_equal(t, [1.0, 0, 0, 0, 0, 0, 0], err_msg=tag)
        else:
            np.testing.assert_array_equal(y, RR.transformed(x, scored, t), err_msg=tag)


@pytest.mark.parametrize('pack', list(PACKS))
@pytest.mark.parametrize('n_p', N_P)
def test_the_defaults_on_the_grid(n_p, pack):
    c, pr, mols = grid_case(n_p, pack)
    r = run(c)
    np.testing.assert_array_equal(r['terms_in'], score(c)[0])
    check_run(c, pr, mols, r, 64, 257, 3.0, f'N_p = {n_p}, {pack}')
    if n_p >= 64:
        assert (r['n_steps'] > 0).any() and (r['terms'] != r['terms_in']).any(), 'no case passes vacuously'
    print(f'N_p = {n_p}, {pack}: steps {r["n_steps"].tolist()}, evaluations {r["n_evals"].tolist()}, status {r["status"].tolist()}')


def test_more_candidates_than_the_list_holds_walk_the_pocket_in_global_memory():
    dev = _dev()
    c = IR.build_case(7, 4800, [6], S=1, dead=False)
    pack, pocket = tensors(c)
    kw = dict(max_steps=4, max_shift=20.0)
    out = capi.score_minimize(*pack, *pocket, W, check=False, **kw)
    r = {k: (None if x is None else x.cpu().numpy()) for k, x in out.items()}
    # the resolved protein roles are the kernel's own here (compared bit for bit with the restatement's in test_gpu_interactions.py and
    # above): the restatement's all-pairs distances of 4800 atoms would take a gigabyte
    pr = r['protein_role']
    lel, lrole, scored = RR.molecule_inputs(c['pos'][0], c['v'][0], CLASS_Z)
    x = c['pos'][0]
    c0 = RR.centroid(x, scored)
    reach = np.sqrt(((x.astype(np.float64)[scored] - c0) ** 2).sum(1).max()) + 8.0 + 20.0
    candidates = int(((pr >= 0) & (c['pelem'] != 0) & (np.sqrt(((c['ppos'].astype(np.float64) - c0) ** 2).sum(1)) <= reach)).sum())
    assert candidates > capi.RELAX_LIST_CAPACITY, candidates
    mols = {(0, 0): (0, 6, lel, lrole, scored)}
    check_run(c, pr, mols, r, 4, 17, 20.0, 'beyond the list')
    w = RR.relax_molecule(x, lel, lrole, c['ppos'], c['pelem'], pr, RSUM, W, max_steps=4, max_shift=20.0)
    terms_in, pairs_in = (z[0, 0] for z in score(c))
    np.testing.assert_array_equal(r['terms_in'][0, 0], terms_in)
    check_terms(r['terms_in'][0, 0], w['terms_in'], pairs_in, 'beyond the list, input')
    assert (np.abs(r['grad_in'][0, 0] - w['grad_in']) <= pairs_in).all() and r['n_steps'][0, 0] > 0
    print(f'{candidates} candidates: kernel {r["n_steps"][0, 0]} steps to {RR.energy(r["terms"][0, 0], W):.6f}, restatement '
          f'{w["n_steps"]} steps to {RR.energy(w["terms"], W):.6f}')


def test_the_list_and_the_walk_in_global_memory_give_identical_bytes():
    c = IR.build_case(11, 300, [5, 70, 0, 31, 129], S=2)
    listed = run(c)
    assert (listed['n_steps'] > 0).any()
    for capacity in (0, 64):                                                    # no molecule listed; only those with few candidates
        walked = run(c, _list_capacity=capacity)
        for k in RR.KEYS:
            if listed[k] is not None:
                assert walked[k].tobytes() == listed[k].tobytes(), (capacity, k)


def test_an_oversize_molecule_keeps_its_positions_and_is_refused_by_the_binding():
    c = IR.build_case(5, 130, [20, 513, 33], S=2)
    with pytest.raises(ValueError, match='at most 512'):
        run(c, check=True)
    r = run(c, max_steps=8)
    assert (r['n_pairs'][:, 1] == -1).all() and (r['status'][:, 1] == -1).all() and not r['n_steps'][:, 1].any() and not r['n_evals'][:, 1].any()
    assert (r['terms'][:, 1] == SR.INT64_MIN).all() and (r['terms_in'][:, 1] == SR.INT64_MIN).all() and not r['grad_in'][:, 1].any()
    assert r['pos'][:, 20:533].tobytes() == c['pos'][:, 20:533].tobytes()
    alone = dict(c, pos=np.concatenate([c['pos'][:, :20], c['pos'][:, 533:]], 1), v=np.concatenate([c['v'][:, :20], c['v'][:, 533:]], 1),
                 ptr=np.asarray([0, 20, 53], np.int32))
    a = run(alone, max_steps=8)
    assert (a['n_steps'] > 0).any()
    for k in INT_KEYS + ('transform',):
        np.testing.assert_array_equal(a[k], r[k][:, [0, 2]], err_msg=k)
    np.testing.assert_array_equal(a['pos'], np.concatenate([r['pos'][:, :20], r['pos'][:, 533:]], 1))


def test_empty_packs_an_empty_pocket_and_two_calls_give_identical_bytes():
    for S, sizes in ((0, [4, 9]), (2, [])):
        e = IR.build_case(1, 70, sizes, S=S)
        r = run(e)
        assert r['terms'].shape == (S, len(sizes), 5) and r['transform'].shape == (S, len(sizes), 7) and r['pos'].tobytes() == e['pos'].tobytes()
    e = IR.build_case(1, 0, [4, 9], S=2)
    r = run(e)
    assert not r['terms'].any() and not r['n_pairs'].any() and not r['n_steps'].any() and (r['n_evals'] == 1).all()
    assert (r['status'] == RR.CONVERGED).all() and r['pos'].tobytes() == e['pos'].tobytes()
    c = IR.build_case(11, 300, [5, 70, 0, 31, 129], S=2)
    c['v'][:, :5] = 0                                                            # a molecule of hydrogens: no scored atom
    first, again = run(c), run(c)
    for k in RR.KEYS:
        if first[k] is not None:
            assert again[k].tobytes() == first[k].tobytes(), k
    assert not first['n_steps'][:, 0].any() and first['pos'][:, :5].tobytes() == c['pos'][:, :5].tobytes() and (first['n_steps'] > 0).any()
    pack, pocket = tensors(c)
    for kw, match in ((dict(max_shift=0.0), 'max_shift'), (dict(max_shift=float('nan')), 'max_shift'), (dict(max_steps=-1), 'max_steps'),
                      (dict(max_evals=0), 'max_evals')):
        with pytest.raises(ValueError, match=match):
            capi.score_minimize(*pack, *pocket, W, **kw)
    with pytest.raises(ValueError, match='weights'):
        capi.score_minimize(*pack, *pocket, W[:4])


def docked():
    p, l = load_golden('pocket_1h36.npz'), load_golden('ligand_1h36_docked.npz')
    cls = {'H': 0, 'C': 1, 'N': 3, 'O': 5, 'F': 7, 'P': 8, 'S': 10, 'Cl': 12, 'Br': 12}      # Br is outside the table: taken as Cl
    return p, l['pos'].astype(np.float32), np.asarray([cls[str(e)] for e in l['elements']], np.int64)


def fixture_case(poses, lv):
    p = load_golden('pocket_1h36.npz')
    elem, kind, _ = quality.pocket_kinds(p['feat'])
    n = len(lv)
    return dict(pos=np.concatenate(poses)[None].astype(np.float32), v=np.concatenate([lv] * len(poses))[None],
                ptr=np.arange(len(poses) + 1, dtype=np.int32) * n, ppos=p['pos'], pelem=elem, pkind=kind, prole=IR.pocket_roles(p['feat']))


def rmsd(x, y):
    return float(np.sqrt(((np.asarray(x, np.float64) - np.asarray(y, np.float64)) ** 2).sum(-1).mean()))


def test_the_1h36_pocket_and_its_docked_ligand():
    _, lpos, lv = docked()
    poses = [lpos, lpos + np.asarray([1.5, 0, 0], np.float32), lpos + np.asarray([4, 0, 0], np.float32), lpos + np.float32(30)]
    c = fixture_case(poses, lv)
    pr = IR.protein_roles(c['ppos'], c['pelem'], c['pkind'], c['prole'], 40)
    n = len(lv)
    mols = {(0, g): (g * n, (g + 1) * n) + RR.molecule_inputs(poses[g], lv, CLASS_Z) for g in range(4)}
    r = run(c)
    check_run(c, pr, mols, r, 64, 257, 3.0, '1h36')
    e_in = [RR.energy(t, W) for t in r['terms_in'][0]]
    e_out = [RR.energy(t, W) for t in r['terms'][0]]
    moved = [rmsd(r['pos'][0, g * n:(g + 1) * n], poses[g]) for g in range(4)]
    print(f'1h36: {e_in} -> {e_out}, moved {moved}, steps {r["n_steps"][0].tolist()}, evaluations {r["n_evals"][0].tolist()}, '
          f'status {r["status"][0].tolist()}')
    np.testing.assert_allclose(e_in[:3], [-14.68, 7.38, 206.8], atol=0.06)
    # the figures the restatement gives (tests/test_relax_host.py pins them): the same minimum, whichever way the last bits fall
    np.testing.assert_allclose(e_out[:2], [-14.747, -14.737], atol=0.03)
    assert 0.04 < moved[0] < 0.2 and abs(moved[1] - 1.53) < 0.1
    assert r['status'][0, 2] & RR.AT_CAP and np.sqrt((r['transform'][0, 2, 4:] ** 2).sum()) <= 3.0 and e_out[2] < e_in[2]
    assert r['n_steps'][0, 3] == 0 and r['n_evals'][0, 3] == 1 and r['status'][0, 3] == RR.CONVERGED and e_out[3] == 0.0


def test_a_planted_minimum_is_found_again():
    """The docked pose relaxed with 200 steps is x* with E*.  Eight copies, each moved by 0.3 A and turned by 5 degrees about random axes,
    relaxed with the defaults: each recovers at least 90 % of E0 - E* and ends with an RMSD to x* of at most a quarter of its starting
    RMSD.  Conditions, not measurements: a translation-only optimiser recovers 35 - 77 % and stays where it started (the host test)."""
    _, lpos, lv = docked()
    n = len(lv)
    star = run(fixture_case([lpos], lv), max_steps=200)
    x_star, e_star = star['pos'][0], RR.energy(star['terms'][0, 0], W)
    rng = np.random.default_rng(2024)
    centre = x_star.astype(np.float64)[lv != 0].mean(0)
    poses = []
    for _ in range(8):
        axis, way = rng.normal(size=3), rng.normal(size=3)
        axis, way = axis / np.linalg.norm(axis), way / np.linalg.norm(way)
        half = np.radians(5.0) / 2.0
        R = RR.rotation(np.concatenate([[np.cos(half)], np.sin(half) * axis]))
        poses.append(((x_star.astype(np.float64) - centre) @ R.T + centre + 0.3 * way).astype(np.float32))
    r = run(fixture_case(poses, lv))
    for g in range(8):
        e0, e1 = RR.energy(r['terms_in'][0, g], W), RR.energy(r['terms'][0, g], W)
        start, end = rmsd(poses[g], x_star), rmsd(r['pos'][0, g * n:(g + 1) * n], x_star)
        print(f'copy {g}: E {e0:.4f} -> {e1:.4f} (E* {e_star:.4f}, recovered {(e0 - e1) / (e0 - e_star):.4f}), RMSD to x* {start:.4f} -> {end:.4f}')
        assert e0 - e1 >= 0.9 * (e0 - e_star), g
        assert end <= 0.25 * start, g


EXACT = ('n_included', 'scored', 'n_converged', 'n_out_of_budget', 'n_at_cap', 'sum_steps', 'sum_evals', 'n_samples', 'n_ref')


def test_pocket_relax_the_pack_and_sample_relax_through_a_result_dictionary():
    dev = _dev()
    p, lpos, lv = docked()
    rng = np.random.default_rng(0)
    T = 2
    # three samples: the docked pose, a jittered copy, and a part of it moved 30 A away; two frames that end in those poses
    final = [lpos, (lpos + rng.normal(0, 0.5, lpos.shape)).astype(np.float32), lpos[:17] + np.float32(30)]
    pos_traj = [np.stack([(x + rng.normal(0, 0.3 * (T - 1 - t), x.shape)).astype(np.float32) for t in range(T)]).astype(np.float64) for x in final]
    v_traj = [np.stack([lv[:len(x)]] * T) for x in final]
    data = types.SimpleNamespace(protein_pos=torch.from_numpy(p['pos']), protein_atom_feature=torch.from_numpy(p['feat'].astype(np.int64)))
    result = {'data': data, 'pred_ligand_pos_traj': pos_traj, 'pred_ligand_v_traj': v_traj}
    elem, kind, _ = quality.pocket_kinds(p['feat'])
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    pocket = (t(p['pos'], torch.float32), t(elem, torch.int32), t(kind, torch.int32), t(IR.pocket_roles(p['feat']), torch.int32), 40, RSUM, W)

    def raw_outputs(pos, v, ptr):
        pack = (t(pos, torch.float32), t(v, torch.int64), t(ptr, torch.int32), CLASS_Z, AROMATIC)
        bond_ptr = capi.bond_graph(*pack, (), None, False, True)['bond_ptr']
        ring = capi.ring_report(*pack, None, bond_ptr, False)['bond_ring']
        out = capi.score_minimize(*pack, *pocket, 8.0, 1.75, bond_ptr, ring)
        return {k: x.cpu().numpy() for k, x in out.items()}

    q = raw_outputs(lpos[None], lv[None], [0, len(lv)])
    ref_scores = tuple(float(SR.energies(q[k], q['n_rot'])[2][0, 0]) for k in ('terms_in', 'terms'))
    assert ref_scores[1] < ref_scores[0] < 0
    for eval_step, frames in ((-1, slice(T - 1, T)), ('all', slice(0, T))):
        pos = np.concatenate([x[frames] for x in pos_traj], 1).astype(np.float32)
        v = np.concatenate([x[frames] for x in v_traj], 1)
        raw = raw_outputs(pos, v, [0, 25, 50, 67])
        S = raw['status'].shape[0]
        expect = quality.RelaxReport.from_outputs(raw, np.ones((S, 3), bool), pos, [25, 25, 17], ref_scores=ref_scores)
        got = quality.sample_relax(result, eval_step, reference_ligand=(lpos, lv), device=dev)
        pack = quality.SamplePack(result, eval_step, device=dev)
        method = pack.relax(data, reference_ligand=(lpos, lv))
        assert pack.relaxed_pos.cpu().numpy().tobytes() == raw['pos'].tobytes()
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
        assert got.num_frames == S and s['mean_score_min'] < s['mean_score'] and s['mean_gain'] > 0 and s['better_than_ref_min'] <= 1 / 3
        assert s['best_score_min'] <= s['median_score_min'] and 0 < s['mean_rmsd'] and s['mean_shift'] <= 3.0 and s['mean_evals'] > 1
        np.testing.assert_allclose([s['ref_score'], s['ref_score_min']], ref_scores, rtol=1e-6)
    # the stateless form gives the kernel's outputs on the same pocket
    x = quality.pocket_relax(p['pos'], p['feat'], pos, v, ligand_ptr=torch.tensor([0, 25, 50, 67], dtype=torch.int32), device=dev)
    for k, a in (('raw_terms_in', raw['terms_in']), ('raw_terms', raw['terms']), ('n_pairs', raw['n_pairs']), ('n_rot', raw['n_rot']),
                 ('n_steps', raw['n_steps']), ('n_evals', raw['n_evals']), ('status', raw['status']), ('transform', raw['transform'])):
        np.testing.assert_array_equal(getattr(x, k), a, err_msg=k)
    assert x.pos.cpu().numpy().tobytes() == raw['pos'].tobytes()
    np.testing.assert_allclose(x.score, SR.energies(raw['terms'], raw['n_rot'])[2], rtol=1e-6)
    np.testing.assert_allclose(x.score_in, SR.energies(raw['terms_in'], raw['n_rot'])[2], rtol=1e-6)
    assert x.rmsd[-1, 2] == 0 and x.rmsd[-1, 0] > 0 and (x.shift <= 3.0).all()
