"""CPU-only checks of the rigid-body relaxation ("Pose relaxation"): a local optimisation under this project's
heuristic score, not AutoDock Vina's minimize; rigid-body only: three translations and three rotations, no torsions.

  1. the analytic gradient of tests/_relax_ref.py, the restatement the GPU tests compare td_score_minimize with, against central
     differences of its own unrounded energy on the docked 1h36 ligand, at three poses where no pair lies within reach of a breakpoint
     or of the cutoff.  The tolerance is the difference quotient's own truncation error, estimated from h and h / 2, plus the float64
     rounding of the energy differences; it is not a fixed number;
  2. the restatement on the four poses of test_gpu_score.py's shifted pack, pinned to the figures it gives (DESIGN.md records them);
  3. a planted minimum: the docked pose relaxed with 200 steps is x*; eight copies moved by 0.3 A and turned by 5 degrees come back,
     and a translation-only optimiser (the torque zeroed) does not: the conditions tell the two apart;
  4. the ABI surface, every refusal of the binding, quality.RelaxReport's arithmetic, tools/evaluate_samples.py --minimize and
     tools/export_sdf.py --relaxed with the bindings patched by the restatements, and the output without --minimize unchanged.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

import _bonds_ref as BR
import _interactions_ref as IR
import _pocket_ref as PR
import _relax_ref as RR
import _score_ref as SR
from conftest import load_golden
from targetdiff_amd import capi, molfile, quality
from test_bonds_host import load_tool
from test_interactions_host import typed_pocket, typed_result
from test_pocket_host import save_with_pockets
from test_sample_pack_host import numpy_binding  # noqa: F401  (the fixture that patches the other bindings)

f32 = np.float32
CLASS_Z = quality.class_atomic_numbers('add_aromatic')
AROMATIC = BR.CLASS_AROMATIC
W = SR.WEIGHTS
RSUM = SR.radius_sums()
_CACHE = {}


def fixture():
    """the 1h36 pocket with its resolved roles and the docked ligand with the roles of the docked pose, once"""
    if 'fixture' not in _CACHE:
        p, l = load_golden('pocket_1h36.npz'), load_golden('ligand_1h36_docked.npz')
        cls = {'H': 0, 'C': 1, 'N': 3, 'O': 5, 'F': 7, 'P': 8, 'S': 10, 'Cl': 12, 'Br': 12}  # Br is outside the table: taken as Cl
        lpos, lv = l['pos'].astype(f32), np.asarray([cls[str(e)] for e in l['elements']], np.int64)
        elem, kind, _ = quality.pocket_kinds(p['feat'])
        pr = IR.protein_roles(p['pos'], elem, kind, IR.pocket_roles(p['feat']), 40)
        _CACHE['fixture'] = (p['pos'], elem, pr, lpos, lv)
    return _CACHE['fixture']


def relax(x, lv, **kw):
    ppos, elem, pr, _, _ = fixture()
    lel, lrole, _ = RR.molecule_inputs(x, lv, CLASS_Z)
    return RR.relax_molecule(x, lel, lrole, ppos, elem, pr, RSUM, W, **kw)


def rmsd(x, y):
    return float(np.sqrt(((np.asarray(x, np.float64) - np.asarray(y, np.float64)) ** 2).sum(-1).mean()))


def test_the_analytic_gradient_against_central_differences():
    ppos, elem, pr, lpos, lv = fixture()
    lel, lrole, scored = RR.molecule_inputs(lpos, lv, CLASS_Z)
    c0 = RR.centroid(lpos, scored)
    x0 = lpos.astype(np.float64) - c0
    rmol = float(np.sqrt((x0[scored] ** 2).sum(1).max()))
    h = 1e-4
    reach = h * (1.0 + rmol)                                                     # how far a step of h in any of the six moves an atom
    energy = lambda q, t: RR.unrounded(RR.pose64(x0, q, t, c0), lel, lrole, c0 + t, ppos, elem, pr, RSUM, 8.0, W)
    rng = np.random.default_rng(5)
    poses = []
    for _ in range(400):                                                         # states near the docked one, kept when every pair is clear
        q, t = RR.moved(np.asarray([1.0, 0, 0, 0]), np.zeros(3), np.concatenate([rng.normal(0, 0.2, 3), rng.normal(0, 0.05, 3)]))
        if energy(q, t)[2] > 2.0 * reach:
            poses.append((q, t))
        if len(poses) == 3:
            break
    assert len(poses) == 3
    for q, t in poses:
        E, grad, margin = energy(q, t)
        assert margin > reach, 'a pair within reach of a breakpoint or of the cutoff'
        for k in range(6):
            quotient = []
            for step in (h, h / 2):
                delta = np.zeros(6)
                delta[k] = step
                up, down = energy(*RR.moved(q, t, delta))[0], energy(*RR.moved(q, t, -delta))[0]
                quotient.append((up - down) / (2 * step))
            # D(h) = E' + c h^2 + ...: D(h) - D(h / 2) is 3/4 of D(h)'s truncation error; the rounding of 2 N energies of size |E|
            tol = 2.0 * abs(quotient[0] - quotient[1]) + 64 * np.finfo(np.float64).eps * (abs(E) + 30.0) / h
            assert abs(grad[k] - quotient[0]) <= tol, (k, grad[k], quotient, tol)
            assert tol < 1e-3 * max(1.0, abs(grad[k])), 'the check has teeth'
    # the rounded evaluation at the docked pose gives the same gradient up to its units
    terms, g, pairs = RR.evaluate(lpos, lel, lrole, c0, ppos, elem, pr, RSUM, 8.0, W)
    _, grad, _ = energy(np.asarray([1.0, 0, 0, 0]), np.zeros(3))
    assert pairs == 2045 and np.abs(g / SR.UNIT - grad).max() <= pairs / SR.UNIT


def test_the_restatement_on_the_shifted_poses_of_1h36():
    _, _, _, lpos, lv = fixture()
    poses = [lpos, lpos + np.asarray([1.5, 0, 0], f32), lpos + np.asarray([4, 0, 0], f32), lpos + f32(30)]
    r = [relax(x, lv) for x in poses]
    e_in, e_out = [RR.energy(x['terms_in'], W) for x in r], [RR.energy(x['terms'], W) for x in r]
    print([(a, b, x['n_steps'], x['n_evals'], x['status'], rmsd(x['pos'], y)) for a, b, x, y in zip(e_in, e_out, r, poses)])
    np.testing.assert_allclose(e_in[:3], [-14.68, 7.38, 206.8], atol=0.06)
    # pinned: what this restatement gives ("Pose relaxation")
    np.testing.assert_allclose(e_out[:2], [-14.7474, -14.7372], atol=5e-3)
    assert abs(rmsd(r[0]['pos'], poses[0]) - 0.0916) < 0.01 and r[0]['status'] & RR.CONVERGED and 5 <= r[0]['n_steps'] <= 64
    assert abs(rmsd(r[1]['pos'], poses[1]) - 1.53) < 0.02 and 10 <= r[1]['n_steps'] <= 64 and r[1]['n_evals'] <= 257
    assert rmsd(r[1]['pos'], poses[0]) < 0.1                                     # back at the docked pose
    assert r[2]['status'] & RR.AT_CAP and np.sqrt((r[2]['transform'][4:] ** 2).sum()) <= 3.0 and e_out[2] < e_in[2]
    assert r[3]['n_steps'] == 0 and r[3]['n_evals'] == 1 and r[3]['status'] == RR.CONVERGED and e_out[3] == 0
    assert r[3]['pos'].tobytes() == poses[3].tobytes()
    for x, y in zip(r, poses):                                                   # the contract, whatever the trajectory
        lel, lrole, scored = RR.molecule_inputs(y, lv, CLASS_Z)
        if x['n_steps']:
            np.testing.assert_array_equal(x['pos'], RR.transformed(y, scored, x['transform']))
        ppos, elem, pr, _, _ = fixture()
        np.testing.assert_array_equal(RR.evaluate(x['pos'], lel, lrole, np.zeros(3), ppos, elem, pr, RSUM, 8.0, W)[0], x['terms'])
        assert all(a >= b for a, b in zip(x['trace'], x['trace'][1:]))
    zero = relax(poses[1], lv, max_steps=0)
    assert zero['n_evals'] == 1 and zero['status'] == RR.OUT_OF_BUDGET and (zero['terms'] == zero['terms_in']).all()
    few = relax(poses[1], lv, max_evals=5)
    assert few['n_evals'] == 5 and few['status'] & RR.OUT_OF_BUDGET


def test_a_planted_minimum_is_found_again_and_not_by_translation_alone():
    _, _, _, lpos, lv = fixture()
    star = relax(lpos, lv, max_steps=200)
    x_star, e_star = star['pos'], RR.energy(star['terms'], W)
    rng = np.random.default_rng(2024)
    centre = x_star.astype(np.float64)[lv != 0].mean(0)
    for g in range(8):
        axis, way = rng.normal(size=3), rng.normal(size=3)
        axis, way = axis / np.linalg.norm(axis), way / np.linalg.norm(way)
        half = np.radians(5.0) / 2.0
        R = RR.rotation(np.concatenate([[np.cos(half)], np.sin(half) * axis]))
        x = ((x_star.astype(np.float64) - centre) @ R.T + centre + 0.3 * way).astype(f32)
        start = rmsd(x, x_star)
        full, flat = relax(x, lv), relax(x, lv, torque=False)
        e0 = RR.energy(full['terms_in'], W)
        got = lambda r: ((e0 - RR.energy(r['terms'], W)) / (e0 - e_star), rmsd(r['pos'], x_star))
        print(f'copy {g}: start {start:.4f}; recovered, RMSD: {got(full)}; translation only: {got(flat)}')
        assert got(full)[0] >= 0.9 and got(full)[1] <= 0.25 * start, g
        assert got(flat)[0] < 0.9 and got(flat)[1] > 0.25 * start, g           # the conditions have teeth


def test_the_library_exports_td_score_minimize_and_refuses_bad_budgets():
    lib = capi.load_library()
    assert hasattr(lib, 'td_score_minimize') and len(capi.SIGNATURES['td_score_minimize'][1]) == 37
    assert lib.td_abi_version() == capi.ABI_VERSION == 5
    assert (capi.RELAX_MAX_STEPS, capi.RELAX_MAX_SHIFT) == (RR.MAX_STEPS, RR.MAX_SHIFT) == (64, 3.0)
    assert (capi.RELAX_CONVERGED, capi.RELAX_OUT_OF_BUDGET, capi.RELAX_AT_CAP) == (RR.CONVERGED, RR.OUT_OF_BUDGET, RR.AT_CAP) == (1, 2, 4)
    assert capi.RELAX_KEYS == RR.KEYS
    doc = ' '.join(capi.score_minimize.__doc__.split())
    assert "not AutoDock Vina's ``minimize``" in doc and 'rigid-body only: three translations and three rotations, no torsions' in doc
    cz = np.asarray(CLASS_Z, np.int32)
    dbl = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    rs, w = np.ascontiguousarray(RSUM.reshape(-1)), np.asarray(W)

    def call(weights=w, max_steps=64, max_evals=257, max_shift=3.0, cutoff=8.0):
        # an empty pack and an empty pocket: every refusal comes before anything touches a device
        return lib.td_score_minimize(None, None, None, 0, 0, 0, cz.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), cz.size, None, None, None, None,
                                     None, 0, 40, cutoff, 1.75, dbl(rs), None, 0, None, None if weights is None else dbl(weights), max_steps,
                                     max_evals, max_shift, *([None] * 12))

    for kw, word in ((dict(max_shift=0.0), b'max_shift'), (dict(max_shift=-1.0), b'max_shift'), (dict(max_shift=float('nan')), b'max_shift'),
                     (dict(max_shift=float('inf')), b'max_shift'), (dict(max_steps=-1), b'max_steps'), (dict(max_evals=0), b'max_evals'),
                     (dict(max_evals=-3), b'max_evals'), (dict(weights=None), b'null'), (dict(weights=np.asarray([1, 2, np.inf, 0, 0.0])), b'weights'),
                     (dict(cutoff=0.0), b'cutoff')):
        assert call(**kw) == -1 and word in lib.td_last_error(), kw            # TD_EINVAL


def test_every_refusal_of_the_binding():
    c = IR.build_case(3, 20, [4, 6])
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt)
    pack = (t(c['pos'], torch.float32), t(c['v'], torch.int64), t(c['ptr'], torch.int32), CLASS_Z, AROMATIC)
    pocket = (t(c['ppos'], torch.float32), t(c['pelem'], torch.int32), t(c['pkind'], torch.int32), t(c['prole'], torch.int32), 40, RSUM)
    for kw, match in ((dict(max_shift=0.0), 'max_shift'), (dict(max_shift=float('nan')), 'max_shift'), (dict(max_shift=float('inf')), 'max_shift'),
                      (dict(max_steps=-1), 'max_steps'), (dict(max_steps=2.5), 'max_steps'), (dict(max_evals=0), 'max_evals'),
                      (dict(cutoff=-1.0), 'cutoff'), (dict(hetero_cutoff=float('nan')), 'cutoff'),
                      (dict(bond_ptr=torch.zeros(3, dtype=torch.int64)), 'come together')):
        with pytest.raises(ValueError, match=match):
            capi.score_minimize(*pack, *pocket, W, **kw)
    for weights in (W[:4], W + (1.0,), (1.0, 2.0, float('nan'), 0.0, 0.0)):
        with pytest.raises(ValueError, match='weights'):
            capi.score_minimize(*pack, *pocket, weights)
    bad = RSUM.copy()
    bad[3, 2] = 6.5
    with pytest.raises(ValueError, match='rsum'):
        capi.score_minimize(*pack, *pocket[:5], bad, W)
    big = IR.build_case(3, 20, [4, 513])
    with pytest.raises(ValueError, match='at most 512'):
        capi.score_minimize(t(big['pos'], torch.float32), t(big['v'], torch.int64), t(big['ptr'], torch.int32), CLASS_Z, AROMATIC, *pocket, W)
    with pytest.raises(RuntimeError, match='HIP device'):                       # valid arguments: only the device is missing
        capi.score_minimize(*pack, *pocket, W)
    assert capi._relax_inputs(W, 7, None, 2)[1:] == (7, 29, 2.0) and capi._relax_inputs(W, 0, None, 1.0)[2] == 1


def hand_outputs():
    """one frame of four molecules of two atoms, one of them refused by the kernel"""
    unit = 1 << 24
    terms_in = np.asarray([[[0, 0, 2 * unit, 0, 0], [unit, 0, 0, 0, 0], [0, 0, 0, 0, unit], [SR.INT64_MIN] * 5]], np.int64)
    terms = np.asarray([[[0, 0, unit, 0, 0], [unit, 0, 0, 0, 0], [0, 0, 0, 0, 2 * unit], [SR.INT64_MIN] * 5]], np.int64)
    transform = np.zeros((1, 4, 7))
    transform[..., 0] = 1.0
    transform[0, 0, 4:] = [3.0, 0.0, 4.0]
    pos_in = np.zeros((1, 8, 3), f32)
    pos = pos_in.copy()
    pos[0, 0:2] += f32([3.0, 0.0, 4.0])                                          # moved by 5
    pos[0, 4] += f32([0.0, 2.0, 0.0])                                            # one of two atoms moved by 2: RMSD sqrt(2)
    raw = dict(pos=pos, terms_in=terms_in, terms=terms, n_rot=np.asarray([[2, 0, 1, -1]]), n_steps=np.asarray([[4, 0, 7, 0]]),
               n_evals=np.asarray([[9, 1, 30, 0]]), status=np.asarray([[5, 1, 2, -1]]), transform=transform)
    return raw, pos_in


def test_relax_report_arithmetic_merge_and_the_exclusion_of_refused_molecules():
    raw, pos_in = hand_outputs()
    w = np.asarray(quality.SCORE_WEIGHTS)
    before = np.asarray([2 * w[2] / (1 + 0.117), w[0], w[4] / 1.0585])
    after = np.asarray([w[2] / (1 + 0.117), w[0], 2 * w[4] / 1.0585])
    rep = quality.RelaxReport.from_outputs(raw, np.ones((1, 4), bool), pos_in, [2, 2, 2, 2])
    np.testing.assert_array_equal(rep.n_included, [3])
    np.testing.assert_array_equal(rep.scored, [[True, True, True, False]])
    np.testing.assert_allclose(rep.scores_in[0, :3], before, rtol=1e-15)
    np.testing.assert_allclose(rep.scores[0, :3], after, rtol=1e-15)
    assert np.isnan(rep.scores[0, 3]) and rep.n_samples == 4 and rep.sum_ref is None
    np.testing.assert_array_equal([rep.n_converged, rep.n_out_of_budget, rep.n_at_cap, rep.sum_steps, rep.sum_evals], [[2], [1], [1], [11], [40]])
    s = rep.summary(0)
    assert list(s) == ['mean_score', 'median_score', 'best_score', 'mean_score_min', 'median_score_min', 'best_score_min', 'mean_gain',
                       'share_negative_min', 'mean_rmsd', 'mean_shift', 'converged', 'out_of_budget', 'at_cap', 'mean_steps', 'mean_evals']
    np.testing.assert_allclose([s['mean_score'], s['median_score'], s['best_score']], [before.sum() / 3, np.median(before), before.min()], rtol=1e-15)
    np.testing.assert_allclose([s['mean_score_min'], s['median_score_min'], s['best_score_min']], [after.sum() / 3, np.median(after), after.min()],
                               rtol=1e-15)
    np.testing.assert_allclose(s['mean_gain'], (before - after).sum() / 3, rtol=1e-14)
    np.testing.assert_allclose([s['mean_rmsd'], s['mean_shift']], [(5.0 + 0.0 + np.sqrt(2.0)) / 3, 5.0 / 3], rtol=1e-15)
    assert s['share_negative_min'] == 2 / 3 and s['converged'] == 2 / 3 and s['out_of_budget'] == 1 / 3 and s['at_cap'] == 1 / 3
    assert s['mean_steps'] == 11 / 3 and s['mean_evals'] == 40 / 3 and len(rep.lines(0)) == len(s)
    # with the known ligand: the share strictly below its minimised score
    ref = quality.RelaxReport.from_outputs(raw, np.ones((1, 4), bool), pos_in, [2, 2, 2, 2], ref_scores=(0.5, float(after[1])))
    r = ref.summary(0)
    assert r['ref_score'] == 0.5 and r['ref_score_min'] == after[1] and r['better_than_ref_min'] == 1 / 3
    # an excluded molecule, and merged over two pockets: the sums add, the per-molecule values join
    part = quality.RelaxReport.from_outputs(raw, np.asarray([[True, False, True, True]]), pos_in, [2, 2, 2, 2])
    both = quality.RelaxReport.merged([rep, part])
    union = np.concatenate([after, after[[0, 2]]])
    b = both.summary(0)
    assert both.scores.shape == (1, 8) and both.n_samples == 8 and both.n_included[0] == 5
    np.testing.assert_allclose([b['median_score_min'], b['mean_score_min'], b['mean_steps']], [np.median(union), union.sum() / 5, 22 / 5], rtol=1e-14)
    with pytest.raises(ValueError, match='reference ligand'):
        quality.RelaxReport.merged([rep, ref])
    none = quality.RelaxReport.from_outputs(raw, np.zeros((1, 4), bool), pos_in, [2, 2, 2, 2])
    assert all(x != x for x in none.summary(0).values()) and none.lines(0)[0] == 'mean_score:\tNone'


@pytest.fixture
def relax_binding(numpy_binding, monkeypatch):  # noqa: F811
    """numpy_binding, and capi.score_minimize, capi.score_report and capi.pocket_report patched by their restatements too"""
    def patched(name, fn):
        def binding(*a, **kw):
            numpy_binding.append((name, kw.get('check')))
            return fn(*a, **kw)
        return binding

    monkeypatch.setattr(capi, 'score_minimize', patched('score_minimize', RR.torch_score_minimize))
    monkeypatch.setattr(capi, 'score_report', patched('score_report', SR.torch_score_report))
    monkeypatch.setattr(capi, 'pocket_report', patched('pocket_report', PR.torch_pocket_report))
    return numpy_binding


def expected_report(res, data, eval_step, reference_ligand=None, **budget):
    """(RelaxReport, raw outputs) of a result through the restatement alone"""
    frames = slice(None) if eval_step == 'all' else slice(len(res[2][0]) - 1, None)
    sizes = [p.shape[1] for p in res[2]]
    pos = np.concatenate([p[frames] for p in res[2]], 1).astype(f32)
    v = np.concatenate([x[frames] for x in res[3]], 1)
    elem, kind, _ = quality.pocket_kinds(data.protein_atom_feature)
    pocket = (data.protein_pos.numpy(), elem, kind, IR.pocket_roles(data.protein_atom_feature.numpy()), 40, RSUM)
    score = lambda w, k: float(SR.energies(w[k], w['n_rot'])[2][0, 0])
    ref_scores = None
    if reference_ligand is not None:
        q = RR.score_minimize(reference_ligand[0][None], reference_ligand[1][None], [0, len(reference_ligand[1])], CLASS_Z, AROMATIC, *pocket,
                              **budget)
        ref_scores = (score(q, 'terms_in'), score(q, 'terms'))
    w = RR.score_minimize(pos, v, np.cumsum([0] + sizes), CLASS_Z, AROMATIC, *pocket, **budget)
    return quality.RelaxReport.from_outputs(w, np.ones(w['status'].shape, bool), pos, sizes, ref_scores=ref_scores), w


def two_files():
    results = {10: typed_result(5, [6, 9, 14], 2), 2: typed_result(6, [4, 11, 5, 1], 2)}
    pockets = {10: typed_pocket(1), 2: typed_pocket(2, 45)}
    ligand = (np.asarray(results[10][2][0][-1], f32), np.asarray(results[10][3][0][-1], np.int64))
    return results, pockets, ligand


def assert_same(got, want):
    assert type(got) is type(want) and vars(got).keys() == vars(want).keys()
    for k, x in vars(want).items():
        if isinstance(x, np.ndarray):
            assert np.array_equal(getattr(got, k), x, equal_nan=x.dtype.kind == 'f'), k
    for s in range(want.num_frames):
        np.testing.assert_equal(got.summary(s), want.summary(s))


def test_sample_relax_the_pack_and_the_stateless_form(relax_binding):
    results, pockets, ligand = two_files()
    res, data = results[2], pockets[2]
    as_dict = {'data': data, 'pred_ligand_pos_traj': res[2], 'pred_ligand_v_traj': res[3]}
    want, w = expected_report(res, data, 'all', ligand, max_steps=6)
    assert_same(quality.sample_relax(as_dict, 'all', reference_ligand=ligand, max_steps=6, device='cpu'), want)
    assert (w['n_steps'] > 0).any() and 'ref_score_min' in want.summary(-1)
    pack = quality.SamplePack(as_dict, -1, device='cpu')
    got = pack.relax(quality.PocketSide(data, 'cpu'), max_steps=6, max_shift=0.5)
    assert_same(got, expected_report(res, data, -1, max_steps=6, max_shift=0.5)[0])
    np.testing.assert_array_equal(pack.relaxed_pos.numpy(), expected_report(res, data, -1, max_steps=6, max_shift=0.5)[1]['pos'])
    with pytest.raises(ValueError, match='carries no pocket'):
        quality.sample_relax(res, device='cpu')
    x = quality.pocket_relax(data.protein_pos, data.protein_atom_feature, res[2][1][-1].astype(f32), res[3][1][-1],
                             ligand_ptr=torch.tensor([0, 11], dtype=torch.int32), max_steps=6, device='cpu')
    last = expected_report(res, data, -1, max_steps=6)
    np.testing.assert_array_equal(x.raw_terms[0, 0], last[1]['terms'][0, 1])
    np.testing.assert_array_equal(x.score[0, 0], last[0].scores[0, 1])
    np.testing.assert_array_equal(x.pos.numpy()[0], last[1]['pos'][0, 4:15])
    assert x.n_steps[0, 0] == last[1]['n_steps'][0, 1] and x.rmsd.shape == (1, 1) and (x.shift <= 3.0).all()
    for doc in (quality.pocket_relax.__doc__, quality.sample_relax.__doc__, quality.Relaxed.__doc__):
        assert 'AutoDock Vina' in doc
    for doc in (quality.pocket_relax.__doc__, quality.sample_relax.__doc__):
        assert "not AutoDock Vina's ``minimize``" in doc and 'rigid-body only: three translations and three rotations, no torsions' in ' '.join(doc.split())


def test_the_evaluate_tool_with_and_without_minimize(relax_binding, tmp_path, monkeypatch, capsys):
    results, pockets, ligand = two_files()
    (tmp_path / 'samples').mkdir()
    save_with_pockets(tmp_path / 'samples', results, pockets)
    np.savez(tmp_path / 'ref.npz', ligand_pos=ligand[0], ligand_v=ligand[1])
    monkeypatch.chdir(tmp_path)
    tool = load_tool('evaluate_samples')
    base = ['--sample_path', 'samples', '--device', 'cpu', '--reference_npz', 'ref.npz']
    capsys.readouterr()
    plain = tool.main(base + ['--score'])
    plain_stdout = capsys.readouterr().out
    with open(tmp_path / 'samples' / 'eval_results' / 'quality.json', 'rb') as f:
        plain_bytes = f.read()
    assert 'minimize' not in plain and 'score_minimize' not in [n for n, _ in relax_binding] and 'mean_score_min' not in plain_stdout
    out = tool.main(base + ['--score', '--minimize', '--min_steps', '5', '--max_shift', '1.5'])
    stdout = capsys.readouterr().out
    with open(tmp_path / 'samples' / 'eval_results' / 'quality.json') as f:
        written = json.load(f)
    # everything but the new section is what it was without the flag
    assert {k: x for k, x in written.items() if k != 'minimize'} == json.loads(plain_bytes)
    assert stdout.startswith(plain_stdout[:plain_stdout.index('wrote ')]) and stdout.endswith(plain_stdout[plain_stdout.index('wrote '):])
    want = quality.RelaxReport.merged([expected_report(results[i], pockets[i], -1, ligand, max_steps=5, max_shift=1.5)[0] for i in (2, 10)])
    s = want.summary(-1)
    for k, x in s.items():
        assert out['minimize'][k] == x and f'{k}:\t{x:.4f}' in stdout, k
    assert out['minimize']['num_included'] == 7 and out['minimize']['max_steps'] == 5 and out['minimize']['max_shift'] == 1.5
    assert s['mean_score_min'] <= s['mean_score'] and s['mean_gain'] > 0 and s['mean_score'] == out['score']['mean_score']
    assert 'ref_score_min' in s and "not\nAutoDock Vina's ``minimize``" in tool.__doc__ and 'no torsions' in tool.__doc__


def test_the_export_tool_writes_relaxed_coordinates(relax_binding, tmp_path):
    results, pockets, _ = two_files()
    save_with_pockets(tmp_path, results, pockets)
    tool = load_tool('export_sdf')
    common = ['--sample_path', str(tmp_path), '--device', 'cpu']
    plain = tool.main(common + ['--out', str(tmp_path / 'plain')])
    out = tool.main(common + ['--out', str(tmp_path / 'relaxed'), '--relaxed'])
    moved = 0
    for i in results:
        rep, w = expected_report(results[i], pockets[i], -1)
        recs = molfile.read_sdf(str(tmp_path / 'relaxed' / f'result_{i}.sdf'))
        base = molfile.read_sdf(str(tmp_path / 'plain' / f'result_{i}.sdf'))
        assert out[f'result_{i}']['written'] == plain[f'result_{i}']['written'] == len(recs) == len(base)
        ptr = np.cumsum([0] + [p.shape[1] for p in results[i][2]])
        for m, b in zip(recs, base):
            g = int(m['name'].rsplit('_', 1)[1])
            assert m['name'] == b['name'] and m['bonds'] == b['bonds'] and 'score' not in b['properties']
            assert m['properties']['score'] == f'{rep.scores_in[0, g]:.4f}' and m['properties']['score_min'] == f'{rep.scores[0, g]:.4f}'
            heavy = np.asarray(CLASS_Z)[results[i][3][g][-1]] != 1
            np.testing.assert_allclose(m['pos'], w['pos'][0, ptr[g]:ptr[g + 1]][heavy], atol=1e-4)
            moved += int(w['n_steps'][0, g] > 0)
    assert moved > 0
    with pytest.raises(SystemExit, match='carries no pocket'):
        from test_bonds_host import save_results
        (tmp_path / 'bare').mkdir()
        save_results(tmp_path / 'bare', results)
        tool.main(['--sample_path', str(tmp_path / 'bare'), '--device', 'cpu', '--out', str(tmp_path / 'none'), '--relaxed'])
