"""CPU-only checks of the docking search ("Docking search"): a rigid-body global search under this project's heuristic
score, not AutoDock Vina's dock: three translations and three rotations, no torsions.

  1. tests/_dock_ref.py, the restatement the GPU tests compare td_score_dock with, holds the contract on 1h36: the final terms are the
     evaluation of the written pose, the pose is the transform's bit for bit, |t| <= max_shift, chain 0 round 0 is
     _relax_ref.relax_molecule, and the best never rises with more rounds or more chains on a prefix of the draws;
  2. redocking: the planted pose x* of test_relax_host.py, three displaced copies that the relaxation alone leaves more than 2 A from x*
     and that the search at 16 x 16 brings back within 0.25 A;
  3. the ABI surface, every refusal of the C entry and of the binding, quality.DockReport's arithmetic, sample_dock / SamplePack.dock,
     tools/evaluate_samples.py --dock and tools/export_sdf.py --docked with the bindings patched by the restatements, and the output
     without --dock unchanged.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

import _dock_ref as DR
import _interactions_ref as IR
import _relax_ref as RR
import _score_ref as SR
from targetdiff_amd import capi, molfile, quality
from test_bonds_host import load_tool
from test_pocket_host import save_with_pockets
from test_relax_host import AROMATIC, CLASS_Z, RSUM, W, fixture, relax, relax_binding, rmsd, two_files  # noqa: F401  (relax_binding: a fixture)
from test_sample_pack_host import numpy_binding  # noqa: F401  (the fixture relax_binding builds on)

f32 = np.float32
# Redocking.  The copies are drawn as test_relax_host.py draws its eight: from default_rng(7), in the order 40 deg / 1 A, 90 / 1.5,
# 180 / 2, 120 / 1, 60 / 2, about random axes through the centre of x* and along random directions.  Kept: 90 / 1.5, 180 / 2, 60 / 2.
# What the restatement gives at 16 chains x 16 rounds with draws default_rng(seed).random((16, 17, 7)), RMSD to x* in A:
#   copy        relaxation alone   seed 116   1       2       3       4       5       6       7       chains within 0.5 of the winner
#   90 / 1.5    7.482              0.019    0.058   0.021   0.031   0.045   0.032   0.047   0.025     4 - 6 of 16
#   180 / 2     3.212              0.015    0.020   0.024   0.020   0.018   0.012   0.030   0.023     1 - 6 of 16
#   60 / 2      7.662              0.019    0.014   0.016   0.008   0.027   0.017   0.018   0.028     5 - 10 of 16
# (4 500 - 10 000 evaluations per molecule.)  Not kept: 40 / 1, which the relaxation alone brings back (0.05 A), and 120 / 1, which the
# search finds with five of the eight seeds only (10.65 A at -10.8 with seeds 1, 4 and 6): a pose that only some seeds find is no input.
REDOCK_CASES, REDOCK_KEPT, REDOCK_SEED = ((40, 1.0), (90, 1.5), (180, 2.0), (120, 1.0), (60, 2.0)), (1, 2, 4), 116


def redocking_copies(x_star, lv):
    rng = np.random.default_rng(7)
    centre = x_star.astype(np.float64)[lv != 0].mean(0)
    copies = []
    for angle, shift in REDOCK_CASES:
        axis, way = rng.normal(size=3), rng.normal(size=3)
        axis, way = axis / np.linalg.norm(axis), way / np.linalg.norm(way)
        half = np.radians(angle) / 2.0
        R = RR.rotation(np.concatenate([[np.cos(half)], np.sin(half) * axis]))
        copies.append(((x_star.astype(np.float64) - centre) @ R.T + centre + shift * way).astype(f32))
    return [copies[k] for k in REDOCK_KEPT]


def dock(x, lv, draws, **kw):
    ppos, elem, pr, _, _ = fixture()
    lel, lrole, _ = RR.molecule_inputs(x, lv, CLASS_Z)
    return DR.dock_molecule(x, lel, lrole, ppos, elem, pr, RSUM, W, draws, **kw)


def test_the_restatement_holds_the_contract_on_1h36():
    ppos, elem, pr, lpos, lv = fixture()
    x = lpos + np.asarray([1.5, 0, 0], f32)
    lel, lrole, scored = RR.molecule_inputs(x, lv, CLASS_Z)
    draws = np.random.default_rng(3).random((3, 3, 7))
    budget = dict(max_steps=12, max_shift=1.75)
    r = dock(x, lv, draws, **budget)
    # the final terms are the evaluation of the written pose, and the pose is the transform's
    np.testing.assert_array_equal(RR.evaluate(r['pos'], lel, lrole, np.zeros(3), ppos, elem, pr, RSUM, 8.0, W)[0], r['terms'])
    np.testing.assert_array_equal(r['pos'], RR.transformed(x, scored, r['transform']))
    clamped = 0
    for k, ch in enumerate(r['chains']):
        np.testing.assert_array_equal(RR.evaluate(RR.transformed(x, scored, r['chain_transform'][k]), lel, lrole, np.zeros(3), ppos, elem, pr, RSUM, 8.0,
                                                  W)[0], r['chain_terms'][k])
        assert np.sqrt((ch['t'] ** 2).sum()) <= 1.75 and abs((ch['q'] ** 2).sum() - 1.0) < 1e-12
        assert 1 <= ch['accepts'] <= 3 and ch['n_evals'] >= 3 and ch['history'] == sorted(ch['history'], reverse=True)
        clamped += bool(ch['status'] & RR.AT_CAP)
    assert r['n_evals'] == r['chain_evals'].sum() and r['best_chain'] == int(np.argmin([c['inter'] for c in r['chains']]))
    # the clamp itself: a mutation that leaves the ball comes back inside it, and says so
    q, t, capped = DR.mutated([1.0, 0, 0, 0], [1.0, 1.0, 0.9], [0.99] * 6, 2.0, 0.1, 1.75)
    assert capped and 1.75 * (1 - 2.0 ** -39) < np.sqrt((t ** 2).sum()) <= 1.75 and abs((q ** 2).sum() - 1.0) < 1e-15
    assert not DR.mutated([1.0, 0, 0, 0], [0.0, 0, 0], [0.5] * 6, 2.0, 0.1, 1.75)[2]
    np.testing.assert_array_equal(np.concatenate(DR.mutated([1.0, 0, 0, 0], [0.0, 0, 0], [0.5] * 6, 2.0, 0.1, 1.75)[:2]), [1.0, 0, 0, 0, 0, 0, 0])
    # chain 0 round 0 is the relaxation
    alone = relax(x, lv, **budget)
    first = r['chains'][0]['first']
    for k in ('pos', 'terms', 'terms_in', 'grad_in', 'n_pairs', 'n_steps', 'n_evals', 'status'):
        np.testing.assert_array_equal(first[k], alone[k], err_msg=k)
    np.testing.assert_array_equal(np.concatenate([first['q'], first['t']]), alone['transform'])
    one = dock(x, lv, draws[:1, :1], **budget)
    for k in ('pos', 'terms', 'terms_in', 'grad_in', 'n_pairs', 'n_steps', 'n_evals', 'status', 'transform'):
        np.testing.assert_array_equal(one[k], alone[k], err_msg=k)
    # the best never rises with more rounds or more chains on a prefix of the draws
    e = lambda res: RR.energy(res['terms'], W)
    fewer_rounds, fewer_chains = dock(x, lv, draws[:, :2], **budget), dock(x, lv, draws[:2], **budget)
    assert e(r) <= e(fewer_rounds) <= e(dock(x, lv, draws[:, :1], **budget)) and e(r) <= e(fewer_chains) <= e(one) <= RR.energy(alone['terms'], W)
    for k in range(3):
        assert r['chains'][k]['history'][:2] == fewer_rounds['chains'][k]['history']
    np.testing.assert_array_equal(r['chain_terms'][:2], fewer_chains['chain_terms'])
    np.testing.assert_array_equal(r['chain_transform'][:2], fewer_chains['chain_transform'])
    print(f'1h36 shifted 1.5 A: relaxation {RR.energy(alone["terms"], W):.4f}, search {e(r):.4f} by chain {r["best_chain"]}, {clamped} chains capped')


def test_redocking_finds_the_planted_pose_that_the_relaxation_alone_misses():
    _, _, _, lpos, lv = fixture()
    star = relax(lpos, lv, max_steps=200)
    x_star, e_star = star['pos'], RR.energy(star['terms'], W)
    copies = redocking_copies(x_star, lv)
    assert len(copies) >= 3
    for g, x in enumerate(copies):
        alone = relax(x, lv)
        r = dock(x, lv, np.random.default_rng(REDOCK_SEED).random((16, 17, 7)))
        e = np.asarray([ch['inter'] for ch in r['chains']])
        print(f'copy {g}: start {rmsd(x, x_star):.3f} A; the relaxation alone ends {rmsd(alone["pos"], x_star):.3f} A from x* at '
              f'{RR.energy(alone["terms"], W):.4f}; the search {rmsd(r["pos"], x_star):.4f} A at {e.min():.4f} (E* {e_star:.4f}), chain '
              f'{r["best_chain"]}, {int((e < e.min() + 0.5).sum())} of 16 chains agree, {r["n_evals"]} evaluations')
        assert rmsd(alone['pos'], x_star) > 2.0, g
        assert rmsd(r['pos'], x_star) <= 0.25, g


def test_the_library_exports_td_score_dock_and_refuses_bad_arguments():
    lib = capi.load_library()
    assert hasattr(lib, 'td_score_dock') and len(capi.SIGNATURES['td_score_dock'][1]) == 47
    assert lib.td_abi_version() == capi.ABI_VERSION == 5
    assert (capi.DOCK_CHAINS, capi.DOCK_ROUNDS, capi.DOCK_AMPLITUDE, capi.DOCK_TEMPERATURE) == (DR.N_CHAINS, DR.N_ROUNDS, DR.AMPLITUDE, DR.TEMPERATURE)
    assert (DR.N_CHAINS, DR.N_ROUNDS, DR.AMPLITUDE, DR.TEMPERATURE, capi.DOCK_DRAWS) == (16, 16, 2.0, 1.2, DR.DRAWS)
    assert capi.DOCK_KEYS == DR.KEYS and (capi.DOCK_MAX_CHAINS, capi.DOCK_MAX_ROUNDS) == (64, 256)
    doc = ' '.join(capi.score_dock.__doc__.split())
    assert ("a rigid-body global search under this project's heuristic score, not AutoDock Vina's ``dock``: three translations and three "
            'rotations, no torsions') in doc
    cz = np.asarray(CLASS_Z, np.int32)
    dbl = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    rs, w = np.ascontiguousarray(RSUM.reshape(-1)), np.asarray(W)

    def call(weights=w, max_steps=64, max_evals=257, max_shift=3.0, cutoff=8.0, n_chains=16, n_rounds=16, amplitude=2.0, temperature=1.2):
        # an empty pack and an empty pocket: every refusal comes before anything touches a device
        return lib.td_score_dock(None, None, None, 0, 0, 0, cz.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), cz.size, None, None, None, None,
                                 None, 0, 40, cutoff, 1.75, dbl(rs), None, 0, None, None if weights is None else dbl(weights), max_steps,
                                 max_evals, max_shift, n_chains, n_rounds, amplitude, temperature, *([None] * 18))

    for kw, word in ((dict(n_chains=0), b'n_chains'), (dict(n_chains=65), b'n_chains'), (dict(n_chains=-1), b'n_chains'), (dict(n_rounds=-1), b'n_rounds'),
                     (dict(n_rounds=257), b'n_rounds'), (dict(amplitude=0.0), b'amplitude'), (dict(amplitude=-2.0), b'amplitude'),
                     (dict(amplitude=float('nan')), b'amplitude'), (dict(amplitude=float('inf')), b'amplitude'), (dict(temperature=0.0), b'temperature'),
                     (dict(temperature=-1.0), b'temperature'), (dict(temperature=float('nan')), b'temperature'),
                     (dict(temperature=float('inf')), b'temperature'), (dict(max_shift=0.0), b'max_shift'), (dict(max_shift=float('nan')), b'max_shift'),
                     (dict(max_steps=-1), b'max_steps'), (dict(max_evals=0), b'max_evals'), (dict(weights=None), b'null'),
                     (dict(weights=np.asarray([1, 2, np.inf, 0, 0.0])), b'weights'), (dict(cutoff=0.0), b'cutoff')):
        assert call(**kw) == -1 and word in lib.td_last_error(), kw            # TD_EINVAL


def test_every_refusal_of_the_binding():
    c = IR.build_case(3, 20, [4, 6])
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt)
    pack = (t(c['pos'], torch.float32), t(c['v'], torch.int64), t(c['ptr'], torch.int32), CLASS_Z, AROMATIC)
    pocket = (t(c['ppos'], torch.float32), t(c['pelem'], torch.int32), t(c['pkind'], torch.int32), t(c['prole'], torch.int32), 40, RSUM)
    good = torch.rand(1, 2, 2, 2, 7, dtype=torch.float64)
    for kw, match in ((dict(n_chains=0), 'n_chains'), (dict(n_chains=65), 'n_chains'), (dict(n_chains=2.5), 'n_chains'), (dict(n_rounds=-1), 'n_rounds'),
                      (dict(n_rounds=257), 'n_rounds'), (dict(n_rounds=0.5), 'n_rounds'), (dict(amplitude=0.0), 'amplitude'),
                      (dict(amplitude=float('inf')), 'amplitude'), (dict(temperature=0.0), 'temperature'), (dict(temperature=float('nan')), 'temperature'),
                      (dict(max_shift=0.0), 'max_shift'), (dict(max_steps=-1), 'max_steps'), (dict(max_evals=0), 'max_evals'),
                      (dict(cutoff=-1.0), 'cutoff'), (dict(bond_ptr=torch.zeros(3, dtype=torch.int64)), 'come together'),
                      (dict(n_chains=2, n_rounds=1, draws=good[:, :, :1]), 'draws'), (dict(n_chains=2, n_rounds=1, draws=good.float()), 'draws'),
                      (dict(n_chains=2, n_rounds=1, draws=good.numpy()), 'draws'), (dict(n_chains=2, n_rounds=1, draws=good + 1.0), r'\[0, 1\)'),
                      (dict(n_chains=2, n_rounds=1, draws=-good - 0.1), r'\[0, 1\)')):
        with pytest.raises(ValueError, match=match):
            capi.score_dock(*pack, *pocket, W, **kw)
    with pytest.raises(ValueError, match='weights'):
        capi.score_dock(*pack, *pocket, W[:4])
    big = IR.build_case(3, 20, [4, 513])
    with pytest.raises(ValueError, match='at most 512'):
        capi.score_dock(t(big['pos'], torch.float32), t(big['v'], torch.int64), t(big['ptr'], torch.int32), CLASS_Z, AROMATIC, *pocket, W)
    for kw in (dict(), dict(n_chains=2, n_rounds=1, draws=good)):
        with pytest.raises(RuntimeError, match='HIP device'):                   # valid arguments: only the device is missing
            capi.score_dock(*pack, *pocket, W, **kw)
    a, b = (capi._dock_inputs(3, 2, 2.0, 1.2, seed, None, 1, 2, torch.device('cpu'))[4] for seed in (4, 4))
    assert a.shape == (1, 2, 3, 3, 7) and a.dtype == torch.float64 and torch.equal(a, b) and bool(((a >= 0) & (a < 1)).all())
    assert not torch.equal(a, capi._dock_inputs(3, 2, 2.0, 1.2, 5, None, 1, 2, torch.device('cpu'))[4])


def hand_outputs():
    """one frame of four molecules of two atoms and three chains, one molecule refused by the kernel"""
    unit = 1 << 24
    bad = [SR.INT64_MIN] * 5
    terms_in = np.asarray([[[0, 0, 4 * unit, 0, 0], [unit, 0, 0, 0, 0], [0, 0, 0, 0, unit], bad]], np.int64)
    terms_min = np.asarray([[[0, 0, 2 * unit, 0, 0], [unit, 0, 0, 0, 0], [0, 0, 0, 0, 2 * unit], bad]], np.int64)
    terms = np.asarray([[[0, 0, unit, 0, 0], [2 * unit, 0, 0, 0, 0], [0, 0, 0, 0, 4 * unit], bad]], np.int64)
    chain_terms = np.zeros((1, 4, 3, 5), np.int64)
    chain_terms[0, 0, :, 2] = [2 * unit, unit, unit]                             # inter 2 w2, w2, w2: the first of the lowest is chain 1, two agree
    chain_terms[0, 1, :, 0] = [unit, 2 * unit, unit]                             # w0 < 0: chain 1 wins, all within 0.5
    chain_terms[0, 2, :, 4] = [4 * unit, 2 * unit, 0]                            # w4 = -0.587: chain 0 wins, the others are 1.17 and 2.35 above
    chain_terms[0, 3] = SR.INT64_MIN
    transform = np.zeros((1, 4, 7))
    transform[..., 0] = 1.0
    pos_in = np.zeros((1, 8, 3), f32)
    pos = pos_in.copy()
    pos[0, 0:2] += f32([3.0, 0.0, 4.0])                                          # moved by 5
    pos[0, 4] += f32([0.0, 2.0, 0.0])                                            # one of two atoms moved by 2: RMSD sqrt(2)
    n_rot, status = np.asarray([[2, 0, 1, -1]]), np.asarray([[5, 1, 2, -1]])
    raw = dict(pos=pos, terms_in=terms_in, terms=terms, n_rot=n_rot, n_steps=np.asarray([[40, 9, 70, 0]]), n_evals=np.asarray([[90, 10, 300, 0]]),
               status=status, transform=transform, best_chain=np.asarray([[1, 1, 0, 0]]), chain_terms=chain_terms)
    raw_min = dict(terms_in=terms_in, terms=terms_min, n_rot=n_rot, status=status, transform=transform)
    return raw, raw_min, pos_in


def test_dock_report_arithmetic_merge_and_the_exclusion_of_refused_molecules():
    raw, raw_min, pos_in = hand_outputs()
    w = np.asarray(quality.SCORE_WEIGHTS)
    rot = np.asarray([1 + 0.117, 1.0, 1.0585])
    before = np.asarray([4 * w[2], w[0], w[4]]) / rot
    middle = np.asarray([2 * w[2], w[0], 2 * w[4]]) / rot
    after = np.asarray([w[2], 2 * w[0], 4 * w[4]]) / rot
    rep = quality.DockReport.from_outputs(raw, raw_min, np.ones((1, 4), bool), pos_in, [2, 2, 2, 2])
    np.testing.assert_array_equal(rep.n_included, [3])
    np.testing.assert_array_equal(rep.scored, [[True, True, True, False]])
    for got, want in ((rep.scores_in, before), (rep.scores_min, middle), (rep.scores, after)):
        np.testing.assert_allclose(got[0, :3], want, rtol=1e-15)
        assert np.isnan(got[0, 3])
    assert rep.n_samples == 4 and rep.sum_ref is None and rep.sum_evals[0] == 400
    np.testing.assert_allclose(rep.sum_agree, [2 / 3 + 1.0 + 1 / 3], rtol=1e-15)
    s = rep.summary(0)
    assert list(s) == ['mean_score', 'median_score', 'best_score', 'mean_score_min', 'median_score_min', 'best_score_min', 'mean_score_dock',
                       'median_score_dock', 'best_score_dock', 'mean_gain_dock', 'share_negative_dock', 'mean_rmsd_dock', 'chains_agree',
                       'mean_evals_dock']
    for tag, x in (('', before), ('_min', middle), ('_dock', after)):
        np.testing.assert_allclose([s['mean_score' + tag], s['median_score' + tag], s['best_score' + tag]], [x.sum() / 3, np.median(x), x.min()],
                                   rtol=1e-15)
    np.testing.assert_allclose(s['mean_gain_dock'], (middle - after).sum() / 3, rtol=1e-14)
    np.testing.assert_allclose([s['mean_rmsd_dock'], s['chains_agree'], s['mean_evals_dock']], [(5.0 + np.sqrt(2.0)) / 3, 2 / 3, 400 / 3], rtol=1e-15)
    assert s['share_negative_dock'] == 2 / 3 and len(rep.lines(0)) == len(s)
    # with the known ligand: the share strictly below its docked score
    ref = quality.DockReport.from_outputs(raw, raw_min, np.ones((1, 4), bool), pos_in, [2, 2, 2, 2], ref_score=float(after[1]))
    r = ref.summary(0)
    assert r['ref_score_dock'] == after[1] and r['better_than_ref_dock'] == 1 / 3 and list(r)[-2:] == ['ref_score_dock', 'better_than_ref_dock']
    # an excluded molecule, and merged over two pockets: the sums add, the per-molecule values join
    part = quality.DockReport.from_outputs(raw, raw_min, np.asarray([[True, False, True, True]]), pos_in, [2, 2, 2, 2])
    both = quality.DockReport.merged([rep, part])
    union = np.concatenate([after, after[[0, 2]]])
    b = both.summary(0)
    assert both.scores.shape == (1, 8) and both.n_samples == 8 and both.n_included[0] == 5
    np.testing.assert_allclose([b['median_score_dock'], b['mean_score_dock'], b['mean_evals_dock'], b['chains_agree']],
                               [np.median(union), union.sum() / 5, 790 / 5, (2.0 + 1.0) / 5], rtol=1e-14)
    with pytest.raises(ValueError, match='reference ligand'):
        quality.DockReport.merged([rep, ref])
    none = quality.DockReport.from_outputs(raw, raw_min, np.zeros((1, 4), bool), pos_in, [2, 2, 2, 2])
    assert all(x != x for x in none.summary(0).values()) and none.lines(0)[0] == 'mean_score:\tNone'


@pytest.fixture
def dock_binding(relax_binding, monkeypatch):  # noqa: F811
    """relax_binding, and capi.score_dock patched by its restatement too"""
    def binding(*a, **kw):
        relax_binding.append(('score_dock', kw.get('check')))
        return DR.torch_score_dock(*a, **kw)

    monkeypatch.setattr(capi, 'score_dock', binding)
    return relax_binding


SEARCH = dict(n_chains=2, n_rounds=1, max_steps=4)


def expected_report(res, data, reference_ligand=None, seed=0, max_shift=3.0, **search):
    """(DockReport, raw outputs) of the final poses of a result through the restatements alone, with the binding's default draws"""
    search = dict(SEARCH, **search)
    sizes = [p.shape[1] for p in res[2]]
    pos = np.concatenate([p[-1:] for p in res[2]], 1).astype(f32)
    v = np.concatenate([x[-1:] for x in res[3]], 1)
    elem, kind, _ = quality.pocket_kinds(data.protein_atom_feature)
    pocket = (data.protein_pos.numpy(), elem, kind, IR.pocket_roles(data.protein_atom_feature.numpy()), 40, RSUM)
    draws = lambda B: capi._dock_inputs(search['n_chains'], search['n_rounds'], 2.0, 1.2, seed, None, 1, B, torch.device('cpu'))[4].numpy()
    ref_score = None
    if reference_ligand is not None:
        q = DR.score_dock(reference_ligand[0][None], reference_ligand[1][None], [0, len(reference_ligand[1])], CLASS_Z, AROMATIC, *pocket,
                          max_shift=max_shift, draws=draws(1), **search)
        ref_score = float(SR.energies(q['terms'], q['n_rot'])[2][0, 0])
    ptr = np.cumsum([0] + sizes)
    w = DR.score_dock(pos, v, ptr, CLASS_Z, AROMATIC, *pocket, max_shift=max_shift, draws=draws(len(sizes)), **search)
    m = RR.score_minimize(pos, v, ptr, CLASS_Z, AROMATIC, *pocket, max_steps=search['max_steps'], max_shift=max_shift)
    return quality.DockReport.from_outputs(w, m, np.ones(w['status'].shape, bool), pos, sizes, ref_score=ref_score), w, m


def assert_same(got, want):
    assert type(got) is type(want) and vars(got).keys() == vars(want).keys()
    for k, x in vars(want).items():
        if isinstance(x, np.ndarray):
            assert np.array_equal(getattr(got, k), x, equal_nan=x.dtype.kind == 'f'), k
    np.testing.assert_equal(got.summary(-1), want.summary(-1))


def test_sample_dock_the_pack_and_the_stateless_form(dock_binding):
    results, pockets, ligand = two_files()
    res, data = results[2], pockets[2]
    as_dict = {'data': data, 'pred_ligand_pos_traj': res[2], 'pred_ligand_v_traj': res[3]}
    want, w, m = expected_report(res, data, ligand)
    assert_same(quality.sample_dock(as_dict, reference_ligand=ligand, device='cpu', **SEARCH), want)
    s = want.summary(-1)
    assert (w['n_steps'] > 0).any() and 'ref_score_dock' in s and s['mean_score_dock'] <= s['mean_score_min'] <= s['mean_score']
    assert s['mean_gain_dock'] >= 0 and 0 < s['chains_agree'] <= 1 and s['mean_evals_dock'] >= 4
    pack = quality.SamplePack(as_dict, -1, device='cpu')
    got = pack.dock(quality.PocketSide(data, 'cpu'), seed=3, max_shift=0.5, **SEARCH)
    other, w3, _ = expected_report(res, data, seed=3, max_shift=0.5)
    assert_same(got, other)
    np.testing.assert_array_equal(pack.docked_pos.numpy(), w3['pos'])
    # a single frame only, and the refusal says why
    for call in (lambda: quality.sample_dock(as_dict, 'all', device='cpu'), lambda: quality.SamplePack(as_dict, 'all', device='cpu').dock(data),
                 lambda: quality.pocket_dock(data.protein_pos, data.protein_atom_feature, res[2][1].astype(f32), res[3][1],
                                             ligand_ptr=torch.tensor([0, 11], dtype=torch.int32), device='cpu')):
        with pytest.raises(ValueError, match='long-lived workgroups'):
            call()
    with pytest.raises(ValueError, match='carries no pocket'):
        quality.sample_dock(res, device='cpu')
    x = quality.pocket_dock(data.protein_pos, data.protein_atom_feature, res[2][1][-1].astype(f32), res[3][1][-1],
                            ligand_ptr=torch.tensor([0, 11], dtype=torch.int32), device='cpu', **SEARCH)
    alone = DR.score_dock(res[2][1][-1:].astype(f32), res[3][1][-1:], [0, 11], CLASS_Z, AROMATIC, data.protein_pos.numpy(),
                          *quality.pocket_kinds(data.protein_atom_feature)[:2], IR.pocket_roles(data.protein_atom_feature.numpy()), 40, RSUM,
                          draws=capi._dock_inputs(2, 1, 2.0, 1.2, 0, None, 1, 1, torch.device('cpu'))[4].numpy(), **SEARCH)
    np.testing.assert_array_equal(x.raw_terms, alone['terms'])
    np.testing.assert_array_equal(x.pos.numpy(), alone['pos'])
    np.testing.assert_array_equal(x.chain_transform, alone['chain_transform'])
    assert x.score.shape == x.score_min.shape == x.rmsd.shape == x.agree.shape == (1, 1) and x.score[0, 0] <= x.score_min[0, 0] <= x.score_in[0, 0]
    for doc in (quality.pocket_dock.__doc__, quality.sample_dock.__doc__, quality.Docked.__doc__, quality.DockReport.__doc__):
        assert ("rigid-body global search under this project's heuristic score, not AutoDock Vina's ``dock``: three translations and three "
                'rotations, no torsions') in ' '.join(doc.split())


def test_the_evaluate_tool_with_and_without_dock(dock_binding, tmp_path, monkeypatch, capsys):
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
    assert 'dock' not in plain and 'score_dock' not in [n for n, _ in dock_binding] and 'mean_score_dock' not in plain_stdout
    out = tool.main(base + ['--score', '--dock', '--dock_chains', '2', '--dock_rounds', '1', '--dock_seed', '5', '--min_steps', '4'])
    stdout = capsys.readouterr().out
    with open(tmp_path / 'samples' / 'eval_results' / 'quality.json') as f:
        written = json.load(f)
    # everything but the new section is what it was without the flag
    assert {k: x for k, x in written.items() if k != 'dock'} == json.loads(plain_bytes)
    assert stdout.startswith(plain_stdout[:plain_stdout.index('wrote ')]) and stdout.endswith(plain_stdout[plain_stdout.index('wrote '):])
    want = quality.DockReport.merged([expected_report(results[i], pockets[i], ligand, seed=5)[0] for i in (2, 10)])
    s = want.summary(-1)
    for k, x in s.items():
        assert out['dock'][k] == x and f'{k}:\t{x:.4f}' in stdout, k
    assert out['dock']['num_included'] == 7 and (out['dock']['n_chains'], out['dock']['n_rounds'], out['dock']['seed']) == (2, 1, 5)
    assert s['mean_score_dock'] <= s['mean_score_min'] <= s['mean_score'] == out['score']['mean_score'] and 'ref_score_dock' in s
    doc = ' '.join(tool.__doc__.split())
    assert "rigid-body global search under this project's heuristic score, not AutoDock Vina's ``dock``: three translations and three rotations, no torsions" in doc
    with pytest.raises(SystemExit, match='long-lived workgroups'):
        tool.main(base + ['--dock', '--eval_step', 'all'])


def test_the_export_tool_writes_docked_coordinates(dock_binding, tmp_path):
    results, pockets, _ = two_files()
    save_with_pockets(tmp_path, results, pockets)
    tool = load_tool('export_sdf')
    common = ['--sample_path', str(tmp_path), '--device', 'cpu']
    plain = tool.main(common + ['--out', str(tmp_path / 'plain')])
    out = tool.main(common + ['--out', str(tmp_path / 'docked'), '--docked', '--dock_chains', '2', '--dock_rounds', '1'])
    moved = 0
    for i in results:
        rep, w, _ = expected_report(results[i], pockets[i], max_steps=64)
        recs = molfile.read_sdf(str(tmp_path / 'docked' / f'result_{i}.sdf'))
        base = molfile.read_sdf(str(tmp_path / 'plain' / f'result_{i}.sdf'))
        assert out[f'result_{i}']['written'] == plain[f'result_{i}']['written'] == len(recs) == len(base)
        ptr = np.cumsum([0] + [p.shape[1] for p in results[i][2]])
        for m, b in zip(recs, base):
            g = int(m['name'].rsplit('_', 1)[1])
            assert m['name'] == b['name'] and m['bonds'] == b['bonds'] and 'score_dock' not in b['properties']
            assert m['properties']['score'] == f'{rep.scores_in[0, g]:.4f}' and m['properties']['score_min'] == f'{rep.scores_min[0, g]:.4f}'
            assert m['properties']['score_dock'] == f'{rep.scores[0, g]:.4f}'
            heavy = np.asarray(CLASS_Z)[results[i][3][g][-1]] != 1
            np.testing.assert_allclose(m['pos'], w['pos'][0, ptr[g]:ptr[g + 1]][heavy], atol=1e-4)
            moved += int((w['transform'][0, g] != [1.0, 0, 0, 0, 0, 0, 0]).any())
    assert moved > 0
    with pytest.raises(SystemExit, match='choose one'):
        tool.main(common + ['--out', str(tmp_path / 'both'), '--docked', '--relaxed'])
    with pytest.raises(SystemExit, match='carries no pocket'):
        from test_bonds_host import save_results
        (tmp_path / 'bare').mkdir()
        save_results(tmp_path / 'bare', results)
        tool.main(['--sample_path', str(tmp_path / 'bare'), '--device', 'cpu', '--out', str(tmp_path / 'none'), '--docked'])
