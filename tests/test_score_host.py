"""CPU-only checks of the docking-style score ("Docking-style score"): a Vina-style score on this project's
heuristic typing, not AutoDock Vina's number.

  1. tests/_score_ref.py, the restatement the GPU tests compare td_score_report with, against hand-computed cases: single pairs at known
     surface distances, the strict cutoff, hydrogens, and the rotatable bonds of hand-built molecules;
  2. the library exports td_score_report and the ABI version stays 5;
  3. the 1h36 pocket and its docked ligand, docked and shifted, against figures computed with an independent numpy prototype;
  4. quality.ScoreReport's arithmetic, ``merged`` over two pockets and the exclusion of the molecules the kernel refused;
  5. quality.sample_score, tools/evaluate_samples.py --score and tools/export_sdf.py --max-score / --sort-by-score with the bindings
     patched by the restatements.
"""
import json
import math

import numpy as np
import pytest
import torch

import _bonds_ref as BR
import _interactions_ref as IR
import _pocket_ref as PR
import _score_ref as SR
from conftest import load_golden
from targetdiff_amd import capi, quality
from test_bonds_host import load_tool
from test_interactions_host import typed_pocket, typed_result
from test_pocket_host import save_with_pockets
from test_sample_pack_host import numpy_binding  # noqa: F401  (the fixture that patches the other bindings)

f32 = np.float32
CLASS_Z = quality.class_atomic_numbers('add_aromatic')
AROMATIC = BR.CLASS_AROMATIC
H, C, N, O = 0, 1, 3, 5                                                         # classes of 'add_aromatic'
PH, PC, PN, PO = 0, 1, 2, 3                                                     # protein element indices
UNIT = 2.0 ** 24


def one_molecule(lpos, lcls, ppos, pelem, prole, rsum=None, **kw):
    """the restatement on one frame of one molecule and a hand-built pocket of one kind"""
    n_p = len(ppos)
    r = SR.score_report(np.asarray(lpos, f32)[None], np.asarray(lcls, np.int64)[None], [0, len(lcls)], CLASS_Z, AROMATIC,
                        np.asarray(ppos, f32).reshape(n_p, 3), np.asarray(pelem, np.int32), np.zeros(n_p, np.int32),
                        np.asarray(prole, np.int32), 40, SR.radius_sums() if rsum is None else rsum, **kw)
    return r['terms'][0, 0], int(r['n_pairs'][0, 0]), r


def test_the_constants_are_the_issue_s_and_the_two_tables_agree():
    assert quality.SCORE_WEIGHTS == SR.WEIGHTS == (-0.035579, -0.005156, 0.840245, -0.035069, -0.587439)
    assert quality.SCORE_ROT_WEIGHT == SR.ROT_WEIGHT == 0.0585 and quality.SCORE_CUTOFF == 8.0
    assert quality.SCORE_LIGAND_RADII == SR.LIGAND_RADII == (0, 1.9, 1.8, 1.7, 1.5, 2.1, 2.0, 1.8)
    assert quality.SCORE_PROTEIN_RADII == SR.PROTEIN_RADII == (0, 1.9, 1.8, 1.7, 2.0, 2.0)
    rs = quality.score_radius_sums()
    np.testing.assert_array_equal(rs, SR.radius_sums())
    assert rs.shape == (8, 6) and rs[1, 1] == 1.9 + 1.9 and rs[3, 2] == 1.7 + 1.8 and ((rs > 0) & (rs <= 6)).all()
    assert quality.SCORE_TERM_NAMES == capi.SCORE_TERM_NAMES == SR.TERMS


def test_single_pairs_at_known_surface_distances():
    # a C - C pair at surface distance 0: radii of 2 A, the atoms 4 A apart, so r - rsum is exactly 0; both carbons are hydrophobic
    rsum = SR.radius_sums((0, 2.0, 1.8, 1.7, 1.5, 2.1, 2.0, 1.8), (0, 2.0, 1.8, 1.7, 2.0, 2.0))
    terms, pairs, r = one_molecule([[0, 0, 0]], [C], [[4, 0, 0]], [PC], [0], rsum)
    assert pairs == 1 and r['protein_role'][0] == IR.HYDROPHOBIC
    np.testing.assert_array_equal(terms, SR.fixed([1.0, math.exp(-2.25), 0.0, 1.0, 0.0]))
    assert terms[0] == terms[3] == 1 << 24 and terms[1] == round(math.exp(-2.25) * UNIT)
    # a ligand O (donor and acceptor by its valence deficit) and a protein donor N at d = -0.35: half a hydrogen bond, d^2 of repulsion
    terms, pairs, _ = one_molecule([[0, 0, 0]], [O], [[3.15, 0, 0]], [PN], [IR.DONOR])
    assert pairs == 1 and terms[3] == 0
    np.testing.assert_allclose(terms[[2, 4]] / UNIT, [0.1225, 0.5], atol=1e-6)
    np.testing.assert_allclose(terms[:2] / UNIT, [math.exp(-0.49), math.exp(-(3.35 / 2) ** 2)], atol=1e-6)
    # the same N without the donor bit, and an acceptor N against a ligand atom that only accepts... no hydrogen bond without a partner
    assert one_molecule([[0, 0, 0]], [O], [[3.15, 0, 0]], [PN], [0])[0][4] == 0
    assert one_molecule([[0, 0, 0]], [O], [[3.15, 0, 0]], [PN], [IR.ACCEPTOR])[0][4] > 0      # the O donates too
    # the hydrophobic term between its two ends, and zero from d = 1.5 on
    for r_, want in ((3.8 + 1.0, 0.5), (3.8 + 0.25, 1.0), (3.8 + 1.5, 0.0), (3.8 + 2.0, 0.0)):
        terms, _, _ = one_molecule([[0, 0, 0]], [C], [[r_, 0, 0]], [PC], [0])
        np.testing.assert_allclose(terms[3] / UNIT, want, atol=1e-6)
        assert terms[2] == 0 and terms[4] == 0
    # below d = -0.7 the hydrogen bond is whole
    assert one_molecule([[0, 0, 0]], [O], [[2.5, 0, 0]], [PN], [IR.DONOR])[0][4] == 1 << 24


def test_the_cutoff_is_strict_and_hydrogens_count_nowhere():
    just_inside = np.nextafter(f32(8), f32(0))
    assert one_molecule([[0, 0, 0]], [C], [[8, 0, 0]], [PC], [0])[1] == 0
    assert one_molecule([[0, 0, 0]], [C], [[just_inside, 0, 0]], [PC], [0])[1] == 1
    assert one_molecule([[0, 0, 0]], [C], [[4, 0, 0]], [PC], [0], cutoff=4.0)[1] == 0
    assert one_molecule([[0, 0, 0]], [C], [[4, 0, 0]], [PC], [0], cutoff=4.5)[1] == 1
    # a ligand H, a protein H (even one whose role is not -1), a class outside the table and a protein atom without a role
    terms, pairs, _ = one_molecule([[0, 0, 0]], [H], [[3, 0, 0]], [PC], [0])
    assert pairs == 0 and not terms.any()
    terms, pairs, _ = one_molecule([[0, 0, 0]], [C], [[3, 0, 0]], [PH], [0])
    assert pairs == 0 and not terms.any()
    assert one_molecule([[0, 0, 0]], [13], [[3, 0, 0]], [PC], [0])[1] == 0 and one_molecule([[0, 0, 0]], [C], [[3, 0, 0]], [PC], [-1])[1] == 0
    # of a C with its H beside a protein C with its H only the heavy pair counts; the H still makes the ligand N a donor
    terms, pairs, _ = one_molecule([[0, 0, 0], [1.0, 0, 0]], [C, H], [[4, 0, 0], [4, 1, 0]], [PC, PH], [0, 0])
    assert pairs == 1


def ring(cx=0.0, start=0.0):
    return [[cx + 1.5 * math.cos(start + k * math.pi / 3), 1.5 * math.sin(start + k * math.pi / 3), 0.0] for k in range(6)]


def test_rotatable_bonds_of_hand_built_molecules():
    rot = lambda pos, cls=None: SR.rotors(np.asarray(pos, f32), np.full(len(pos), C) if cls is None else np.asarray(cls), CLASS_Z, AROMATIC)
    chain = [[0, 0, 0], [1.5, 0, 0], [2.2, 1.3, 0], [3.7, 1.3, 0]]
    assert rot(chain[:2]) == 0                                                   # ethane-like
    assert rot(chain[:3]) == 0                                                   # propane-like: every bond has a terminal end
    assert rot(chain) == 1                                                       # butane-like: the middle bond
    assert rot(ring()) == 0                                                      # a ring bond: never
    assert rot(ring() + [[3.0, 0, 0], [3.7, 1.3, 0]]) == 1                        # a 6-ring with a 2-atom tail: the bond to the ring
    assert rot(ring() + ring(4.5, math.pi)) == 1                                 # two 6-rings joined by one bond
    # hydrogens are not heavy: a butane-like chain whose ends are H has no rotatable bond; with a class outside the table neither
    assert rot(chain, [H, C, C, H]) == 0 and rot(chain, [13, C, C, C]) == 0
    # a double bond does not rotate: the middle atoms 1.3 A apart
    assert rot([[0, 0, 0], [1.5, 0, 0], [2.8, 0, 0], [3.5, 1.3, 0]]) == 0
    m = SR.RR.molecule(np.asarray(ring() + ring(4.5, math.pi), f32), np.full(12, C), CLASS_Z, AROMATIC)
    assert len(m['o']) == 13 and sorted(m['ring'].tolist()) == [0] + [6] * 12 and (m['o'] == 1).all()


def test_the_library_exports_td_score_report_and_the_abi_version_stays():
    lib = capi.load_library()
    assert hasattr(lib, 'td_score_report') and 'td_score_report' in capi.SIGNATURES
    # the entry point as declared: 26 arguments (pack 8, class_aromatic, pocket 6, two cutoffs, rsum, three rotor inputs, four
    # outputs, the stream)
    assert len(capi.SIGNATURES['td_score_report'][1]) == 26
    assert lib.td_abi_version() == capi.ABI_VERSION == 5


def docked():
    p, l = load_golden('pocket_1h36.npz'), load_golden('ligand_1h36_docked.npz')
    cls = {'H': 0, 'C': 1, 'N': 3, 'O': 5, 'F': 7, 'P': 8, 'S': 10, 'Cl': 12, 'Br': 12}      # Br is outside the table: taken as Cl
    return p, l['pos'].astype(f32), np.asarray([cls[str(e)] for e in l['elements']], np.int64)


_CACHE = {}


def shifted():
    """{docked, shifted 1.5 A, shifted 4 A, far} of 1h36 through the restatement, once"""
    if 'w' not in _CACHE:
        p, lpos, lv = docked()
        elem, kind, names = quality.pocket_kinds(p['feat'])
        role = quality.pocket_roles(p['feat'])
        np.testing.assert_array_equal(role, IR.pocket_roles(p['feat']))
        poses = [lpos, lpos + np.asarray([1.5, 0, 0], f32), lpos + np.asarray([4, 0, 0], f32), lpos + f32(30)]
        w = SR.score_report(np.concatenate(poses)[None].astype(f32), np.concatenate([lv] * 4)[None], np.arange(5) * len(lv), CLASS_Z, AROMATIC,
                            p['pos'], elem, kind, role, 40, SR.radius_sums())
        _CACHE['w'] = (w, int((lv != 0).sum()))
    return _CACHE['w']


def test_the_1h36_pocket_and_its_docked_ligand_docked_and_shifted():
    w, heavy = shifted()
    np.testing.assert_array_equal(w['n_pairs'][0, [0, 1, 3]], [2045, 2006, 0])
    terms, inter, score = SR.energies(w['terms'], w['n_rot'])
    np.testing.assert_allclose(terms[0, 0], [89.64, 1588.51, 0.405, 103.95, 0.0], atol=0.006)
    np.testing.assert_allclose(inter[0, :3], [-14.68, 7.38, 206.8], atol=0.06)
    assert inter[0, 0] < inter[0, 1] < inter[0, 2] and inter[0, 0] < 0
    assert not w['terms'][0, 3].any() and inter[0, 3] == 0 and score[0, 3] == 0
    assert (w['n_rot'][0] == w['n_rot'][0, 0]).all() and w['n_rot'][0, 0] > 0  # a shift changes no bond
    assert inter[0, 0] < score[0, 0] < 0 and abs(score[0, 0]) < abs(inter[0, 0])
    np.testing.assert_array_equal(score, inter / (1 + 0.0585 * w['n_rot']))
    # the package's arithmetic is the restatement's
    for a, b in zip(quality.score_energies(w['terms'], w['n_rot']), (terms, inter, score)):
        np.testing.assert_array_equal(a, b)
    # the pack {docked, shifted 1.5, far} against the docked ligand
    pick = [0, 1, 3]
    raw = dict(terms=w['terms'][:, pick], n_pairs=w['n_pairs'][:, pick], n_rot=w['n_rot'][:, pick])
    rep = quality.ScoreReport.from_outputs(raw, np.ones((1, 3), bool), np.full((1, 3), heavy), ref_score=float(score[0, 0]))
    s = rep.summary(-1)
    assert s['better_than_ref'] == 0 and s['share_negative'] == 1 / 3 and s['no_pairs'] == 1 / 3
    assert s['ref_score'] == s['best_score'] == score[0, 0] and s['median_score'] == 0 and s['mean_pairs'] == (2045 + 2006) / 3
    np.testing.assert_allclose(s['mean_efficiency'], score[0, pick].sum() / heavy / 3, rtol=1e-12)


def hand_report(scale=1, ref_score=None):
    """two frames of four molecules, one of them refused by the kernel"""
    terms = np.zeros((2, 4, 5), np.int64)
    terms[0] = [[1 << 24, 2 << 24, 0, 3 << 24, 0], [0, 0, 1 << 24, 0, 0], [0, 0, 0, 0, 1 << 23], [SR.INT64_MIN] * 5]
    terms[1] = terms[0] * 2
    terms[1, 3] = SR.INT64_MIN
    terms[:, :3] *= scale
    raw = dict(terms=terms, n_pairs=np.asarray([[5, 1, 0, -1], [7, 2, 0, -1]]), n_rot=np.asarray([[2, 0, 1, -1], [2, 0, 1, -1]]))
    inc = np.asarray([[True, True, True, True], [True, False, True, True]])
    heavy = np.asarray([[10, 4, 0, 7]] * 2)
    return quality.ScoreReport.from_outputs(raw, inc, heavy, ref_score=ref_score), raw, inc


def test_score_report_arithmetic_merge_and_the_exclusion_of_refused_molecules():
    rep, raw, inc = hand_report()
    w = np.asarray(quality.SCORE_WEIGHTS)
    inter = np.asarray([w[0] + 2 * w[1] + 3 * w[3], w[2], 0.5 * w[4]])
    score = inter / (1 + 0.0585 * np.asarray([2, 0, 1]))
    np.testing.assert_array_equal(rep.n_included, [3, 2])                        # the refused molecule is out of both frames
    np.testing.assert_array_equal(rep.scored, [[True, True, True, False], [True, False, True, False]])
    np.testing.assert_allclose(rep.scores[0, :3], score, rtol=1e-15)
    assert np.isnan(rep.scores[0, 3]) and np.isnan(rep.scores[1, 1]) and rep.n_samples == 4 and rep.sum_ref is None
    np.testing.assert_array_equal(rep.sum_rotors, [3, 3])
    np.testing.assert_array_equal(rep.sum_pairs, [6, 7])
    np.testing.assert_array_equal(rep.n_no_pairs, [1, 1])
    np.testing.assert_array_equal(rep.n_efficiency, [2, 1])                      # a molecule without heavy atoms has no efficiency
    s = rep.summary(0)
    assert list(s) == ['mean_score', 'median_score', 'best_score', 'share_negative', 'mean_inter', 'mean_gauss1', 'mean_gauss2', 'mean_repulsion',
                       'mean_hydrophobic', 'mean_hbond', 'mean_rotors', 'mean_efficiency', 'mean_pairs', 'no_pairs']
    np.testing.assert_allclose([s['mean_score'], s['median_score'], s['best_score']], [score.sum() / 3, np.median(score), score.min()], rtol=1e-15)
    np.testing.assert_allclose([s['mean_inter'], s['mean_gauss1'], s['mean_hydrophobic'], s['mean_repulsion'], s['mean_hbond']],
                               [inter.sum() / 3, w[0] / 3, 3 * w[3] / 3, w[2] / 3, 0.5 * w[4] / 3], rtol=1e-15)
    assert s['share_negative'] == 2 / 3 and s['mean_rotors'] == 1 and s['mean_pairs'] == 2 and s['no_pairs'] == 1 / 3
    np.testing.assert_allclose(s['mean_efficiency'], (score[0] / 10 + score[1] / 4) / 2, rtol=1e-15)
    np.testing.assert_allclose(rep.summary(1)['mean_score'], (2 * inter[0] / (1 + 0.117) + 2 * inter[2] / 1.0585) / 2, rtol=1e-15)
    assert len(rep.lines(0)) == len(s) and rep.lines(0)[0].startswith('mean_score:\t')
    # with a reference: the share strictly below it
    ref, _, _ = hand_report(ref_score=float(score[0]))
    assert ref.summary(0)['ref_score'] == score[0] and ref.summary(0)['better_than_ref'] == 1 / 3      # only the hydrogen bond scores below it
    assert score[2] < score[0] < 0 < score[1] and ref.summary(1)['better_than_ref'] == 1        # twice the terms: both are below
    # merged over two pockets: the sums add, the per-molecule values join, the median is over the union
    other, _, _ = hand_report(scale=3)
    both = quality.ScoreReport.merged([rep, other])
    assert both.scores.shape == (2, 8) and both.n_samples == 8
    np.testing.assert_array_equal(both.n_included, [6, 4])
    union = np.concatenate([score, 3 * inter / (1 + 0.0585 * np.asarray([2, 0, 1]))])
    b = both.summary(0)
    np.testing.assert_allclose([b['median_score'], b['best_score'], b['mean_score']], [np.median(union), union.min(), union.sum() / 6], rtol=1e-14)
    assert b['median_score'] != (s['median_score'] + other.summary(0)['median_score']) / 2
    np.testing.assert_allclose(b['mean_inter'], (rep.sum_inter[0] + other.sum_inter[0]) / 6, rtol=1e-15)
    with pytest.raises(ValueError, match='reference ligand'):
        quality.ScoreReport.merged([rep, ref])
    refs = quality.ScoreReport.merged([ref, hand_report(scale=3, ref_score=-1.0)[0]])
    assert refs.summary(0)['ref_score'] == (score[0] - 1.0) / 2 and refs.n_ref[0] == 2
    single = quality.ScoreReport.merged([rep])
    np.testing.assert_array_equal(single.scores, rep.scores)
    # an empty frame: every mean is NaN, and prints as None
    none = quality.ScoreReport.from_outputs(raw, np.zeros((2, 4), bool), np.ones((2, 4)))
    assert all(x != x for x in none.summary(0).values()) and none.lines(0)[0] == 'mean_score:\tNone'


@pytest.fixture
def score_binding(numpy_binding, monkeypatch):  # noqa: F811
    """numpy_binding, and capi.score_report and capi.pocket_report patched by their restatements too"""
    def patched(name, fn):
        def binding(*a, **kw):
            numpy_binding.append((name, kw.get('check')))
            return fn(*a, **kw)
        return binding

    monkeypatch.setattr(capi, 'score_report', patched('score_report', SR.torch_score_report))
    monkeypatch.setattr(capi, 'pocket_report', patched('pocket_report', PR.torch_pocket_report))
    return numpy_binding


def expected_report(res, data, eval_step, reference_ligand=None, include=None, cutoff=8.0):
    """ScoreReport of a result through the restatement alone"""
    frames = slice(None) if eval_step == 'all' else slice(len(res[2][0]) - 1, None)
    sizes = [p.shape[1] for p in res[2]]
    pos = np.concatenate([p[frames] for p in res[2]], 1).astype(f32)
    v = np.concatenate([x[frames] for x in res[3]], 1)
    elem, kind, names = quality.pocket_kinds(data.protein_atom_feature)
    pocket = (data.protein_pos.numpy(), elem, kind, IR.pocket_roles(data.protein_atom_feature.numpy()), 40, SR.radius_sums(), cutoff)
    ref_score = None
    if reference_ligand is not None:
        q = SR.score_report(reference_ligand[0][None], reference_ligand[1][None], [0, len(reference_ligand[1])], CLASS_Z, AROMATIC, *pocket)
        ref_score = float(SR.energies(q['terms'], q['n_rot'])[2][0, 0])
    w = SR.score_report(pos, v, np.cumsum([0] + sizes), CLASS_Z, AROMATIC, *pocket)
    ptr = np.cumsum([0] + sizes)
    heavy = np.stack([[int((np.asarray(CLASS_Z)[v[s, a:b]] != 1).sum()) for a, b in zip(ptr[:-1], ptr[1:])] for s in range(v.shape[0])])
    inc = np.ones(w['n_pairs'].shape, bool) if include is None else include
    return quality.ScoreReport.from_outputs(w, inc, heavy, ref_score=ref_score), w


def assert_same(got, want):
    assert type(got) is type(want) and vars(got).keys() == vars(want).keys()
    for k, x in vars(want).items():
        if isinstance(x, np.ndarray):
            assert np.array_equal(getattr(got, k), x, equal_nan=x.dtype.kind == 'f'), k
    for s in range(want.num_frames):
        np.testing.assert_equal(got.summary(s), want.summary(s))


def two_files():
    results = {10: typed_result(5, [6, 9, 14], 3), 2: typed_result(6, [4, 11, 5, 1], 3)}
    pockets = {10: typed_pocket(1), 2: typed_pocket(2, 45)}
    ligand = (np.asarray(results[10][2][0][-1], f32), np.asarray(results[10][3][0][-1], np.int64))
    return results, pockets, ligand


def test_sample_score_and_the_pack_share_the_bond_graph(score_binding):
    results, pockets, ligand = two_files()
    for i, res in results.items():
        as_dict = {'data': pockets[i], 'pred_ligand_pos_traj': res[2], 'pred_ligand_v_traj': res[3]}
        for eval_step in (-1, 'all'):
            for ref in (None, ligand):
                want, w = expected_report(res, pockets[i], eval_step, ref)
                assert_same(quality.sample_score(as_dict, eval_step, reference_ligand=ref, device='cpu'), want)
        assert w['n_pairs'].max() > 0 and (w['terms'].sum((0, 1)) > 0).sum() >= 4
        pack = quality.SamplePack(as_dict, 'all', device='cpu')
        side = quality.PocketSide(pockets[i], 'cpu')
        del score_binding[:]
        pack.rings('complete')
        first = pack.score(side, 'complete', ligand)
        again = pack.score(side, 'complete', ligand, cutoff=3.0)
        # the pack's graph and ring sizes are made once; the reference's own graph per call; the pack is looked at once on the host
        names = [n for n, _ in score_binding]
        assert names.count('score_report') == 4 and names.count('bond_graph') == 1 + 2 and names.count('ring_report') == 1 + 1 + 2
        assert [c for n, c in score_binding if n == 'score_report'] == [None, False, None, False]
        inc = (pack.graph['n_fragments'] == 1).numpy()
        assert_same(first, expected_report(res, pockets[i], 'all', ligand, inc)[0])
        assert_same(again, expected_report(res, pockets[i], 'all', ligand, inc, cutoff=3.0)[0])
        assert (again.sum_pairs <= first.sum_pairs).all() and again.sum_pairs.sum() < first.sum_pairs.sum()
        with pytest.raises(ValueError, match='include is'):
            pack.score(side, include='stable')
    with pytest.raises(ValueError, match='carries no pocket'):
        quality.sample_score(results[2], device='cpu')
    x = quality.pocket_score(pockets[2].protein_pos, pockets[2].protein_atom_feature, res[2][1][-1].astype(f32), res[3][1][-1],
                             ligand_ptr=torch.tensor([0, 11], dtype=torch.int32), device='cpu')
    want, w = expected_report(res, pockets[2], -1)
    np.testing.assert_array_equal(x.raw_terms[0, 0], w['terms'][0, 1])
    np.testing.assert_array_equal(x.score[0, 0], want.scores[0, 1])
    assert x.n_rot[0, 0] == w['n_rot'][0, 1] and x.efficiency[0, 0] == x.score[0, 0] / x.heavy_atoms[0, 0]


def test_the_evaluate_tool_with_and_without_score(score_binding, tmp_path, monkeypatch, capsys):
    results, pockets, ligand = two_files()
    (tmp_path / 'samples').mkdir()
    save_with_pockets(tmp_path / 'samples', results, pockets)
    np.savez(tmp_path / 'ref.npz', ligand_pos=ligand[0], ligand_v=ligand[1])
    monkeypatch.chdir(tmp_path)
    tool = load_tool('evaluate_samples')
    base = ['--sample_path', 'samples', '--device', 'cpu', '--reference_npz', 'ref.npz', '--eval_step', 'all']
    capsys.readouterr()
    plain = tool.main(base + ['--pocket'])
    plain_stdout = capsys.readouterr().out
    with open(tmp_path / 'samples' / 'eval_results' / 'quality.json', 'rb') as f:
        plain_bytes = f.read()
    assert 'score' not in plain and 'score_report' not in [n for n, _ in score_binding] and 'mean_score' not in plain_stdout
    out = tool.main(base + ['--pocket', '--score'])
    stdout = capsys.readouterr().out
    # everything but the score section is what it was without the flag
    with open(tmp_path / 'samples' / 'eval_results' / 'quality.json') as f:
        written = json.load(f)
    assert {k: x for k, x in written.items() if k != 'score'} == json.loads(plain_bytes)
    assert stdout.startswith(plain_stdout[:plain_stdout.index('wrote ')]) and stdout.endswith(plain_stdout[plain_stdout.index('wrote '):])
    want = quality.ScoreReport.merged([expected_report(results[i], pockets[i], 'all', ligand)[0] for i in (2, 10)])
    s = want.summary(-1)
    for k, x in s.items():
        assert out['score'][k] == x and f'{k}:\t{x:.4f}' in stdout, k
    assert out['score']['num_included'] == 7 and out['score']['score_cutoff'] == 8.0 and len(out['score']['curve']) == 3
    assert out['score']['weights']['hbond'] == -0.587439 and out['score']['rot_weight'] == 0.0585
    assert 'better_than_ref' in s and 'ref_score' in s and out['score']['curve'][0] == want.summary(0)
    complete = tool.main(base + ['--score', '--score_cutoff', '3.0', '--include', 'complete'])
    parts = []
    for i in (2, 10):
        pack = quality.SamplePack(results[i], 'all', device='cpu')
        parts.append(expected_report(results[i], pockets[i], 'all', ligand, (pack.graph['n_fragments'] == 1).numpy(), cutoff=3.0)[0])
    np.testing.assert_equal({k: complete['score'][k] for k in s}, {k: (None if x != x else x) for k, x in quality.ScoreReport.merged(parts).summary(-1).items()})
    assert 'NOT AutoDock Vina' in tool.__doc__ and complete['score']['score_cutoff'] == 3.0


def test_the_export_tool_filters_and_sorts_by_score(score_binding, tmp_path, capsys):
    results, pockets, _ = two_files()
    save_with_pockets(tmp_path, results, pockets)
    tool = load_tool('export_sdf')
    from targetdiff_amd import molfile
    scores = {i: expected_report(results[i], pockets[i], -1)[0].scores[0] for i in results}
    bound = float(np.median(np.concatenate(list(scores.values()))))
    common = ['--sample_path', str(tmp_path), '--device', 'cpu']
    plain = tool.main(common + ['--out', str(tmp_path / 'plain')])
    assert all('score' not in m['properties'] for m in molfile.read_sdf(str(tmp_path / 'plain' / 'result_10.sdf')))
    out = tool.main(common + ['--out', str(tmp_path / 'kept'), '--max-score', repr(bound)])
    ordered = tool.main(common + ['--out', str(tmp_path / 'sorted'), '--sort-by-score'])
    both = tool.main(common + ['--out', str(tmp_path / 'both'), '--max-score', repr(bound), '--sort-by-score', '--unique'])
    total = 0
    for i, sc in scores.items():
        stem = f'result_{i}'
        keep = np.nonzero(sc <= bound)[0]
        total += len(keep)
        kept = molfile.read_sdf(str(tmp_path / 'kept' / f'{stem}.sdf'))
        assert [m['name'] for m in kept] == [f'sample_{g}' for g in keep] and out[stem]['written'] == out[stem]['max_score'] == len(keep)
        assert [m['properties']['score'] for m in kept] == [f'{sc[g]:.4f}' for g in keep]
        srt = molfile.read_sdf(str(tmp_path / 'sorted' / f'{stem}.sdf'))
        assert [m['name'] for m in srt] == [f'sample_{g}' for g in np.argsort(sc, kind='stable')] and ordered[stem]['written'] == plain[stem]['written'] == len(sc)
        got = [float(m['properties']['score']) for m in molfile.read_sdf(str(tmp_path / 'both' / f'{stem}.sdf'))]
        assert got == sorted(got) and len(got) == both[stem]['written'] <= len(keep) and all(x <= round(bound, 4) + 1e-4 for x in got)
    assert 0 < total < sum(len(sc) for sc in scores.values())
    with pytest.raises(SystemExit, match='carries no pocket'):
        from test_bonds_host import save_results
        (tmp_path / 'bare').mkdir()
        save_results(tmp_path / 'bare', results)
        tool.main(['--sample_path', str(tmp_path / 'bare'), '--device', 'cpu', '--out', str(tmp_path / 'none'), '--sort-by-score'])
