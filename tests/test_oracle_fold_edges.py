"""The oracle restatement against the fixtures of the LayerNorm fold's edges (oracle/make_golden_fold.py), and checks that those fixtures are
adversarial as designed: the folded scale M of the product's edge MLPs (csrc/pack.cpp FoldedMlp) spans 1e4 .. 1e12, and the near-dead set
has units on both sides of the round-6 dead floor whose term is far above the single-forward tolerance.  CPU only.

Tolerance: the rule of tests/test_oracle_golden_r6.py, max(2e-5, 2 x |fp32 reference - float64 reference|)."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import restatement as R
from oracle import weights
from oracle.make_golden import SEED, small_batch
from oracle.make_golden_fold import FOLD_SCALES
from _tol import TOL_FWD
from test_oracle_golden_r6 import KEYS, md, regime_tolerance

FOLD_FIXTURES = [f'forward_fold_m{tag}.npz' for tag, _ in FOLD_SCALES] + ['forward_fold_near_dead.npz']
DEAD_RATIO = 2.0 ** -30           # pack.cpp: a unit is dead when its dropped term is at most 2^-30 of the MLP's largest unit's


def fold_state_dict(name):
    if name == 'forward_fold_near_dead.npz':
        return weights.near_dead_state_dict(SEED)
    return weights.fold_scale_state_dict(SEED, dict((f'forward_fold_m{t}.npz', m) for t, m in FOLD_SCALES)[name])


def dropped_terms(sd, wk, w3k):
    """sqrt(hid) |gamma_n| max_o |w3[o, n]| per unit: what the unit's variable part can add to the MLP's output (|c_n / sigma| <= sqrt(hid))"""
    g = sd[wk].double().numpy()
    return math.sqrt(g.size) * np.abs(g) * np.abs(sd[w3k].double().numpy()).max(axis=0)


def fold_plan(sd):
    """float64 restatement of the fold's decisions per folded MLP: (prefix, M, number of dead units), with the dead-unit rule of pack.cpp"""
    out = []
    for p, wk, bk, w3k in weights.folded_ln_keys(sd):
        d = dropped_terms(sd, wk, w3k)
        dead = ~(d > DEAD_RATIO * d.max())
        a, b = np.abs(sd[wk].double().numpy()), sd[bk].double().numpy()
        r = np.where(dead, 0.0, b / np.where(dead, 1.0, a))
        out.append((p, (math.sqrt(a.size) + max(0.0, float(r.max()))) * (1.0 + 2.0 ** -10), int(dead.sum())))
    return out


@pytest.mark.parametrize('name', FOLD_FIXTURES)
def test_restatement_fold_edges_vs_reference(name):
    g = load_golden(name)
    b = small_batch()[0]
    out = R.model_forward(fold_state_dict(name), None, torch.from_numpy(g['protein_pos']), b.protein_atom_feature.float(),
                          b.protein_element_batch, torch.from_numpy(g['ligand_pos']), torch.from_numpy(g['ligand_v']), b.ligand_element_batch)
    for k in KEYS + ('final_ligand_h',):
        d, tol = md(out[k], g[k]), regime_tolerance(g, k, 2e-5)
        print(name, k, f'{d:.3e} (tolerance {tol:.1e}; restatement vs float64 {md(out[k], g[k + "_f64"]):.3e})')
        assert d <= tol, (name, k, d, tol)
        assert md(out[k], g[k + '_f64']) <= max(2e-5, 2.0 * md(g[k], g[k + '_f64'])), (name, k)


def round6_scales(sd):
    """M of every folded MLP under the round-6 rule (dead: |gamma_n| <= 2^-30 max |gamma|), float64"""
    out = []
    for _, wk, bk, _ in weights.folded_ln_keys(sd):
        a, b = np.abs(sd[wk].double().numpy()), sd[bk].double().numpy()
        live = a > weights.DEAD_FLOOR * a.max()
        out.append((math.sqrt(a.size) + max(0.0, float(np.where(live, b / np.where(live, a, 1.0), 0.0).max()))) * (1.0 + 2.0 ** -10))
    return out


@pytest.mark.parametrize('tag,m_target', FOLD_SCALES)
def test_fold_scale_fixture_reaches_its_m(tag, m_target):
    """All 37 folded MLPs (4 per layer, the edge gate) reach M = m_target within 1 % under the round-6 rule.  Under the product's rule a
    fold-scale unit counts as dead only where its term is negligible (< 1e-2 TOL_FWD): both units at 1e12, whose columns carry 4 / 1e4,
    and one unit at 8e8 where the column's largest entry happens to be small; every MLP below 1e12 keeps M = m_target."""
    sd = weights.fold_scale_state_dict(SEED, m_target)
    plan = fold_plan(sd)
    assert len(plan) == 9 * 4 + 1
    assert all(abs(M / m_target - 1.0) < 0.01 for M in round6_scales(sd)), tag
    at_target = 0
    for (p, M, dead), (_, wk, _, w3k) in zip(plan, weights.folded_ln_keys(sd)):
        d = dropped_terms(sd, wk, w3k)
        if dead:
            assert max(d[n] for n in weights.FOLD_SCALE_UNITS) < 1e-2 * TOL_FWD, (p, dead)
        at_target += abs(M / m_target - 1.0) < 0.01
    assert at_target == (0 if tag == '1e12' else 37), (tag, at_target)
    if m_target > 1e11:
        assert all(M < 1e2 and dead == 2 for _, M, dead in plan)
        live = fold_plan(weights.fold_scale_state_dict(SEED, m_target, scale_columns=False))
        assert all(abs(M / m_target - 1.0) < 0.01 and dead == 0 for _, M, dead in live)


def test_near_dead_fixture_is_adversarial():
    sd = weights.near_dead_state_dict(SEED)
    for p, wk, bk, w3k in weights.folded_ln_keys(sd):
        a = sd[wk].double().abs().numpy()
        floor = weights.DEAD_FLOOR * a.max()
        d = dropped_terms(sd, wk, w3k)
        below = [n for n in weights.NEAR_DEAD_UNITS if a[n] < floor]
        above = [n for n in weights.NEAR_DEAD_UNITS if a[n] > floor]
        assert sorted(below) == [20, 21, 22, 60, 61] and sorted(above) == [40, 41, 42], p
        # a unit the round-6 floor dropped whose term the outputs see, and a live one of the same size just above the floor
        # (the gate's single output column has some small entries: there only the larger of the two is asserted)
        assert max(d[20], d[21]) > 10 * TOL_FWD and d[42] > 10 * TOL_FWD, (p, d[20], d[21], d[42])
        if 'edge_pred_layer' not in p:
            assert min(d[20], d[21]) > 10 * TOL_FWD, (p, d[20], d[21])
        assert max(d[n] for n in weights.NEAR_DEAD_NEGLIGIBLE) < 1e-2 * TOL_FWD, p
    plan = fold_plan(sd)
    assert all(dead == len(weights.NEAR_DEAD_NEGLIGIBLE) for _, _, dead in plan)
    Ms = [M for _, M, _ in plan]
    assert 5e7 < min(Ms) and max(Ms) < 1e9, (min(Ms), max(Ms))


def test_bench_and_regime_weights_are_far_from_the_fold_edges():
    """The seeded weights of bench.py and the round-6 regimes: no MLP near the scales above, dead units only where gamma is exactly 0."""
    for sd, dead in ((weights.make_state_dict(SEED), 0), (weights.trained_like_state_dict(SEED, 4.0), 0),
                     (weights.trained_like_state_dict(SEED, 8.0), 0)):
        for p, M, n in fold_plan(sd):
            assert M < 1e3 and n == dead, (p, M, n)
    sd = weights.ln_dead_state_dict(SEED)
    for (p, M, n), (_, wk, _, _) in zip(fold_plan(sd), weights.folded_ln_keys(sd)):
        assert M < 1e4 and n == int((sd[wk] == 0).sum()), (p, M, n)        # (bias 0.5 on |gamma| ~1e-3: M ~ 1.6e3)
