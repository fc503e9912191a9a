"""The HIP path at the edges of the LayerNorm fold (csrc/pack.cpp FoldedMlp), against fixtures the REAL reference produced
(oracle/make_golden_fold.py): edge MLPs whose folded scale M is 1e4 .. 1e12, and units just below / above the round-6 dead floor with
second-Linear columns of 1e5.  Needs an MI355X: ``-m gpu``; every call goes through the C ABI.

Tolerance, for every combination of the attention passes' arithmetic: as tests/test_gpu_weight_regimes.py, a forward output within
max(TOL_FWD, 2 r) of the float64 reference (r = |reference fp32 - reference float64|); against the fp32 reference, max(2 r, TOL_FWD + r)
-- what an output within TOL_FWD of the float64 values can be from the fp32 reference (on forward_fold_m1e12.npz the shipped path is 4.5e-6
from float64 in pred_ligand_pos and the fp32 reference 2.7e-6 on the other side: 7.1e-6 apart).  The fold's bugs these tests found
were 50 to 10^6 times that.  The layer-0 outputs, which have no float64 run, keep the rule of tests/test_gpu_weight_regimes.py.  The fold's decisions are read back through td_model_get_option ('fold_dead_units', 'fold_fp32_mlps')
and compared with a float64 restatement of its rules (tests/test_oracle_fold_edges.py)."""
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
from _tol import TOL_FWD, close, maxdiff
from test_gpu_weight_regimes import _args, _dev, _model
from test_oracle_fold_edges import FOLD_FIXTURES, fold_plan, fold_state_dict
from test_oracle_golden_r6 import regime_tolerance

COMBOS = ((1, 1, 1), (1, 0, 1), (1, 0, 0), (0, 0, 0))          # edge_key_split, edge_first_layer_f16, edge_second_layer_f16
KEYS = ('pred_ligand_pos', 'pred_ligand_v', 'final_h', 'final_ligand_h')
F16_MAX_M = 2.0 ** 16             # pack.cpp TD_F16_MAX_M: an attention MLP with a larger folded scale runs both layers in fp32


def _set(model, dev, split, l1, l2):
    nm = model._native(dev)
    nm.set_option('edge_key_split', split)
    nm.set_option('edge_first_layer_f16', l1)
    nm.set_option('edge_second_layer_f16', l2)
    return nm


def expected_decisions(sd):
    """(dead units over all 37 folded MLPs, attention MLPs moved off the f16 pieces) by the float64 restatement of the fold's rules"""
    plan = fold_plan(sd)
    return sum(d for _, _, d in plan), sum(1 for p, M, _ in plan if 'edge_pred_layer' not in p and M > F16_MAX_M)


@pytest.mark.parametrize('name', FOLD_FIXTURES)
def test_forward_fold_edges_vs_reference(name):
    """Every combination of the attention passes' arithmetic against the reference; the HIP-vs-float64 distance is printed per fixture and
    combination first (the precision-versus-M curve), then asserted."""
    dev = _dev()
    g = load_golden(name)
    sd = fold_state_dict(name)
    runs = {}
    for combo in COMBOS:
        model = _model(sd)
        _set(model, dev, *combo)
        p = model(*_args(g, dev), return_all=True)
        runs[combo] = p
        d64 = {k: maxdiff(p[k], g[k + '_f64']) for k in KEYS}
        r64 = {k: maxdiff(g[k], g[k + '_f64']) for k in KEYS}
        print(f'fold curve {name} split/f16 first/f16 second {combo}: HIP vs float64 ' +
              ' '.join(f'{k} {d64[k]:.3e} (reference {r64[k]:.3e})' for k in KEYS))
    for combo, p in runs.items():
        what = (name, 'split / f16 first / f16 second', combo)
        for k in KEYS:
            r64 = maxdiff(g[k], g[k + '_f64'])
            close(p[k], g[k], max(2.0 * r64, TOL_FWD + r64), what + (k,))
            close(p[k], g[k + '_f64'], max(TOL_FWD, 2.0 * r64), what + (k, 'vs float64'))
        close(p['layer_pred_ligand_v'][0], g['layer0_pred_ligand_v'], regime_tolerance(g, 'pred_ligand_v', TOL_FWD), what + ('layer 0 v',))
        close(p['layer_pred_ligand_pos'][0], g['layer0_pred_ligand_pos'], regime_tolerance(g, 'pred_ligand_pos', TOL_FWD), what + ('layer 0 pos',))


def _regime(name):
    from oracle import weights
    from oracle.make_golden import SEED
    return {'bench': lambda: weights.make_state_dict(2021), 'trained_g4': lambda: weights.trained_like_state_dict(SEED, 4.0),
            'trained_g8': lambda: weights.trained_like_state_dict(SEED, 8.0), 'ln_dead': lambda: weights.ln_dead_state_dict(SEED)}[name]()


@pytest.mark.parametrize('name', ['bench', 'trained_g4', 'trained_g8', 'ln_dead'] + FOLD_FIXTURES)
def test_fold_decisions_are_visible(name):
    """fold_dead_units / fold_fp32_mlps match the float64 restatement of the fold's rules.  The benchmark's weights and the round-6 regimes
    keep every attention MLP on the f16 pieces (the benchmarked path does not change); the fixtures above F16_MAX_M do not; the near-dead
    set counts exactly its negligible units dead.  Both names are read-only."""
    dev = _dev()
    sd = _regime(name) if not name.endswith('.npz') else fold_state_dict(name)
    dead, fp32 = expected_decisions(sd)
    nm = _model(sd)._native(dev)
    print(f'{name}: fold_dead_units {nm.get_option("fold_dead_units")} (expected {dead}), fold_fp32_mlps {nm.get_option("fold_fp32_mlps")} (expected {fp32})')
    assert nm.get_option('fold_dead_units') == dead and nm.get_option('fold_fp32_mlps') == fp32
    if name in ('bench', 'trained_g4', 'trained_g8', 'ln_dead', 'forward_fold_m1e4.npz', 'forward_fold_m1e12.npz'):
        assert fp32 == 0          # (1e12: its large-bias units are negligible, dead, and M is back to ~40)
    if name in ('forward_fold_m1e6.npz', 'forward_fold_m1e8.npz', 'forward_fold_m8e8.npz', 'forward_fold_near_dead.npz'):
        assert fp32 == 36
    for opt in ('fold_dead_units', 'fold_fp32_mlps'):
        with pytest.raises(RuntimeError, match='td_model_set_option failed'):
            nm.set_option(opt, 0)
    # the shipped defaults and the model options are unchanged by the fallback: it is per MLP, at pack time
    assert nm.get_option('edge_first_layer_f16') == 1 and nm.get_option('edge_second_layer_f16') == 1


@pytest.mark.parametrize('name', ['forward_fold_m1e8.npz', 'live_m1e12'])
def test_fallback_runs_the_fp32_layers(name):
    """With every attention MLP past F16_MAX_M the shipped defaults compute what the f16 options switched off compute, bit for bit.
    live_m1e12: fold_scale_state_dict(1e12) with the units' columns unscaled -- live units at M = 1e12, where the first Linear's power-of-two
    scale is clipped; its constants saturate the gate (no fixture: it is an input for the fold's decisions), the outputs stay finite."""
    from oracle import weights
    from oracle.make_golden import SEED
    dev = _dev()
    g = load_golden('forward_fold_m1e8.npz')
    sd = fold_state_dict(name) if name.endswith('.npz') else weights.fold_scale_state_dict(SEED, 1e12, scale_columns=False)
    outs = []
    for combo in ((1, 1, 1), (1, 0, 0)):
        model = _model(sd)
        nm = _set(model, dev, *combo)
        assert nm.get_option('fold_fp32_mlps') == 36
        outs.append(model(*_args(g, dev)))
    for k in ('pred_ligand_pos', 'pred_ligand_v', 'final_h'):
        assert torch.isfinite(outs[0][k]).all() and torch.equal(outs[0][k], outs[1][k]), (name, k)


def test_fold_refuses_a_live_unit_whose_scale_overflows():
    """A unit under the round-6 |gamma| floor whose second-Linear column is large is live (its dropped term would be ~1e-5 of the
    output); with a bias of 1e8 on |gamma| = 1e-10 it takes M to 1e18, whose square leaves the fp32 range: td_model_create refuses the
    model with a clear error instead of dropping the unit."""
    from oracle import weights
    from oracle.make_golden import SEED
    dev = _dev()
    sd = weights.make_state_dict(SEED)
    k = 'refine_net.base_block.2.x2h_layers.0.hv_func.net.'
    sd[k + '1.weight'][17] = 1e-10
    sd[k + '1.bias'][17] = 1e8
    sd[k + '3.weight'][:, 17] *= 1e5
    with pytest.raises(RuntimeError, match='LayerNorm'):
        _model(sd)._native(dev)
    sd[k + '3.weight'][:, 17] *= 1e-5          # the same unit with its ordinary column is negligible: dead, the model is accepted
    nm = _model(sd)._native(dev)
    assert nm.get_option('fold_dead_units') == 1 and nm.get_option('fold_fp32_mlps') == 0
