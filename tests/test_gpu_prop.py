"""Binding-affinity predictor on the GPU (td_prop_forward through targetdiff_amd.prop) against the real reference's fixtures
(tools/make_golden_prop.py): outputs and per-layer h, the k-NN graph bit for bit, both output forms, PropPredNetEnc on a final_h
embedding computed on the device, invariances, reruns and a pack of ~100 complexes.

Tolerances are relative: max |difference| / max(1, max |value|), because the pooled sums over a complex's ~600 nodes are large.
Against the reference's float64 run the fp32 reference itself is 4e-7 (gain 1) / 1e-6 (weights at 3x, biases at 6x) away; the GPU is
held to TOL_PROP = 2e-5 on outputs and per-layer h alike.
"""
import json

import numpy as np
import pytest
import torch

import _prop_ref as P
from _tol import close
from conftest import load_golden
from targetdiff_amd import prop

pytestmark = pytest.mark.gpu

TOL_PROP = 2e-5
DEV = 'cuda:0'
FIXTURES = ['prop_1h36.npz', 'prop_enc_final_h.npz', 'prop_enc_all.npz', 'prop_gain.npz', 'prop_unsorted.npz']
INPUTS = ('protein_pos', 'protein_feat', 'ligand_pos', 'ligand_feat', 'batch_protein', 'batch_ligand')


def rel_close(a, b, tol, what):
    b = torch.as_tensor(np.asarray(b, np.float64)) if not torch.is_tensor(b) else b.double().cpu()
    s = max(1.0, float(b.abs().max()))
    return close(a.double().cpu() / s, b / s, tol, what)


def model_for(g):
    if 'config' in g:
        cfg = json.loads(str(g['config']))
        m = prop.PropPredNetEnc(cfg, P.PROTEIN_FEAT_DIM, P.LIGAND_FEAT_DIM, cfg['enc_ligand_dim'], cfg['enc_node_dim'],
                                cfg['enc_graph_dim'], cfg['enc_feature_type'], output_dim=1)
    else:
        m = prop.PropPredNet(P.MODEL_CONFIG, P.PROTEIN_FEAT_DIM, P.LIGAND_FEAT_DIM)
    m.load_state_dict(P.make_state_dict(P.spec_of(g), int(g['seed']), float(g['gain']), float(g['bias_gain'])), strict=True)
    return m.to(DEV)


def inputs(g, dev=DEV):
    return [torch.from_numpy(np.ascontiguousarray(g[k])).to(dev) for k in INPUTS]


def enc_args(g, dev=DEV):
    t = lambda k: torch.from_numpy(g[k]).to(dev) if k in g else None
    return [t('enc_ligand'), t('final_h') if 'final_h' in g else t('enc_node'), t('enc_graph')]


def call(m, g, args, kind, extra=False):
    if isinstance(m, prop.PropPredNetEnc):
        return m(*args, kind, *enc_args(g), return_extra=extra)
    return m(*args, kind, return_extra=extra)


@pytest.mark.parametrize('name', FIXTURES)
def test_prop_against_reference(name):
    g = load_golden(name)
    m = model_for(g)
    args = inputs(g)
    kind = torch.from_numpy(g['output_kind']).to(DEV)
    out, extra = call(m, g, args, None, extra=True)
    assert torch.equal(extra['nbr'].cpu().long(), torch.from_numpy(g['nbr']).long()), 'k-NN graph differs from the fixture'
    if 'out_all_f64' in g:
        rel_close(out, g['out_all_f64'], TOL_PROP, f'{name} out [B, O] vs float64')
    if 'out_all' in g:
        rel_close(out, g['out_all'], TOL_PROP, f'{name} out [B, O] vs fp32 reference')
    if 'h_layers' in g:
        rows = torch.from_numpy(g['layer_rows'])
        rel_close(extra['h_layers'].cpu()[:, rows], g['h_layers'], TOL_PROP, f'{name} per-layer h')
    out_k = call(m, g, args, kind)
    assert out_k.shape == (len(g['output_kind']), 1)
    if 'out_kind_f64' in g:
        rel_close(out_k, g['out_kind_f64'], TOL_PROP, f'{name} out[kind] vs float64')
    if 'out_kind' in g:
        rel_close(out_k, g['out_kind'], TOL_PROP, f'{name} out[kind] vs fp32 reference')
    # the selected column is the [B, O] form's column, bit for bit
    assert torch.equal(out_k[:, 0], out[torch.arange(out.shape[0]), kind - 1])


def test_final_h_from_fetch_embedding_on_device():
    """ScorePosNet3D.fetch_embedding (HIP) -> PropPredNetEnc (HIP): the final_h embedding never leaves the device."""
    from oracle import weights
    from targetdiff_amd.models import ScorePosNet3D
    g = load_golden('prop_enc_final_h.npz')
    diff = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG), weights.PROTEIN_FEATURE_DIM, weights.LIGAND_FEATURE_DIM)
    diff.load_state_dict(weights.make_state_dict(2021), strict=False)
    diff = diff.to(DEV).eval()
    pp, pf, lp, lf, bp, bl = inputs(g)
    lv = torch.from_numpy(g['ligand_v']).to(DEV)
    emb = diff.fetch_embedding(pp, pf, bp, lp, lv, bl)
    final_h = emb['final_h']
    assert final_h.is_cuda
    rel_close(final_h, g['final_h'], TOL_PROP, 'fetch_embedding final_h')
    m = model_for(g)
    kind = torch.from_numpy(g['output_kind']).to(DEV)
    out = m(pp, pf, lp, lf, bp, bl, kind, None, final_h, None)
    rel_close(out, g['out_kind_f64'], TOL_PROP, 'affinity from the on-device final_h')


def test_rigid_motion_invariance():
    g = load_golden('prop_1h36.npz')
    m = model_for(g)
    pp, pf, lp, lf, bp, bl = inputs(g)
    base = m(pp, pf, lp, lf, bp, bl, None)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64))
    R = q.float().to(DEV)
    t = torch.tensor([4.0, -7.5, 2.25], device=DEV)
    moved = m(pp @ R.T + t, pf, lp @ R.T + t, lf, bp, bl, None)
    rel_close(moved, base, TOL_PROP, 'rotated + translated')


def test_permuting_complexes():
    g = load_golden('prop_1h36.npz')
    m = model_for(g)
    pp, pf, lp, lf, bp, bl = inputs(g)
    base = m(pp, pf, lp, lf, bp, bl, None)
    perm = torch.tensor([2, 0, 1], device=DEV)          # complex b -> position perm[b]
    out = m(pp, pf, lp, lf, perm[bp], perm[bl], None)
    # same complexes, same atoms in the same per-complex order: the same arithmetic, bit for bit
    assert torch.equal(out[perm], base)


def test_rerun_bit_identical():
    g = load_golden('prop_enc_final_h.npz')
    m = model_for(g)
    args = inputs(g)
    a, ea = call(m, g, args, None, extra=True)
    b, eb = call(m, g, args, None, extra=True)
    assert torch.equal(a, b) and torch.equal(ea['h_layers'], eb['h_layers']) and torch.equal(ea['final_h'], eb['final_h'])


def test_pack_of_100_complexes():
    """The fixture's three complexes inside a batch of 100 (1h36 with jittered ligands elsewhere): the same outputs."""
    g = load_golden('prop_1h36.npz')
    m = model_for(g)
    golden = P.fixture_complexes()
    cx = [P.complex_1h36(seed=s, jitter=0.5) for s in range(97)]
    at = 61
    cx[at:at] = golden
    b = P.batch_of(cx)
    args = [torch.from_numpy(np.ascontiguousarray(b[k])).to(DEV) for k in INPUTS]
    out = m(*args, None)
    assert out.shape == (100, 3) and torch.isfinite(out).all()
    rel_close(out[at:at + 3], g['out_all_f64'], TOL_PROP, 'golden complexes inside a pack of 100')
