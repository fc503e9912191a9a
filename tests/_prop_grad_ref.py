"""Gradients of the binding-affinity predictor: the fixture cases of tools/make_golden_prop_grad.py, seeded projection directions, the
loss of the float64 restatement (_prop_ref.restate, differentiated by torch autograd) and a float64 Adam loop on it."""
from __future__ import annotations

import json
import zlib

import numpy as np
import torch

import _prop_ref as P

NDIR = 16                      # projection directions per parameter
SMALL = 4096                   # tensors of at most this many elements are stored in full
PROJ_SEED = 77


def directions(key, shape):
    """NDIR seeded unit Gaussian directions for the tensor `key` of `shape`: [NDIR, numel] float64."""
    g = torch.Generator().manual_seed(PROJ_SEED * 1_000_003 + zlib.crc32(key.encode()))
    d = torch.randn(NDIR, int(np.prod(shape)), generator=g, dtype=torch.float64)
    return d / d.norm(dim=1, keepdim=True)


def summarize(grads):
    """{key: gradient} -> arrays of the fixture: norm, projections and (small tensors) the full gradient, float64."""
    out = {}
    for k, g in grads.items():
        g = g.detach().double().reshape(-1)
        out[f'norm/{k}'] = np.float64(g.norm().item())
        out[f'proj/{k}'] = (directions(k, g.shape) @ g).numpy()
        if g.numel() <= SMALL:
            out[f'full/{k}'] = g.numpy()
    return out


# ------------------------------------------------------------------------------------------ fixture cases
CASES = {
    # name: (model, seed, gain, bias_gain, kind?, upstream gradient seed or None)
    'prop_grad_kind': ('net', 2024, 1.0, 1.0, True, None),
    'prop_grad_all3': ('net', 2024, 1.0, 1.0, False, 41),
    'prop_grad_enc_final_h': ('enc_final_h', 2025, 1.0, 1.0, True, None),
    'prop_grad_enc_all': ('enc_all', 2026, 1.0, 1.0, True, None),
    'prop_grad_gain': ('net', 2027, 3.0, 6.0, True, None),
}


def model_config(kind):
    if kind == 'net':
        return None
    if kind == 'enc_final_h':
        return P.enc_config()
    return P.enc_config(5, 16, 7, 'full')


def case_inputs(kind, golden):
    """(inp, output_kind [B], y [B], enc dict) of a case; enc features come from the committed prop fixtures."""
    inp = P.batch_of(P.fixture_complexes())
    B = 3
    y = np.random.RandomState(31).normal(6.0, 1.5, size=B).astype(np.float32)
    enc = {}
    if kind == 'net':
        out_kind = np.array([2, 1, 3], np.int64)
    else:
        out_kind = np.ones(B, np.int64)
    if kind == 'enc_final_h':
        enc['node'] = golden('prop_enc_final_h.npz')['final_h']
    elif kind == 'enc_all':
        g = golden('prop_enc_all.npz')
        enc = {'ligand': g['enc_ligand'], 'node': g['enc_node'], 'graph': g['enc_graph']}
    return inp, out_kind, y, enc


def upstream(seed, B, O):
    return np.random.RandomState(seed).normal(size=(B, O)).astype(np.float32)


def spec_for(kind):
    """state_dict (key, shape) list in the reference's order."""
    from targetdiff_amd import prop
    cfg = model_config(kind)
    if cfg is None:
        m = prop.PropPredNet(P.MODEL_CONFIG, P.PROTEIN_FEAT_DIM, P.LIGAND_FEAT_DIM)
    else:
        m = prop.PropPredNetEnc(cfg, P.PROTEIN_FEAT_DIM, P.LIGAND_FEAT_DIM, cfg['enc_ligand_dim'], cfg['enc_node_dim'],
                                cfg['enc_graph_dim'], cfg['enc_feature_type'], output_dim=1)
    return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]


def is_param(key):
    return not key.endswith('offset')


def restate_loss(sd, cfg, inp, out_kind, y, enc, up=None, trace=None):
    """Loss of the float64 restatement: MSE(out[kind], y), or sum(out * up) when `up` is given (no output_kind)."""
    r = P.restate(sd, cfg, inp, output_kind=None if up is not None else out_kind, enc_ligand=enc.get('ligand'),
                  enc_node=enc.get('node'), enc_graph=enc.get('graph'), trace=trace)
    out = r['out']
    if up is not None:
        return (out * torch.as_tensor(up, dtype=torch.float64)).sum(), out
    return torch.mean((out.view(-1) - torch.as_tensor(y, dtype=torch.float64)) ** 2), out


def restate_grads(sd32, cfg, inp, out_kind, y, enc, up=None):
    """float64 autograd of the restatement: (loss, out, {param key: gradient})."""
    sd = {k: v.detach().double().requires_grad_(is_param(k)) for k, v in sd32.items()}
    loss, out = restate_loss(sd, cfg, inp, out_kind, y, enc, up)
    keys = [k for k in sd if is_param(k)]
    grads = torch.autograd.grad(loss, [sd[k] for k in keys], allow_unused=True)
    return loss.detach(), out.detach(), {k: (g if g is not None else torch.zeros_like(sd[k])) for k, g in zip(keys, grads)}


def cfg_of(kind):
    cfg = model_config(kind)
    return P.MODEL_CONFIG if cfg is None else cfg


def load_case(name, golden):
    """Everything a test needs of a fixture case: (fixture, kind, cfg, sd32, inp, out_kind, y, enc, up)."""
    kind, seed, gain, bias_gain, use_kind, up_seed = CASES[name]
    g = golden(name + '.npz')
    inp, out_kind, y, enc = case_inputs(kind, golden)
    cfg = cfg_of(kind)
    sd32 = P.make_state_dict(P.spec_of(g), seed, gain, bias_gain)
    up = upstream(up_seed, 3, 3) if up_seed is not None else None
    return g, kind, cfg, sd32, inp, out_kind, y, enc, up


def fixture_json(name):
    return json.dumps(CASES[name])
