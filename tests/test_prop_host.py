"""Binding-affinity predictor, CPU side: the float64 restatement (tests/_prop_ref.py) against every prop_*.npz fixture of the real
reference, the mirror's state_dict against the reference's, strict loading, refused configurations and the exported symbols."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import _prop_ref as P
from conftest import load_golden
from targetdiff_amd import prop

FIXTURES = ['prop_1h36.npz', 'prop_enc_final_h.npz', 'prop_enc_all.npz', 'prop_gain.npz', 'prop_unsorted.npz']
INPUTS = ('protein_pos', 'protein_feat', 'ligand_pos', 'ligand_feat', 'batch_protein', 'batch_ligand')


def _model_for(g):
    cfg = json.loads(str(g['config'])) if 'config' in g else P.MODEL_CONFIG
    if 'config' in g:
        m = prop.PropPredNetEnc(cfg, P.PROTEIN_FEAT_DIM, P.LIGAND_FEAT_DIM, cfg['enc_ligand_dim'], cfg['enc_node_dim'],
                                cfg['enc_graph_dim'], cfg['enc_feature_type'], output_dim=1)
    else:
        m = prop.PropPredNet(cfg, P.PROTEIN_FEAT_DIM, P.LIGAND_FEAT_DIM)
    return m, cfg


def _sd(g):
    return P.make_state_dict(P.spec_of(g), int(g['seed']), float(g['gain']), float(g['bias_gain']))


def _enc(g):
    return dict(enc_ligand=g.get('enc_ligand'), enc_node=g['final_h'] if 'final_h' in g else g.get('enc_node'),
                enc_graph=g.get('enc_graph'))


@pytest.mark.parametrize('name', FIXTURES)
def test_restatement_matches_reference(name):
    g = load_golden(name)
    m, cfg = _model_for(g)
    inp = {k: g[k] for k in INPUTS}
    sd = _sd(g)
    enc = _enc(g)
    # the reference's compose order (torch argsort, unstable) differs from the project's stable one only inside a complex: a
    # permutation of a complex's rows, which changes the k-NN tie rule and the order of sums, nothing else
    batch = np.concatenate([g['batch_protein'], g['batch_ligand']])
    ro, so = g['reference_order'], P.composed_order(g['batch_protein'], g['batch_ligand'])
    assert np.array_equal(np.sort(ro), np.arange(len(batch))) and np.array_equal(batch[ro], batch[so])
    for key, kind in (('out_all', None), ('out_kind', g['output_kind'])):
        if key in g:
            r = P.restate(sd, cfg, inp, kind, **enc)
            assert P.rel_err(r['out'], g[key]) < 2e-5, key
    for key, kind in (('out_all_f64', None), ('out_kind_f64', g['output_kind'])):
        if key in g:
            r = P.restate(sd, cfg, inp, kind, **enc)
            assert P.rel_err(r['out'], g[key]) < 1e-10, key
    r = P.restate(sd, cfg, inp, None, **enc)
    assert np.array_equal(r['nbr'], g['nbr'].astype(np.int64))
    if 'h_layers' in g:
        assert P.rel_err(r['h_layers'][:, g['layer_rows']], g['h_layers']) < 2e-5


@pytest.mark.parametrize('name', FIXTURES)
def test_state_dict_keys_and_shapes(name):
    g = load_golden(name)
    m, _ = _model_for(g)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == P.spec_of(g)


def test_load_state_dict_strict_round_trip():
    g = load_golden('prop_enc_final_h.npz')
    m, cfg = _model_for(g)
    sd = _sd(g)
    m.load_state_dict(sd, strict=True)
    m2, _ = _model_for(g)
    m2.load_state_dict(m.state_dict(), strict=True)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_get_model_matches_config_kind():
    cfg = {'model': P.enc_config()}
    assert type(prop.get_model(cfg, 27, P.LIGAND_FEAT_DIM)).__name__ == 'PropPredNetEnc'
    cfg = {'model': P.MODEL_CONFIG}
    m = prop.get_model(cfg, 27, P.LIGAND_FEAT_DIM)
    assert type(m).__name__ == 'PropPredNet' and m.output_dim == 3


@pytest.mark.parametrize('change', [dict(hidden_dim=128), dict(num_r_gaussian=32), dict(act_fn='silu'), dict(norm=True),
                                    dict(knn=65), dict(edge_dim=4)])
def test_unsupported_configs_raise(change):
    cfg = dict(P.MODEL_CONFIG)
    cfg['encoder'] = dict(cfg['encoder'], **change)
    with pytest.raises(NotImplementedError, match='got'):
        prop.PropPredNet(cfg, 27, P.LIGAND_FEAT_DIM)


def test_unsupported_hidden_channels_raise():
    with pytest.raises(NotImplementedError, match='got 128'):
        prop.PropPredNet(dict(P.MODEL_CONFIG, hidden_channels=128), 27, P.LIGAND_FEAT_DIM)


def test_holders_raise_in_forward():
    m = prop.PropPredNet(P.MODEL_CONFIG, 27, P.LIGAND_FEAT_DIM)
    with pytest.raises(RuntimeError, match='libtargetdiff_hip'):
        m.encoder.net[0](torch.zeros(1, 256))
    with pytest.raises(RuntimeError, match='CPU path'):
        m(torch.zeros(2, 3), torch.zeros(2, 27), torch.zeros(1, 3), torch.zeros(1, P.LIGAND_FEAT_DIM), torch.zeros(2, dtype=torch.long),
          torch.zeros(1, dtype=torch.long), None)


def test_library_exports_prop_symbols():
    from targetdiff_amd import capi
    lib = capi.LIB_PATH
    if not os.path.exists(lib):
        pytest.skip('library not built')
    out = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True, check=True).stdout
    for sym in ('td_prop_num_weights', 'td_prop_create', 'td_prop_destroy', 'td_prop_workspace_bytes', 'td_prop_forward'):
        assert f' T {sym}' in out, sym


def test_native_config_refuses_without_library_error():
    """td_prop_num_weights returns 0 for a configuration the kernels do not support (the C ABI's refusal)."""
    import ctypes
    from targetdiff_amd import capi
    lib = capi.load_library()
    c = capi.TdPropConfig(hidden_dim=128, num_layers=6, knn=48, num_r_gaussian=64, cutoff=10.0, protein_feat_dim=27,
                          ligand_feat_dim=30, enc_ligand_dim=0, enc_node_dim=0, enc_graph_dim=0, output_dim=3)
    assert lib.td_prop_num_weights(ctypes.byref(c)) == 0
    c.hidden_dim = 256
    m = prop.PropPredNet(P.MODEL_CONFIG, 27, 30)
    assert lib.td_prop_num_weights(ctypes.byref(c)) == sum(m.state_dict()[k].numel() for k in capi.prop_flat_key_order(6))
    h = ctypes.c_void_p()
    c.knn = 0
    w = np.zeros(10, np.float32)
    assert lib.td_prop_create(ctypes.byref(c), w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 10, ctypes.byref(h)) == -1
    assert b'unsupported' in lib.td_last_error()
