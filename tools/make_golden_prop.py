"""Fixtures of the binding-affinity predictor from the REAL reference (build container only: needs the reference tree):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_prop.py

Imports models/property_pred/prop_model.py unmodified through oracle.reference_loader.  The reference's encoder asks for
knn_graph(..., flow='target_to_source'); oracle.shims.knn_graph serves 'source_to_target' only, so this script installs, in
sys.modules['torch_geometric.nn'], a wrapper that swaps the two rows of the shim's result (row 0 = the query node = dst).

  prop_1h36.npz        PropPredNet (3 outputs) on 1h36 + docked ligand, a synthetic complex and one of < 49 nodes; with output_kind
                       and without; per-layer h (forward hooks; the ligand rows and every row of the last complex), the graph
                       and the float64 run.
  prop_enc_final_h.npz PropPredNetEnc (final_h config) fed with final_h from the reference's ScorePosNet3D.fetch_embedding
                       (oracle/weights.py diffusion weights) on the same complexes.
  prop_enc_all.npz     PropPredNetEnc with all three enc_* features (widths 5 / 16 / 7).
  prop_gain.npz        PropPredNet with weights at 3x nn.Linear's range and biases at 6x: fp32 and float64 runs.
  prop_unsorted.npz    PropPredNet on the batch with its atoms interleaved across complexes (unsorted batch vectors).
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from oracle import reference_loader, shims, weights  # noqa: E402
from oracle.make_golden import build_reference_model  # noqa: E402
import _prop_ref as P  # noqa: E402

SEED = 2024


def knn_graph_t2s(x, k, batch=None, loop=False, flow='source_to_target', cosine=False, num_workers=1):
    ei = shims.knn_graph(x, k, batch=batch, loop=loop, cosine=cosine, num_workers=num_workers)
    return ei if flow == 'source_to_target' else ei.flip(0)


def load_prop():
    reference_loader.load()
    tgnn = sys.modules['torch_geometric.nn']
    wrapped = types.ModuleType('torch_geometric.nn')
    wrapped.__dict__.update(tgnn.__dict__)
    wrapped.knn_graph = knn_graph_t2s
    sys.modules['torch_geometric.nn'] = wrapped
    sys.modules['torch_geometric'].nn = wrapped
    import importlib
    return importlib.import_module('models.property_pred.prop_model')


def ed(d):
    return shims.EasyDict({k: ed(v) if isinstance(v, dict) else v for k, v in d.items()})


def build(pm, cfg, enc=None, seed=SEED, gain=1.0, bias_gain=1.0):
    if enc is None:
        model = pm.PropPredNet(ed(cfg), P.PROTEIN_FEAT_DIM, P.LIGAND_FEAT_DIM, output_dim=3)
    else:
        model = pm.PropPredNetEnc(ed(cfg), P.PROTEIN_FEAT_DIM, P.LIGAND_FEAT_DIM, cfg['enc_ligand_dim'], cfg['enc_node_dim'],
                                  cfg['enc_graph_dim'], cfg['enc_feature_type'], output_dim=1)
    spec = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    sd = P.make_state_dict(spec, seed, gain, bias_gain)
    model.load_state_dict(sd, strict=True)
    return model.eval(), spec


def tens(inp):
    return {k: torch.from_numpy(v) for k, v in inp.items()}


def run(model, inp, kind, enc=None, hooks=True):
    t = tens(inp)
    layers = []

    def hook(m, i, o):
        layers.append((i[0] + o).detach().clone())
    hs = [layer.register_forward_hook(hook) for layer in model.encoder.net] if hooks else []
    args = [t['protein_pos'], t['protein_feat'], t['ligand_pos'], t['ligand_feat'], t['batch_protein'], t['batch_ligand'], kind]
    if enc is not None:
        args += [enc.get('ligand'), to_reference_rows(inp, enc.get('node')), enc.get('graph')]
    with torch.no_grad():
        out = model(*args)
    for h in hs:
        h.remove()
    if not layers:
        return out, None
    # hooks see the reference's composed order (torch argsort, not stable on CPU): bring the rows into the project's order
    inv_ref = np.argsort(reference_order(inp))
    stable = P.composed_order(inp['batch_protein'], inp['batch_ligand'])
    return out, torch.stack(layers)[:, torch.from_numpy(inv_ref[stable])]


def run64(model, inp, kind, enc=None):
    m = model.double()
    t = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in tens(inp).items()}
    args = [t['protein_pos'], t['protein_feat'], t['ligand_pos'], t['ligand_feat'], t['batch_protein'], t['batch_ligand'], kind]
    if enc is not None:
        args += [None if enc.get(k) is None else enc[k].double() for k in ('ligand', 'node', 'graph')]
        args[8] = to_reference_rows(inp, args[8])
    with torch.no_grad():
        out = m(*args)
    model.float()
    return out


def reference_order(inp):
    return torch.cat([torch.from_numpy(inp['batch_protein']), torch.from_numpy(inp['batch_ligand'])]).argsort().numpy()


def to_reference_rows(inp, node_feature):
    """enc_node_feature rows in the project's composed order (stable: the order fetch_embedding's final_h has) -> the reference's
    composed order, so that the reference pairs every atom's h with that atom's own feature row.  PropPredNetEnc concatenates
    h_ctx and enc_node_feature row by row (prop_model.py:147-148), and h_ctx comes from an unstable argsort."""
    if node_feature is None:
        return None
    inv_stable = np.argsort(P.composed_order(inp['batch_protein'], inp['batch_ligand']))
    return node_feature[torch.from_numpy(inv_stable[reference_order(inp)])]


def edges(inp, k):
    order = P.composed_order(inp['batch_protein'], inp['batch_ligand'])
    pos = torch.from_numpy(np.concatenate([inp['protein_pos'], inp['ligand_pos']])[order])
    batch = torch.from_numpy(np.concatenate([inp['batch_protein'], inp['batch_ligand']])[order])
    ei = knn_graph_t2s(pos, k, batch, flow='target_to_source')
    nbr = np.full((pos.shape[0], k), -1, np.int32)
    fill = np.zeros(pos.shape[0], np.int64)
    for dst, src in ei.t().tolist():
        nbr[dst, fill[dst]] = src
        fill[dst] += 1
    return nbr


def layer_rows(inp):
    """Composed rows whose per-layer h the fixture keeps (a subset, to keep the fixture small): the ligand rows of every complex
    and every row of the last complex (fewer than k + 1 nodes: padded neighbour rows)."""
    order = P.composed_order(inp['batch_protein'], inp['batch_ligand'])
    batch = np.concatenate([inp['batch_protein'], inp['batch_ligand']])[order]
    is_lig = order >= len(inp['batch_protein'])
    return np.nonzero((batch == batch.max()) | is_lig)[0].astype(np.int64)


def save(name, **arrays):
    path = os.path.join(P.GOLDEN, name)
    np.savez_compressed(path, **arrays)
    print(f'wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB)')


def main():
    torch.set_num_threads(8)
    pm = load_prop()
    inp = P.batch_of(P.fixture_complexes())
    B = 3
    kind = torch.tensor([2, 1, 3])
    k = P.MODEL_CONFIG['encoder']['knn']
    rows = layer_rows(inp)
    common = dict(**inp, output_kind=kind.numpy(), reference_order=reference_order(inp), nbr=edges(inp, k), layer_rows=rows)

    # ---- 1: PropPredNet, both output forms, per-layer h, float64
    model, spec = build(pm, P.MODEL_CONFIG)
    out_all, layers = run(model, inp, None)
    out_kind, _ = run(model, inp, kind, hooks=False)
    out64 = run64(model, inp, None)
    save('prop_1h36.npz', **common, seed=SEED, gain=1.0, bias_gain=1.0, state_dict_spec=json.dumps(spec),
         out_all=out_all.numpy(), out_kind=out_kind.numpy(), out_all_f64=out64.numpy(), h_layers=layers[:, rows].numpy())
    print('   fp32 reference vs float64:', P.rel_err(out_all, out64))

    # ---- 2: PropPredNetEnc (final_h) with final_h from the reference diffusion model's fetch_embedding
    ref = reference_loader.load()
    diff, _ = build_reference_model(ref)
    g = np.random.RandomState(5)
    ligand_v = torch.from_numpy(g.randint(0, weights.LIGAND_FEATURE_DIM, size=len(inp['batch_ligand'])).astype(np.int64))
    t = tens(inp)
    with torch.no_grad():
        emb = diff.fetch_embedding(t['protein_pos'], t['protein_feat'], t['batch_protein'], t['ligand_pos'], ligand_v, t['batch_ligand'])
    final_h = emb['final_h'].detach()
    cfg = P.enc_config()
    kind1 = torch.ones(B, dtype=torch.long)              # output_dim 1: the only valid kind
    enc_common = dict(common, output_kind=kind1.numpy())
    model, spec = build(pm, cfg, enc=True, seed=SEED + 1)
    enc = {'node': final_h}
    out_kind, layers = run(model, inp, kind1, enc)
    out_all, _ = run(model, inp, None, enc, hooks=False)
    out64 = run64(model, inp, kind1, enc)
    save('prop_enc_final_h.npz', **enc_common, seed=SEED + 1, gain=1.0, bias_gain=1.0, state_dict_spec=json.dumps(spec),
         config=json.dumps(cfg), ligand_v=ligand_v.numpy(), final_h=final_h.numpy(), out_kind=out_kind.numpy(),
         out_all=out_all.numpy(), out_kind_f64=out64.numpy())

    # ---- 3: all three enc_* features
    cfg = P.enc_config(5, 16, 7, 'full')
    model, spec = build(pm, cfg, enc=True, seed=SEED + 2)
    r = np.random.RandomState(9)
    N = len(inp['batch_protein']) + len(inp['batch_ligand'])
    enc = {'ligand': torch.from_numpy(r.normal(size=(len(inp['batch_ligand']), 5)).astype(np.float32)),
           'node': torch.from_numpy(r.normal(size=(N, 16)).astype(np.float32)),
           'graph': torch.from_numpy(r.normal(size=(B, 7)).astype(np.float32))}
    out_kind, _ = run(model, inp, kind1, enc, hooks=False)
    out64 = run64(model, inp, kind1, enc)
    save('prop_enc_all.npz', **enc_common, seed=SEED + 2, gain=1.0, bias_gain=1.0, state_dict_spec=json.dumps(spec), config=json.dumps(cfg),
         enc_ligand=enc['ligand'].numpy(), enc_node=enc['node'].numpy(), enc_graph=enc['graph'].numpy(), out_kind=out_kind.numpy(),
         out_kind_f64=out64.numpy())

    # ---- 4: larger gains, float64 yardstick
    model, spec = build(pm, P.MODEL_CONFIG, seed=SEED + 3, gain=3.0, bias_gain=6.0)
    out_all, layers = run(model, inp, None)
    out64 = run64(model, inp, None)
    save('prop_gain.npz', **common, seed=SEED + 3, gain=3.0, bias_gain=6.0, state_dict_spec=json.dumps(spec), out_all=out_all.numpy(),
         out_all_f64=out64.numpy(), h_layers=layers[:, rows].numpy())
    print('   gain: fp32 reference vs float64:', P.rel_err(out_all, out64))

    # ---- 5: unsorted batch vectors (the same atoms, interleaved across complexes)
    r = np.random.RandomState(13)
    pp, lp = r.permutation(len(inp['batch_protein'])), r.permutation(len(inp['batch_ligand']))
    un = dict(protein_pos=inp['protein_pos'][pp], protein_feat=inp['protein_feat'][pp], batch_protein=inp['batch_protein'][pp],
              ligand_pos=inp['ligand_pos'][lp], ligand_feat=inp['ligand_feat'][lp], batch_ligand=inp['batch_ligand'][lp])
    model, spec = build(pm, P.MODEL_CONFIG)
    out_all, _ = run(model, un, None, hooks=False)
    out_kind, _ = run(model, un, kind, hooks=False)
    save('prop_unsorted.npz', **un, output_kind=kind.numpy(), reference_order=reference_order(un), nbr=edges(un, k), seed=SEED,
         gain=1.0, bias_gain=1.0, state_dict_spec=json.dumps(spec), out_all=out_all.numpy(), out_kind=out_kind.numpy())


if __name__ == '__main__':
    main()
