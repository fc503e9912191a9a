"""Fixtures of tests/test_oracle_vs_reference.py from the REAL reference (TEST INFRASTRUCTURE; needs a reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python -m oracle.make_golden_fresh [--keep-existing]

  reference_fresh.npz      the reference model (weights.make_state_dict(77)) on fresh synthetic batches: forward (seeds 1, 2, with
                           final_h), likelihood_estimation with its recorded Gaussian / uniform draws, the EGNN refine net
                           (weights.make_egnn_state_dict(9), 4 layers), the forward on unsorted batch vectors and on their
                           stable-sorted order, and three steps of the reference's own sampling loop on the unsorted vectors
                           (counter draws, base 9100).  Inputs that are not regenerated from a seed are stored beside the outputs.
  reference_state_dict.npz key order and shapes of the reference ScorePosNet3D state_dict (configs/training.yml), with the values of
                           its 15 frozen schedule Parameters and of its buffers; the learnable tensors' values are not stored.
  reference_api.json       the parameters (name, repr of the default) of the reference's call signatures the mirror replaces.
  reference_driver_calls.npz   every call the reference's batching driver (scripts/sample_diffusion.py:31-116) makes into its own
                           model in the two runs of make_golden_r2.gen_driver_small (driver_small.npz): the keyword arguments, the
                           state of the counter draws on entry, and the model's answer.
"""
from __future__ import annotations

import importlib
import inspect
import json
import os

import numpy as np
import torch

from . import reference_loader, shims, weights
from . import make_golden
from .make_golden import GOLDEN_DIR, _save
from .make_golden_r2 import counter_draws

FORWARD_SEEDS = (1, 2)
LIKELIHOOD_T = (12, 0, 999, 400)
UNSORTED_STEPS = 3
UNSORTED_DRAW_BASE = 9100


def fresh_batch(seed):
    """The synthetic two-pocket batch of tests/test_oracle_vs_reference.py."""
    from targetdiff_amd import workloads
    pockets = [workloads.synthetic_pocket(500 + seed, 70, 3.0, 9.0), workloads.synthetic_pocket(600 + seed, 40, 3.0, 8.0)]
    b = workloads.pack_samples(pockets, 2, [8, 11, 6, 9])
    lpos, lv = workloads.init_ligand(b, generator=torch.Generator().manual_seed(seed), spread=1.5)
    return b, lpos, lv


def unsorted_permutations(b, lpos):
    g = torch.Generator().manual_seed(12)
    return torch.randperm(b.protein_pos.shape[0], generator=g), torch.randperm(lpos.shape[0], generator=g)


def egnn_inputs(b, lpos):
    from . import restatement as R
    g = torch.Generator().manual_seed(10)
    return R.compose_context(torch.randn(b.protein_pos.shape[0], 128, generator=g), torch.randn(lpos.shape[0], 128, generator=g),
                             b.protein_pos, lpos, b.protein_element_batch, b.ligand_element_batch)


def _np(t):
    return t.detach().cpu().numpy()


def fresh(ref):
    model, _ = make_golden.build_reference_model(ref, seed=77)
    out = {}
    for seed in FORWARD_SEEDS:
        b, lpos, lv = fresh_batch(seed)
        ppos, lposc, _ = ref.center_pos(b.protein_pos, lpos, b.protein_element_batch, b.ligand_element_batch, mode='protein')
        with torch.no_grad():
            want = model(ppos, b.protein_atom_feature.float(), b.protein_element_batch, lposc, lv, b.ligand_element_batch)
        for k in ('pred_ligand_pos', 'pred_ligand_v', 'final_h'):
            out[f'forward{seed}_{k}'] = _np(want[k])

    b, lpos, lv = fresh_batch(3)
    rec = {}
    o_normal, o_rand = torch.Tensor.normal_, torch.rand_like

    def normal_(self, *a, **k):
        r = o_normal(self, *a, **k)
        rec['noise'] = r.clone()
        return r

    def rand_like(x, *a, **k):
        r = o_rand(x, *a, **k)
        rec['uniform'] = r.clone()
        return r
    torch.Tensor.normal_, torch.rand_like = normal_, rand_like
    try:
        torch.manual_seed(5)
        want = model.likelihood_estimation(b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch, lpos, lv,
                                           b.ligand_element_batch, torch.tensor(LIKELIHOOD_T, dtype=torch.long))
    finally:
        torch.Tensor.normal_, torch.rand_like = o_normal, o_rand
    out['likelihood_noise'], out['likelihood_uniform'] = _np(rec['noise']), _np(rec['uniform'])
    out['likelihood_terms'] = np.stack([_np(w) for w in want])

    egnn_mod = importlib.import_module('models.egnn')
    net = egnn_mod.EGNN(num_layers=4, hidden_dim=128, edge_feat_dim=4, num_r_gaussian=1, k=32, cutoff_mode='knn').eval()
    net.load_state_dict(weights.make_egnn_state_dict(9, num_layers=4), strict=True)
    b, lpos, _ = fresh_batch(4)
    h, x, batch, mask = egnn_inputs(b, lpos)
    with torch.no_grad():
        want = net(h, x, mask, batch)
    out['egnn_x'], out['egnn_h'] = _np(want['x']), _np(want['h'])

    b, lpos, lv = fresh_batch(4)
    pp, pl = unsorted_permutations(b, lpos)
    ppos, pv, bp = b.protein_pos[pp], b.protein_atom_feature.float()[pp], b.protein_element_batch[pp]
    xl, vl, bl = lpos[pl], lv[pl], b.ligand_element_batch[pl]
    cp, cl, _ = ref.center_pos(ppos, xl, bp, bl, mode='protein')
    with torch.no_grad():
        want = model(cp, pv, bp, cl, vl, bl)
        sp, sl = torch.sort(bp, stable=True).indices, torch.sort(bl, stable=True).indices
        pre = model(cp[sp], pv[sp], bp[sp], cl[sl], vl[sl], bl[sl])
    for k in ('pred_ligand_pos', 'pred_ligand_v', 'final_h'):
        out[f'unsorted_{k}'], out[f'unsorted_presorted_{k}'] = _np(want[k]), _np(pre[k])
    with counter_draws(UNSORTED_DRAW_BASE), torch.no_grad():
        r = model.sample_diffusion(ppos, pv, bp, xl, vl, bl, num_steps=UNSORTED_STEPS, center_pos_mode='protein')
    out['unsorted_pos_traj'] = np.stack([_np(p) for p in r['pos_traj']])
    out['unsorted_v_traj'] = np.stack([_np(v) for v in r['v_traj']])
    return out


def state_dict_layout(ref):
    torch.manual_seed(123)
    model = ref.ScorePosNet3D(shims.EasyDict(weights.DEFAULT_MODEL_CONFIG), weights.PROTEIN_FEATURE_DIM, weights.LIGAND_FEATURE_DIM)
    sd = model.state_dict()
    frozen = [k for k, p in model.named_parameters() if not p.requires_grad]
    buffers = [k for k, _ in model.named_buffers()]
    out = {'keys': np.array(list(sd)), 'shapes': np.array([json.dumps(list(v.shape)) for v in sd.values()]),
           'frozen': np.array(frozen), 'buffers': np.array(buffers)}
    for k in frozen + buffers:
        out['value:' + k] = _np(sd[k])
    return out


def api(ref, drv):
    ut = importlib.import_module('models.uni_transformer')
    fns = {'ScorePosNet3D.__init__': ref.ScorePosNet3D.__init__, 'ScorePosNet3D.forward': ref.ScorePosNet3D.forward,
           'ScorePosNet3D.sample_diffusion': ref.ScorePosNet3D.sample_diffusion,
           'ScorePosNet3D.fetch_embedding': ref.ScorePosNet3D.fetch_embedding,
           'ScorePosNet3D.likelihood_estimation': ref.ScorePosNet3D.likelihood_estimation,
           'get_refine_net': ref.get_refine_net, 'sample_diffusion_ligand': drv.sample_diffusion_ligand,
           'unbatch_v_traj': drv.unbatch_v_traj,
           'UniTransformerO2TwoUpdateGeneral.__init__': ut.UniTransformerO2TwoUpdateGeneral.__init__,
           'UniTransformerO2TwoUpdateGeneral.forward': ut.UniTransformerO2TwoUpdateGeneral.forward}
    return {name: [[p.name, repr(p.default)] for p in inspect.signature(inspect.unwrap(f)).parameters.values()]
            for name, f in fns.items()}


def _returned(r):
    """A sample_diffusion answer -> (arrays, description of its structure)."""
    arrays, desc = {}, {}
    for k, v in r.items():
        if isinstance(v, list):
            desc[k] = {'list': len(v), 'types': sorted({type(e).__name__ for e in v}), 'devices': sorted({e.device.type for e in v})}
            arrays[k] = np.stack([_np(e) for e in v]) if v else np.zeros((0,), np.float32)
        else:
            desc[k] = {'type': type(v).__name__}
            arrays[k] = _np(v)
    return arrays, desc


def driver_calls(ref, drv):
    """Both runs of make_golden_r2.gen_driver_small, with the reference model's sample_diffusion observed."""
    from .make_golden import SEED
    from .make_golden_r2 import driver_data
    model, _ = make_golden.build_reference_model(ref, seed=SEED)
    seen, arrays, state = [], {}, {}
    inner = model.sample_diffusion

    def observed(*args, **kwargs):
        assert not args, 'the driver passes keywords only'
        entry = dict(state['count'])
        r = inner(**kwargs)
        i = len(seen)
        kw = {}
        for k, v in kwargs.items():
            if torch.is_tensor(v):
                arrays[f'call{i}.{k}'] = _np(v)
                kw[k] = {'tensor': f'call{i}.{k}'}
            else:
                kw[k] = v
        ret, desc = _returned(r)
        arrays.update({f'call{i}.returned.{k}': a for k, a in ret.items()})
        seen.append({'base': state['base'], 'count': entry, 'kwargs': kw, 'returned': desc})
        return r
    model.sample_diffusion = observed
    runs = [(3100, dict(data=driver_data(), num_samples=5, num_steps=4, pos_only=False, sample_num_atoms='prior')),
            (3200, dict(data=driver_data(ref_ligand_atoms=9), num_samples=3, num_steps=3, pos_only=True, sample_num_atoms='ref'))]
    np.random.seed(SEED)
    for base, kw in runs:
        with counter_draws(base, lambda kind, n: n) as count:
            state.update(base=base, count=count)
            drv.sample_diffusion_ligand(model, kw.pop('data'), kw.pop('num_samples'), batch_size=2, device='cpu',
                                        center_pos_mode='protein', **kw)
    arrays['meta'] = np.array(json.dumps({'num_classes': int(model.num_classes), 'calls': seen}))
    return arrays


def main():
    ref = reference_loader.load()
    drv = reference_loader.load_driver()
    _save(os.path.join(GOLDEN_DIR, 'reference_fresh.npz'), **fresh(ref))
    _save(os.path.join(GOLDEN_DIR, 'reference_state_dict.npz'), **state_dict_layout(ref))
    _save(os.path.join(GOLDEN_DIR, 'reference_driver_calls.npz'), **driver_calls(ref, drv))
    path = os.path.join(GOLDEN_DIR, 'reference_api.json')
    text = json.dumps(api(ref, drv), indent=1) + '\n'
    if make_golden.KEEP_EXISTING and os.path.exists(path):
        with open(path) as f:
            assert f.read() == text, (path, 'regenerated fixture differs from the committed one')
        print('kept', os.path.basename(path), '(regenerated values identical)')
        return
    with open(path, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
