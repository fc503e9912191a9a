"""Gradient fixtures of the binding-affinity predictor from the REAL reference (build container only: needs the reference tree):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_prop_grad.py

Runs the unmodified models/property_pred/prop_model.py (through tools/make_golden_prop.py's loader) with torch autograd, in float64
and in fp32, on the weights of _prop_ref.make_state_dict and the complexes of _prop_ref.fixture_complexes() (1h36 + docked ligand, a
synthetic pocket, one complex of fewer than 49 nodes), pos_noise_std = 0.  The loss is get_loss's MSE of out[kind] against seeded y,
or, for prop_grad_all3 (no output_kind), sum(out * U) for a seeded upstream gradient U [B, 3].  The cases are
tests/_prop_grad_ref.CASES:

  prop_grad_kind         PropPredNet with output_kind
  prop_grad_all3         PropPredNet without output_kind, seeded upstream gradient
  prop_grad_enc_final_h  PropPredNetEnc, final_h config (final_h of prop_enc_final_h.npz)
  prop_grad_enc_all      PropPredNetEnc with all three enc_* features (those of prop_enc_all.npz)
  prop_grad_gain         PropPredNet, weights at 3x nn.Linear's range, biases at 6x

Each file holds y, kind, loss and prediction (float64 and fp32), and per parameter the gradient's norm, its projections onto 16 seeded
unit Gaussian directions (_prop_grad_ref.directions) and, for tensors of at most 4,096 elements, the full gradient -- with the
prefixes f64/ and f32/.  r = the fp32 reference's distance from float64 (the largest of: full small tensors, max |difference| / max
|g64|; projections and norms, |difference| / |g64|_2) is stored as `r`.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import make_golden_prop as MG  # noqa: E402
import _prop_ref as P  # noqa: E402
import _prop_grad_ref as PG  # noqa: E402


def golden(name):
    return np.load(os.path.join(P.GOLDEN, name))


def reference_grads(pm, name, dtype):
    kind, seed, gain, bias_gain, use_kind, up_seed = PG.CASES[name]
    cfg = PG.model_config(kind)
    model, spec = MG.build(pm, PG.cfg_of(kind), enc=cfg, seed=seed, gain=gain, bias_gain=bias_gain)
    model = model.to(dtype).train()
    inp, out_kind, y, enc = PG.case_inputs(kind, golden)
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    f = lambda a: None if a is None else torch.as_tensor(np.asarray(a)).to(dtype)
    args = [f(t['protein_pos']), f(t['protein_feat']), f(t['ligand_pos']), f(t['ligand_feat']), t['batch_protein'], t['batch_ligand'],
            torch.from_numpy(out_kind) if use_kind else None]
    if cfg is not None:
        node = enc.get('node')
        args += [f(enc.get('ligand')), None if node is None else MG.to_reference_rows(inp, f(node)), f(enc.get('graph'))]
    model.zero_grad()
    out = model(*args)
    if up_seed is not None:
        loss = (out * torch.from_numpy(PG.upstream(up_seed, 3, 3)).to(dtype)).sum()
    else:
        loss = torch.nn.MSELoss()(out.view(-1), torch.from_numpy(y).to(dtype))      # get_loss, pos_noise_std = 0
    loss.backward()
    grads = {k: p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p) for k, p in model.named_parameters()}
    return loss.detach(), out.detach(), grads, spec


def main():
    torch.set_num_threads(1)            # the reference's scatter backward sums in thread order: one thread makes reruns bit-identical
    pm = MG.load_prop()
    for name in PG.CASES:
        loss64, out64, g64, spec = reference_grads(pm, name, torch.float64)
        loss32, out32, g32, _ = reference_grads(pm, name, torch.float32)
        s64, s32 = PG.summarize(g64), PG.summarize(g32)
        r = 0.0
        for k in g64:
            n = float(s64[f'norm/{k}'])
            if n == 0.0:
                continue
            r = max(r, abs(float(s32[f'norm/{k}']) - n) / n, float(np.max(np.abs(s32[f'proj/{k}'] - s64[f'proj/{k}']))) / n)
            if f'full/{k}' in s64:
                r = max(r, float(np.max(np.abs(s32[f'full/{k}'] - s64[f'full/{k}'])) / np.max(np.abs(s64[f'full/{k}']))))
        kind, *_ = PG.CASES[name]
        _, out_kind, y, _ = PG.case_inputs(kind, golden)
        arrays = dict(case=PG.fixture_json(name), state_dict_spec=json.dumps(spec), y=y, kind=out_kind, r=np.float64(r),
                      **{'f64/loss': loss64.numpy(), 'f32/loss': loss32.numpy(), 'f64/pred': out64.numpy(), 'f32/pred': out32.numpy()},
                      **{f'f64/{k}': v for k, v in s64.items()}, **{f'f32/{k}': v for k, v in s32.items()})
        path = os.path.join(P.GOLDEN, name + '.npz')
        np.savez_compressed(path, **arrays)
        print(f'wrote {path} ({os.path.getsize(path) / 1e6:.3f} MB), fp32 reference vs float64: r = {r:.3g}')


if __name__ == '__main__':
    main()
