"""Fixture of the affinity predictor's shape / regime cases from the REAL reference (build container only: needs the reference tree):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_prop_shapes.py

For every case of tests/_prop_shapes_ref.CASES it runs the unmodified models/property_pred/prop_model.py (through
tools/make_golden_prop.py's loader; the k-NN shim searches in the project's composed order, see knn_graph_project_ties) with torch
autograd on the CPU, in float64 and in fp32, on the case's seeded weights and inputs, and writes ONE file,
tests/golden/prop_shapes.npz, with the same entries per case (prefix '<case>/'):

  out     float64 outputs [B, O] ([B, 1] with output_kind); left out for the large reduction cases (_prop_shapes_ref.LARGE)
  loss    float64 loss
  norm    float64 gradient norm of every parameter [P]        } parameter order = the model's own (the `keys` entry, JSON)
  proj    16 projections of every parameter's gradient [P, 16] } directions: _prop_grad_ref.directions
  r       the fp32 reference's distance from float64, as tools/make_golden_prop_grad.py defines it, the largest over the run as it is
          and _prop_shapes_ref.ORDERS renumberings of the hidden units (the same function, every fp32 sum in another order)
  crc     CRC-32 of the case's inputs (the inputs themselves are regenerated from the case table)

No weights, no program text.  A case (other than the gain-3 one) whose r exceeds TOL_GRAD / 2 sits on a ReLU kink within fp32
rounding: the script names it and exits with an error -- take that case's next candidate seed (the rule above
_prop_shapes_ref.RESEEDED) and write the fixture again.
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import make_golden_prop as MG  # noqa: E402
import _prop_ref as P  # noqa: E402
import _prop_shapes_ref as S  # noqa: E402


def reference_module(pm):
    """The reference's two classes taking plain-dict configs (the reference reads attributes)."""
    return types.SimpleNamespace(PropPredNet=lambda cfg, *a, **k: pm.PropPredNet(MG.ed(cfg), *a, **k),
                                 PropPredNetEnc=lambda cfg, *a, **k: pm.PropPredNetEnc(MG.ed(cfg), *a, **k))


ROWS = {}          # 'to_project': reference composed row -> the project's composed row, for the case being run


def knn_graph_project_ties(x, k, batch=None, loop=False, flow='source_to_target', cosine=False, num_workers=1):
    """The k-NN shim, searched in the project's composed order.  The reference composes a batch with an unstable argsort, so inside a
    complex its rows are in another order than the project's (stable) one; a k-NN tie goes to the lower index, and on the tie-heavy
    cases (lattice, coincident atoms, hubs) the two orders would pick different neighbours.  Same graph otherwise."""
    to_project = torch.from_numpy(ROWS['to_project'])
    from_project = torch.argsort(to_project)
    return from_project[MG.knn_graph_t2s(x[from_project], k, batch[from_project], loop=loop, flow=flow, cosine=cosine)]


def reference_grads(ref, name, dtype, order=0):
    """(loss, out, gradients) of the reference; order >= 1: with the hidden units renumbered (_prop_shapes_ref.renumber_hidden), the
    gradients brought back to the original numbering."""
    case, cfg, sd32, inp, out_kind, y, enc, up = S.load(name)
    if order:
        sd32 = S.renumber_hidden(sd32, order)
    ROWS['to_project'] = np.argsort(P.composed_order(inp['batch_protein'], inp['batch_ligand']))[MG.reference_order(inp)]
    model = S.build_model(case, ref)
    assert tuple((k, tuple(v.shape)) for k, v in model.state_dict().items()) == S.spec(name), f'{name}: state_dict spec differs'
    model.load_state_dict(sd32, strict=True)
    model = model.to(dtype).train()
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    f = lambda a: None if a is None else torch.as_tensor(np.asarray(a)).to(dtype)
    args = [f(t['protein_pos']), f(t['protein_feat']), f(t['ligand_pos']), f(t['ligand_feat']), t['batch_protein'], t['batch_ligand'],
            None if out_kind is None else torch.from_numpy(out_kind)]
    if case.kind == 'enc':
        node = enc.get('node')
        args += [f(enc.get('ligand')), None if node is None else MG.to_reference_rows(inp, f(node)), f(enc.get('graph'))]
    model.zero_grad()
    out = model(*args)
    if up is not None:
        loss = (out * torch.from_numpy(up).to(dtype)).sum()
    else:
        loss = torch.nn.MSELoss()(out.view(-1), torch.from_numpy(y).to(dtype))          # get_loss, pos_noise_std = 0
    loss.backward()
    grads = {k: p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p) for k, p in model.named_parameters()}
    return loss.detach(), out.detach(), S.original_numbering(grads, order) if order else grads


def fp32_distance(ref, name, g64, stop_above=None):
    """r: the largest distance from float64 of the reference's fp32 gradients, over the run as it is and ORDERS renumberings of the
    hidden units (other orders of every fp32 sum).  With `stop_above`, returns at the first order beyond it."""
    r = 0.0
    for order in range(S.ORDERS + 1):
        r = max(r, S.distance(reference_grads(ref, name, torch.float32, order)[2], g64))
        if stop_above is not None and r > stop_above:
            break
    return r


def main():
    torch.set_num_threads(1)            # the reference's scatter backward sums in thread order: one thread makes reruns bit-identical
    ref = reference_module(MG.load_prop())
    sys.modules['models.property_pred.prop_egnn'].knn_graph = knn_graph_project_ties
    arrays, bad = {}, []
    for name, case in S.CASES.items():
        _, _, _, inp, _, _, enc, _ = S.load(name)
        loss64, out64, g64 = reference_grads(ref, name, torch.float64)
        renumbered = reference_grads(ref, name, torch.float64, 1)[2]          # the renumbering is the same function: float64 agrees
        assert S.distance(renumbered, g64) < 1e-10, name
        keys, norm, proj = S.summarize(case, g64)
        r = fp32_distance(ref, name, g64)
        arrays[f'{name}/keys'] = json.dumps(keys)
        arrays[f'{name}/loss'] = loss64.numpy()
        arrays[f'{name}/norm'] = norm
        arrays[f'{name}/proj'] = proj
        arrays[f'{name}/r'] = np.float64(r)
        arrays[f'{name}/crc'] = S.inputs_crc(inp, enc)
        if name not in S.LARGE:
            arrays[f'{name}/out'] = out64.numpy()
        ok = name in S.GAIN_CASES or r <= S.TOL_GRAD / 2
        print(f'{name:22s} fp32 reference vs float64: r = {r:.3e}' + ('' if ok else '   > TOL_GRAD / 2: change the seed'))
        if not ok:
            bad.append(name)
    if bad:
        raise SystemExit(f'not written: r > TOL_GRAD / 2 for {bad}')
    path = os.path.join(P.GOLDEN, 'prop_shapes.npz')
    np.savez_compressed(path, **arrays)
    print(f'wrote {path} ({os.path.getsize(path) / 1e6:.3f} MB)')


if __name__ == '__main__':
    main()
