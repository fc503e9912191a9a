"""Cost of one validation of the C2 pocket with its docked ligand (tests/golden/pocket_1h36.npz, ligand_1h36_docked.npz):

    python tools/loss_bench.py [--levels 10] [--repeats 5]

One JSON line.  Times are HIP events on the current stream after one untimed call, the median of ``repeats`` and every value reported, all
in one process on the same device tensors:

  * ``validate_fused_ms`` / ``validate_unfused_ms``   validation.validate on the one-complex batch: the ``levels`` copies as one pack and one
                                                      denoiser call, beside the reference's loop of ``levels`` calls (both with the final AUROC);
  * ``loss_single_ms``                                one get_diffusion_loss at one level: ``levels`` of these are the unfused loop's body;
  * ``forward_single_ms``                             the denoiser alone on that batch (native.model_forward);
  * ``diffusion_loss_kernel_ms``                      td_diffusion_loss alone (both stages) on the fused pack's predictions;
  * ``auroc_kernel_ms`` / ``auroc_kernel_64k_ms``     td_auroc alone on the validation's rows, and on 65536 rows of 13 classes.

Seeded random weights (oracle/weights.py): the losses mean nothing, the times do.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

from oracle import weights  # noqa: E402
from targetdiff_amd import capi, quality, validation  # noqa: E402
from targetdiff_amd.models import ScorePosNet3D  # noqa: E402
from quality_bench import event_ms  # noqa: E402

SYMBOL_Z = {'H': 1, 'C': 6, 'N': 7, 'O': 8, 'F': 9, 'P': 15, 'S': 16, 'Cl': 17, 'Br': 17}      # Br has no class: written as Cl, as tools/make_golden_quality.py does


def docked_complex(dev):
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'pocket_1h36.npz')) as z:
        ppos, pfeat = z['pos'], z['feat'].astype(np.float32)
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'ligand_1h36_docked.npz')) as z:
        lpos, elements = z['pos'], [str(e) for e in z['elements']]
    cz = list(quality.class_atomic_numbers('add_aromatic'))
    v = [cz.index(SYMBOL_Z[e]) for e in elements]              # the first (non-aromatic) class of the element
    return validation.collate([{'protein_pos': ppos, 'protein_atom_feature': pfeat, 'ligand_pos': lpos,
                                'ligand_atom_feature_full': np.asarray(v, np.int64)}], dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--levels', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    reps = max(5, args.repeats)
    model = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG), 27, 13)
    model.load_state_dict(weights.make_state_dict(2021), strict=False)
    model = model.to(dev).eval()
    b = docked_complex(dev)
    L = args.levels
    out = {'build_tag': capi.build_tag(), 'levels': L, 'protein_atoms': int(b['protein_pos'].shape[0]),
           'ligand_atoms': int(b['ligand_pos'].shape[0]), 'repeats': reps}
    torch.manual_seed(0)
    out['validate_fused_ms'] = event_ms(lambda: validation.validate(model, [b], num_levels=L, fused=True), reps)
    out['validate_unfused_ms'] = event_ms(lambda: validation.validate(model, [b], num_levels=L, fused=False), reps)
    args6 = (b['protein_pos'], b['protein_atom_feature'], b['protein_element_batch'], b['ligand_pos'], b['ligand_atom_feature_full'],
             b['ligand_element_batch'])
    t = torch.tensor([500], device=dev)
    out['loss_single_ms'] = event_ms(lambda: model.get_diffusion_loss(*args6, time_step=t), reps)
    r = model.get_diffusion_loss(*args6, time_step=t)
    native = model._native(dev)
    pptr = native.graph_ptr(b['protein_element_batch'], 1)
    lptr = native.graph_ptr(b['ligand_element_batch'], 1)
    ppos = b['protein_pos'] - b['protein_pos'].mean(0)
    out['forward_single_ms'] = event_ms(lambda: native.model_forward(ppos.contiguous(), b['protein_atom_feature'], pptr, r['ligand_pos_perturbed'],
                                                                    r['ligand_v_perturbed'], lptr, want_final_h=False), reps)
    # the fused pack's loss kernel alone: L copies of the graph, copy l at level l
    Nl = int(b['ligand_pos'].shape[0])
    rep = lambda x: x.repeat((L,) + (1,) * (x.dim() - 1)).contiguous()
    t_all = torch.as_tensor(validation.levels_of(model.num_timesteps, L), dtype=torch.int32, device=dev)
    lptr_all = torch.arange(0, (L + 1) * Nl, Nl, dtype=torch.int32, device=dev)
    pk = [rep(r[k]) for k in ('x0', 'ligand_pos_perturbed')] + [rep(torch.zeros_like(r['x0']))] + \
        [rep(b['ligand_atom_feature_full']), rep(r['ligand_v_perturbed']), rep(r['pred_ligand_pos']), rep(r['pred_ligand_v'])]
    out['diffusion_loss_kernel_ms'] = event_ms(lambda: native.diffusion_loss(t_all, lptr_all, *pk, model.loss_v_weight), reps)
    recon = native.diffusion_loss(t_all, lptr_all, *pk, model.loss_v_weight)['ligand_v_recon']
    labels = rep(b['ligand_atom_feature_full'])
    out['auroc_rows'] = int(recon.shape[0])
    out['auroc_kernel_ms'] = event_ms(lambda: capi.auroc_counts(recon, labels), reps)
    g = torch.Generator().manual_seed(1)
    big = torch.rand(65536, 13, generator=g).softmax(-1).to(dev)
    big_l = torch.randint(0, 13, (65536,), generator=g).to(dev)
    out['auroc_kernel_64k_ms'] = event_ms(lambda: capi.auroc_counts(big, big_l), reps)
    rep_f = validation.validate(model, [b], num_levels=L, fused=True)
    out['loss'], out['atom_auroc'] = rep_f['loss'], rep_f['atom_auroc']
    print(json.dumps(out))


if __name__ == '__main__':
    main()
