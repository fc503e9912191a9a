"""Fixtures for the edges of the product's LayerNorm fold, from the REAL reference (TEST INFRASTRUCTURE; build container only, needs a
reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python -m oracle.make_golden_fold [--keep-existing]

The product folds the LayerNorm of every edge MLP (hk, hv, xk, xv, the global edge gate) into its two Linears and divides by a per-MLP
scale M = (sqrt(128) + max_n beta_n / |gamma_n|)(1 + 2^-10) (csrc/pack.cpp FoldedMlp).  Two kinds of ordinary state_dict reach where that
form can lose precision or drop a term; both start from oracle.weights.trained_like_state_dict(SEED, 4):

  forward_fold_m{1e4,1e6,1e8,8e8,1e12}.npz   oracle.weights.fold_scale_state_dict: two live units per folded MLP set M to the value in
                           the name (8e8: about the largest a live unit reaches with |beta| <= 4; 1e12: a bias of 1e4, past the point
                           where the first Linear's power-of-two scale has to be clipped to keep the LayerNorm's radicand in range).
  forward_fold_near_dead.npz   oracle.weights.near_dead_state_dict: units at half and twice the round-6 dead floor (2^-30 of the MLP's
                           largest |gamma|) with biases -1 / 0 / +1, most with their second-Linear column scaled by 1e5.

Each holds one forward (return_all) on the small batch: the outputs, final_ligand_h, the layer-0 predictions, and the same run in float64
(``*_f64``, as oracle/make_golden_r6.py does it).  No per-layer h / x: the files stay small.  Weights are regenerated from the seed.
"""
from __future__ import annotations

import os

import torch

from . import reference_loader, weights
from .make_golden import GOLDEN_DIR, SEED, _save, small_batch
from .make_golden_r6 import build, float64_run

FOLD_SCALES = (('1e4', 1e4), ('1e6', 1e6), ('1e8', 1e8), ('8e8', 8e8), ('1e12', 1e12))
F64_KEYS = ('pred_ligand_pos', 'pred_ligand_v', 'final_h', 'final_ligand_h')


def gen_forward(ref, name, sd):
    b, lpos, lv = small_batch()
    ppos, lposc, _ = ref.center_pos(b.protein_pos, lpos, b.protein_element_batch, b.ligand_element_batch, mode='protein')
    with torch.no_grad():
        p = build(ref, sd)(ppos, b.protein_atom_feature.float(), b.protein_element_batch, lposc, lv, b.ligand_element_batch, return_all=True)
    with float64_run(), torch.no_grad():
        p64 = build(ref, sd).double()(ppos.double(), b.protein_atom_feature.double(), b.protein_element_batch, lposc.double(), lv,
                                      b.ligand_element_batch)
    assert p64['final_h'].dtype == torch.float64
    _save(os.path.join(GOLDEN_DIR, name), protein_pos=ppos.numpy(), ligand_pos=lposc.numpy(), ligand_v=lv.numpy(),
          pred_ligand_pos=p['pred_ligand_pos'].numpy(), pred_ligand_v=p['pred_ligand_v'].numpy(),
          final_ligand_h=p['final_ligand_h'].numpy(), final_h=p['final_h'].numpy(),
          layer0_pred_ligand_v=p['layer_pred_ligand_v'][0].numpy(), layer0_pred_ligand_pos=p['layer_pred_ligand_pos'][0].numpy(),
          **{k + '_f64': p64[k].numpy() for k in F64_KEYS})
    print(f'{name}: fp32 reference vs its float64 run:', {k: f'{float((p[k].double() - p64[k]).abs().max()):.2e}' for k in F64_KEYS},
          f'|pred_v| max {float(p["pred_ligand_v"].abs().max()):.3f}  |h| max {float(p["final_h"].abs().max()):.2f}')


def main():
    ref = reference_loader.load()
    torch.set_num_threads(8)
    for tag, m in FOLD_SCALES:
        gen_forward(ref, f'forward_fold_m{tag}.npz', weights.fold_scale_state_dict(SEED, m))
    gen_forward(ref, 'forward_fold_near_dead.npz', weights.near_dead_state_dict(SEED))


if __name__ == '__main__':
    main()
