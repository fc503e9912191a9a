"""Validation of a ScorePosNet3D checkpoint: the ``[Validate]`` line of the reference's training script (scripts/train_diffusion.py:153-208)
without the training -- the loss at ten fixed noise levels and the atom-type AUROC of the reconstructed types.  Forward only: no gradient,
no optimiser, no scheduler step ("Diffusion loss and validation").

    report = validate(model, batches)              # batches: dicts / objects with the reference's field names
    print(format_line(it, report))

A batch carries ``protein_pos``, ``protein_atom_feature``, ``protein_element_batch``, ``ligand_pos``, ``ligand_atom_feature_full`` and
``ligand_element_batch`` (a PyG batch of the reference's dataset does; ``collate`` makes one from a list of per-complex dicts).
"""
from __future__ import annotations

import numpy as np
import torch

from . import capi

FIELDS = ('protein_pos', 'protein_atom_feature', 'protein_element_batch', 'ligand_pos', 'ligand_atom_feature_full', 'ligand_element_batch')


def _field(batch, name):
    return batch[name] if isinstance(batch, dict) else getattr(batch, name)


def collate(items, device=None):
    """A batch (dict) from per-complex dicts with ``protein_pos`` [n_p, 3], ``protein_atom_feature`` [n_p, F], ``ligand_pos`` [n_l, 3] and
    ``ligand_atom_feature_full`` [n_l] int64: concatenated, with the two batch vectors."""
    T = lambda x, dt: torch.as_tensor(x).to(dt)
    out = {
        'protein_pos': torch.cat([T(d['protein_pos'], torch.float32) for d in items]),
        'protein_atom_feature': torch.cat([T(d['protein_atom_feature'], torch.float32) for d in items]),
        'ligand_pos': torch.cat([T(d['ligand_pos'], torch.float32) for d in items]),
        'ligand_atom_feature_full': torch.cat([T(d['ligand_atom_feature_full'], torch.int64) for d in items]),
        'protein_element_batch': torch.cat([torch.full((len(d['protein_pos']),), i, dtype=torch.int64) for i, d in enumerate(items)]),
        'ligand_element_batch': torch.cat([torch.full((len(d['ligand_pos']),), i, dtype=torch.int64) for i, d in enumerate(items)]),
    }
    return {k: v.to(device) for k, v in out.items()} if device is not None else out


def levels_of(num_timesteps, num_levels=10):
    """The fixed time steps of the reference's validate(): np.linspace(0, T - 1, num_levels).astype(int) (:165)"""
    return np.linspace(0, num_timesteps - 1, num_levels).astype(int)


def _uniform_like(lpos, C):
    return lpos.new_empty(lpos.shape[0], C)


def _level_losses(model, b, levels, fused, noise_source):
    """The three losses of every level (fp32 scalars as Python floats, [L] each) and ligand_v_recon of every level ([L * N_l, C], level-major)
    for one batch."""
    ppos, pv, bp, lpos, lv, bl = (_field(b, k) for k in FIELDS)
    pv = pv.float()
    dev = ppos.device
    B = int(bp.max().item()) + 1
    L, Nl, C = len(levels), lpos.shape[0], model.num_classes
    if not fused:                      # the reference's loop (:165-184)
        rows, recon = [], []
        for l, t in enumerate(levels):
            ns = None
            if noise_source is not None:
                ns = lambda s, name, like, l=l: noise_source(l, name, like if like is not None else _uniform_like(lpos, C))
            r = model.get_diffusion_loss(ppos, pv, bp, lpos, lv, bl, time_step=torch.tensor([int(t)] * B, device=dev), noise_source=ns)
            rows.append((float(r['loss']), float(r['loss_pos']), float(r['loss_v'])))
            recon.append(r['ligand_v_recon'])
        return B, rows, torch.cat(recon, dim=0)
    # fused: the L copies of the batch as one pack of L * B graphs, copy l at level l, one forward
    rep = lambda x: x.repeat((L,) + (1,) * (x.dim() - 1))
    shift = lambda bv: (bv.unsqueeze(0) + B * torch.arange(L, device=dev).unsqueeze(1)).reshape(-1)
    time_step = torch.as_tensor(np.asarray(levels), dtype=torch.int64, device=dev).repeat_interleave(B)
    ns = None
    if noise_source is not None:       # level l takes noise_source(l, ...): the draws of the unfused loop
        def ns(s, name, like):
            like_l = lpos if name == 'noise' else _uniform_like(lpos, C)
            return torch.cat([noise_source(l, name, like_l) for l in range(L)], dim=0)
    r = model.get_diffusion_loss(rep(ppos), rep(pv), shift(bp), rep(lpos), rep(lv), shift(bl), time_step=time_step, noise_source=ns)
    lp = r['loss_pos_graph'].view(L, B).mean(dim=1)                                        # torch.mean over the graphs of a level (:543, :551)
    lvv = r['loss_v_graph'].view(L, B).mean(dim=1)
    loss = lp + lvv * model.loss_v_weight                                                  # :552, fp32
    rows = list(zip(loss.tolist(), lp.tolist(), lvv.tolist()))
    return B, rows, r['ligand_v_recon']


@torch.no_grad()
def validate(model, batches, num_levels=10, fused=True, noise_source=None):
    """validate() of scripts/train_diffusion.py:153-208 over ``batches``: every batch at the ``num_levels`` fixed time steps, sums of
    ``float(loss) * batch_size`` in Python floats divided by the number of (graph, level) evaluations, and get_auroc over the
    ``ligand_v_recon`` rows of every batch and level against the true types.  The rows and labels stay on the device; one td_auroc call
    counts the pairs at the end.

    ``fused=True`` packs the ``num_levels`` copies of a batch into one pack of ``num_levels * B`` graphs and runs the denoiser once per
    batch; ``fused=False`` is the reference's loop, one call per level.  ``noise_source(l, name, like)`` supplies the draws of level l
    (``name`` 'noise': like [N_l, 3]; 'uniform': like [N_l, C]) -- the same draws in both forms.

    Returns ``loss``, ``loss_pos``, ``loss_v``, ``atom_auroc``, ``per_class_auroc`` ({class: auroc}) and ``per_level``: ``levels`` and the
    three losses of every level, averaged over the graphs like the totals."""
    was_training = model.training
    model.eval()
    levels = levels_of(model.num_timesteps, num_levels)
    L = len(levels)
    sums = np.zeros(3)
    per_level = np.zeros((L, 3))
    sum_n = n_level = 0
    all_pred, all_true = [], []
    try:
        for b in batches:
            B, rows, recon = _level_losses(model, b, levels, fused, noise_source)
            for l, row in enumerate(rows):
                for k in range(3):
                    sums[k] += row[k] * B                                                  # float(loss) * batch_size (:179-181)
                    per_level[l, k] += row[k] * B
                sum_n += B
            n_level += B
            all_pred.append(recon)
            all_true.append(_field(b, 'ligand_atom_feature_full').repeat(L))
    finally:
        model.train(was_training)
    if sum_n == 0:
        raise ValueError('validate: no batches')
    atom_auroc, per_class = capi.auroc(torch.cat(all_pred, dim=0).contiguous(), torch.cat(all_true, dim=0).contiguous())
    per_level /= n_level
    return {'loss': sums[0] / sum_n, 'loss_pos': sums[1] / sum_n, 'loss_v': sums[2] / sum_n, 'atom_auroc': atom_auroc,
            'per_class_auroc': per_class,
            'per_level': {'levels': [int(t) for t in levels], 'loss': per_level[:, 0].tolist(), 'loss_pos': per_level[:, 1].tolist(),
                          'loss_v': per_level[:, 2].tolist()}}


def format_line(it, report):
    """The reference's log line (scripts/train_diffusion.py:199-203)"""
    return '[Validate] Iter %05d | Loss %.6f | Loss pos %.6f | Loss v %.6f e-3 | Avg atom auroc %.6f' % (
        it, report['loss'], report['loss_pos'], report['loss_v'] * 1000, report['atom_auroc'])
