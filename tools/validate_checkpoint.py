"""The ``[Validate]`` line of the reference's training script (scripts/train_diffusion.py:153-208) for a checkpoint, on the GPU:

    python tools/validate_checkpoint.py CONFIG --checkpoint CKPT --data FILE.pt|synthetic:N [--levels 10] [--batch-size 4] [--unfused]

CONFIG is a training configuration of the reference (configs/training.yml: its ``model`` section is used).  CKPT is a checkpoint as the
reference's train script saves it (a dict with the state_dict under ``'model'``) or a bare state_dict; ``synthetic:SEED`` takes the seeded
random weights of oracle/weights.py instead (a dry run: the numbers mean nothing).  FILE.pt is a list of dicts with the reference's field
names -- ``protein_pos`` [n_p, 3], ``protein_atom_feature`` [n_p, F], ``ligand_pos`` [n_l, 3], ``ligand_atom_feature_full`` [n_l] int64 --
already featurised: nothing is perceived here (no RDKit).  ``synthetic:N`` makes N seeded pocket / ligand pairs (targetdiff_amd.workloads).

Prints the reference's log line and one JSON line with the report (per level, per class).  Forward only: no gradient, no optimiser.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from targetdiff_amd import validation, workloads  # noqa: E402
from targetdiff_amd.models import ScorePosNet3D  # noqa: E402


def synthetic_items(n, num_classes):
    items = []
    for i in range(n):
        pocket = workloads.synthetic_pocket(500 + i, 120 + 20 * (i % 4), 3.0, 10.0)
        b = workloads.pack_samples([pocket], 1, [12 + 3 * (i % 5)])
        pos, v = workloads.init_ligand(b, num_classes=num_classes, generator=torch.Generator().manual_seed(900 + i))
        items.append({'protein_pos': b.protein_pos, 'protein_atom_feature': b.protein_atom_feature.float(), 'ligand_pos': pos,
                      'ligand_atom_feature_full': v})
    return items


def load_weights(checkpoint):
    """``(state_dict, strict)`` of CKPT: a file as the reference's train script saves it -- a pickled dict that holds its EasyDict ``config``
    beside ``'model'`` (scripts/train_diffusion.py:222-226), hence ``weights_only=False``, as tools/batch_sample.py loads it -- or a bare
    state_dict; ``synthetic:SEED``: the seeded random weights of oracle/weights.py, which carry no schedule constants (strict=False)."""
    if checkpoint.startswith('synthetic:'):
        from oracle import weights
        return weights.make_state_dict(int(checkpoint.split(':', 1)[1])), False
    ckpt = torch.load(checkpoint, map_location='cpu', weights_only=False)
    return (ckpt['model'] if isinstance(ckpt, dict) and 'model' in ckpt else ckpt), True


def model_from(model_cfg, sd, strict):
    """The mirror for a state_dict: the feature widths are read off its embedding weights"""
    protein_dim = sd['protein_atom_emb.weight'].shape[1]
    time_cols = 0
    if int(_get(model_cfg, 'time_emb_dim', 0) or 0) > 0:
        time_cols = 1 if _get(model_cfg, 'time_emb_mode', 'simple') == 'simple' else int(_get(model_cfg, 'time_emb_dim'))
    num_classes = sd['ligand_atom_emb.weight'].shape[1] - time_cols
    model = ScorePosNet3D(model_cfg, protein_dim, num_classes)
    model.load_state_dict(sd, strict=strict)
    return model, num_classes


def _get(cfg, key, default=None):
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('config')
    ap.add_argument('--checkpoint', required=True)
    ap.add_argument('--data', required=True)
    ap.add_argument('--levels', type=int, default=10)
    ap.add_argument('--batch-size', type=int, default=4)
    ap.add_argument('--unfused', action='store_true', help='one denoiser call per level, as the reference loops')
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--iter', type=int, default=0, help='the iteration number the log line shows')
    args = ap.parse_args()
    import yaml
    with open(args.config) as f:
        cfg = yaml.safe_load(f)
    model_cfg = cfg.get('model', cfg)
    sd, strict = load_weights(args.checkpoint)
    model, num_classes = model_from(model_cfg, sd, strict)
    dev = torch.device(args.device)
    model = model.to(dev).eval()
    if args.data.startswith('synthetic:'):
        items = synthetic_items(int(args.data.split(':', 1)[1]), num_classes)
    else:
        items = torch.load(args.data, map_location='cpu', weights_only=False)      # the fields may be numpy arrays
    batches = (validation.collate(items[i:i + args.batch_size], dev) for i in range(0, len(items), args.batch_size))
    report = validation.validate(model, batches, num_levels=args.levels, fused=not args.unfused)
    print(validation.format_line(args.iter, report))
    print(json.dumps({**report, 'complexes': len(items), 'fused': not args.unfused,
                      'per_class_auroc': {str(k): v for k, v in report['per_class_auroc'].items()}}))


if __name__ == '__main__':
    main()
