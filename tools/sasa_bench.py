"""Cost of a solvent-accessible-surface report on the C2 shape (1h36 pocket x 100 samples with the prior sizes, the complete 1000-frame
trajectory):

    timeout -k 10 300 python tools/sasa_bench.py --step final && \\
    timeout -k 10 600 python tools/sasa_bench.py --step trajectory && \\
    timeout -k 10 600 python tools/sasa_bench.py --step sample

One JSON line per step, and every step is a process of its own: run each under its own ``timeout`` and chain them with ``&&``, as
above, so that a step that faults or hangs ends the run.  The trajectory is the synthetic one of tools/pocket_bench.py (a compact random
cloud per sample that jitters from frame to frame, uniformly random classes, at the centroid of the pocket's docked ligand): the cost
depends on the sizes and on how many spheres meet, not on the chemistry.  Timed with HIP events on the current stream after one untimed
call, the median of ``repeats`` and every value reported, on packed device tensors (check=False: no host look):

  * ``--step final``       ``sasa_last_ms``: capi.sasa_report on the 100 final poses, 96 points, the 1.4 A probe, no per-atom outputs and no
                           bits; ``sasa_full_last_ms``: with them; ``sasa_apo_only_ms``: the same pocket with an empty pack (the apo kernel
                           alone); ``pocket_last_ms``: capi.pocket_report on the same pack, for scale.
  * ``--step trajectory``  ``sasa_all_ms`` and ``pocket_all_ms``: the same two on all frames.
  * ``--step sample``      ``sample_sasa_last_ms`` / ``sample_sasa_all_ms``: quality.sample_sasa: host packing, the copy to the device, the
                           host's look at the pack, the launch, the copy back, the areas.

``points_per_frame`` is ligand atoms with a class x 96; ``free_last``, ``bound_last`` and ``pocket_buried_last`` are the point counts
of the final poses, and ``buried_share_last`` what the clouds held.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

from targetdiff_amd import capi, quality  # noqa: E402
from quality_bench import event_ms, synthetic_result  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--step', type=str, required=True, choices=['final', 'trajectory', 'sample'])
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--points', type=int, default=quality.SASA_POINTS)
    ap.add_argument('--probe', type=float, default=quality.SASA_PROBE)
    ap.add_argument('--lib', type=str, default=None, help='time this build of the library instead of the tree\'s (an A/B of a kernel change)')
    args = ap.parse_args()
    if args.lib is not None:
        capi.load_library(os.path.abspath(args.lib))
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'pocket_1h36.npz')) as z:
        ppos_np, feat, sizes = z['pos'].astype(np.float32), z['feat'].astype(np.int64), [int(s) for s in z['prior_sizes_seed2021']]
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'ligand_1h36_docked.npz')) as z:
        centre = z['pos'].astype(np.float64).mean(0)
    frames = args.frames if args.step != 'final' else 1
    res = synthetic_result(sizes, frames)
    pos_traj = [(p + centre).astype(np.float32).astype(np.float64) for p in res[2]]
    result = {'data': types.SimpleNamespace(protein_pos=ppos_np, protein_atom_feature=feat), 'pred_ligand_pos_traj': pos_traj,
              'pred_ligand_v_traj': res[3]}
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    reps = max(5, args.repeats)
    out = {'step': args.step, 'build_tag': capi.build_tag(), 'samples': len(sizes), 'frames': frames, 'atoms_per_frame': int(sum(sizes)),
           'largest_sample': max(sizes), 'protein_atoms': int(len(ppos_np)), 'points': args.points, 'probe': args.probe, 'repeats': reps,
           'points_per_frame': int(sum(sizes)) * args.points}
    if args.step == 'sample':
        out['sample_sasa_last_ms'] = event_ms(lambda: quality.sample_sasa(result, -1, probe=args.probe, points=args.points), reps)
        out['sample_sasa_all_ms'] = event_ms(lambda: quality.sample_sasa(result, 'all', probe=args.probe, points=args.points), reps)
        rep = quality.sample_sasa(result, 'all', probe=args.probe, points=args.points)
        out.update({k: round(x, 4) for k, x in rep.summary(-1).items()})
        print(json.dumps(out))
        return
    pos = torch.from_numpy(np.concatenate(pos_traj, axis=1).astype(np.float32)).to(dev)
    v = torch.from_numpy(np.concatenate(res[3], axis=1)).to(dev)
    ptr = torch.as_tensor(np.cumsum([0] + sizes), dtype=torch.int32, device=dev)
    cz = quality.class_atomic_numbers('add_aromatic')
    side = quality.PocketSide((ppos_np, feat), dev)
    ppos, selem = side.pos, side.kinds('element')[0]
    lr, pr = quality.sasa_reaches(args.probe)
    dirs = torch.from_numpy(quality.sasa_directions(args.points)).to(dev)
    sasa = lambda p, c, q=ptr, full=False: capi.sasa_report(p, c, q, cz, ppos, selem, lr, pr, dirs, None, full, full, check=False)
    elem, (kind, names) = side.elem, side.kinds()
    thr = quality.pocket_clash_thresholds()
    poc = lambda p, c: capi.pocket_report(p, c, ptr, cz, ppos, elem, kind, len(names), quality.DEFAULT_CONTACT_CUTOFF, thr, None, None, False,
                                          False, check=False)
    key = 'last' if args.step == 'final' else 'all'
    out[f'sasa_{key}_ms'] = event_ms(lambda: sasa(pos, v), reps)
    out[f'pocket_{key}_ms'] = event_ms(lambda: poc(pos, v), reps)
    if args.step == 'final':
        out['sasa_full_last_ms'] = event_ms(lambda: sasa(pos, v, ptr, True), reps)
        none = torch.zeros(1, dtype=torch.int32, device=dev)
        out['sasa_apo_only_ms'] = event_ms(lambda: sasa(pos[:, :0].contiguous(), v[:, :0].contiguous(), none), reps)
    last = sasa(pos[-1:].contiguous(), v[-1:].contiguous())
    s = quality.Sasa(last, ptr, selem, lr, pr, args.points)
    out['free_last'], out['bound_last'] = int(last['free'].sum()), int(last['bound'].sum())
    out['pocket_buried_last'], out['buried_share_last'] = int(last['pocket_buried'].sum()), round(float(s.buried_share.mean()), 4)
    out['point_rate_per_s'] = round(out['points_per_frame'] * frames / (out[f'sasa_{key}_ms']['median'] * 1e-3))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
