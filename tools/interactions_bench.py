"""Cost of a typed interaction report on the C2 shape (1h36 pocket x 100 samples with the prior sizes, the complete 1000-frame trajectory):

    python tools/interactions_bench.py [--frames 1000] [--repeats 5] [--lib OTHER/libtargetdiff_hip.so]

One JSON line.  The trajectory is that of tools/pocket_bench.py (the synthetic clouds of tools/quality_bench.py moved to the centroid of
the pocket's docked ligand): the cost depends on the sizes, on how many ligand atoms hold a role and on how many pairs fall below the
larger cutoff, not on the chemistry.  Timed with HIP events on the current stream after one untimed call, the median of ``repeats`` and
every value reported, all in one process on the same packed device tensors (check=False: no host look at the offsets):

  * ``interactions_all_ms`` / ``interactions_last_ms``            capi.interaction_report with the 40 residue kinds and the default
                                                                  cutoffs, no per-atom outputs and no bits, on all frames / on the
                                                                  final poses;
  * ``interactions_full_all_ms``                                  the first with the per-atom outputs and the bits;
  * ``pocket_all_ms`` / ``pocket_last_ms``                        the yardstick: capi.pocket_report on the same pack (4 A cutoff, the
                                                                  clash table, no per-atom outputs and no bits);
  * ``sample_interactions_all_ms`` / ``sample_interactions_last_ms``  quality.sample_interactions: host packing, the copy to the device,
                                                                  the launch, the copy back.

``pairs_per_frame`` is ligand atoms with a class x protein atoms that take part.  ``hbonds_last``, ``hydrophobic_last``,
``donors_last``, ``acceptors_last``, ``hydrophobic_atoms_last`` and ``protein_hydrophobic`` say what the clouds and the pocket held.
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
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--lib', type=str, default=None, help='time this build of the library instead of the tree\'s (an A/B of a kernel change)')
    args = ap.parse_args()
    if args.lib is not None:
        capi.load_library(os.path.abspath(args.lib))
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'pocket_1h36.npz')) as z:
        ppos_np, feat, sizes = z['pos'].astype(np.float32), z['feat'].astype(np.int64), [int(s) for s in z['prior_sizes_seed2021']]
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'ligand_1h36_docked.npz')) as z:
        centre = z['pos'].astype(np.float64).mean(0)
    res = synthetic_result(sizes, args.frames)
    pos_traj = [(p + centre).astype(np.float32).astype(np.float64) for p in res[2]]
    result = {'data': types.SimpleNamespace(protein_pos=ppos_np, protein_atom_feature=feat), 'pred_ligand_pos_traj': pos_traj,
              'pred_ligand_v_traj': res[3]}
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    reps = max(5, args.repeats)
    out = {'build_tag': capi.build_tag(), 'samples': len(sizes), 'frames': args.frames, 'atoms_per_frame': int(sum(sizes)),
           'largest_sample': max(sizes), 'protein_atoms': int(len(ppos_np)), 'repeats': reps}
    pos = torch.from_numpy(np.concatenate(pos_traj, axis=1).astype(np.float32)).to(dev)
    v = torch.from_numpy(np.concatenate(res[3], axis=1)).to(dev)
    ptr = torch.as_tensor(np.cumsum([0] + sizes), dtype=torch.int32, device=dev)
    pos1, v1 = pos[-1:].contiguous(), v[-1:].contiguous()
    cz = quality.class_atomic_numbers('add_aromatic')
    side = quality.PocketSide((ppos_np, feat), dev)
    ppos, elem, (kind, names), role = side.pos, side.elem, side.kinds(), side.roles()
    thr = quality.pocket_clash_thresholds()
    act = lambda p, c, full=False: capi.interaction_report(p, c, ptr, cz, ppos, elem, kind, role, len(names), return_atoms=full,
                                                           return_bits=full, check=False)
    poc = lambda p, c: capi.pocket_report(p, c, ptr, cz, ppos, elem, kind, len(names), quality.DEFAULT_CONTACT_CUTOFF, thr, None, None,
                                          False, False, check=False)
    out['interactions_all_ms'] = event_ms(lambda: act(pos, v), reps)
    out['interactions_last_ms'] = event_ms(lambda: act(pos1, v1), reps)
    out['interactions_full_all_ms'] = event_ms(lambda: act(pos, v, True), reps)
    out['pocket_all_ms'] = event_ms(lambda: poc(pos, v), reps)
    out['pocket_last_ms'] = event_ms(lambda: poc(pos1, v1), reps)
    out['sample_interactions_all_ms'] = event_ms(lambda: quality.sample_interactions(result, 'all'), reps)
    out['sample_interactions_last_ms'] = event_ms(lambda: quality.sample_interactions(result, -1), reps)
    last = act(pos1, v1)
    rep = quality.sample_interactions(result, 'all')
    assert int(last['n_hbonds'].sum()) == int(rep.sum_hbonds[-1]) and int(last['n_hydrophobic'].sum()) == int(rep.sum_hydrophobic[-1])
    assert int(last['kind_hist'].sum()) == int(rep.kind_hist[-1].sum()) == int((last['n_donated'] + last['n_accepted'] + last['n_hydrophobic']).sum())
    out['pairs_per_frame'] = int(sum(sizes)) * int((last['protein_role'] >= 0).sum())
    out['ratio_all'] = round(out['interactions_all_ms']['median'] / out['pocket_all_ms']['median'], 3)
    out['ratio_last'] = round(out['interactions_last_ms']['median'] / out['pocket_last_ms']['median'], 3)
    for k in ('n_hbonds', 'n_hydrophobic', 'n_donors', 'n_acceptors', 'n_hydrophobic_atoms'):
        out[k[2:] + '_last'] = int(last[k].sum())
    out['protein_hydrophobic'] = int(((last['protein_role'] & quality.ROLE_HYDROPHOBIC) != 0).sum())
    out['no_hbond_last'], out['polar_in_hbond_last'] = rep.no_hbond(-1), rep.polar_in_hbond(-1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
