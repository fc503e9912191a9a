"""Cost of the docking-style score on the C2 shape (1h36 pocket x 100 samples with the prior sizes, the complete 1000-frame trajectory):

    python tools/score_bench.py [--frames 1000] [--repeats 5] [--lib OTHER/libtargetdiff_hip.so]

One JSON line.  The trajectory is that of tools/interactions_bench.py (the synthetic clouds of tools/quality_bench.py moved to the
centroid of the pocket's docked ligand): the cost depends on the sizes and on how many pairs fall below the 8 A cutoff, not on the
chemistry.  Timed with HIP events on the current stream after one untimed call, the median of ``repeats`` and every value reported, all
in one process on the same packed device tensors (check=False: no host look at the offsets):

  * ``score_all_ms`` / ``score_last_ms``                  capi.score_report with the rotor inputs (bond_ptr of bond_graph and bond_ring of
                                                          ring_report, made once, outside the timing), on all frames / the final poses;
  * ``score_norot_all_ms`` / ``score_norot_last_ms``      the same without the rotor inputs: the role kernel and the pair kernel alone;
  * ``pocket_all_ms`` / ``pocket_last_ms``                the yardstick: capi.pocket_report on the same pack (4 A cutoff, the clash
                                                          table, no per-atom outputs and no bits);
  * ``sample_score_all_ms`` / ``sample_score_last_ms``    quality.sample_score: host packing, the copy to the device, the bond graph, the
                                                          ring sizes, the launch, the copy back.

``pairs_per_frame`` is ligand heavy atoms x protein atoms that take part; ``n_pairs_last`` the pairs of the last frame inside the cutoff.
The score is a Vina-style one on this project's heuristic typing, not AutoDock Vina's number.
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
    cz, aro = quality.class_atomic_numbers('add_aromatic'), quality.class_aromatic('add_aromatic')
    side = quality.PocketSide((ppos_np, feat), dev)
    ppos, elem, (kind, names), role = side.pos, side.elem, side.kinds(), side.roles()
    thr, rsum = quality.pocket_clash_thresholds(), quality.score_radius_sums()

    def rotor_inputs(p, c):
        bond_ptr = capi.bond_graph(p, c, ptr, cz, aro, (), None, False, True, check=False)['bond_ptr']
        return bond_ptr, capi.ring_report(p, c, ptr, cz, aro, None, bond_ptr, False, check=False)['bond_ring']

    rot, rot1 = rotor_inputs(pos, v), rotor_inputs(pos1, v1)
    score = lambda p, c, r=(None, None): capi.score_report(p, c, ptr, cz, aro, ppos, elem, kind, role, len(names), rsum, quality.SCORE_CUTOFF,
                                                           quality.DEFAULT_HETERO_CUTOFF, *r, check=False)
    poc = lambda p, c: capi.pocket_report(p, c, ptr, cz, ppos, elem, kind, len(names), quality.DEFAULT_CONTACT_CUTOFF, thr, None, None,
                                          False, False, check=False)
    out['score_all_ms'] = event_ms(lambda: score(pos, v, rot), reps)
    out['score_last_ms'] = event_ms(lambda: score(pos1, v1, rot1), reps)
    out['score_norot_all_ms'] = event_ms(lambda: score(pos, v), reps)
    out['score_norot_last_ms'] = event_ms(lambda: score(pos1, v1), reps)
    out['pocket_all_ms'] = event_ms(lambda: poc(pos, v), reps)
    out['pocket_last_ms'] = event_ms(lambda: poc(pos1, v1), reps)
    out['sample_score_all_ms'] = event_ms(lambda: quality.sample_score(result, 'all'), reps)
    out['sample_score_last_ms'] = event_ms(lambda: quality.sample_score(result, -1), reps)
    last = score(pos1, v1, rot1)
    rep = quality.sample_score(result, 'all')
    assert int(last['n_pairs'].sum()) == int(rep.sum_pairs[-1]) and int(last['n_rot'].sum()) == int(rep.sum_rotors[-1])
    heavy = int(quality._heavy_atoms(v1.cpu().numpy(), cz, sizes).sum())
    part = (last['protein_role'] >= 0) & (elem != 0)
    out['pairs_per_frame'] = heavy * int(part.sum())
    out['n_pairs_last'] = int(last['n_pairs'].sum())
    out['rotors_last'] = int(last['n_rot'].sum())
    out['ratio_all'] = round(out['score_all_ms']['median'] / out['pocket_all_ms']['median'], 3)
    out['ratio_last'] = round(out['score_last_ms']['median'] / out['pocket_last_ms']['median'], 3)
    out['mean_score_last'], out['no_pairs_last'] = rep.mean_score(-1), rep.summary(-1)['no_pairs']
    print(json.dumps(out))


if __name__ == '__main__':
    main()
