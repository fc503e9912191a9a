"""Cost of the rigid-body relaxation on the C2 shape (1h36 pocket x the 100 final poses with the prior sizes):

    python tools/relax_bench.py [--repeats 5] [--max_steps 64] [--lib OTHER/libtargetdiff_hip.so]

One JSON line.  The poses are the last frame of tools/score_bench.py's trajectory (the synthetic clouds of tools/quality_bench.py moved
to the centroid of the pocket's docked ligand): the cost depends on the sizes, on how many pairs fall below the 8 A cutoff and on how
many evaluations the optimiser takes, not on the chemistry.  Timed with HIP events on the current stream after one untimed call, the
median of ``repeats`` and every value reported, all in one process on the same packed device tensors (check=False):

  * ``minimize_ms``        one capi.score_minimize call with the rotor inputs (made once, outside the timing): one persistent workgroup per
                           molecule, every iteration on the device;
  * ``score_ms``           capi.score_report on the same pack, once;
  * ``host_loop_ms``       ``score_ms`` times ``mean_evals``, the mean evaluations per molecule: what a host loop of one td_score_report per
                           trial pose would pay at the least (it would also need a gradient, and the slowest molecule sets its length);
  * ``sample_relax_ms``    quality.sample_relax: host packing, the copy to the device, the bond graph, the ring sizes, the launch, the copy
                           back.

``mean_steps``, ``mean_evals``, ``max_evals_seen`` and the status shares are those of the timed call; ``mean_score`` / ``mean_score_min``
the scores before and after.  It is a local optimisation under this project's heuristic score, not AutoDock Vina's minimize; rigid-body
only: three translations and three rotations, no torsions.
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
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--max_steps', type=int, default=quality.RELAX_MAX_STEPS)
    ap.add_argument('--lib', type=str, default=None, help='time this build of the library instead of the tree\'s (an A/B of a kernel change)')
    args = ap.parse_args()
    if args.lib is not None:
        capi.load_library(os.path.abspath(args.lib))
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'pocket_1h36.npz')) as z:
        ppos_np, feat, sizes = z['pos'].astype(np.float32), z['feat'].astype(np.int64), [int(s) for s in z['prior_sizes_seed2021']]
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'ligand_1h36_docked.npz')) as z:
        centre = z['pos'].astype(np.float64).mean(0)
    res = synthetic_result(sizes, 1000)                                         # score_bench.py's trajectory: its last frame is the same
    pos_traj = [(p + centre).astype(np.float32).astype(np.float64) for p in res[2]]
    result = {'data': types.SimpleNamespace(protein_pos=ppos_np, protein_atom_feature=feat), 'pred_ligand_pos_traj': pos_traj,
              'pred_ligand_v_traj': res[3]}
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    reps = max(5, args.repeats)
    out = {'build_tag': capi.build_tag(), 'samples': len(sizes), 'atoms': int(sum(sizes)), 'largest_sample': max(sizes),
           'protein_atoms': int(len(ppos_np)), 'repeats': reps, 'max_steps': args.max_steps}
    pos = torch.from_numpy(np.concatenate(pos_traj, axis=1).astype(np.float32)[-1:]).to(dev).contiguous()
    v = torch.from_numpy(np.concatenate(res[3], axis=1)[-1:]).to(dev).contiguous()
    ptr = torch.as_tensor(np.cumsum([0] + sizes), dtype=torch.int32, device=dev)
    cz, aro = quality.class_atomic_numbers('add_aromatic'), quality.class_aromatic('add_aromatic')
    side = quality.PocketSide((ppos_np, feat), dev)
    ppos, elem, (kind, names), role = side.pos, side.elem, side.kinds(), side.roles()
    rsum = quality.score_radius_sums()
    bond_ptr = capi.bond_graph(pos, v, ptr, cz, aro, (), None, False, True, check=False)['bond_ptr']
    rot = (bond_ptr, capi.ring_report(pos, v, ptr, cz, aro, None, bond_ptr, False, check=False)['bond_ring'])
    pocket = (ppos, elem, kind, role, len(names), rsum)
    cut = (quality.SCORE_CUTOFF, quality.DEFAULT_HETERO_CUTOFF)
    relax = lambda: capi.score_minimize(pos, v, ptr, cz, aro, *pocket, quality.SCORE_WEIGHTS, *cut, *rot, max_steps=args.max_steps, check=False)
    score = lambda: capi.score_report(pos, v, ptr, cz, aro, *pocket, *cut, *rot, check=False)
    out['minimize_ms'] = event_ms(relax, reps)
    out['score_ms'] = event_ms(score, reps)
    out['sample_relax_ms'] = event_ms(lambda: quality.sample_relax(result, -1, max_steps=args.max_steps), reps)
    r = relax()
    evals, steps, status = r['n_evals'].cpu().numpy(), r['n_steps'].cpu().numpy(), r['status'].cpu().numpy()
    rep = quality.sample_relax(result, -1, max_steps=args.max_steps)
    assert int(rep.sum_evals[-1]) == int(evals.sum()) and int(rep.sum_steps[-1]) == int(steps.sum())
    out['mean_steps'], out['mean_evals'], out['max_evals_seen'] = float(steps.mean()), float(evals.mean()), int(evals.max())
    out['host_loop_ms'] = round(out['score_ms']['median'] * out['mean_evals'], 4)
    out['ratio_host_loop'] = round(out['host_loop_ms'] / out['minimize_ms']['median'], 3)
    for name, bit in (('converged', capi.RELAX_CONVERGED), ('out_of_budget', capi.RELAX_OUT_OF_BUDGET), ('at_cap', capi.RELAX_AT_CAP)):
        out[name] = float(((status & bit) != 0).mean())
    s = rep.summary(-1)
    out['mean_score'], out['mean_score_min'], out['mean_rmsd'] = s['mean_score'], s['mean_score_min'], s['mean_rmsd']
    print(json.dumps(out))


if __name__ == '__main__':
    main()
