"""Cost of the docking search on the C2 shape (1h36 pocket x the 100 final poses with the prior sizes):

    python tools/dock_bench.py [--repeats 5] [--chains 16] [--rounds 16] [--seed 0] [--lib OTHER/libtargetdiff_hip.so]

One JSON line.  The poses are tools/relax_bench.py's (the synthetic clouds of tools/quality_bench.py moved to the centroid of the
pocket's docked ligand): the cost depends on the sizes, on how many pairs fall below the 8 A cutoff and on how many evaluations the
descents take, not on the chemistry.  Timed with HIP events on the current stream after one untimed call, the median of ``repeats`` and
every value reported, all in one process on the same packed device tensors (check=False), the draws made once outside the timing:

  * ``dock_ms``            one capi.score_dock call with the rotor inputs: ``chains`` persistent workgroups per molecule, every round of
                           every chain on the device, and the small selecting launch;
  * ``minimize_ms``        capi.score_minimize on the same pack, once;
  * ``host_loop_floor_ms`` ``minimize_ms`` times ``rounds`` + 1 times ceil(chains B / B) = ``chains``: what a host loop of one
                           td_score_minimize launch per round over a pack of the chains' states would pay at the least (it would also
                           move every chain's Metropolis state across the bus each round);
  * ``sample_dock_ms``     quality.sample_dock: host packing, the copy to the device, the bond graph, the ring sizes, the relaxation
                           beside the search, the launches, the copy back.

``mean_evals`` and ``max_evals_seen`` (per molecule, summed over its chains), ``chains_agree`` and the three mean scores are those of
the timed call.  It is a rigid-body global search under this project's heuristic score, not AutoDock Vina's dock: three translations
and three rotations, no torsions.
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
    ap.add_argument('--chains', type=int, default=quality.DOCK_CHAINS)
    ap.add_argument('--rounds', type=int, default=quality.DOCK_ROUNDS)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--lib', type=str, default=None, help='time this build of the library instead of the tree\'s (an A/B of a kernel change)')
    args = ap.parse_args()
    if args.lib is not None:
        capi.load_library(os.path.abspath(args.lib))
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'pocket_1h36.npz')) as z:
        ppos_np, feat, sizes = z['pos'].astype(np.float32), z['feat'].astype(np.int64), [int(s) for s in z['prior_sizes_seed2021']]
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'ligand_1h36_docked.npz')) as z:
        centre = z['pos'].astype(np.float64).mean(0)
    res = synthetic_result(sizes, 1000)                                         # relax_bench.py's trajectory: its last frame is the same
    pos_traj = [(p + centre).astype(np.float32).astype(np.float64) for p in res[2]]
    result = {'data': types.SimpleNamespace(protein_pos=ppos_np, protein_atom_feature=feat), 'pred_ligand_pos_traj': pos_traj,
              'pred_ligand_v_traj': res[3]}
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    reps = max(5, args.repeats)
    out = {'build_tag': capi.build_tag(), 'samples': len(sizes), 'atoms': int(sum(sizes)), 'largest_sample': max(sizes),
           'protein_atoms': int(len(ppos_np)), 'repeats': reps, 'chains': args.chains, 'rounds': args.rounds, 'seed': args.seed}
    pos = torch.from_numpy(np.concatenate(pos_traj, axis=1).astype(np.float32)[-1:]).to(dev).contiguous()
    v = torch.from_numpy(np.concatenate(res[3], axis=1)[-1:]).to(dev).contiguous()
    ptr = torch.as_tensor(np.cumsum([0] + sizes), dtype=torch.int32, device=dev)
    cz, aro = quality.class_atomic_numbers('add_aromatic'), quality.class_aromatic('add_aromatic')
    side = quality.PocketSide((ppos_np, feat), dev)
    ppos, elem, (kind, names), role = side.pos, side.elem, side.kinds(), side.roles()
    bond_ptr = capi.bond_graph(pos, v, ptr, cz, aro, (), None, False, True, check=False)['bond_ptr']
    rot = (bond_ptr, capi.ring_report(pos, v, ptr, cz, aro, None, bond_ptr, False, check=False)['bond_ring'])
    pocket = (ppos, elem, kind, role, len(names), quality.score_radius_sums(), quality.SCORE_WEIGHTS, quality.SCORE_CUTOFF,
              quality.DEFAULT_HETERO_CUTOFF)
    draws = capi._dock_inputs(args.chains, args.rounds, quality.DOCK_AMPLITUDE, quality.DOCK_TEMPERATURE, args.seed, None, 1, len(sizes), dev)[4]
    dock = lambda: capi.score_dock(pos, v, ptr, cz, aro, *pocket, *rot, n_chains=args.chains, n_rounds=args.rounds, draws=draws, check=False)
    relax = lambda: capi.score_minimize(pos, v, ptr, cz, aro, *pocket, *rot, check=False)
    search = dict(n_chains=args.chains, n_rounds=args.rounds, seed=args.seed)
    out['dock_ms'] = event_ms(dock, reps)
    out['minimize_ms'] = event_ms(relax, reps)
    out['host_loop_floor_ms'] = round(out['minimize_ms']['median'] * (args.rounds + 1) * args.chains, 4)
    out['sample_dock_ms'] = event_ms(lambda: quality.sample_dock(result, -1, **search), reps)
    evals = dock()['n_evals'].cpu().numpy()
    rep = quality.sample_dock(result, -1, **search)
    assert int(rep.sum_evals[-1]) == int(evals.sum())
    out['mean_evals'], out['max_evals_seen'] = float(evals.mean()), int(evals.max())
    s = rep.summary(-1)
    for k in ('mean_score', 'mean_score_min', 'mean_score_dock', 'chains_agree', 'mean_rmsd_dock'):
        out[k] = s[k]
    print(json.dumps(out))


if __name__ == '__main__':
    main()
