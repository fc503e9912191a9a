"""Cost of a ring report on the C2 shape (1h36 pocket x 100 samples with the prior sizes, the complete 1000-frame trajectory):

    python tools/rings_bench.py [--frames 1000] [--repeats 5]

One JSON line.  The trajectory is the synthetic one of tools/quality_bench.py (a compact random cloud per sample that jitters from frame
to frame, uniformly random classes): the cost depends on the sizes and on how many bonds and cycles the clouds have, not on the
chemistry.  Timed with HIP events on the current stream after one untimed call, the median of ``repeats`` and every value reported,
all in one process on the same packed device tensors (check=False: no host look at the offsets):

  * ``ring_report_all_ms`` / ``ring_report_last_ms``   capi.ring_report without the per-bond outputs (mask, counts, atom sizes, ring_hist)
                                                       on all frames / on the final poses;
  * ``ring_report_bonds_last_ms``                      the same with bond_ptr: bond_ring and the ring-aware category too, the host
                                                       read of bond_ptr's last entry included;
  * ``bond_graph_all_ms`` / ``bond_graph_last_ms``     capi.bond_graph (the eight default profiles, fragments and bond_ptr) beside them;
  * ``bond_list_last_ms``                              capi.bond_list for the final poses;
  * ``sample_rings_all_ms`` / ``sample_rings_last_ms`` quality.sample_rings: host packing, the copy to the device, the launch, the copy back.

``ring_ratio_last`` and ``ring_bonds_last`` say what the clouds held, so that a time can be read against the work it paid for.
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

from targetdiff_amd import capi, quality  # noqa: E402
from quality_bench import event_ms, synthetic_result  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'pocket_1h36.npz')) as z:
        sizes = [int(s) for s in z['prior_sizes_seed2021']]
    res = synthetic_result(sizes, args.frames)
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    reps = max(5, args.repeats)
    out = {'build_tag': capi.build_tag(), 'samples': len(sizes), 'frames': args.frames, 'atoms_per_frame': int(sum(sizes)),
           'largest_sample': max(sizes), 'repeats': reps}
    pos = torch.from_numpy(np.concatenate(res[2], axis=1).astype(np.float32)).to(dev)
    v = torch.from_numpy(np.concatenate(res[3], axis=1)).to(dev)
    ptr = torch.as_tensor(np.cumsum([0] + sizes), dtype=torch.int32, device=dev)
    pos1, v1 = pos[-1:].contiguous(), v[-1:].contiguous()
    cz, aro, bprof = quality.class_atomic_numbers('add_aromatic'), quality.class_aromatic('add_aromatic'), quality.default_bond_profiles()
    out['ring_report_all_ms'] = event_ms(lambda: capi.ring_report(pos, v, ptr, cz, aro, check=False), reps)
    out['ring_report_last_ms'] = event_ms(lambda: capi.ring_report(pos1, v1, ptr, cz, aro, check=False), reps)
    out['bond_graph_all_ms'] = event_ms(lambda: capi.bond_graph(pos, v, ptr, cz, aro, bprof, None, True, True, check=False), reps)
    out['bond_graph_last_ms'] = event_ms(lambda: capi.bond_graph(pos1, v1, ptr, cz, aro, bprof, None, True, True, check=False), reps)
    g1 = capi.bond_graph(pos1, v1, ptr, cz, aro, bprof, None, True, True, check=False)
    out['bond_list_last_ms'] = event_ms(lambda: capi.bond_list(pos1, v1, ptr, cz, aro, g1['bond_ptr'], check=False), reps)
    out['ring_report_bonds_last_ms'] = event_ms(lambda: capi.ring_report(pos1, v1, ptr, cz, aro, None, g1['bond_ptr'], check=False), reps)
    out['sample_rings_all_ms'] = event_ms(lambda: quality.sample_rings(res, 'all'), reps)
    out['sample_rings_last_ms'] = event_ms(lambda: quality.sample_rings(res, -1), reps)
    r1 = capi.ring_report(pos1, v1, ptr, cz, aro, None, g1['bond_ptr'], check=False)
    rep = quality.sample_rings(res, 'all')
    assert np.array_equal(rep.ring_hist[-1], r1['ring_hist'][0].cpu().numpy())
    out['bonds_last'], out['ring_bonds_last'] = int(g1['bond_ptr'][-1]), int(r1['n_ring_bonds'].sum())
    out['ring_ratio_last'] = {str(k): round(x, 3) for k, x in rep.ring_ratio(-1).items()}
    out['no_ring_first_last'] = [rep.no_ring(0), rep.no_ring(-1)]
    print(json.dumps(out))


if __name__ == '__main__':
    main()
