"""Cost of a local geometry report on the C2 shape (1h36 pocket x 100 samples with the prior sizes, the complete 1000-frame trajectory):

    python tools/geometry_bench.py [--frames 1000] [--repeats 5]

One JSON line.  The trajectory is the synthetic one of tools/quality_bench.py (a compact random cloud per sample that jitters from frame
to frame, uniformly random classes): the cost depends on the sizes and on how many bonds, angles and torsions the clouds have, not on
the chemistry.  Timed with HIP events on the current stream after one untimed call, the median of ``repeats`` and every value reported,
all in one process on the same packed device tensors (check=False: no host look at the offsets):

  * ``geometry_all_ms`` / ``geometry_last_ms``              capi.geometry_report with the default profiles' element and category
                                                            filters but no ring filter, and the clash pass, on all frames / on the
                                                            final poses;
  * ``geometry_ring_all_ms`` / ``geometry_ring_last_ms``    the same with the default profiles as they are (three of them filter on the
                                                            ring), bond_ptr and bond_ring made beforehand and not timed;
  * ``geometry_no_clash_all_ms``                            the first without the clash pass;
  * ``bond_graph_all_ms`` / ``bond_graph_last_ms``          capi.bond_graph (the eight default profiles, fragments and bond_ptr) beside them;
  * ``ring_report_all_ms`` / ``ring_report_last_ms``        capi.ring_report with the per-bond outputs, which the ring filter needs;
  * ``sample_geometry_all_ms`` / ``sample_geometry_last_ms``  quality.sample_geometry: host packing, the copy to the device, the three
                                                            launches, the copy back.

``angles_last``, ``torsions_last``, ``clashes_last`` and ``crowded_last`` say what the clouds held, so that a time can be read against
the work it paid for.
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
    ringed = quality._cosine_profiles(quality.default_geometry_profiles())
    plain = [(k, z, c, 'any', e) for k, z, c, _, e in ringed]
    thr = quality.clash_thresholds()
    geo = lambda p, c, prof, t=thr, bp=None, br=None: capi.geometry_report(p, c, ptr, cz, aro, prof, None, t, bp, br, False, check=False)
    out['geometry_all_ms'] = event_ms(lambda: geo(pos, v, plain), reps)
    out['geometry_last_ms'] = event_ms(lambda: geo(pos1, v1, plain), reps)
    out['geometry_no_clash_all_ms'] = event_ms(lambda: geo(pos, v, plain, None), reps)
    out['bond_graph_all_ms'] = event_ms(lambda: capi.bond_graph(pos, v, ptr, cz, aro, bprof, None, True, True, check=False), reps)
    out['bond_graph_last_ms'] = event_ms(lambda: capi.bond_graph(pos1, v1, ptr, cz, aro, bprof, None, True, True, check=False), reps)
    g, g1 = (capi.bond_graph(p, c, ptr, cz, aro, (), None, False, True, check=False) for p, c in ((pos, v), (pos1, v1)))
    out['ring_report_all_ms'] = event_ms(lambda: capi.ring_report(pos, v, ptr, cz, aro, None, g['bond_ptr'], False, check=False), reps)
    out['ring_report_last_ms'] = event_ms(lambda: capi.ring_report(pos1, v1, ptr, cz, aro, None, g1['bond_ptr'], False, check=False), reps)
    r = capi.ring_report(pos, v, ptr, cz, aro, None, g['bond_ptr'], False, check=False)
    r1 = capi.ring_report(pos1, v1, ptr, cz, aro, None, g1['bond_ptr'], False, check=False)
    out['geometry_ring_all_ms'] = event_ms(lambda: geo(pos, v, ringed, thr, g['bond_ptr'], r['bond_ring']), reps)
    out['geometry_ring_last_ms'] = event_ms(lambda: geo(pos1, v1, ringed, thr, g1['bond_ptr'], r1['bond_ring']), reps)
    out['sample_geometry_all_ms'] = event_ms(lambda: quality.sample_geometry(res, 'all'), reps)
    out['sample_geometry_last_ms'] = event_ms(lambda: quality.sample_geometry(res, -1), reps)
    last = geo(pos1, v1, ringed, thr, g1['bond_ptr'], r1['bond_ring'])
    rep = quality.sample_geometry(res, 'all')
    assert int(last['n_clashes'].sum()) == int(rep.sum_clashes[-1]) and int(last['n_angles'].sum()) == int(rep.n_angles[-1])
    assert int(last['hist'].sum()) == int(rep.hist[-1].sum())
    out['angles_last'], out['torsions_last'] = int(last['n_angles'].sum()), int(last['n_torsions'].sum())
    out['clashes_last'], out['crowded_last'] = int(last['n_clashes'].sum()), int(last['n_crowded'].sum())
    out['clash_free_first_last'] = [rep.clash_free(0), rep.clash_free(-1)]
    print(json.dumps(out))


if __name__ == '__main__':
    main()
