"""Cost of a sample-quality report on the C2 shape (1h36 pocket x 100 samples with the prior sizes, the complete 1000-frame trajectory):

    python tools/quality_bench.py [--frames 1000] [--repeats 5] [--cpu-frames 5]

One JSON line.  The trajectory is synthetic in the driver's format (per sample [frames, n_i, 3] float64 holding fp32 values and
[frames, n_i] classes): a compact random cloud per sample, N(0, 1.6 A) per coordinate, that jitters by N(0, 0.1 A) from frame to frame,
with uniformly random classes -- the cost of the report depends on the sizes, not on the chemistry.  Timed with HIP events on the
current stream after one untimed call, the median of ``repeats`` and every value reported:

  * ``sample_quality_all_ms``   quality.sample_quality(result, 'all'): host packing, the copy to the device, one launch, the copy back;
  * ``sample_quality_last_ms``  quality.sample_quality(result, -1): the final poses only;
  * ``kernel_all_ms``           capi.quality_report alone on the packed device tensors of all frames (check=False: no host look at
                                the offsets), i.e. the memsets, the kernel and the allocation of the outputs;
  * ``kernel_last_ms``          the same on the final poses only;
  * ``bond_graph_all_ms`` / ``bond_graph_last_ms``  capi.bond_graph (the eight default bond profiles, fragments and bond_ptr asked
                                for, check=False) on the same two packs, in the same process: to be read beside the two lines above;
  * ``bond_list_last_ms``       capi.bond_list for the final poses, its one host synchronisation included.

``numpy_cpu_estimate_s``: the restated rule in vectorised numpy (tests/_quality_ref.py) on ``cpu-frames`` evenly spaced frames in the same
process, scaled to all frames -- an estimate, labelled as one; the reference's own per-molecule Python double loop is slower still and
is not on this machine.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, 'tests'))

from targetdiff_amd import capi, quality  # noqa: E402


def synthetic_result(sizes, frames, seed=2021):
    rng = np.random.default_rng(seed)
    pos_traj, v_traj = [], []
    for n in sizes:
        base = rng.normal(0.0, 1.6, (1, n, 3))
        pos_traj.append((base + rng.normal(0.0, 0.1, (frames, n, 3))).astype(np.float32).astype(np.float64))
        v_traj.append(rng.integers(0, 13, (frames, n)))
    return ([p[-1] for p in pos_traj], [v[-1] for v in v_traj], pos_traj, v_traj, [], [], [0.0])


def event_ms(fn, repeats):
    fn()                                        # warm-up: library load, allocator, first launch
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(round(a.elapsed_time(b), 3))
    return {'median': statistics.median(out), 'all': out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--cpu-frames', type=int, default=5)
    args = ap.parse_args()
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'pocket_1h36.npz')) as z:
        sizes = [int(s) for s in z['prior_sizes_seed2021']]
    res = synthetic_result(sizes, args.frames)
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    out = {'build_tag': capi.build_tag(), 'samples': len(sizes), 'frames': args.frames, 'atoms_per_frame': int(sum(sizes)),
           'largest_sample': max(sizes), 'repeats': max(5, args.repeats)}
    reps = max(5, args.repeats)
    out['sample_quality_all_ms'] = event_ms(lambda: quality.sample_quality(res, 'all', reference={}), reps)
    out['sample_quality_last_ms'] = event_ms(lambda: quality.sample_quality(res, -1, reference={}), reps)
    pos = torch.from_numpy(np.concatenate(res[2], axis=1).astype(np.float32)).to(dev)
    v = torch.from_numpy(np.concatenate(res[3], axis=1)).to(dev)
    ptr = torch.as_tensor(np.cumsum([0] + sizes), dtype=torch.int32, device=dev)
    cz, prof = quality.class_atomic_numbers('add_aromatic'), quality.default_profiles()
    out['kernel_all_ms'] = event_ms(lambda: capi.quality_report(pos, v, ptr, cz, prof, None, False, check=False), reps)
    pos1, v1 = pos[-1:].contiguous(), v[-1:].contiguous()
    out['kernel_last_ms'] = event_ms(lambda: capi.quality_report(pos1, v1, ptr, cz, prof, None, False, check=False), reps)
    aro, bprof = quality.class_aromatic('add_aromatic'), quality.default_bond_profiles()
    out['bond_graph_all_ms'] = event_ms(lambda: capi.bond_graph(pos, v, ptr, cz, aro, bprof, None, True, True, check=False), reps)
    out['bond_graph_last_ms'] = event_ms(lambda: capi.bond_graph(pos1, v1, ptr, cz, aro, bprof, None, True, True, check=False), reps)
    g1 = capi.bond_graph(pos1, v1, ptr, cz, aro, bprof, None, True, True, check=False)
    out['bond_list_last_ms'] = event_ms(lambda: capi.bond_list(pos1, v1, ptr, cz, aro, g1['bond_ptr'], check=False), reps)
    gall = capi.bond_graph(pos, v, ptr, cz, aro, bprof, None, True, True, check=False)
    out['bonds_last'], out['complete_first_last'] = int(g1['bond_ptr'][-1]), [int((gall['n_fragments'][k] == 1).sum()) for k in (0, -1)]
    rep = quality.sample_quality(res, 'all', reference={})
    out['atm_stable_first_last'] = [float(rep.atm_stable[0]), float(rep.atm_stable[-1])]

    import _quality_ref as QR
    pick = sorted(set(int(x) for x in np.linspace(0, args.frames - 1, max(1, args.cpu_frames))))
    pos_np, v_np, ptr_np = pos[pick].cpu().numpy(), v[pick].cpu().numpy(), ptr.cpu().numpy()
    t0 = time.perf_counter()
    want = QR.quality_report(pos_np, v_np, ptr_np, cz, prof)
    dt = time.perf_counter() - t0
    assert np.array_equal(want['hist'], rep.hist[pick]) and np.array_equal(want['stable_atoms'].sum(1), rep.stable_atoms[pick])
    out['numpy_cpu_estimate_s'] = {'frames_measured': len(pick), 'measured_s': round(dt, 3), 'scaled_to_all_frames_s': round(dt / len(pick) * args.frames, 1),
                                   'note': 'vectorised numpy restatement, scaled: an estimate'}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
