"""Cost of fingerprints and their comparison on the C2 shape (1h36 pocket x 100 samples with the prior sizes, the complete 1000-frame
trajectory):

    python tools/diversity_bench.py [--frames 1000] [--repeats 5]

One JSON line.  The trajectory is the synthetic one of tools/quality_bench.py, as in tools/rings_bench.py, and the times are taken the
same way: HIP events on the current stream after one untimed call, the median of ``repeats`` and every value reported, all in one process
on the same packed device tensors (check=False: no host look at the offsets):

  * ``fingerprint_all_ms`` / ``fingerprint_last_ms``       capi.fingerprint (radius 2, 8 key rounds, no atom keys) on all frames / on the final poses;
  * ``fingerprint_r0k0_all_ms``                            the same with radius 0 and no further round: what loading the molecule and building
                                                           its bit rows costs, so that the rounds' share can be read off;
  * ``similarity_all_ms`` / ``similarity_last_ms``         capi.fingerprint_similarity of those fingerprints (no pair matrix, no query set);
  * ``similarity_common_last_ms``                          the same with the [B, B] matrix of common bits and a one-molecule query set;
  * ``ring_report_all_ms`` / ``ring_report_last_ms``       capi.ring_report beside them, on the same pack;
  * ``sample_diversity_all_ms`` / ``sample_diversity_last_ms``  quality.sample_diversity: host packing, the copy to the device, both launches, the copy back.

``diversity_last``, ``uniqueness_last`` and ``mean_bits_last`` say what the clouds held.
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
    cz, aro = quality.class_atomic_numbers('add_aromatic'), quality.class_aromatic('add_aromatic')
    out['fingerprint_all_ms'] = event_ms(lambda: capi.fingerprint(pos, v, ptr, cz, aro, check=False), reps)
    out['fingerprint_last_ms'] = event_ms(lambda: capi.fingerprint(pos1, v1, ptr, cz, aro, check=False), reps)
    out['fingerprint_r0k0_all_ms'] = event_ms(lambda: capi.fingerprint(pos, v, ptr, cz, aro, 0, 0, check=False), reps)
    fp, fp1 = capi.fingerprint(pos, v, ptr, cz, aro, check=False), capi.fingerprint(pos1, v1, ptr, cz, aro, check=False)
    sim = lambda f, **kw: capi.fingerprint_similarity(f['fp_words'], f['n_bits'], f['key'], **kw)
    out['similarity_all_ms'] = event_ms(lambda: sim(fp), reps)
    out['similarity_last_ms'] = event_ms(lambda: sim(fp1), reps)
    qw, qb = fp1['fp_words'][0, :1].contiguous(), fp1['n_bits'][0, :1].contiguous()
    out['similarity_common_last_ms'] = event_ms(lambda: sim(fp1, q_words=qw, q_bits=qb, return_common=True), reps)
    out['ring_report_all_ms'] = event_ms(lambda: capi.ring_report(pos, v, ptr, cz, aro, check=False), reps)
    out['ring_report_last_ms'] = event_ms(lambda: capi.ring_report(pos1, v1, ptr, cz, aro, check=False), reps)
    out['sample_diversity_all_ms'] = event_ms(lambda: quality.sample_diversity(res, 'all'), reps)
    out['sample_diversity_last_ms'] = event_ms(lambda: quality.sample_diversity(res, -1), reps)
    rep = quality.sample_diversity(res, 'all')
    last = quality.sample_diversity(res, -1)
    assert rep.summary(-1) == last.summary(-1)
    out['diversity_last'], out['uniqueness_last'] = rep.diversity(-1), rep.uniqueness(-1)
    out['diversity_first'], out['uniqueness_first'] = rep.diversity(0), rep.uniqueness(0)
    out['mean_bits_last'] = float(fp1['n_bits'].double().mean())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
