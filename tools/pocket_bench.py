"""Cost of a pocket contact report on the C2 shape (1h36 pocket x 100 samples with the prior sizes, the complete 1000-frame trajectory):

    python tools/pocket_bench.py [--frames 1000] [--repeats 5] [--lib OTHER/libtargetdiff_hip.so]

One JSON line.  The trajectory is the synthetic one of tools/quality_bench.py (a compact random cloud per sample that jitters from frame
to frame, uniformly random classes), moved to the centroid of the pocket's docked ligand so that the clouds sit where ligands do: the
cost depends on the sizes and on how many pairs fall below the limits, not on the chemistry.  Timed with HIP events on the current
stream after one untimed call, the median of ``repeats`` and every value reported, all in one process on the same packed device tensors
(check=False: no host look at the offsets):

  * ``pocket_all_ms`` / ``pocket_last_ms``          capi.pocket_report with the 40 residue kinds, the 4 A cutoff and the clash table, no
                                                    per-atom outputs and no bits, on all frames / on the final poses;
  * ``pocket_full_all_ms``                          the first with the per-atom outputs and the bits;
  * ``pocket_no_clash_all_ms``                      the first without the clash pass;
  * ``geometry_all_ms`` / ``geometry_last_ms``      capi.geometry_report on the same pack (the default profiles without a ring filter, and
                                                    the clash pass), for scale;
  * ``clash_report_ms``                             capi.clash_report (guidance: one radius per protein atom, one pose per graph, fp32) on
                                                    the same pocket x the 100 final poses, for scale;
  * ``sample_pocket_all_ms`` / ``sample_pocket_last_ms``  quality.sample_pocket: host packing, the copy to the device, the launch, the
                                                    copy back.

``pairs_per_frame`` is ligand atoms with a class x protein atoms that take part; ``pair_rate_all_per_s`` is pairs / ``pocket_all_ms``.
``contacts_last``, ``clashes_last`` and ``no_contact_last`` say what the clouds held.
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
    res = ([p[-1] for p in pos_traj], res[1], pos_traj, res[3], [], [], [0.0])
    result = {'data': types.SimpleNamespace(protein_pos=ppos_np, protein_atom_feature=feat), 'pred_ligand_pos_traj': res[2],
              'pred_ligand_v_traj': res[3]}
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    reps = max(5, args.repeats)
    out = {'build_tag': capi.build_tag(), 'samples': len(sizes), 'frames': args.frames, 'atoms_per_frame': int(sum(sizes)),
           'largest_sample': max(sizes), 'protein_atoms': int(len(ppos_np)), 'repeats': reps}
    pos = torch.from_numpy(np.concatenate(res[2], axis=1).astype(np.float32)).to(dev)
    v = torch.from_numpy(np.concatenate(res[3], axis=1)).to(dev)
    ptr = torch.as_tensor(np.cumsum([0] + sizes), dtype=torch.int32, device=dev)
    pos1, v1 = pos[-1:].contiguous(), v[-1:].contiguous()
    cz, aro = quality.class_atomic_numbers('add_aromatic'), quality.class_aromatic('add_aromatic')
    side = quality.PocketSide((ppos_np, feat), dev)
    ppos, elem, (kind, names) = side.pos, side.elem, side.kinds()
    thr = quality.pocket_clash_thresholds()
    poc = lambda p, c, t=thr, full=False: capi.pocket_report(p, c, ptr, cz, ppos, elem, kind, len(names), quality.DEFAULT_CONTACT_CUTOFF, t,
                                                              None, None, full, full, check=False)
    out['pocket_all_ms'] = event_ms(lambda: poc(pos, v), reps)
    out['pocket_last_ms'] = event_ms(lambda: poc(pos1, v1), reps)
    out['pocket_full_all_ms'] = event_ms(lambda: poc(pos, v, thr, True), reps)
    out['pocket_no_clash_all_ms'] = event_ms(lambda: poc(pos, v, None), reps)
    plain = [(k, z, c, 'any', e) for k, z, c, _, e in quality._cosine_profiles(quality.default_geometry_profiles())]
    gthr = quality.clash_thresholds()
    geo = lambda p, c: capi.geometry_report(p, c, ptr, cz, aro, plain, None, gthr, None, None, False, check=False)
    out['geometry_all_ms'] = event_ms(lambda: geo(pos, v), reps)
    out['geometry_last_ms'] = event_ms(lambda: geo(pos1, v1), reps)
    B, Np = len(sizes), len(ppos_np)
    ppos_b = ppos.repeat(B, 1).contiguous()
    sigma = torch.full((B * Np,), 3.0, dtype=torch.float32, device=dev)
    pptr = torch.arange(B + 1, dtype=torch.int32, device=dev) * Np
    lpos = pos1[0].contiguous()
    capi.clash_report(ppos_b, sigma, pptr, ptr, lpos)                            # its host look at the offsets is part of every call
    out['clash_report_ms'] = event_ms(lambda: capi.clash_report(ppos_b, sigma, pptr, ptr, lpos), reps)
    out['sample_pocket_all_ms'] = event_ms(lambda: quality.sample_pocket(result, 'all'), reps)
    out['sample_pocket_last_ms'] = event_ms(lambda: quality.sample_pocket(result, -1), reps)
    last = poc(pos1, v1)
    rep = quality.sample_pocket(result, 'all')
    assert int(last['n_contacts'].sum()) == int(rep.sum_contacts[-1]) and int(last['n_clashes'].sum()) == int(rep.sum_clashes[-1])
    assert int(last['kind_hist'].sum()) == int(rep.kind_hist[-1].sum()) == int(last['n_contacts'].sum())
    takes_part = int(((elem >= 0) & (kind >= 0)).sum())
    out['pairs_per_frame'] = int(sum(sizes)) * takes_part
    out['pair_rate_all_per_s'] = round(out['pairs_per_frame'] * args.frames / (out['pocket_all_ms']['median'] * 1e-3))
    out['contacts_last'], out['clashes_last'] = int(last['n_contacts'].sum()), int(last['n_clashes'].sum())
    out['no_contact_last'], out['buried_share_last'] = rep.no_contact(-1), rep.buried_share(-1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
