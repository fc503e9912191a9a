"""Cost of sampling time programs on the C2 shape (1h36 pocket x 100 samples, prior sizes), one process, three cases:

    python tools/program_bench.py [--calls 100] [--jump-length 10] [--resamplings 10] [--fraction 0.4] [--repeats 1] [--graph]

  default    the sampler as it was: T = 1000 unit steps, no program
  strided    TimeProgram.strided(T, calls): `calls` denoiser calls down to clean data
  jumps      the same with .with_resampling(jump_length, resamplings) and the first `fraction` of every ligand's atoms fixed

One JSON line per case: steps of either kind, ms per denoise step and per renoise step (device time between two events recorded around
every step, summed per kind), the wall time of the whole call (set-up, steps, the trajectory copy) and ligands per second from it.  A
10-step run before the first case takes the one-time set-up (module load, the first launch of every kernel) out of the figures.  The
yardstick for "a program costs nothing per denoise step" is the default case of the SAME call: machines of one pool differ by several
per cent, so a stored number does not serve.  ``--graph`` runs on a side stream, where the denoise steps replay as a captured hipGraph;
the default is bench.py's (the device's default stream, launch by launch).
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--jump-length', type=int, default=10)
    ap.add_argument('--resamplings', type=int, default=10)
    ap.add_argument('--fraction', type=float, default=0.4)
    ap.add_argument('--repeats', type=int, default=1)
    ap.add_argument('--graph', action='store_true')
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    import numpy as np
    import torch
    from oracle import weights
    from targetdiff_amd import capi, workloads
    from targetdiff_amd.models import ScorePosNet3D
    from targetdiff_amd.schedule import RENOISE, TimeProgram

    dev = torch.device('cuda:0')
    with np.load(os.path.join(here, 'tests', 'golden', 'pocket_1h36.npz')) as z:
        pocket, sizes = workloads.Pocket(z['pos'], z['feat'].astype(np.int64), '1h36_pocket10'), [int(s) for s in z['prior_sizes_seed2021']]
    model = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG), 27, 13)
    model.load_state_dict(weights.make_state_dict(2021), strict=False)
    model = model.to(dev).eval()
    T = model.num_timesteps
    batch = workloads.pack_samples([pocket], 100, sizes).to(dev)
    gen = torch.Generator(device='cpu').manual_seed(2021)
    lpos, lv = workloads.init_ligand(workloads.pack_samples([pocket], 100, sizes), generator=gen)
    lpos, lv = lpos.to(dev), lv.to(dev)
    start = np.cumsum([0] + sizes)
    mask = torch.zeros(lpos.shape[0], dtype=torch.bool)
    for g, n in enumerate(sizes):
        mask[start[g]:start[g] + int(round(args.fraction * n))] = True
    fixed = dict(fixed_mask=mask.to(dev), fixed_pos=lpos.clone(), fixed_v=lv.clone())
    stream = torch.cuda.Stream(device=dev) if args.graph else None
    strided = TimeProgram.strided(T, args.calls)

    def run(extra, kinds):
        torch.manual_seed(2021)
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s = model.begin_sampling(batch.protein_pos, batch.protein_atom_feature.float(), batch.protein_element_batch, lpos, lv,
                                     batch.ligand_element_batch, center_pos_mode='protein', max_graph_nodes=pocket.num_atoms + max(sizes),
                                     **extra)
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(s.S + 1)]
            marks[0].record()
            while not s.done:
                s.step()
                marks[s.s].record()
            r = s.finish()
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        assert torch.isfinite(r['pos']).all()
        per = [marks[k].elapsed_time(marks[k + 1]) for k in range(s.S)]
        kinds = [0] * s.S if kinds is None else kinds
        den = [ms for ms, k in zip(per, kinds) if k != RENOISE]
        ren = [ms for ms, k in zip(per, kinds) if k == RENOISE]
        return dict(steps=s.S, denoise_steps=len(den), renoise_steps=len(ren), ms_per_denoise_step=round(sum(den) / max(len(den), 1), 4),
                    ms_per_renoise_step=round(sum(ren) / len(ren), 4) if ren else None, wall_s=round(wall, 4),
                    ligands_per_s=round(100 / wall, 3), graph_replay=bool(s.session.last_step_was_graph()))

    run(dict(num_steps=10), None)          # one-time set-up
    jumps = strided.with_resampling(args.jump_length, args.resamplings)
    cases = [('default', {}, None), ('strided', dict(time_program=strided), strided.kind.tolist()),
             ('jumps', dict(time_program=jumps, **fixed), jumps.kind.tolist())]
    for name, extra, kinds in cases:
        runs = [run(extra, kinds) for _ in range(args.repeats)]
        best = sorted(runs, key=lambda x: x['wall_s'])[len(runs) // 2]
        print(json.dumps(dict(case=name, build_tag=capi.build_tag(), graph=bool(args.graph), n_ligand_atoms=int(lpos.shape[0]),
                              fixed_atoms=int(mask.sum()) if 'fixed_mask' in extra else 0, repeats=args.repeats, **best,
                              wall_s_all=[x['wall_s'] for x in runs])), flush=True)


if __name__ == '__main__':
    main()
