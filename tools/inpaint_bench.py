"""Step time of scaffold-constrained sampling against the unconstrained step, on the C2 shape (1h36 pocket x 100 samples, prior sizes):

    python tools/inpaint_bench.py [--tree DIR] [--steps 60] [--warmup 10] [--repeats 3] [--fraction 0.4] [--graph]

One JSON line: the library's build tag, ms per step with no mask and -- where the tree has the feature -- with the first
``fraction`` of every ligand's atoms fixed (known positions = the initial ones, known types = the initial ones: the cost does not
depend on the values).  Timing is bench.py's: ``warmup`` untimed steps, then ``steps`` steps between two device synchronisations,
wall clock; ``repeats`` fresh samplers, the median and every value reported.  ``--graph`` runs the steps on a side stream, where the
step replays as a captured hipGraph; the default is bench.py's (the device's default stream, launch by launch).

``--tree DIR`` imports targetdiff_amd from another checkout (with its own built library): the way to time the parent commit and this
one inside the same GPU visit, each in a process of its own.  The yardstick for "the unmasked step did not get slower" is the parent;
the margin is the spread between two runs of the parent inside the same visit (EXPERIMENTS.md).
"""
from __future__ import annotations

import argparse
import contextlib
import inspect
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default=None, help='checkout to import targetdiff_amd from (default: this one)')
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--fraction', type=float, default=0.4)
    ap.add_argument('--graph', action='store_true')
    ap.add_argument('--label', default='')
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tree = os.path.abspath(args.tree) if args.tree else here
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    from targetdiff_amd import capi, workloads
    from targetdiff_amd.models import ScorePosNet3D
    assert os.path.abspath(os.path.dirname(os.path.dirname(capi.__file__))) == tree, capi.__file__
    sys.path.insert(1, here)
    from oracle import weights

    dev = torch.device('cuda:0')
    with np.load(os.path.join(here, 'tests', 'golden', 'pocket_1h36.npz')) as z:
        pocket, sizes = workloads.Pocket(z['pos'], z['feat'].astype(np.int64), '1h36_pocket10'), [int(s) for s in z['prior_sizes_seed2021']]
    model = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG), 27, 13)
    model.load_state_dict(weights.make_state_dict(2021), strict=False)
    model = model.to(dev).eval()
    batch = workloads.pack_samples([pocket], 100, sizes).to(dev)
    gen = torch.Generator(device='cpu').manual_seed(2021)
    lpos, lv = workloads.init_ligand(workloads.pack_samples([pocket], 100, sizes), generator=gen)
    lpos, lv = lpos.to(dev), lv.to(dev)
    has_feature = 'fixed_mask' in inspect.signature(model.begin_sampling).parameters
    start = np.cumsum([0] + sizes)
    mask = torch.zeros(lpos.shape[0], dtype=torch.bool)
    for g, n in enumerate(sizes):
        mask[start[g]:start[g] + int(round(args.fraction * n))] = True
    mask = mask.to(dev)
    stream = torch.cuda.Stream(device=dev) if args.graph else None

    def timed(extra):
        torch.manual_seed(2021)
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            s = model.begin_sampling(batch.protein_pos, batch.protein_atom_feature.float(), batch.protein_element_batch, lpos, lv,
                                     batch.ligand_element_batch, num_steps=args.warmup + args.steps, center_pos_mode='protein',
                                     max_graph_nodes=pocket.num_atoms + max(sizes), **extra)
            for _ in range(args.warmup):
                s.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            replay = s.session.last_step_was_graph()
        return ms, replay

    out = {'label': args.label, 'tree': os.path.relpath(tree, here), 'build_tag': capi.build_tag(), 'has_feature': has_feature,
           'steps': args.steps, 'warmup': args.warmup, 'n_ligand_atoms': int(lpos.shape[0]), 'fixed_atoms': int(mask.sum()),
           'graph_replay': None}
    plain, masked = [], []
    for _ in range(args.repeats):          # interleaved: drift of the machine hits both alike
        ms, out['graph_replay'] = timed({})
        plain.append(round(ms, 4))
        if has_feature:
            masked.append(round(timed(dict(fixed_mask=mask, fixed_pos=lpos.clone(), fixed_v=lv.clone()))[0], 4))
    out['unmasked_ms_per_step'] = {'median': statistics.median(plain), 'all': plain}
    if has_feature:
        out['masked_ms_per_step'] = {'median': statistics.median(masked), 'all': masked}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
