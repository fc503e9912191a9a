"""Step time of clash-guided sampling against the unguided step, on the C2 shape (1h36 pocket x 100 samples, prior sizes):

    python tools/guidance_bench.py [--tree DIR] [--steps 60] [--warmup 10] [--repeats 3] [--radius 3.0] [--graph] [--kernel-only N]

One JSON line: the library's build tag, ms per step unguided and -- where the tree has the feature -- guided (``ClashGuidance(radius)``
with the default weight and cap: the cost does not depend on them), both in one process, interleaved.  Timing is bench.py's:
``warmup`` untimed steps, then ``steps`` steps between two device synchronisations, wall clock; ``repeats`` fresh samplers, the median
and every value reported.  ``--graph`` runs the steps on a side stream, where the step replays as a captured hipGraph; the default is
bench.py's (the device's default stream, launch by launch).

``--kernel-only N``: instead, N calls of the stateless shift kernel on the C2 pack's initial state and nothing else -- the process to
put under ``rocprofv3 --kernel-trace --stats`` for the kernel's own duration.

``--tree DIR`` imports targetdiff_amd from another checkout (with its own built library): the way to time the parent commit and this
one inside the same GPU visit, each in a process of its own.  The yardstick for "the unguided step did not get slower" is the parent;
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
    ap.add_argument('--radius', type=float, default=3.0)
    ap.add_argument('--graph', action='store_true')
    ap.add_argument('--kernel-only', type=int, default=0)
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
    batch = workloads.pack_samples([pocket], 100, sizes).to(dev)
    gen = torch.Generator(device='cpu').manual_seed(2021)
    lpos, lv = workloads.init_ligand(workloads.pack_samples([pocket], 100, sizes), generator=gen)
    lpos, lv = lpos.to(dev), lv.to(dev)
    out = {'label': args.label, 'tree': os.path.relpath(tree, here), 'build_tag': capi.build_tag(), 'n_ligand_atoms': int(lpos.shape[0]),
           'n_protein_atoms': int(batch.protein_pos.shape[0]), 'graphs': 100}

    if args.kernel_only > 0:
        from targetdiff_amd import guidance
        pptr, lptr = capi.graph_ptr(batch.protein_element_batch, 100), capi.graph_ptr(batch.ligand_element_batch, 100)
        sigma = torch.full((batch.protein_pos.shape[0],), args.radius, dtype=torch.float32, device=dev)
        ppos = batch.protein_pos.contiguous().float()
        shift = torch.empty_like(lpos)
        for _ in range(args.kernel_only):
            capi.clash_shift(ppos, sigma, pptr, lptr, lpos, guidance.DEFAULT_WEIGHT, guidance.DEFAULT_MAX_SHIFT, out=shift, check=False)
        torch.cuda.synchronize()
        out.update(kernel_calls=args.kernel_only, moved_atoms=int((shift.abs().sum(-1) > 0).sum()))
        print(json.dumps(out))
        return

    model = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG), 27, 13)
    model.load_state_dict(weights.make_state_dict(2021), strict=False)
    model = model.to(dev).eval()
    has_feature = 'guidance' in inspect.signature(model.begin_sampling).parameters
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

    out.update(has_feature=has_feature, steps=args.steps, warmup=args.warmup, radius=args.radius, graph_replay=None)
    plain, guided = [], []
    for _ in range(args.repeats):          # interleaved: drift of the machine hits both alike
        ms, out['graph_replay'] = timed({})
        plain.append(round(ms, 4))
        if has_feature:
            from targetdiff_amd.guidance import ClashGuidance
            guided.append(round(timed(dict(guidance=ClashGuidance(radius=args.radius)))[0], 4))
    out['unguided_ms_per_step'] = {'median': statistics.median(plain), 'all': plain}
    if has_feature:
        out['guided_ms_per_step'] = {'median': statistics.median(guided), 'all': guided}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
