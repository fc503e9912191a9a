"""Training throughput of the binding-affinity predictor (PropPredNet, configs/prop/pdbbind_general_egnn.yml: hidden 256, 6 layers,
k = 48): steps per second of get_loss + backward + clip_grad_norm_ + Adam on batches of 1h36 + docked-ligand copies (jittered, seeded),
with the forward (td_prop_forward_train) and the backward (td_prop_backward) timed on their own.  One JSON line with the build tag.

    python tools/prop_train_bench.py [--batches 4,16,100] [--iters 10] [--warmup 2] [--rocprof]

B = 4 is the configs' batch_size.  FLOPs executed per edge: forward 2 * 256 * (256 + 64) = 164 kFLOP; backward 459 kFLOP = the
recompute (164), W2^T dz2 (131), dW2 (131) and dW1r (33).  The line reports the fraction of the fp32 matrix peak (157.3 TFLOP/s,
MI355X) each pass reaches on those counts.  --rocprof re-runs the B = 100 case in a child process under
`rocprofv3 --kernel-trace --stats` (its own time limit) and prints the per-kernel split.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

FP32_MATRIX_PEAK = 157.3e12
FWD_EDGE_FLOP = 2 * 256 * (256 + 64)
BWD_EDGE_FLOP = FWD_EDGE_FLOP + 2 * 256 * 256 * 2 + 2 * 256 * 64


def run(batches, iters, warmup):
    import numpy as np
    import torch
    import _prop_ref as P
    from targetdiff_amd import capi, prop
    dev = torch.device('cuda:0')
    m = prop.PropPredNet(P.MODEL_CONFIG, P.PROTEIN_FEAT_DIM, P.LIGAND_FEAT_DIM)
    spec = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    m.load_state_dict(P.make_state_dict(spec, 2024), strict=True)
    m = m.to(dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    res = {}
    for B in batches:
        b = P.batch_of([P.complex_1h36(seed=s, jitter=0.5) for s in range(B)])
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in b.items()}
        batch = types.SimpleNamespace(protein_pos=t['protein_pos'], protein_atom_feature=t['protein_feat'], ligand_pos=t['ligand_pos'],
                                      ligand_atom_feature_full=t['ligand_feat'], protein_element_batch=t['batch_protein'],
                                      ligand_element_batch=t['batch_ligand'], kind=torch.tensor([1 + s % 3 for s in range(B)], device=dev),
                                      y=torch.linspace(4, 8, B, device=dev))
        ev = lambda: torch.cuda.Event(enable_timing=True)
        fwd = bwd = step = 0.0
        for it in range(warmup + iters):
            e = [ev() for _ in range(4)]
            e[0].record()
            opt.zero_grad()
            loss = m.get_loss(batch, pos_noise_std=0.1)
            e[1].record()
            loss.backward()
            e[2].record()
            torch.nn.utils.clip_grad_norm_(m.parameters(), 8.0)
            opt.step()
            e[3].record()
            torch.cuda.synchronize()
            if it >= warmup:
                fwd += e[0].elapsed_time(e[1])
                bwd += e[1].elapsed_time(e[2])
                step += e[0].elapsed_time(e[3])
        fwd, bwd, step = fwd / iters, bwd / iters, step / iters
        N = len(b['batch_protein']) + len(b['batch_ligand'])
        edges = 6 * N * P.MODEL_CONFIG['encoder']['knn']
        res[B] = {'step_ms': round(step, 3), 'steps_per_s': round(1e3 / step, 2), 'forward_ms': round(fwd, 3), 'backward_ms': round(bwd, 3),
                  'nodes': N, 'forward_edge_fp32_matrix_peak_fraction': round(edges * FWD_EDGE_FLOP / (fwd * 1e-3) / FP32_MATRIX_PEAK, 3),
                  'backward_edge_fp32_matrix_peak_fraction': round(edges * BWD_EDGE_FLOP / (bwd * 1e-3) / FP32_MATRIX_PEAK, 3),
                  'workspace_bytes_per_node': int(m._native.lib.td_prop_train_workspace_bytes(
                      m._native.handle, len(b['batch_protein']), len(b['batch_ligand']), B)) // N}
    return {'metric': 'prop_train_steps_per_s', 'build_tag': capi.build_tag(), 'iters': iters, 'warmup': warmup, 'results': res}


def rocprof(out_dir):
    cmd = ['timeout', '-k', '10', '300', 'rocprofv3', '--kernel-trace', '--stats', '-d', out_dir, '-o', 'prop_train', '--output-format',
           'csv', '--', sys.executable, os.path.abspath(__file__), '--batches', '100', '--iters', '2', '--warmup', '1']
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f'rocprofv3 run failed with exit status {rc}', file=sys.stderr)
        return rc
    stats = sorted(glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True))
    if not stats:
        print('no kernel_stats.csv written', file=sys.stderr)
        return 1
    with open(stats[-1]) as f:
        rows = list(csv.DictReader(f))
    split = [{'kernel': r['Name'][:60], 'calls': int(r['Calls']), 'total_ms': round(float(r['TotalDurationNs']) / 1e6, 3),
              'percent': round(float(r['Percentage']), 1)} for r in rows[:12]]
    print(json.dumps({'metric': 'prop_train_kernel_split_B100', 'kernels': split}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='4,16,100')
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rocprof', action='store_true')
    ap.add_argument('--rocprof-dir', default='prop_train_rocprof', help='where rocprofv3 writes its CSV files')
    a = ap.parse_args()
    if a.rocprof:
        sys.exit(rocprof(a.rocprof_dir))
    print(json.dumps(run([int(x) for x in a.batches.split(',')], a.iters, a.warmup)))


if __name__ == '__main__':
    main()
