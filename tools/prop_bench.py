"""Throughput of the binding-affinity predictor (PropPredNet, configs/prop/pdbbind_general_egnn.yml: hidden 256, 6 layers, k = 48)
on the 1h36 pocket with B docked-ligand copies (jittered, seeded): complexes per second for each B, one JSON line with the build tag.

    python tools/prop_bench.py [--batches 1,16,100] [--iters 20] [--warmup 3] [--rocprof]

--rocprof re-runs the B = 100 case in a child process under `rocprofv3 --kernel-trace --stats` (its own time limit) and prints the
per-kernel split.  FLOPs: per edge the two edge Linears execute 2 * 256 * (256 + 64) = 164 kFLOP (the 512-wide h_i / h_j part of the
first Linear runs once per node); the line reports the fraction of the fp32 matrix peak (157.3 TFLOP/s, MI355X) they reach.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

FP32_MATRIX_PEAK = 157.3e12


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
    res = {}
    for B in batches:
        b = P.batch_of([P.complex_1h36(seed=s, jitter=0.5) for s in range(B)])
        args = [torch.from_numpy(np.ascontiguousarray(b[k])).to(dev) for k in
                ('protein_pos', 'protein_feat', 'ligand_pos', 'ligand_feat', 'batch_protein', 'batch_ligand')]
        for _ in range(warmup):
            m(*args, None)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            m(*args, None)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        N = len(b['batch_protein']) + len(b['batch_ligand'])
        edges = N * P.MODEL_CONFIG['encoder']['knn']
        flop = 6 * edges * 2 * 256 * (256 + 64)
        res[B] = {'ms': round(ms, 3), 'complexes_per_s': round(B / ms * 1e3, 1), 'nodes': N,
                  'edge_fp32_matrix_peak_fraction': round(flop / (ms * 1e-3) / FP32_MATRIX_PEAK, 3)}
    return {'metric': 'prop_complexes_per_s', 'build_tag': capi.build_tag(), 'iters': iters, 'warmup': warmup, 'results': res}


def rocprof(out_dir):
    cmd = ['timeout', '-k', '10', '300', 'rocprofv3', '--kernel-trace', '--stats', '-d', out_dir, '-o', 'prop', '--output-format', 'csv', '--',
           sys.executable, os.path.abspath(__file__), '--batches', '100', '--iters', '3', '--warmup', '1']
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
              'percent': round(float(r['Percentage']), 1)} for r in rows[:10]]
    print(json.dumps({'metric': 'prop_kernel_split_B100', 'kernels': split}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,16,100')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rocprof', action='store_true')
    ap.add_argument('--rocprof-dir', default='prop_rocprof', help='where rocprofv3 writes its CSV files')
    a = ap.parse_args()
    if a.rocprof:
        sys.exit(rocprof(a.rocprof_dir))
    print(json.dumps(run([int(x) for x in a.batches.split(',')], a.iters, a.warmup)))


if __name__ == '__main__':
    main()
