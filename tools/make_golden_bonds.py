"""Fixtures of the bond graph from the REAL reference (build container only: needs the reference tree and scipy):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_bonds.py [--reference DIR] [name ...]

Imports the reference's utils/evaluation/{analyze, eval_bond_length, eval_bond_length_config}.py unmodified, as
tools/make_golden_quality.py does, and records for a pack of frames [S, N_l, 3] of B molecules ("Bond graph"):

  * per pair i < j of every molecule  analyze.get_bond_order on the float64 distance check_stability forms: ``pair_order`` (uint8, all
                  pairs in (frame, molecule, i, j) order) and from it the bond list ``bond_atoms`` [nb, 2], ``bond_order``,
                  ``bond_category`` (the order, or 4 when both classes are aromatic and the order is 1 or 2), ``bond_length``
                  (float64) and ``bond_ptr`` [S * B + 1];
  * per molecule  scipy.sparse.csgraph.connected_components of the bonds: ``fragment`` [S, N_l] (the smallest index of each atom's
                  component), ``n_fragments``, ``largest_fragment`` and ``n_bonds`` [S, B];
  * per frame, over the molecules of ``include``: eval_bond_length.get_bond_length_profile of the ((z1, z2, category), d) list as
                  ``profile_dist`` [S, 8, bins + 1] (NaN rows where the reference's profile has no such key) with ``profile_n``
                  [S, 8] entries, and eval_bond_length_profile against the reference's EMPIRICAL_DISTRIBUTIONS as ``profile_js``
                  [S, 8] (NaN where it gives None), the eight types in the order of targetdiff_amd.quality.BOND_TYPES.

The packs are those of the quality fixtures (tests/golden/quality_{docked, thresholds, sizes}.npz; of quality_sizes the eight
molecules of up to 300 atoms).  Files: bonds_docked, bonds_thresholds, bonds_sizes and bonds_reference_distributions (the
reference's eight empirical bond-length distributions as plain arrays).  Fixed zip timestamps: a second run reproduces them bit for bit.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

from make_golden_quality import GOLDEN, load_reference, save  # noqa: E402


def record(ref, pos, v, ptr, include=None):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    from targetdiff_amd.quality import BOND_TYPES, class_aromatic, class_atomic_numbers
    A = ref.analyze
    cz, aro = np.asarray(class_atomic_numbers('add_aromatic')), np.asarray(class_aromatic('add_aromatic'))
    S, N, B = pos.shape[0], pos.shape[1], len(ptr) - 1
    assert pos.dtype == np.float32
    nbins = len(ref.config.DISTANCE_BINS) + 1
    out = dict(n_bonds=np.zeros((S, B), np.int32), n_fragments=np.zeros((S, B), np.int32), largest_fragment=np.zeros((S, B), np.int32),
               fragment=np.zeros((S, N), np.int32), bond_ptr=np.zeros(S * B + 1, np.int64), profile_n=np.zeros((S, len(BOND_TYPES)), np.int64),
               profile_dist=np.full((S, len(BOND_TYPES), nbins), np.nan), profile_js=np.full((S, len(BOND_TYPES)), np.nan))
    pair_order, atoms, order, cat, length = [], [], [], [], []
    for s in range(S):
        lengths = []
        for g in range(B):
            a, b = int(ptr[g]), int(ptr[g + 1])
            n = b - a
            p64, c = pos[s, a:b].astype(np.float64), v[s, a:b]
            z = [int(x) for x in cz[c]]
            rows, cols = [], []
            for i in range(n):
                for j in range(i + 1, n):
                    dist = np.sqrt(np.sum((p64[i] - p64[j]) ** 2))                   # analyze.check_stability's distance
                    o = A.get_bond_order(A.atom_decoder[z[i]], A.atom_decoder[z[j]], dist)
                    pair_order.append(o)
                    if o > 0:
                        k = 4 if aro[c[i]] and aro[c[j]] and o <= 2 else o
                        rows.append(i); cols.append(j)
                        atoms.append((a + i, a + j)); order.append(o); cat.append(k); length.append(dist)
                        if include is None or include[s, g]:
                            lengths.append(((z[i], z[j], k), dist))
            out['n_bonds'][s, g] = len(rows)
            out['bond_ptr'][s * B + g + 1] = out['bond_ptr'][s * B + g] + len(rows)
            if n:
                nc, lab = connected_components(csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n)), directed=False)
                first = np.full(nc, n)
                np.minimum.at(first, lab, np.arange(n))
                out['fragment'][s, a:b] = first[lab]
                out['n_fragments'][s, g], out['largest_fragment'][s, g] = nc, np.bincount(lab).max()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            profile = ref.bond_length.get_bond_length_profile(lengths)
        metrics = ref.bond_length.eval_bond_length_profile(profile)
        for p, t in enumerate(BOND_TYPES):
            out['profile_n'][s, p] = sum(1 for bt, _ in lengths if ref.bond_length._format_bond_type(bt) == t)
            if t in profile:
                out['profile_dist'][s, p] = profile[t]
            val = metrics['JSD_' + ref.bond_length._bond_type_str(t)]
            if val is not None:
                out['profile_js'][s, p] = val
    out.update(pair_order=np.asarray(pair_order, np.uint8), bond_atoms=np.asarray(atoms, np.int32).reshape(-1, 2),
               bond_order=np.asarray(order, np.uint8), bond_category=np.asarray(cat, np.uint8), bond_length=np.asarray(length, np.float64))
    return out


def gen_docked(ref):
    g = np.load(os.path.join(GOLDEN, 'quality_docked.npz'))
    r = record(ref, g['pos'], g['v'], g['ptr'])
    rings = r['n_bonds'] - np.diff(g['ptr'])[None] + r['n_fragments']
    print('docked: bonds', r['n_bonds'][0].tolist(), 'fragments', r['n_fragments'][0].tolist(), 'rings', rings[0].tolist())
    assert (r['n_bonds'][0, 0], r['n_fragments'][0, 0], rings[0, 0]) == (27, 1, 3) and r['n_fragments'][0, 1:].tolist() == [3, 3, 8, 16]
    save('bonds_docked', **r)


def gen_thresholds(ref):
    g = np.load(os.path.join(GOLDEN, 'quality_thresholds.npz'))
    r = record(ref, g['pos'], g['v'], g['ptr'])
    assert set(r['n_fragments'][0].tolist()) == {1, 2} and np.array_equal(r['n_fragments'][0], 2 - r['n_bonds'][0])
    assert np.array_equal(r['pair_order'], g['nr_bonds'][0, ::2])
    print('thresholds: bonded', int(r['n_bonds'].sum()), 'of', r['n_bonds'].size)
    save('bonds_thresholds', **r)


def gen_sizes(ref):
    g = np.load(os.path.join(GOLDEN, 'quality_sizes.npz'))
    ptr = g['ptr'][:9]                                                   # the ninth molecule (600 atoms) is above TD_BOND_MAX_ATOMS
    assert np.diff(ptr).tolist() == [0, 1, 2, 63, 64, 65, 130, 300]
    N = int(ptr[-1])
    pos, v, include = g['pos'][:, :N], g['v'][:, :N], g['include'][:, :8]
    r = record(ref, pos, v, ptr, include)
    print('sizes: bonds', r['n_bonds'].tolist(), 'fragments', r['n_fragments'].tolist(), 'profile entries', r['profile_n'].sum(0).tolist())
    save('bonds_sizes', pos=pos, v=v, ptr=ptr, include=include, **r)


def gen_reference_distributions(ref):
    from targetdiff_amd.quality import BOND_TYPES
    emp = ref.config.EMPIRICAL_DISTRIBUTIONS
    assert set(emp) == set(BOND_TYPES) == set(ref.config.BOND_TYPES)
    save('bonds_reference_distributions', bond_types=np.asarray(BOND_TYPES, np.int64),
         distributions=np.asarray([emp[t] for t in BOND_TYPES], np.float64), distance_bins=np.asarray(ref.config.DISTANCE_BINS, np.float64))


GENERATORS = {'docked': gen_docked, 'thresholds': gen_thresholds, 'sizes': gen_sizes, 'reference_distributions': gen_reference_distributions}


def main(argv):
    from oracle.reference_loader import REFERENCE_ROOT as ref_dir
    sys.dont_write_bytecode = True          # the reference tree is read-only by contract
    if '--reference' in argv:
        i = argv.index('--reference')
        ref_dir = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    ref = load_reference(ref_dir)
    for name in (argv or list(GENERATORS)):
        GENERATORS[name](ref)


if __name__ == '__main__':
    main(sys.argv[1:])
