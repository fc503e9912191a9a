"""Recorded fingerprints of the docked pack (tests/golden/quality_docked.npz), as the pure-Python restatement gives them:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_fingerprints.py

Writes tests/golden/fingerprint_known.npz: ``fp_words`` [1, 5, 32] int64, ``n_bits`` [1, 5] int32, ``key`` [1, 5] int64 and ``atom_key``
[1, N] int64 at radius 2 and 8 key rounds, and ``key_r0`` / ``n_bits_r0`` at radius 0 and no further round.  The file pins the hash
definition ("Fingerprints and diversity": the mixing function, the invariant's layout, the round update, the key)
against silent change: the restatement and the kernel are both held to it.  Needs no GPU and no reference tree; fixed zip timestamps: a
second run reproduces the file bit for bit.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(2, os.path.join(ROOT, 'tests'))

from make_golden_quality import GOLDEN, save  # noqa: E402


def main():
    import _fingerprint_ref as FR
    from targetdiff_amd.quality import class_aromatic, class_atomic_numbers
    cz, aro = class_atomic_numbers('add_aromatic'), class_aromatic('add_aromatic')
    with np.load(os.path.join(GOLDEN, 'quality_docked.npz')) as z:
        pos, v, ptr = z['pos'], z['v'], z['ptr']
    r = FR.fingerprints(pos, v, ptr, cz, aro, 2, 8)
    r0 = FR.fingerprints(pos, v, ptr, cz, aro, 0, 0)
    save('fingerprint_known', fp_words=r['fp_words'], n_bits=r['n_bits'], key=r['key'], atom_key=r['atom_key'], key_r0=r0['key'],
         n_bits_r0=r0['n_bits'])


if __name__ == '__main__':
    main()
