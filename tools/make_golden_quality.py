"""Fixtures of the sample-quality metrics from the REAL reference (build container only: needs the reference tree):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_quality.py [--reference DIR] [name ...]

Imports the reference's utils/evaluation/{analyze, eval_bond_length, eval_bond_length_config, eval_atom_type}.py unmodified
(``utils.data`` is stubbed in sys.modules first: it imports RDKit and only bond_distance_from_mol, which is not called, uses it) and
records, for packs of frames [S, N_l, 3] of B molecules:

  * per molecule  analyze.check_stability(pos, atomic numbers, return_nr_bonds=True): mol_stable [S, B], stable_atoms [S, B],
                  nr_bonds [S, N_l];
  * per frame, over the molecules of ``include`` [S, B]: eval_bond_length.get_pair_length_profile of the concatenated
                  pair_distance_from_pos_v lists (dist_<profile> [S, 101], NaN rows when nothing entered), the number of entries
                  n_<profile> [S], the element Counter as counts [S, 8] (H C N O F P S Cl), and js_<profile> / js_atom_type [S] from
                  eval_pair_length_profile / eval_atom_type_distribution (NaN where the reference has nothing to compare).

Positions are fp32 and go to the reference as float64, which is what the sampler's driver hands to evaluate_diffusion.py.  The class
-> atomic number table is targetdiff_amd.quality.class_atomic_numbers('add_aromatic') (the reference's own lives in utils/transforms.py
behind an RDKit import).  Files (tests/golden/): quality_docked, quality_thresholds, quality_sizes, quality_traj and
quality_reference_distributions (the reference's two empirical pair distributions and seven type frequencies as plain arrays).
The archives are written with fixed zip timestamps, so a second run reproduces them bit for bit.
"""
from __future__ import annotations

import collections
import io
import os
import sys
import types
import warnings
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, ROOT)

ELEMENTS = (1, 6, 7, 8, 9, 15, 16, 17)
PLAIN_CLASS = {1: 0, 6: 1, 7: 3, 8: 5, 9: 7, 15: 8, 16: 10, 17: 12}       # add_aromatic class of a non-aromatic atom
PROFILES = ('CC_2A', 'All_12A')
TILE = 256                                                               # QL_TILE of csrc/quality.hip


def load_reference(path):
    sys.path.insert(0, path)
    sys.modules.setdefault('utils.data', types.ModuleType('utils.data'))
    from utils.evaluation import analyze, eval_atom_type, eval_bond_length, eval_bond_length_config
    return types.SimpleNamespace(analyze=analyze, atom_type=eval_atom_type, bond_length=eval_bond_length, config=eval_bond_length_config)


def save(name, **arrays):
    path = os.path.join(GOLDEN, name + '.npz')
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    print(f'{name}.npz: {os.path.getsize(path)} bytes')
    assert os.path.getsize(path) < 1 << 20


def record(ref, pos, v, ptr, include=None, per_atom=True):
    """the reference's results for pos [S, N, 3] fp32, v [S, N] classes, ptr [B + 1], include [S, B] bool or None"""
    from targetdiff_amd.quality import class_atomic_numbers
    cz = np.asarray(class_atomic_numbers('add_aromatic'))
    S, N, B = pos.shape[0], pos.shape[1], len(ptr) - 1
    assert pos.dtype == np.float32
    out = dict(mol_stable=np.zeros((S, B), np.uint8), stable_atoms=np.zeros((S, B), np.int32), nr_bonds=np.zeros((S, N), np.int32),
               counts=np.zeros((S, 8), np.int64), js_atom_type=np.full(S, np.nan))
    for k in PROFILES:
        out['dist_' + k], out['n_' + k], out['js_' + k] = np.full((S, 101), np.nan), np.zeros(S, np.int64), np.full(S, np.nan)
    for s in range(S):
        pairs, counter = [], collections.Counter()
        for g in range(B):
            a, b = int(ptr[g]), int(ptr[g + 1])
            p64, z = pos[s, a:b].astype(np.float64), [int(x) for x in cz[v[s, a:b]]]
            ok, ns, n, nb = ref.analyze.check_stability(p64, z, return_nr_bonds=True)
            assert n == b - a
            out['mol_stable'][s, g], out['stable_atoms'][s, g], out['nr_bonds'][s, a:b] = ok, ns, nb
            if include is None or include[s, g]:
                counter += collections.Counter(z)
                pairs += ref.bond_length.pair_distance_from_pos_v(p64, z)
        out['counts'][s] = [counter[e] for e in ELEMENTS]
        out['n_CC_2A'][s] = len([d for d in pairs if d[0] == (6, 6) and d[1] < 2])
        out['n_All_12A'][s] = len([d for d in pairs if d[1] < 12])
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                      # 0 / 0 of an empty profile
            profile = ref.bond_length.get_pair_length_profile(pairs)
        filled = {k: d for k, d in profile.items() if out['n_' + k][s] > 0}
        for k, d in filled.items():
            out['dist_' + k][s] = d
        for k, val in ref.bond_length.eval_pair_length_profile(filled).items():
            if val is not None:
                out['js_' + k[4:]][s] = val
        if sum(counter.values()) > 0:
            out['js_atom_type'][s] = ref.atom_type.eval_atom_type_distribution(counter)
    if not per_atom:
        del out['nr_bonds']
    return out


def gen_docked(ref):
    d = np.load(os.path.join(GOLDEN, 'ligand_1h36_docked.npz'))
    z = np.array([{'C': 6, 'N': 7, 'O': 8, 'Br': 17}[e] for e in d['elements']])           # Br is outside the table: written as Cl
    v1 = np.array([PLAIN_CLASS[int(x)] + (1 if x == 6 and i % 2 else 0) for i, x in enumerate(z)], dtype=np.int64)   # odd carbons aromatic
    base = d['pos'].astype(np.float32)
    sigmas = (0.05, 0.1, 0.2, 0.4)
    for seed in range(100):
        rng = np.random.default_rng(seed)
        mols = [base] + [(base.astype(np.float64) + rng.normal(0.0, s, base.shape)).astype(np.float32) for s in sigmas]
        pos = np.concatenate(mols)[None]
        v = np.tile(v1, 5)[None]
        ptr = np.arange(6, dtype=np.int32) * 25
        r = record(ref, pos, v, ptr)
        orders = set()
        for m in mols:
            from_ref = [ref.analyze.get_bond_order(ref.analyze.atom_decoder[int(z[i])], ref.analyze.atom_decoder[int(z[j])],
                                                   float(np.sqrt(np.sum((m[i].astype(np.float64) - m[j].astype(np.float64)) ** 2))))
                        for i in range(25) for j in range(i + 1, 25)]
            orders |= set(from_ref)
        if r['mol_stable'][0].tolist() == [1, 0, 0, 0, 0] and orders == {0, 1, 2, 3}:
            break
    else:
        raise AssertionError('no seed gives a stable original, unstable copies and all bond orders')
    print('docked: seed', seed, 'stable atoms', r['stable_atoms'][0].tolist(), 'of 25; molecule-stable', r['mol_stable'][0].tolist())
    save('quality_docked', pos=pos, v=v, ptr=ptr, seed=np.int64(seed), sigmas=np.array(sigmas),
         note=np.array('tests/golden/ligand_1h36_docked.npz with its Br written as Cl (Br is outside the bond-length table), then four '
                       'fp32 copies jittered by N(0, sigma) per coordinate, default_rng(seed)'), **r)


def fp32_order(ref, p32, z):
    """the rule with fp32 arithmetic throughout: what a kernel that skips float64 would compute"""
    d = p32[0] - p32[1]
    dist = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], dtype=np.float32)
    D = np.float32(100.0) * dist
    a, b = ref.analyze.atom_decoder[z[0]], ref.analyze.atom_decoder[z[1]]
    A = ref.analyze
    if D < np.float32(A.bonds1[a][b] + A.margin1):
        if D < np.float32(A.bonds2[a][b] + A.margin2):
            return 3 if D < np.float32(A.bonds3[a][b] + A.margin3) else 2
        return 1
    return 0


def gen_thresholds(ref):
    A = ref.analyze
    pos, v, level = [], [], []
    for za in ELEMENTS:
        for zb in ELEMENTS:
            a, b = A.atom_decoder[za], A.atom_decoder[zb]
            for k, (table, margin) in enumerate(((A.bonds1, A.margin1), (A.bonds2, A.margin2), (A.bonds3, A.margin3))):
                if table[a][b] < 0:
                    continue
                thr = (table[a][b] + margin) / 100.0
                p1 = (thr * np.array([1.0, 2.0, 2.0]) / 3.0).astype(np.float32)
                for step in (-2, -1, 0, 1, 2):
                    q = p1.copy()
                    for _ in range(abs(step)):
                        q[0] = np.nextafter(q[0], np.float32(np.inf if step > 0 else -np.inf))
                    pos += [np.zeros(3, np.float32), q]
                    v += [PLAIN_CLASS[za], PLAIN_CLASS[zb]]
                    level.append(k + 1)
    pos, v = np.array(pos, dtype=np.float32)[None], np.array(v, dtype=np.int64)[None]
    B = len(level)
    assert B == 425, B
    ptr = np.arange(B + 1, dtype=np.int32) * 2
    r = record(ref, pos, v, ptr)
    from targetdiff_amd.quality import class_atomic_numbers
    cz = class_atomic_numbers('add_aromatic')
    flips = sum(fp32_order(ref, pos[0, 2 * g:2 * g + 2], [cz[v[0, 2 * g]], cz[v[0, 2 * g + 1]]]) != r['nr_bonds'][0, 2 * g] for g in range(B))
    print(f'thresholds: {B} molecules, {flips} change order under fp32 evaluation; orders seen {sorted(set(r["nr_bonds"][0].tolist()))}')
    assert flips >= 100, flips
    save('quality_thresholds', pos=pos, v=v, ptr=ptr, level=np.array(level, np.int8), fp32_flips=np.int64(flips), **r)


def gen_sizes(ref):
    d = np.load(os.path.join(GOLDEN, 'ligand_1h36_docked.npz'))
    p = d['pos'].astype(np.float64)
    rg2 = ((p - p.mean(0)) ** 2).sum(1).mean()
    density = len(p) / (4.0 / 3.0 * np.pi * (np.sqrt(5.0 / 3.0 * rg2)) ** 3)          # atoms per A^3 of the equivalent uniform ball
    sizes = [0, 1, 2, 63, 64, 65, 130, 300, 2 * TILE + 88]
    assert sizes[-1] > 2 * TILE
    ptr = np.cumsum([0] + sizes).astype(np.int32)
    rng = np.random.default_rng(7)
    S, N, B = 3, int(ptr[-1]), len(sizes)
    pos, v = np.zeros((S, N, 3), np.float32), np.zeros((S, N), np.int64)
    for s in range(S):
        for g, n in enumerate(sizes):
            R = (n / density / (4.0 / 3.0 * np.pi)) ** (1.0 / 3.0)
            u = rng.normal(size=(n, 3))
            u /= np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-30)
            pts = u * R * rng.uniform(size=(n, 1)) ** (1.0 / 3.0) + rng.normal(0, 20.0, 3)
            pos[s, ptr[g]:ptr[g + 1]] = pts.astype(np.float32)
        v[s] = rng.integers(0, 13, N)
    v[2, ptr[2]:ptr[3]] = [PLAIN_CLASS[7], PLAIN_CLASS[8]]             # frame 2's two-atom molecule: a pair, but not C-C
    pos[2, ptr[2] + 1] = pos[2, ptr[2]] + np.float32(1.3)
    include = np.ones((S, B), bool)
    include[1] = [1, 0, 1, 0, 1, 1, 0, 1, 1]
    include[2] = [1, 1, 1, 0, 0, 0, 0, 0, 0]                          # frame 2: CC_2A stays empty, All_12A has one entry
    r = record(ref, pos, v, ptr, include)
    assert r['n_CC_2A'][2] == 0 and r['n_All_12A'][2] == 1 and r['n_CC_2A'][0] > 0
    assert (r['nr_bonds'] > 0).any()
    print('sizes:', sizes, 'stable atoms', r['stable_atoms'].tolist(), 'entries', r['n_CC_2A'].tolist(), r['n_All_12A'].tolist())
    save('quality_sizes', pos=pos, v=v, ptr=ptr, include=include, **r)


def gen_traj(ref):
    g = np.load(os.path.join(GOLDEN, 'sample_small_1000.npz'))
    batch = np.load(os.path.join(GOLDEN, 'forward_small.npz'))['batch_ligand']
    ptr = np.concatenate([[0], np.cumsum(np.bincount(batch))]).astype(np.int32)
    pos, v = g['pos_traj'].astype(np.float32), g['v_traj'].astype(np.int64)
    r = record(ref, pos, v, ptr, per_atom=False)
    n = r['n_All_12A']
    hist = np.rint(np.nan_to_num(r['dist_All_12A']) * n[:, None]).astype(np.int64)
    assert (hist.sum(1) == n).all() and hist.max() < 2 ** 15
    ok = n > 0
    assert np.array_equal(hist[ok] / n[ok, None], r['dist_All_12A'][ok])           # the counts reproduce the reference's distribution
    print('traj: stable atoms per frame, first / last', r['stable_atoms'][0].tolist(), r['stable_atoms'][-1].tolist())
    save('quality_traj', ptr=ptr, stable_atoms=r['stable_atoms'].astype(np.int16), mol_stable=r['mol_stable'],
         n_All_12A=n.astype(np.int32), hist_All_12A=hist.astype(np.int16), n_CC_2A=r['n_CC_2A'].astype(np.int32),
         counts=r['counts'].astype(np.int16))


def gen_reference_distributions(ref):
    pair = ref.config.PAIR_EMPIRICAL_DISTRIBUTIONS
    keys = list(ref.atom_type.ATOM_TYPE_DISTRIBUTION)
    assert keys == [6, 7, 8, 9, 15, 16, 17]
    save('quality_reference_distributions', CC_2A=np.asarray(pair['CC_2A'], np.float64), All_12A=np.asarray(pair['All_12A'], np.float64),
         atom_type=np.asarray([ref.atom_type.ATOM_TYPE_DISTRIBUTION[k] for k in keys], np.float64), atom_type_keys=np.asarray(keys, np.int64))


GENERATORS = {'docked': gen_docked, 'thresholds': gen_thresholds, 'sizes': gen_sizes, 'traj': gen_traj,
              'reference_distributions': gen_reference_distributions}


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
