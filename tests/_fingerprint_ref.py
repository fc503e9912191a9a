"""Pure-Python restatement of the fingerprint rule ("Fingerprints and diversity"): the bonds from
tests/_bonds_ref.py, then the refinement on Python integers masked to 64 bits, and the comparison of a frame's molecules on Python
floats in ascending order.  Pinned to networkx, to known answers and to recorded values on the host (tests/test_fingerprint_host.py);
the GPU tests compare the kernels with it.  It shares no code with targetdiff_amd."""
import numpy as np

import _bonds_ref as BR

MAX_ATOMS = BR.MAX_ATOMS
BITS, WORDS = 2048, 32
M64 = (1 << 64) - 1
FP_KEYS = ('fp_words', 'n_bits', 'key', 'atom_key')
SIM_KEYS = ('sim_sum', 'sim_max', 'first_equal', 'common')


def mix(x):
    """the splitmix64 finaliser"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def signed(x):
    """a uint64 as the int64 that holds its bits"""
    return x - (1 << 64) if x >> 63 else x


def invariants(m, cls, class_z, class_aromatic=None):
    """[(Z, aromatic, degree, valence) or None for an atom of no class] of a _bonds_ref.molecule"""
    cls = np.asarray(cls)
    out = []
    for a, c in enumerate(cls.tolist()):
        if not 0 <= c < len(class_z):
            out.append(None)
            continue
        row = m['order'][a]
        out.append((int(class_z[c]), int(bool(class_aromatic[c])) if class_aromatic is not None else 0, int((row > 0).sum()), int(row.sum())))
    return out


def refine(inv, bonds, radius=2, key_rounds=8):
    """inv: invariants(); bonds: [(i, j, category)].  Returns dict(ids [rounds + 1][n] (0 for no class), bits: set of fingerprint bits,
    key, atom_key [n])"""
    n = len(inv)
    nbr = [[] for _ in range(n)]
    for i, j, c in bonds:
        nbr[i].append((j, c))
        nbr[j].append((i, c))
    valid = [x is not None for x in inv]
    ids = [[mix(x[0] | x[1] << 8 | x[2] << 16 | x[3] << 24) if x is not None else 0 for x in inv]]
    for r in range(1, key_rounds + 1):
        prev = ids[-1]
        ids.append([mix((mix(prev[i] ^ r) + sum(mix(prev[j] ^ mix(c)) for j, c in nbr[i])) & M64) if valid[i] else 0 for i in range(n)])
    bits = {ids[r][i] % BITS for r in range(radius + 1) for i in range(n) if valid[i]}
    total = sum(mix(ids[-1][i]) for i in range(n) if valid[i]) & M64
    key = mix(total ^ mix((sum(valid) << 32 | len(bonds)) & M64))
    return dict(ids=ids, bits=bits, key=key, atom_key=ids[-1])


def words_of(bits):
    w = [0] * WORDS
    for b in bits:
        w[b >> 6] |= 1 << (b & 63)
    return w


def molecule(pos, cls, class_z, class_aromatic=None, radius=2, key_rounds=8):
    """one molecule: _bonds_ref.molecule plus inv, bits, words (Python ints), n_bits, key, atom_key"""
    m = BR.molecule(pos, cls, class_z, class_aromatic)
    m['inv'] = invariants(m, cls, class_z, class_aromatic)
    m.update(refine(m['inv'], list(zip(m['i'].tolist(), m['j'].tolist(), m['cat'].tolist())), radius, key_rounds))
    m['words'], m['n_bits'] = words_of(m['bits']), len(m['bits'])
    return m


def fingerprints(pos, v, ptr, class_z, class_aromatic=None, radius=2, key_rounds=8):
    """numpy twin of capi.fingerprint: pos [S, N, 3] fp32, v [S, N], ptr [B + 1] -> fp_words [S, B, 32] int64, n_bits [S, B] int32, key
    [S, B] int64, atom_key [S, N] int64 (0 for the atoms of a refused molecule)"""
    pos, v, ptr = np.asarray(pos), np.asarray(v), np.asarray(ptr)
    assert pos.dtype == np.float32
    S, N, B = pos.shape[0], pos.shape[1], len(ptr) - 1
    out = dict(fp_words=np.zeros((S, B, WORDS), np.int64), n_bits=np.zeros((S, B), np.int32), key=np.zeros((S, B), np.int64),
               atom_key=np.zeros((S, N), np.int64))
    for s in range(S):
        for g in range(B):
            a, b = int(ptr[g]), int(ptr[g + 1])
            if b - a > MAX_ATOMS:
                out['n_bits'][s, g] = -1
                continue
            m = molecule(pos[s, a:b], v[s, a:b], class_z, class_aromatic, radius, key_rounds)
            out['fp_words'][s, g] = [signed(w) for w in m['words']]
            out['n_bits'][s, g], out['key'][s, g] = m['n_bits'], signed(m['key'])
            out['atom_key'][s, a:b] = [signed(x) for x in m['atom_key']]
    return out


def popcount_and(wa, wb):
    """popcount of the AND of two [32] int64 word rows"""
    return sum(bin((int(x) & int(y)) & M64).count('1') for x, y in zip(wa, wb))


def tanimoto(c, na, nb):
    union = na + nb - c
    return float(c) / float(union) if union > 0 else 0.0


def similarity(fp_words, n_bits, key, include=None, q_words=None):
    """numpy twin of capi.fingerprint_similarity: sim_sum, sim_max [S, B] float64, first_equal [S, B] int32, common [S, B, B] int32 and,
    with q_words [Q, 32], query_common [S, B, Q] int32.  The sum runs in ascending b with one add per term."""
    S, B = n_bits.shape
    out = dict(sim_sum=np.zeros((S, B), np.float64), sim_max=np.zeros((S, B), np.float64), first_equal=np.full((S, B), -1, np.int32),
               common=np.zeros((S, B, B), np.int32))
    for s in range(S):
        inc = [n_bits[s, g] >= 0 and (include is None or bool(include[s][g])) for g in range(B)]
        for a in range(B):
            for b in range(B):
                out['common'][s, a, b] = popcount_and(fp_words[s, a], fp_words[s, b])
        for a in range(B):
            if not inc[a]:
                continue
            total, best = 0.0, 0.0
            for b in range(B):
                if not inc[b]:
                    continue
                if out['first_equal'][s, a] < 0 and key[s, b] == key[s, a]:
                    out['first_equal'][s, a] = b
                if b != a:
                    t = tanimoto(int(out['common'][s, a, b]), int(n_bits[s, a]), int(n_bits[s, b]))
                    total += t
                    best = max(best, t)
            out['sim_sum'][s, a], out['sim_max'][s, a] = total, best
    if q_words is not None:
        Q = len(q_words)
        out['query_common'] = np.zeros((S, B, Q), np.int32)
        for s in range(S):
            for a in range(B):
                for q in range(Q):
                    out['query_common'][s, a, q] = popcount_and(fp_words[s, a], q_words[q])
    return out


def diversity(sim, n_bits, include=None, ref_sim=None):
    """one pocket's values per frame, from similarity(): dict of [S] arrays diversity, uniqueness, mean_nearest (nan where there is no
    value), n_included, n_distinct and, with ref_sim [S, B], ref_sim_mean / ref_sim_median / ref_sim_max.  The sums over the molecules
    are numpy's over a [S, B] array with the excluded entries 0."""
    S, B = n_bits.shape
    inc = (n_bits >= 0) & (np.ones((S, B), bool) if include is None else np.asarray(include, bool))
    m = inc.sum(1)
    sum_sim, sum_max = np.where(inc, sim['sim_sum'], 0.0).sum(1), np.where(inc, sim['sim_max'], 0.0).sum(1)
    distinct = ((sim['first_equal'] == np.arange(B)[None]) & inc).sum(1)
    nan = float('nan')
    out = dict(n_included=m, n_distinct=distinct,
               diversity=np.array([1.0 - sum_sim[s] / (float(m[s]) * (float(m[s]) - 1.0)) if m[s] >= 2 else nan for s in range(S)]),
               mean_nearest=np.array([sum_max[s] / float(m[s]) if m[s] >= 2 else nan for s in range(S)]),
               uniqueness=np.array([float(distinct[s]) / float(m[s]) if m[s] >= 1 else nan for s in range(S)]))
    if ref_sim is not None:
        rows = [np.asarray(ref_sim[s], np.float64)[inc[s]] for s in range(S)]
        out['ref_sim_mean'] = np.array([x.sum() / x.size if x.size else nan for x in rows])
        out['ref_sim_median'] = np.array([np.median(x) if x.size else nan for x in rows])
        out['ref_sim_max'] = np.array([x.max() if x.size else nan for x in rows])
    return out


def torch_fingerprint(pos, v, ligand_ptr, class_z, class_aromatic=None, radius=2, key_rounds=8, return_atom_keys=False, check=True):
    """fingerprints with capi.fingerprint's signature on CPU tensors: what the host tests patch the binding with"""
    import torch
    from targetdiff_amd import capi
    capi._fingerprint_inputs(pos, v, ligand_ptr, class_z, class_aromatic, radius, key_rounds, check)
    r = fingerprints(pos.cpu().numpy(), v.cpu().numpy(), ligand_ptr.cpu().numpy(), class_z, class_aromatic, radius, key_rounds)
    out = {k: torch.from_numpy(r[k]) for k in FP_KEYS}
    if not return_atom_keys:
        out['atom_key'] = None
    return out


def torch_similarity(fp_words, n_bits, key, include=None, q_words=None, q_bits=None, return_common=False):
    """similarity with capi.fingerprint_similarity's signature on CPU tensors"""
    import torch
    r = similarity(fp_words.numpy(), n_bits.numpy(), key.numpy(), None if include is None else include.numpy(),
                   None if q_words is None else q_words.numpy())
    out = {k: torch.from_numpy(r[k]) for k in SIM_KEYS}
    if not return_common:
        out['common'] = None
    out['query_common'] = out['query_sim'] = None
    if q_words is not None:
        qc = r['query_common'].astype(np.int64)
        union = n_bits.numpy().astype(np.int64)[:, :, None] + q_bits.numpy().astype(np.int64)[None, None, :] - qc
        out['query_common'] = torch.from_numpy(r['query_common'])
        out['query_sim'] = torch.from_numpy(np.where(union > 0, qc / np.where(union > 0, union, 1), 0.0))
    return out
