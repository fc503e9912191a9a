"""Vectorised numpy float64 restatement of the sample-quality rule (stability, pair profiles, Jensen-Shannon distance), written from
the reference's description and pinned to fixtures made with the reference itself (tests/test_quality_host.py).  The GPU tests and the
host tests use it where no fixture can exist (a sampler's own trajectories); it shares no code with targetdiff_amd.quality."""
import numpy as np

ELEMENTS = (1, 6, 7, 8, 9, 15, 16, 17)            # H C N O F P S Cl
ALLOWED = np.array([1, 4, 3, 2, 1, 5, 4, 1])
MARGINS = (10, 5, 3)
_SYM = {'H': 0, 'C': 1, 'N': 2, 'O': 3, 'F': 4, 'P': 5, 'S': 6, 'Cl': 7}
# bond lengths in pm, upper triangle by element symbol (symmetric); what is not listed is -1
_SINGLE = {'H': dict(H=74, C=109, N=101, O=96, F=92, P=144, S=134, Cl=127), 'C': dict(C=154, N=147, O=143, F=135, P=184, S=182, Cl=177),
           'N': dict(N=145, O=140, F=136, P=177, S=168, Cl=175), 'O': dict(O=148, F=142, P=163, S=151, Cl=164),
           'F': dict(F=142, P=156, S=158, Cl=166), 'P': dict(P=221, S=210, Cl=203), 'S': dict(S=204, Cl=207), 'Cl': dict(Cl=199)}
_DOUBLE = {'C': dict(C=134, N=129, O=120, S=160), 'N': dict(N=125, O=121), 'O': dict(O=121, P=150), 'P': dict(S=186)}
_TRIPLE = {'C': dict(C=120, N=116, O=113), 'N': dict(N=110)}


def _table(upper):
    t = np.full((8, 8), -1, dtype=np.int64)
    for a, row in upper.items():
        for b, val in row.items():
            t[_SYM[a], _SYM[b]] = t[_SYM[b], _SYM[a]] = val
    return t


BONDS = np.stack([_table(_SINGLE), _table(_DOUBLE), _table(_TRIPLE)])          # [3, 8, 8]


def element_index(z):
    z = np.asarray(z)
    e = np.full(z.shape, -1, dtype=np.int64)
    for k, zz in enumerate(ELEMENTS):
        e[z == zz] = k
    if (e < 0).any():
        raise KeyError('atomic number outside the table')
    return e


def pair_distances(pos):
    """[n, n] float64: sqrt((dx dx + dy dy) + dz dz) on the widened coordinates (numpy sums three terms left to right)"""
    p = np.asarray(pos).astype(np.float64)
    d = p[None, :, :] - p[:, None, :]
    sq = d * d
    return np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2])


def bond_orders(dist, elem):
    """[n, n] orders from distances and element indices; the diagonal is 0"""
    D = 100.0 * dist
    e1, e2 = elem[:, None], elem[None, :]
    t1, t2, t3 = (BONDS[k][e1, e2] + MARGINS[k] for k in range(3))
    order = np.where(D < t1, np.where(D < t2, np.where(D < t3, 3, 2), 1), 0)
    np.fill_diagonal(order, 0)
    return order


def molecule(pos, z):
    """(stable, stable atoms, nr_bonds [n]) of one molecule with atomic numbers z: check_stability(..., hs=False)"""
    n = len(z)
    if n == 0:
        return True, 0, np.zeros(0, dtype=np.int64)
    elem = element_index(z)
    nb = bond_orders(pair_distances(pos), elem).sum(1)
    ok = (nb > 0) & (nb <= ALLOWED[elem])
    return bool(ok.sum() == n), int(ok.sum()), nb


def histogram(dist, z, profile):
    """[128] int64 of one molecule's pairs i < j under (z1, z2, cutoff, edges)"""
    z1, z2, cutoff, edges = profile
    n = len(z)
    h = np.zeros(128, dtype=np.int64)
    if n < 2:
        return h
    i, j = np.triu_indices(n, 1)
    zi, zj, d = np.asarray(z)[i], np.asarray(z)[j], dist[i, j]
    fwd = ((z1 == 0) | (zi == z1)) & ((z2 == 0) | (zj == z2))
    bwd = ((z1 == 0) | (zj == z1)) & ((z2 == 0) | (zi == z2))
    keep = (fwd | bwd) & (d < cutoff)
    np.add.at(h, np.searchsorted(np.asarray(edges, dtype=np.float64), d[keep]), 1)
    return h


def quality_report(pos, v, ptr, class_z, profiles=(), include=None):
    """numpy twin of capi.quality_report: pos [S, N, 3] fp32, v [S, N], ptr [B + 1] -> dict of nr_bonds [S, N] int32, stable_atoms
    [S, B] int32, mol_stable [S, B] uint8, hist [S, P, 128] int64, counts [S, 8] int64"""
    pos, v, ptr, class_z = np.asarray(pos), np.asarray(v), np.asarray(ptr), np.asarray(class_z)
    assert pos.dtype == np.float32
    S, N, B, P = pos.shape[0], pos.shape[1], len(ptr) - 1, len(profiles)
    out = dict(nr_bonds=np.zeros((S, N), np.int32), stable_atoms=np.zeros((S, B), np.int32), mol_stable=np.zeros((S, B), np.uint8),
               hist=np.zeros((S, P, 128), np.int64), counts=np.zeros((S, 8), np.int64))
    for s in range(S):
        for g in range(B):
            a, b = int(ptr[g]), int(ptr[g + 1])
            z = class_z[v[s, a:b]]
            ok, ns, nb = molecule(pos[s, a:b], z)
            out['mol_stable'][s, g], out['stable_atoms'][s, g], out['nr_bonds'][s, a:b] = ok, ns, nb
            if include is None or include[s][g]:
                if b > a:
                    out['counts'][s] += np.bincount(element_index(z), minlength=8)
                    dist = pair_distances(pos[s, a:b]) if P else None
                    for p in range(P):
                        out['hist'][s, p] += histogram(dist, z, profiles[p])
    return out


def torch_binding(pos, v, ligand_ptr, class_z, profiles=(), include=None, return_nr_bonds=True, check=True):
    """quality_report with capi.quality_report's signature on CPU tensors: what the host tests patch the binding with"""
    import torch
    from targetdiff_amd import capi
    capi._quality_inputs(pos, v, ligand_ptr, class_z, include, profiles, check)
    r = quality_report(pos.cpu().numpy(), v.cpu().numpy(), ligand_ptr.cpu().numpy(), class_z, profiles,
                       None if include is None else include.cpu().numpy())
    out = {k: torch.from_numpy(x) for k, x in r.items()}
    if not return_nr_bonds:
        out['nr_bonds'] = None
    return out


def rel_entr(x, y):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(x > 0, x * np.log(x / y), np.where(x == 0, 0.0, np.inf))


def js_squared(p, q):
    """Jensen-Shannon divergence (the square of scipy's distance), natural logarithm"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    p, q = p / p.sum(), q / q.sum()
    m = (p + q) / 2.0
    return (rel_entr(p, m).sum() + rel_entr(q, m).sum()) / 2.0


def normalised(h, n_edges):
    h = np.asarray(h)[:n_edges + 1]
    return h / np.sum(h)


def atom_type_distribution(counts):
    """the seven frequencies C N O F P S Cl over all counted atoms, hydrogen in the denominator"""
    total = int(np.sum(counts))
    return np.array([int(counts[ELEMENTS.index(z)]) / total for z in (6, 7, 8, 9, 15, 16, 17)])


def check_against_fixture(r, g, per_atom=True):
    """r: a quality_report result as numpy; g: a fixture of tools/make_golden_quality.record"""
    if per_atom:
        np.testing.assert_array_equal(r['nr_bonds'], g['nr_bonds'])
    np.testing.assert_array_equal(r['stable_atoms'], g['stable_atoms'])
    np.testing.assert_array_equal(r['mol_stable'], g['mol_stable'])
    np.testing.assert_array_equal(r['counts'], g['counts'])
    for p, name in enumerate(('CC_2A', 'All_12A')):
        h = r['hist'][:, p]
        np.testing.assert_array_equal(h.sum(1), g['n_' + name])
        assert not h[:, 101:].any()
        for s in range(h.shape[0]):
            if g['n_' + name][s] > 0:
                np.testing.assert_array_equal(normalised(h[s], 100), g['dist_' + name][s])
            else:
                assert np.isnan(g['dist_' + name][s]).all()
