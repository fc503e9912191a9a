"""Numpy float64 restatement of the local geometry report ("Local geometry"): the bonds from tests/_bonds_ref.py,
the ring sizes from tests/_rings_ref.py, then angles, torsions and internal clashes in the kernel's rounding order (numpy rounds every
elementwise product, sum and difference on its own).  Pinned to networkx, to arccos / arctan2 and to brute-force enumeration on the
host (tests/test_geometry_host.py); the GPU tests compare the kernel with it.  It shares no code with targetdiff_amd.quality."""
import numpy as np

import _bonds_ref as BR
import _quality_ref as QR
import _rings_ref as RR

MAX_ATOMS = BR.MAX_ATOMS
MAX_DEGREE = 8
BINS = 128
RADII = (1.2, 1.7, 1.55, 1.52, 1.47, 1.8, 1.8, 1.75)       # H C N O F P S Cl, Angstrom
COUNT_KEYS = ('n_angles', 'n_torsions', 'n_degenerate', 'n_crowded')
CLASH_KEYS = ('n_clashes', 'atom_clash')
KEYS = COUNT_KEYS + CLASH_KEYS + ('hist',)
_KIND = {'angle': 1, 'torsion': 2}
_RING = {None: 0, 'any': 0, 'chain': 1, 'ring': 2}


def clash_table(scale=0.7, radii=RADII):
    """[8, 8] float64: scale * (r_i + r_j)"""
    r = np.asarray(radii, np.float64)
    return np.float64(scale) * (r[:, None] + r[None, :])


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def terms(adj):
    """(angles [na, 3] as (i, j, k) with j the centre and i < k, torsions [nt, 4] as (i, j, k, l) with j < k, crowded [n]) of a graph"""
    n = len(adj)
    nbr = [np.nonzero(adj[a])[0].tolist() for a in range(n)]
    crowded = np.array([len(x) > MAX_DEGREE for x in nbr], bool)
    ang = [(i, j, k) for j in range(n) if not crowded[j] for a, i in enumerate(nbr[j]) for k in nbr[j][a + 1:]]
    tor = [(i, j, k, l) for j in range(n) if not crowded[j] for k in nbr[j] if k > j and not crowded[k] for i in nbr[j] if i != k
           for l in nbr[k] if l != j and l != i]
    return np.asarray(ang, np.int64).reshape(-1, 3), np.asarray(tor, np.int64).reshape(-1, 4), crowded


def angle_cosines(p, ang):
    """(cosine [na], degenerate [na]) of the angles (i, j, k) on float64 coordinates p; the cosine of a degenerate angle is nan"""
    u, w = p[ang[:, 0]] - p[ang[:, 1]], p[ang[:, 2]] - p[ang[:, 1]]
    den = dot(u, u) * dot(w, w)
    bad = den == 0
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(bad, np.nan, dot(u, w) / np.sqrt(den)), bad


def torsion_cosines(p, tor):
    """(cosine of the unsigned torsion [nt], degenerate [nt]) of the quadruples (i, j, k, l)"""
    b1, b2, b3 = p[tor[:, 1]] - p[tor[:, 0]], p[tor[:, 2]] - p[tor[:, 1]], p[tor[:, 3]] - p[tor[:, 2]]
    n1, n2 = cross(b1, b2), cross(b2, b3)
    den = dot(n1, n1) * dot(n2, n2)
    bad = den == 0
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(bad, np.nan, dot(n1, n2) / np.sqrt(den)), bad


def far_apart(adj):
    """[n, n] bool: more than 3 bonds apart (other fragments included)"""
    a = (adj | np.eye(len(adj), dtype=bool)).astype(np.int64)
    return ~((a @ a @ a) > 0)


def molecule(pos, cls, class_z, class_aromatic=None, clash_threshold=None):
    """One molecule: the dict of _rings_ref.molecule plus z [n] (0: no class), ang / ang_cos / ang_bad, tor / tor_cos / tor_bad /
    tor_cat / tor_ring (category and ring size of the central bond), crowded [n], far [n, n], clash [n, n] (symmetric, bool)"""
    cls = np.asarray(cls)
    n, K = len(cls), len(class_z)
    m = RR.molecule(pos, cls, class_z, class_aromatic)
    valid = (cls >= 0) & (cls < K)
    z = np.where(valid, np.asarray(class_z)[np.where(valid, cls, 0)], 0)
    p = np.asarray(pos).astype(np.float64).reshape(n, 3)
    adj = m['order'] > 0
    ang, tor, crowded = terms(adj)
    ang_cos, ang_bad = angle_cosines(p, ang)
    tor_cos, tor_bad = torsion_cosines(p, tor)
    bond = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(m['i'], m['j']))}
    central = np.asarray([bond[(int(j), int(k))] for _, j, k, _ in tor], np.int64)
    m.update(z=z, ang=ang, ang_cos=ang_cos, ang_bad=ang_bad, tor=tor, tor_cos=tor_cos, tor_bad=tor_bad, tor_cat=np.asarray(m['cat'])[central],
             tor_ring=np.asarray(m['ring'])[central], crowded=crowded, far=far_apart(adj))
    clash = np.zeros((n, n), bool)
    if clash_threshold is not None and n:
        thr = np.asarray(clash_threshold, np.float64).reshape(8, 8)
        e = QR.element_index(np.where(valid, z, 1))
        upper = np.triu(np.ones((n, n), bool), 1)
        clash = upper & valid[:, None] & valid[None, :] & m['far'] & (m['dist'] < thr[e[:, None], e[None, :]])
        clash = clash | clash.T
    m['clash'] = clash
    return m


def _fits(want, z):
    return (want == 0) | (want == z)


def matching(m, profile):
    """the cosines of the non-degenerate angles / torsions of one molecule that (kind, elements, category, ring, ...) takes"""
    kind, zs, category, ring = profile[:4]
    kind, ring = _KIND.get(kind, kind), _RING.get(ring, ring) if ring is None or isinstance(ring, str) else ring
    zs = tuple(int(x) for x in zs) + (0,) * (4 - len(zs))
    z = m['z']
    if kind == 1:
        zi, zj, zk = (z[m['ang'][:, c]] for c in range(3))
        keep = ~m['ang_bad'] & _fits(zs[1], zj) & ((_fits(zs[0], zi) & _fits(zs[2], zk)) | (_fits(zs[0], zk) & _fits(zs[2], zi)))
        c = m['ang_cos'][keep]
    else:
        q = [z[m['tor'][:, c]] for c in range(4)]
        fwd = _fits(zs[0], q[0]) & _fits(zs[1], q[1]) & _fits(zs[2], q[2]) & _fits(zs[3], q[3])
        rev = _fits(zs[0], q[3]) & _fits(zs[1], q[2]) & _fits(zs[2], q[1]) & _fits(zs[3], q[0])
        keep = ~m['tor_bad'] & (fwd | rev)
        if category:
            keep &= m['tor_cat'] == category
        if ring:
            keep &= (m['tor_ring'] > 0) == (ring == 2)
        c = m['tor_cos'][keep]
    return c


def histogram(m, profile):
    """[128] int64 of one molecule under (kind, elements, category, ring, ascending cosine edges)"""
    h = np.zeros(BINS, np.int64)
    np.add.at(h, np.searchsorted(np.asarray(profile[4], np.float64), matching(m, profile), 'left'), 1)
    return h


def geometry_report(pos, v, ptr, class_z, class_aromatic=None, profiles=(), include=None, clash_threshold=None):
    """numpy twin of capi.geometry_report: pos [S, N, 3] fp32, v [S, N], ptr [B + 1]; without a clash table n_clashes and atom_clash
    are None"""
    pos, v, ptr = np.asarray(pos), np.asarray(v), np.asarray(ptr)
    assert pos.dtype == np.float32
    S, N, B, P = pos.shape[0], pos.shape[1], len(ptr) - 1, len(profiles)
    out = {k: np.zeros((S, B), np.int32) for k in COUNT_KEYS + ('n_clashes',)}
    out.update(atom_clash=np.zeros((S, N), np.int32), hist=np.zeros((S, P, BINS), np.int64))
    for s in range(S):
        for g in range(B):
            a, b = int(ptr[g]), int(ptr[g + 1])
            if b - a > MAX_ATOMS:
                for k in COUNT_KEYS + ('n_clashes',):
                    out[k][s, g] = -1
                continue
            m = molecule(pos[s, a:b], v[s, a:b], class_z, class_aromatic, clash_threshold)
            out['n_angles'][s, g], out['n_torsions'][s, g] = (~m['ang_bad']).sum(), (~m['tor_bad']).sum()
            out['n_degenerate'][s, g], out['n_crowded'][s, g] = m['ang_bad'].sum() + m['tor_bad'].sum(), m['crowded'].sum()
            out['n_clashes'][s, g] = m['clash'].sum() // 2
            out['atom_clash'][s, a:b] = m['clash'].sum(1)
            if include is None or include[s][g]:
                for p in range(P):
                    out['hist'][s, p] += histogram(m, profiles[p])
    if clash_threshold is None:
        out['n_clashes'] = out['atom_clash'] = None
    return out


def torch_geometry_report(pos, v, ligand_ptr, class_z, class_aromatic=None, profiles=(), include=None, clash_threshold=None, bond_ptr=None,
                          bond_ring=None, return_atom_clash=True, check=True):
    """geometry_report with capi.geometry_report's signature on CPU tensors: what the host tests patch the binding with.  The ring
    sizes a filter needs are the restatement's own; the ones handed in must equal them."""
    import torch
    from targetdiff_amd import capi
    capi._bond_inputs(pos, v, ligand_ptr, class_z, class_aromatic, include, (), check)
    prof = capi._geometry_profiles(profiles)
    if any(p[3] for p in prof):
        assert bond_ptr is not None and bond_ring is not None
        want = RR.ring_report(pos.cpu().numpy(), v.cpu().numpy(), ligand_ptr.cpu().numpy(), class_z, class_aromatic)
        assert np.array_equal(want['bond_ptr'], bond_ptr.cpu().numpy()) and np.array_equal(want['bond_ring'], bond_ring.cpu().numpy())
    r = geometry_report(pos.cpu().numpy(), v.cpu().numpy(), ligand_ptr.cpu().numpy(), class_z, class_aromatic, prof,
                        None if include is None else include.cpu().numpy(), clash_threshold)
    out = {k: (None if r[k] is None else torch.from_numpy(r[k])) for k in KEYS}
    if not return_atom_clash:
        out['atom_clash'] = None
    return out
