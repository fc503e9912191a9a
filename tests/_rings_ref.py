"""Pure-Python restatement of the ring rule ("Rings"): the bonds from tests/_bonds_ref.py, then per bond a
dictionary breadth-first search with that edge removed.  Pinned to networkx and to known answers on the host (tests/test_rings_host.py);
the GPU tests compare the kernel with it.  It shares no code with targetdiff_amd."""
from collections import deque

import numpy as np

import _bonds_ref as BR

MAX_ATOMS = BR.MAX_ATOMS
GRAPH_KEYS = ('ring_mask', 'n_ring_bonds', 'n_ring_atoms', 'atom_ring', 'ring_hist')
LIST_KEYS = ('bond_ring', 'bond_category')


def bond_ring_sizes(n, bi, bj):
    """[nb]: atoms of the shortest cycle through every bond (bi[k], bj[k]) of a graph on n atoms; 0 for a bridge"""
    nbr = {a: set() for a in range(n)}
    for i, j in zip(bi, bj):
        nbr[int(i)].add(int(j))
        nbr[int(j)].add(int(i))
    out = np.zeros(len(bi), np.int64)
    for k, (i, j) in enumerate(zip(bi, bj)):
        i, j = int(i), int(j)
        dist = {i: 0}
        queue = deque([i])
        while queue and j not in dist:
            a = queue.popleft()
            for b in nbr[a]:
                if b in dist or (a == i and b == j):                   # the edge itself is removed
                    continue
                dist[b] = dist[a] + 1
                queue.append(b)
        out[k] = dist[j] + 1 if j in dist else 0
    return out


def rings_of(n, bi, bj, order, cat):
    """what follows from the bond ring sizes: dict(ring [nb], atom_ring [n], mask, n_ring_bonds, n_ring_atoms, ring_cat [nb])"""
    ring = bond_ring_sizes(n, bi, bj)
    atom = np.zeros(n, np.int64)
    mask = 0
    for i, j, r in zip(bi, bj, ring):
        if r:
            mask |= 1 << min(int(r), 31)
            for a in (int(i), int(j)):
                atom[a] = r if atom[a] == 0 else min(atom[a], r)
    ring_cat = np.where((np.asarray(cat) == 4) & ~np.isin(ring, (5, 6)), order, cat)
    return dict(ring=ring, atom_ring=atom, mask=mask, n_ring_bonds=int((ring > 0).sum()), n_ring_atoms=int((atom > 0).sum()), ring_cat=ring_cat)


def molecule(pos, cls, class_z, class_aromatic=None):
    m = BR.molecule(pos, cls, class_z, class_aromatic)
    m.update(rings_of(len(np.asarray(cls)), m['i'], m['j'], m['o'], m['cat']))
    return m


def ring_report(pos, v, ptr, class_z, class_aromatic=None, include=None):
    """numpy twin of capi.ring_report with a bond_ptr: pos [S, N, 3] fp32, v [S, N], ptr [B + 1]; also bond_atoms and the class-rule
    category of every bond (td_bond_list's), in the same order"""
    pos, v, ptr = np.asarray(pos), np.asarray(v), np.asarray(ptr)
    assert pos.dtype == np.float32
    S, N, B = pos.shape[0], pos.shape[1], len(ptr) - 1
    out = dict(ring_mask=np.zeros((S, B), np.int64), n_ring_bonds=np.zeros((S, B), np.int32), n_ring_atoms=np.zeros((S, B), np.int32),
               atom_ring=np.zeros((S, N), np.int32), ring_hist=np.zeros((S, 32), np.int64), bond_ptr=np.zeros(S * B + 1, np.int64))
    ring, cat, plain, atoms = [], [], [], []
    for s in range(S):
        for g in range(B):
            a, b = int(ptr[g]), int(ptr[g + 1])
            out['bond_ptr'][s * B + g + 1] = out['bond_ptr'][s * B + g]
            if b - a > MAX_ATOMS:
                out['n_ring_bonds'][s, g] = out['n_ring_atoms'][s, g] = -1
                continue
            m = molecule(pos[s, a:b], v[s, a:b], class_z, class_aromatic)
            out['ring_mask'][s, g], out['n_ring_bonds'][s, g], out['n_ring_atoms'][s, g] = m['mask'], m['n_ring_bonds'], m['n_ring_atoms']
            out['atom_ring'][s, a:b] = m['atom_ring']
            out['bond_ptr'][s * B + g + 1] += len(m['o'])
            ring.append(m['ring']); cat.append(m['ring_cat']); plain.append(m['cat']); atoms.append(np.stack([a + m['i'], a + m['j']], 1))
            if include is None or include[s][g]:
                if m['mask'] == 0:
                    out['ring_hist'][s, 0] += 1
                for k in range(32):
                    out['ring_hist'][s, k] += m['mask'] >> k & 1
    cat_of = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)
    out['bond_ring'], out['bond_category'], out['class_category'] = cat_of(ring, np.int16), cat_of(cat, np.uint8), cat_of(plain, np.uint8)
    out['bond_atoms'] = np.concatenate(atoms).astype(np.int32) if atoms else np.zeros((0, 2), np.int32)
    return out


def torch_ring_report(pos, v, ligand_ptr, class_z, class_aromatic=None, include=None, bond_ptr=None, return_atom_ring=True, check=True):
    """ring_report with capi.ring_report's signature on CPU tensors: what the host tests patch the binding with"""
    import torch
    r = ring_report(pos.cpu().numpy(), v.cpu().numpy(), ligand_ptr.cpu().numpy(), class_z, class_aromatic,
                    None if include is None else include.cpu().numpy())
    out = {k: torch.from_numpy(r[k]) for k in GRAPH_KEYS + LIST_KEYS}
    if bond_ptr is None:
        out['bond_ring'] = out['bond_category'] = None
    else:
        assert np.array_equal(r['bond_ptr'], bond_ptr.cpu().numpy())
    if not return_atom_ring:
        out['atom_ring'] = None
    return out
