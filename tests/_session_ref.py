"""CPU expectation for what a sampling session derives from a step's neighbour table (TEST INFRASTRUCTURE), and the geometries that
make the session's merge decide every branch it has.

A session (csrc/session.cpp) merges the ligand atoms into cached protein-only k-NN lists, declares the untouched protein rows "clean",
and derives the step's row lists from the clean flags and the merged table.  All of it is integer work, so the expectation is exact:

* the neighbour table: ``oracle.shims.knn_neighbours`` / ``hybrid_neighbours`` on the composed batch;
* ``dirty``: the ligand rows, plus the protein rows whose row holds a ligand index;
* ``reach``: the dirty rows, plus the rows with a dirty in-neighbour (row i's in-neighbours are the entries of row i);
* ``levels[1..L]``: level 1 = the ligand rows and their in-neighbours, level k + 1 = level k plus its in-neighbours.

Plain loops and sets on purpose: nothing here shares an idea with the kernels it checks.

Geometries.  ``vacancy_lattice``: an integer grid times 2 A whose sites around (1, 2, 2) are the ligand -- every d2 is an exact fp32
integer, so ligand atoms sit at exactly the k-th protein neighbour's distance of many rows (the tie goes to the protein atom: its
index is lower).  ``cloud``: Gaussian protein and ligand with the ligand's offset as a parameter (inside, at the rim, 1000 A away).
Neither is centred: a session takes positions as given, and centring would destroy the exact ties.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import shims

PROTEIN_FEAT_DIM = 27
LIGAND_CLASSES = 13
HOP_LEVELS = 4            # receptive-field levels a session tracks by default (model option session_hop_levels)

# grid, radius (grid units), k  ->  protein atoms, ligand atoms (pinned by tests/test_session_ref_host.py)
LATTICE_CASES = [
    ((10, 6, 5), 2.0, 32, 268, 32),
    ((10, 6, 5), 2.5, 32, 228, 72),
    ((12, 6, 5), 3.0, 16, 262, 98),
    ((14, 7, 6), 3.7, 48, 451, 137),
    ((14, 7, 6), 4.2, 32, 413, 175),
]
LATTICE_CENTRE = (1, 2, 2)
LATTICE_SPACING = 2.0


# ------------------------------------------------------------------------------------------ one graph
def _features(n_prot, n_lig, seed):
    g = torch.Generator().manual_seed(seed)
    pv = torch.zeros(n_prot, PROTEIN_FEAT_DIM)
    pv[torch.arange(n_prot), torch.randint(0, PROTEIN_FEAT_DIM, (n_prot,), generator=g)] = 1.0
    lv = torch.randint(0, LIGAND_CLASSES, (n_lig,), generator=g)
    return pv, lv


def vacancy_lattice(grid, rad, seed=0):
    """One graph: the sites of the ``grid`` = (nx, ny, nz) integer lattice times 2.0 A; those within ``rad`` grid units of (1, 2, 2)
    are the ligand, the others the protein (x-major site order).  Not centred."""
    nx, ny, nz = grid
    prot, lig = [], []
    for ix in range(nx):
        for iy in range(ny):
            for iz in range(nz):
                r2 = (ix - LATTICE_CENTRE[0]) ** 2 + (iy - LATTICE_CENTRE[1]) ** 2 + (iz - LATTICE_CENTRE[2]) ** 2
                site = [LATTICE_SPACING * ix, LATTICE_SPACING * iy, LATTICE_SPACING * iz]
                (lig if r2 <= rad * rad else prot).append(site)
    pv, lv = _features(len(prot), len(lig), seed)
    return dict(ppos=torch.tensor(prot, dtype=torch.float32), pv=pv, lpos=torch.tensor(lig, dtype=torch.float32), lv=lv)


def cloud(n_prot, n_lig, offset, seed, sigma_prot=4.0, sigma_lig=1.5):
    """One graph: protein ~ N(0, sigma_prot^2 I), ligand ~ N(offset, sigma_lig^2 I).  The draws depend on (sizes, seed) only, so the
    same ligand can be put anywhere by ``offset``."""
    g = torch.Generator().manual_seed(seed)
    ppos = sigma_prot * torch.randn(n_prot, 3, generator=g)
    lpos = sigma_lig * torch.randn(n_lig, 3, generator=g) + torch.tensor(offset, dtype=torch.float32)
    pv, lv = _features(n_prot, n_lig, seed + 1)
    return dict(ppos=ppos, pv=pv, lpos=lpos, lv=lv)


def moved(graph, shift):
    """The same graph with its ligand translated by ``shift`` (A)."""
    out = dict(graph)
    out['lpos'] = graph['lpos'] + torch.tensor(shift, dtype=torch.float32)
    return out


# ------------------------------------------------------------------------------------------ a batch of graphs
class Batch:
    """The arrays the library takes (protein / ligand blocks with graph pointers) and the composed view (per graph: protein rows,
    then ligand rows -- models/common.py:120-137) the neighbour table is defined on."""

    def __init__(self, graphs):
        self.B = len(graphs)
        self.ppos = torch.cat([g['ppos'] for g in graphs]).contiguous()
        self.pv = torch.cat([g['pv'] for g in graphs]).contiguous()
        self.lpos = torch.cat([g['lpos'] for g in graphs]).contiguous()
        self.lv = torch.cat([g['lv'] for g in graphs]).contiguous()
        self.n_prot = [int(g['ppos'].shape[0]) for g in graphs]
        self.n_lig = [int(g['lpos'].shape[0]) for g in graphs]
        self.pptr = torch.tensor(np.concatenate([[0], np.cumsum(self.n_prot)]), dtype=torch.int32)
        self.lptr = torch.tensor(np.concatenate([[0], np.cumsum(self.n_lig)]), dtype=torch.int32)
        self.batch_protein = torch.repeat_interleave(torch.arange(self.B), torch.tensor(self.n_prot))
        self.batch_ligand = torch.repeat_interleave(torch.arange(self.B), torch.tensor(self.n_lig))
        xs, mask, sizes = [], [], []
        for g in graphs:
            xs += [g['ppos'], g['lpos']]
            mask += [torch.zeros(g['ppos'].shape[0], dtype=torch.bool), torch.ones(g['lpos'].shape[0], dtype=torch.bool)]
            sizes.append(int(g['ppos'].shape[0] + g['lpos'].shape[0]))
        self.x = torch.cat(xs).contiguous()
        self.mask = torch.cat(mask)
        self.sizes = sizes
        self.node_ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32)
        self.batch = torch.repeat_interleave(torch.arange(self.B), torch.tensor(sizes))
        self.N = int(self.x.shape[0])
        self.Nl = int(self.lpos.shape[0])


# ------------------------------------------------------------------------------------------ expectation
def neighbour_table(batch: Batch, mode: str, k: int) -> torch.Tensor:
    """[N, width] in-neighbour table (-1 padded) of the composed batch under the project's rule (oracle/shims.py)."""
    if mode == 'knn':
        return shims.knn_neighbours(batch.x, k, batch.batch)
    if mode == 'hybrid':
        return shims.hybrid_neighbours(batch.x, k, batch.mask, batch.batch)
    raise ValueError(mode)


def row_lists(table, mask, levels=HOP_LEVELS):
    """(dirty, reach, [level 1, ..., level L]) as sets of row indices."""
    rows = [[int(j) for j in r if j >= 0] for r in table.tolist()]
    lig = [bool(m) for m in mask.tolist()]
    n = len(rows)
    dirty = set()
    for i in range(n):
        if lig[i]:
            dirty.add(i)
        else:
            for j in rows[i]:
                if lig[j]:
                    dirty.add(i)
                    break
    reach = set(dirty)
    for i in range(n):
        for j in rows[i]:
            if j in dirty:
                reach.add(i)
                break
    level = set()
    for i in range(n):
        if lig[i]:
            level.add(i)
            for j in rows[i]:
                level.add(j)
    out = [set(level)]
    for _ in range(1, levels):
        nxt = set(level)
        for i in level:
            for j in rows[i]:
                nxt.add(j)
        level = nxt
        out.append(set(level))
    return dirty, reach, out


def expected_counts(batch: Batch, mode: str, k: int, table=None, levels=HOP_LEVELS):
    """What ``NativeSession.row_counts()`` and ``forward_reach_rows()`` must report: ((N, dirty, [levels]), reach)."""
    if table is None:
        table = neighbour_table(batch, mode, k)
    dirty, reach, lv = row_lists(table, batch.mask, levels)
    return (batch.N, len(dirty), [len(s) for s in lv]), len(reach)


# ------------------------------------------------------------------------------------------ what a geometry promises (host test)
def _d2(a, b):
    """fp32 squared distance under the project's rule: (dx*dx + dy*dy) + dz*dz, every operation rounded on its own."""
    d = (np.asarray(b, np.float32) - np.asarray(a, np.float32)).astype(np.float32)
    return np.float32(np.float32(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])) + np.float32(d[2] * d[2]))


def merge_census(batch: Batch, k: int):
    """Per protein row, from distances alone (no neighbour table): 'dirty' (a ligand atom is strictly closer than the k-th protein
    neighbour, or there are fewer than k protein neighbours), 'tie' (clean, but a ligand atom sits at exactly the k-th protein
    neighbour's d2: clean only because the tie goes to the lower, protein, index) or 'clean'.  Also whether the row has >= k protein
    neighbours.  Returns {row: (kind, has_k_static)}."""
    out = {}
    x = batch.x.numpy()
    ptr = batch.node_ptr.tolist()
    for g in range(batch.B):
        p0, l0, l1 = ptr[g], ptr[g] + batch.n_prot[g], ptr[g + 1]
        for i in range(p0, l0):
            dp = sorted(float(_d2(x[i], x[j])) for j in range(p0, l0) if j != i)
            dl = [float(_d2(x[i], x[j])) for j in range(l0, l1)]
            if len(dp) < k:
                kind = 'dirty' if dl else 'clean'
            else:
                thr = dp[k - 1]
                kind = 'dirty' if any(d < thr for d in dl) else ('tie' if any(d == thr for d in dl) else 'clean')
            out[i] = (kind, len(dp) >= k)
    return out


def min_ligand_protein_d2(batch: Batch) -> float:
    x = batch.x.numpy()
    ptr = batch.node_ptr.tolist()
    best = float('inf')
    for g in range(batch.B):
        p0, l0, l1 = ptr[g], ptr[g] + batch.n_prot[g], ptr[g + 1]
        for i in range(p0, l0):
            for j in range(l0, l1):
                best = min(best, float(_d2(x[i], x[j])))
    return best


def min_pair_d2(batch: Batch) -> float:
    """smallest d2 between two different nodes of one graph (0 = coincident points)"""
    x = batch.x.double()
    ptr = batch.node_ptr.tolist()
    best = float('inf')
    for g in range(batch.B):
        xs = x[ptr[g]:ptr[g + 1]]
        d = torch.cdist(xs, xs)
        d.fill_diagonal_(float('inf'))
        best = min(best, float(d.min()) ** 2)
    return best


# ------------------------------------------------------------------------------------------ the batches of the GPU tests
PROTEIN_SIZES = [5, 20, 31, 32, 33, 100]
LIGAND_SIZES = [1, 40, 63, 64, 65, 127, 128, 129, 200]
INSIDE, RIM, FAR = (1.0, 0.0, 0.0), (7.0, 0.0, 0.0), (1000.0, 0.0, 0.0)


def size_matrix_batch(b):
    """Batch ``b`` of 6: for every ligand size L[i] the protein size P[(i + b) % 6] -- the six batches together hold every
    (protein, ligand) pair once, and each holds every ligand size (one ligand key per lane, two, the overflow passes) next to
    protein blocks with fewer and with more than k atoms.  Ligands alternate between the inside and the rim of the protein."""
    graphs = []
    for i, nl in enumerate(LIGAND_SIZES):
        npr = PROTEIN_SIZES[(i + b) % len(PROTEIN_SIZES)]
        graphs.append(cloud(npr, nl, INSIDE if (i + b) % 2 == 0 else RIM, seed=1000 * npr + nl))
    return Batch(graphs)


GENERAL_SIZES = [(20, 65), (100, 129), (33, 200), (100, 1), (32, 40), (100, 64), (5, 128)]


def general_batch():
    """the sizes the general merge (k of 33 .. 64, hybrid) runs on: includes the 65, 129 and 200 ligand atoms"""
    return Batch([cloud(npr, nl, INSIDE if i % 2 == 0 else RIM, seed=1000 * npr + nl) for i, (npr, nl) in enumerate(GENERAL_SIZES)])


def rows_decided_by_the_last_static_key(batch: Batch, k: int):
    """Protein rows with >= k protein neighbours that are dirty only because a ligand atom lies between the (k-1)-th and the k-th
    protein neighbour (d2 of the (k-1)-th <= nearest ligand d2 < d2 of the k-th): a merge threshold one neighbour too near
    would call them clean."""
    out = []
    x = batch.x.numpy()
    ptr = batch.node_ptr.tolist()
    for g in range(batch.B):
        p0, l0, l1 = ptr[g], ptr[g] + batch.n_prot[g], ptr[g + 1]
        for i in range(p0, l0):
            dp = sorted(float(_d2(x[i], x[j])) for j in range(p0, l0) if j != i)
            if len(dp) < k or k < 2 or l1 == l0:
                continue
            nearest = min(float(_d2(x[i], x[j])) for j in range(l0, l1))
            if dp[k - 2] <= nearest < dp[k - 1]:
                out.append(i)
    return out


def rows_holding_a_late_ligand_atom(batch: Batch, table, first=128):
    """Protein rows whose neighbour row holds a ligand atom that is number ``first`` or later of its graph's ligand: atoms a merge
    reaches only in its second and later passes of 128."""
    out = []
    ptr = batch.node_ptr.tolist()
    rows = table.tolist()
    for g in range(batch.B):
        p0, l0 = ptr[g], ptr[g] + batch.n_prot[g]
        for i in range(p0, l0):
            if any(j >= l0 + first for j in rows[i]):
                out.append(i)
    return out
