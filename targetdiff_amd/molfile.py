"""Molecules on disk without a chemistry toolkit: a plain MDL V2000 SD-file writer for the bond graph of ``quality.bond_graph`` and a
small reader for a known ligand (``read_sdf``, ``ligand_classes``: heavy atoms only).

    g = quality.bond_graph(pos, v, ligand_ptr=ptr, return_fragments=True, return_bonds=True)
    mols = molfile.molecules_from_graph(g, pos, v, frame=-1, largest_fragment=True)
    molfile.write_sdf('samples.sdf', mols)

A molecule is a dict: ``name``, ``symbols`` [n] element symbols, ``pos`` [n, 3], ``bonds`` [(i, j, type)] with 0-based atoms and the
SD-file bond type 1 / 2 / 3 / 4 (aromatic) -- the bond's category ("Bond graph": a convention for export, not
chemistry; no hydrogens, no valence repair, no kekulisation) -- and optional ``properties`` written as data items.
"""
from __future__ import annotations

import re

import numpy as np
import torch

from . import quality

ELEMENT_SYMBOLS = {1: 'H', 6: 'C', 7: 'N', 8: 'O', 9: 'F', 15: 'P', 16: 'S', 17: 'Cl'}
V2000_MAX = 999                                        # the counts line holds three digits


def _record(mol):
    symbols, pos, bonds = list(mol['symbols']), np.asarray(mol['pos'], dtype=np.float64).reshape(-1, 3), list(mol.get('bonds', ()))
    if len(symbols) != len(pos):
        raise ValueError(f'{len(symbols)} symbols for {len(pos)} positions')
    if len(symbols) > V2000_MAX or len(bonds) > V2000_MAX:
        raise ValueError(f'a V2000 record holds at most {V2000_MAX} atoms and bonds (got {len(symbols)}, {len(bonds)})')
    lines = [str(mol.get('name', '')), '  targetdiff_amd          3D', '',
             f'{len(symbols):3d}{len(bonds):3d}  0  0  0  0  0  0  0  0999 V2000']
    for sym, (x, y, z) in zip(symbols, pos):
        lines.append(f'{x:10.4f}{y:10.4f}{z:10.4f} {sym:<3s} 0  0  0  0  0  0  0  0  0  0  0  0')
    for i, j, t in bonds:
        if not (0 <= int(i) < len(symbols) and 0 <= int(j) < len(symbols)) or int(t) not in (1, 2, 3, 4):
            raise ValueError(f'bond ({i}, {j}, {t}): atoms are 0-based indices of the molecule, the type is 1, 2, 3 or 4')
        lines.append(f'{int(i) + 1:3d}{int(j) + 1:3d}{int(t):3d}  0  0  0  0')
    lines.append('M  END')
    for key, val in (mol.get('properties') or {}).items():
        lines += [f'>  <{key}>', str(val), '']
    lines.append('$$$$')
    return '\n'.join(lines) + '\n'


def write_sdf(path, molecules):
    """Write ``molecules`` (dicts as the module describes) to ``path`` as V2000 records; returns their number."""
    records = [_record(m) for m in molecules]
    with open(path, 'w') as f:
        f.write(''.join(records))
    return len(records)


def read_sdf(path):
    """The V2000 records of an SD file as molecules (dicts as the module describes), heavy atoms only: hydrogens and their bonds are
    dropped and the atoms renumbered.  Reads what ``write_sdf`` writes and plain toolkit output (a docked ligand); V3000 records, atom
    lists and query bond types are refused."""
    with open(path) as f:
        text = f.read().replace('\r\n', '\n')
    out = []
    for rec in re.split(r'\$\$\$\$[ \t]*\n?', text):
        lines = rec.split('\n')
        if not rec.strip():
            continue
        if len(lines) < 4:
            raise ValueError(f'{path}: record {len(out)} has no counts line')
        counts = lines[3]
        if 'V2000' not in counts:
            raise ValueError(f'{path}: record {len(out)} is not a V2000 molfile (counts line {counts!r})')
        na, nb = int(counts[0:3]), int(counts[3:6])
        if len(lines) < 4 + na + nb:
            raise ValueError(f'{path}: record {len(out)} ends before its {na} atoms and {nb} bonds')
        symbols, pos = [], []
        for ln in lines[4:4 + na]:
            pos.append((float(ln[0:10]), float(ln[10:20]), float(ln[20:30])))
            symbols.append(ln[31:34].strip())
        heavy = np.asarray([sym != 'H' for sym in symbols], dtype=bool)
        new = np.cumsum(heavy) - 1
        bonds = []
        for ln in lines[4 + na:4 + na + nb]:
            i, j, t = int(ln[0:3]) - 1, int(ln[3:6]) - 1, int(ln[6:9])
            if not (0 <= i < na and 0 <= j < na) or t not in (1, 2, 3, 4):
                raise ValueError(f'{path}: record {len(out)}: bond line {ln!r}')
            if heavy[i] and heavy[j]:
                bonds.append((int(new[i]), int(new[j]), t))
        rest = lines[4 + na + nb:]
        props = {rest[k][rest[k].index('<') + 1:rest[k].rindex('>')]: rest[k + 1] for k in range(len(rest) - 1)
                 if rest[k].startswith('>') and '<' in rest[k]}
        out.append(dict(name=lines[0], symbols=[sym for sym, h in zip(symbols, heavy) if h],
                        pos=np.asarray(pos, dtype=np.float64).reshape(-1, 3)[heavy], bonds=bonds, properties=props))
    return out


def ligand_classes(mol, atom_enc_mode='add_aromatic', drop_unknown=False):
    """(pos [n, 3] fp32, v [n] int64) of a molecule read by ``read_sdf``, ready for ``quality.fingerprints`` or
    ``sample_diversity(reference_ligand=...)``: the class of every atom from its element and, under ``'add_aromatic'``, from whether
    it carries a bond of type 4 -- a kekulised file therefore gives no aromatic class.  The file's bonds are not used beyond that: the
    fingerprint takes its bonds from the bond-length table, as it does for the samples.  An element outside the table (the sampler
    cannot produce it either) is refused, or with ``drop_unknown`` its atoms are left out."""
    cz, aro = quality.class_atomic_numbers(atom_enc_mode), quality.class_aromatic(atom_enc_mode)
    number = {sym: z for z, sym in ELEMENT_SYMBOLS.items()}
    table = {}
    for c, (z, a) in enumerate(zip(cz, aro)):
        table.setdefault((z, bool(a)), c)
    aromatic = np.zeros(len(mol['symbols']), dtype=bool)
    for i, j, t in mol.get('bonds', ()):
        if t == 4:
            aromatic[i] = aromatic[j] = True
    v, known = [], []
    for sym, a in zip(mol['symbols'], aromatic):
        known.append(sym in number)
        if not known[-1]:
            if drop_unknown:
                continue
            raise ValueError(f'element {sym!r} is outside the bond-length table {tuple(ELEMENT_SYMBOLS.values())}')
        z = number[sym]
        c = table.get((z, bool(a)), table.get((z, False)))
        if c is None:
            raise ValueError(f'atom_enc_mode {atom_enc_mode!r} has no class for element {sym}')
        v.append(c)
    return np.asarray(mol['pos'], dtype=np.float32).reshape(-1, 3)[np.asarray(known, dtype=bool)], np.asarray(v, dtype=np.int64)


def molecules_from_graph(graph, pos, v, atom_enc_mode='add_aromatic', frame=-1, only_complete=False, largest_fragment=False, names=None,
                         categories=None, select=None):
    """The molecules of one frame of a ``quality.BondGraph`` made with ``return_fragments=True, return_bonds=True`` on the pack
    (``pos`` [S, N_l, 3] or [N_l, 3], ``v`` alike).  ``only_complete`` drops the molecules of more than one fragment;
    ``largest_fragment`` keeps, of every molecule, the atoms and bonds of its largest fragment (of equal ones the one with the
    smallest label) -- chosen here on the host from ``graph.fragment``.  ``categories``: the bond types to write, one per bond of
    the graph's list; default ``graph.bond_category``; ``graph.ring_category`` of a graph made with ``rings=True`` keeps type 4 to
    bonds inside a ring of 5 or 6 atoms ("Rings").  ``select`` [B] bool: of the molecules that are left, only
    these (tools/export_sdf.py --unique)."""
    if graph.fragment is None or graph.bond_atoms is None:
        raise ValueError('the graph needs return_fragments=True and return_bonds=True')
    to_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    pos, v = to_np(pos), to_np(v)
    if pos.ndim == 2:
        pos, v = pos[None], v[None]
    S, B = graph.n_bonds.shape
    frame = frame % S
    ptr, bptr = to_np(graph.ligand_ptr), to_np(graph.bond_ptr)
    frag, nfrag = to_np(graph.fragment)[frame], to_np(graph.n_fragments)[frame]
    atoms, cats = to_np(graph.bond_atoms), to_np(graph.bond_category if categories is None else categories)
    if len(cats) != len(atoms):
        raise ValueError(f'{len(cats)} categories for {len(atoms)} bonds')
    cz = np.asarray(quality.class_atomic_numbers(atom_enc_mode))
    out = []
    for g in range(B):
        if (only_complete and nfrag[g] != 1) or (select is not None and not select[g]):
            continue
        a, b = int(ptr[g]), int(ptr[g + 1])
        k0, k1 = int(bptr[frame * B + g]), int(bptr[frame * B + g + 1])
        keep = np.ones(b - a, bool)
        if largest_fragment and b > a:
            sizes = np.bincount(frag[a:b], minlength=b - a)
            keep = frag[a:b] == int(np.argmax(sizes))                 # argmax: the first of equal sizes = the smallest label
        new = np.cumsum(keep) - 1
        bonds = [(int(new[i - a]), int(new[j - a]), int(c)) for (i, j), c in zip(atoms[k0:k1], cats[k0:k1]) if keep[i - a] and keep[j - a]]
        out.append(dict(name=names[g] if names is not None else f'sample_{g}', symbols=[ELEMENT_SYMBOLS[int(z)] for z in cz[v[frame, a:b][keep]]],
                        pos=pos[frame, a:b][keep], bonds=bonds,
                        properties=dict(n_fragments=int(nfrag[g]), n_atoms=int(keep.sum()), n_bonds=len(bonds))))
    return out
