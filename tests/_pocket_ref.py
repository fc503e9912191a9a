"""Numpy float64 restatement of the pocket contact report ("Pocket contacts"): fp32 coordinates widened to float64,
d = sqrt((dx dx + dy dy) + dz dz) with numpy's separately rounded elementwise operations, then strict comparisons with the contact cutoff
and the clash table.  Pinned to hand-counted cases on the host (tests/test_pocket_host.py); the GPU tests compare the kernel with it.
It also holds the case builder both share.  It shares no code with targetdiff_amd.quality."""
import numpy as np

MAX_ATOMS = 512
LIGAND_Z = (1, 6, 7, 8, 9, 15, 16, 17)                      # H C N O F P S Cl
PROTEIN_Z = (1, 6, 7, 8, 16, 34)                            # H C N O S Se
RADII = {1: 1.2, 6: 1.7, 7: 1.55, 8: 1.52, 9: 1.47, 15: 1.8, 16: 1.8, 17: 1.75, 34: 1.9}      # van der Waals, Angstrom
MOL_KEYS = ('n_contacts', 'n_contact_atoms', 'n_pocket_atoms', 'min_dist')
CLASH_KEYS = ('n_clashes', 'n_clash_atoms')
ATOM_KEYS = ('atom_contacts', 'atom_clash')
SUM_KEYS = ('kind_hist', 'pocket_freq')
KEYS = MOL_KEYS + CLASH_KEYS + ('n_ref_common',) + ATOM_KEYS + ('bits',) + SUM_KEYS


def clash_table(tolerance=0.5):
    """[8, 6] float64: r_l + r_p - tolerance"""
    rl, rp = np.asarray([RADII[z] for z in LIGAND_Z], np.float64), np.asarray([RADII[z] for z in PROTEIN_Z], np.float64)
    return (rl[:, None] + rp[None, :]) - np.float64(tolerance)


def distances(lig, prot):
    """[n, N_p] float64 of fp32 coordinates: widened, every product and sum rounded on its own, numpy's sqrt"""
    assert lig.dtype == np.float32 and prot.dtype == np.float32
    d = lig.astype(np.float64)[:, None, :] - prot.astype(np.float64)[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def pack_bits(flags):
    """[N_p] bool -> [ceil(N_p / 64)] int64 words: bit j & 63 of word j >> 6"""
    flags = np.asarray(flags, bool)
    W = (len(flags) + 63) // 64
    words = np.zeros(W, np.uint64)
    for j in np.nonzero(flags)[0]:
        words[j >> 6] |= np.uint64(1) << np.uint64(j & 63)
    return words.view(np.int64)


def unpack_bits(words, n):
    """[..., W] int64 words -> [..., n] bool"""
    w = np.ascontiguousarray(words).view(np.uint64)
    j = np.arange(n)
    return ((w[..., j >> 6] >> (j & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


def pocket_report(pos, v, ptr, class_z, ppos, pelem, pkind, n_kinds, cutoff, clash_threshold=None, include=None, ref_bits=None):
    """numpy twin of capi.pocket_report: pos [S, N, 3] fp32, v [S, N], ptr [B + 1], ppos [N_p, 3] fp32, pelem / pkind [N_p]; without a
    table the clash outputs are None, without ref_bits n_ref_common is"""
    pos, v, ptr, ppos = np.asarray(pos), np.asarray(v), np.asarray(ptr), np.asarray(ppos)
    pelem, pkind = np.asarray(pelem), np.asarray(pkind)
    S, N, B, Np, K = pos.shape[0], pos.shape[1], len(ptr) - 1, len(ppos), len(class_z)
    W = (Np + 63) // 64
    takes_part = (pelem >= 0) & (pelem < 6) & (pkind >= 0) & (pkind < n_kinds)
    thr = None if clash_threshold is None else np.asarray(clash_threshold, np.float64).reshape(8, 6)
    ref = None if ref_bits is None else unpack_bits(np.asarray(ref_bits), Np)
    elem_of_z = {z: e for e, z in enumerate(LIGAND_Z)}
    out = {k: np.zeros((S, B), np.int32) for k in ('n_contacts', 'n_contact_atoms', 'n_pocket_atoms', 'n_ref_common') + CLASH_KEYS}
    out.update(min_dist=np.full((S, B), np.inf), atom_contacts=np.zeros((S, N), np.int32), atom_clash=np.zeros((S, N), np.int32),
               bits=np.zeros((S, B, W), np.int64), kind_hist=np.zeros((S, 8, n_kinds), np.int64), pocket_freq=np.zeros((S, Np), np.int32))
    for s in range(S):
        for g in range(B):
            a, b = int(ptr[g]), int(ptr[g + 1])
            if b - a > MAX_ATOMS or (b > a and (a < 0 or b > N)):
                for k in ('n_contacts', 'n_contact_atoms', 'n_pocket_atoms', 'n_ref_common') + CLASH_KEYS:
                    out[k][s, g] = -1
                continue
            cls = v[s, a:b]
            valid = (cls >= 0) & (cls < K)
            el = np.asarray([elem_of_z[class_z[c]] if ok else 0 for c, ok in zip(cls, valid)], np.int64).reshape(-1)
            d = distances(pos[s, a:b], ppos)
            pair = valid[:, None] & takes_part[None, :]
            con = pair & (d < np.float64(cutoff))
            out['n_contacts'][s, g] = con.sum()
            out['atom_contacts'][s, a:b] = con.sum(1)
            out['n_contact_atoms'][s, g] = con.any(1).sum()
            touched = con.any(0)
            out['n_pocket_atoms'][s, g] = touched.sum()
            out['bits'][s, g] = pack_bits(touched)
            if pair.any():
                out['min_dist'][s, g] = d[pair].min()
            if ref is not None:
                out['n_ref_common'][s, g] = (touched & ref).sum()
            if thr is not None:
                cl = pair & (d < thr[el[:, None], np.where(takes_part, pelem, 0)[None, :]])
                out['n_clashes'][s, g] = cl.sum()
                out['atom_clash'][s, a:b] = cl.sum(1)
                out['n_clash_atoms'][s, g] = cl.any(1).sum()
            if include is None or include[s][g]:
                li, pj = np.nonzero(con)
                np.add.at(out['kind_hist'][s], (el[li], pkind[pj]), 1)
                out['pocket_freq'][s] += touched
    if thr is None:
        out['n_clashes'] = out['n_clash_atoms'] = out['atom_clash'] = None
    if ref is None:
        out['n_ref_common'] = None
    return out


def torch_pocket_report(pos, v, ligand_ptr, class_z, protein_pos, protein_elem, protein_kind, n_kinds, contact_cutoff, clash_threshold=None,
                        include=None, ref_bits=None, return_atoms=True, return_bits=True, check=True):
    """pocket_report with capi.pocket_report's signature on CPU tensors: what the host tests patch the binding with"""
    import torch
    from targetdiff_amd import capi
    capi._bond_inputs(pos, v, ligand_ptr, class_z, None, include, (), check)
    _, _, thr = capi._pocket_inputs(pos, protein_pos, protein_elem, protein_kind, n_kinds, contact_cutoff, clash_threshold, ref_bits, check)
    r = pocket_report(pos.cpu().numpy(), v.cpu().numpy(), ligand_ptr.cpu().numpy(), class_z, protein_pos.cpu().numpy(),
                      protein_elem.cpu().numpy(), protein_kind.cpu().numpy(), int(n_kinds), float(contact_cutoff), thr,
                      None if include is None else include.cpu().numpy(), None if ref_bits is None else ref_bits.cpu().numpy())
    out = {k: (None if r[k] is None else torch.from_numpy(r[k])) for k in KEYS}
    if not return_atoms:
        out['atom_contacts'] = out['atom_clash'] = None
    if not return_bits:
        out['bits'] = None
    return out


# ---- the case builder of the host and GPU tests
def build_case(seed, n_p, sizes, S=1, lattice=False, K=13, n_kinds=40, dead=True):
    """One pocket of ``n_p`` atoms and a pack of S frames of molecules of ``sizes``: points of a ball that the pocket and the ligands
    share (``lattice``: coordinates on a 0.5 A grid, exact in fp32, with many equal distances), at a density that gives a few contacts
    per atom under a 4 A cutoff.  ``dead``: some protein atoms of kind -1 and some of element -1.  Returns a dict of numpy arrays: pos
    [S, N, 3] fp32, v [S, N] int64, ptr [B + 1] int32, ppos [n_p, 3] fp32, pelem, pkind [n_p] int32."""
    rng = np.random.default_rng(seed)
    N = int(sum(sizes))
    radius = max(3.0, 1.3 * (n_p + N) ** (1.0 / 3.0))

    def points(shape):
        x = rng.normal(size=shape + (3,))
        x *= (radius * rng.random(shape + (1,)) ** (1.0 / 3.0)) / np.linalg.norm(x, axis=-1, keepdims=True)
        return (np.round(x * 2.0) / 2.0 if lattice else x).astype(np.float32)

    pelem = rng.choice(6, n_p, p=(0.1, 0.5, 0.15, 0.2, 0.03, 0.02)).astype(np.int32)
    pkind = rng.integers(0, n_kinds, n_p).astype(np.int32)
    if dead and n_p:
        pkind[rng.random(n_p) < 0.1] = -1
        pelem[rng.random(n_p) < 0.05] = -1
    return dict(pos=points((S, N)), v=rng.integers(0, K, (S, N)).astype(np.int64), ptr=np.cumsum([0] + list(sizes)).astype(np.int32),
                ppos=points((n_p,)), pelem=pelem, pkind=pkind)
