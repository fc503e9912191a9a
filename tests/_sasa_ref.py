"""Numpy float64 restatement of the solvent-accessible-surface report ("Solvent-accessible surface"): fp32 centres
widened to float64, test point x = c + R u with one product and one add per coordinate, D2 = ((dx dx + dy dy) + dz dz) with numpy's
separately rounded elementwise operations, occluded iff D2 < R R, strictly.  No culling: every point meets every sphere, by plain
broadcasting (in blocks of occluders, to bound the memory).  Pinned to hand cases on the host (tests/test_sasa_host.py); the GPU tests
compare the kernel with it.  It also holds the case builder both share.  It shares no code with targetdiff_amd.quality."""
import numpy as np

MAX_ATOMS = 512
MAX_POINTS = 256
LIGAND_Z = (1, 6, 7, 8, 9, 15, 16, 17)                      # H C N O F P S Cl
PROTEIN_Z = (1, 6, 7, 8, 16, 34)                            # H C N O S Se
RADII = {1: 1.2, 6: 1.7, 7: 1.55, 8: 1.52, 9: 1.47, 15: 1.8, 16: 1.8, 17: 1.75, 34: 1.9}      # van der Waals, Angstrom
MOL_KEYS = ('free', 'bound', 'pocket_buried')
ATOM_KEYS = ('atom_free', 'atom_bound')
POCKET_KEYS = ('pocket_free', 'pocket_mask')
KEYS = MOL_KEYS + ATOM_KEYS + ('bits',) + POCKET_KEYS + ('pocket_buried_sum',)


def directions(P):
    """[P, 3] float64: the golden-section spiral, z_k = 1 - (2k + 1) / P, r = sqrt(1 - z^2), phi = k pi (3 - sqrt 5)"""
    k = np.arange(P, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / np.float64(P)
    r = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def reaches(probe=1.4):
    """([8], [6]) float64: van der Waals radius + probe over the ligand's and the protein's elements"""
    p = np.float64(probe)
    return (np.asarray([RADII[z] for z in LIGAND_Z], np.float64) + p, np.asarray([RADII[z] for z in PROTEIN_Z], np.float64) + p)


def points_of(centres, R, dirs):
    """[n, P, 3] float64: c + R u, the product rounded, then the sum"""
    return centres[:, None, :] + R[:, None, None] * dirs[None, :, :]


def occluded(points, centres, R, self_pairs=False, block=32):
    """[n, P] bool: point (i, k) lies inside some sphere j (D2 < R_j R_j), j != i when ``self_pairs``: the spheres are the points' own"""
    n, P = points.shape[:2]
    hit = np.zeros((n, P), bool)
    R2 = R * R
    for j0 in range(0, len(centres), block):
        c = centres[j0:j0 + block]
        dx, dy, dz = (points[:, :, None, k] - c[None, None, :, k] for k in range(3))
        D2 = (dx * dx + dy * dy) + dz * dz
        inside = D2 < R2[None, None, j0:j0 + block]
        if self_pairs:
            j = np.arange(j0, j0 + len(c))
            inside &= (np.arange(n)[:, None] != j[None, :])[:, None, :]
        hit |= inside.any(2)
    return hit


def pack_mask(exposed):
    """[n, P] bool -> [n, 4] int64 words: bit k & 63 of word k >> 6"""
    n, P = exposed.shape
    words = np.zeros((n, 4), np.uint64)
    for k in range(P):
        words[:, k >> 6] |= exposed[:, k].astype(np.uint64) << np.uint64(k & 63)
    return words.view(np.int64)


def pack_bits(flags):
    """[N_p] bool -> [ceil(N_p / 64)] int64 words: bit j & 63 of word j >> 6"""
    flags = np.asarray(flags, bool)
    words = np.zeros((len(flags) + 63) // 64, np.uint64)
    for j in np.nonzero(flags)[0]:
        words[j >> 6] |= np.uint64(1) << np.uint64(j & 63)
    return words.view(np.int64)


def unpack_bits(words, n):
    """[..., W] int64 words -> [..., n] bool"""
    w = np.ascontiguousarray(words).view(np.uint64)
    j = np.arange(n)
    return ((w[..., j >> 6] >> (j & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


def apo(ppos, pelem, prot_reach, dirs):
    """(takes part [N_p] bool, element [N_p], exposed [N_p, P] bool, points [N_p, P, 3]) of the pocket alone"""
    pelem = np.asarray(pelem)
    part = (pelem >= 0) & (pelem < 6)
    el = np.where(part, pelem, 0)
    c = np.asarray(ppos).astype(np.float64).reshape(-1, 3)
    R = np.asarray(prot_reach, np.float64)[el]
    pts = points_of(c, R, dirs)
    exposed = np.zeros(pts.shape[:2], bool)
    idx = np.nonzero(part)[0]
    if len(idx):
        exposed[idx] = ~occluded(pts[idx], c[idx], R[idx], True)
    return part, el, exposed, pts


def sasa_report(pos, v, ptr, class_z, ppos, pelem, lig_reach, prot_reach, dirs, include=None):
    """numpy twin of capi.sasa_report: pos [S, N, 3] fp32, v [S, N], ptr [B + 1], ppos [N_p, 3] fp32, pelem [N_p], the reaches [8] and
    [6], dirs [P, 3] float64"""
    pos, v, ptr = np.asarray(pos), np.asarray(v), np.asarray(ptr)
    ppos = np.asarray(ppos, np.float32).reshape(-1, 3)
    assert pos.dtype == np.float32
    dirs = np.asarray(dirs, np.float64)
    lig_reach, prot_reach = np.asarray(lig_reach, np.float64), np.asarray(prot_reach, np.float64)
    S, N, B, Np, K, P = pos.shape[0], pos.shape[1], len(ptr) - 1, len(ppos), len(class_z), len(dirs)
    W = (Np + 63) // 64
    elem_of_z = {z: e for e, z in enumerate(LIGAND_Z)}
    part, pel, apo_exposed, ppts = apo(ppos, pelem, prot_reach, dirs)
    pc = ppos.astype(np.float64)
    pR = prot_reach[pel]
    pidx = np.nonzero(part)[0]
    out = dict(free=np.zeros((S, B, 8), np.int32), bound=np.zeros((S, B, 8), np.int32), pocket_buried=np.zeros((S, B, 6), np.int32),
               atom_free=np.zeros((S, N), np.int32), atom_bound=np.zeros((S, N), np.int32), bits=np.zeros((S, B, W), np.int64),
               pocket_free=apo_exposed.sum(1).astype(np.int32), pocket_mask=pack_mask(apo_exposed) if Np else np.zeros((0, 4), np.int64),
               pocket_buried_sum=np.zeros((S, Np), np.int64))
    for s in range(S):
        for g in range(B):
            a, b = int(ptr[g]), int(ptr[g + 1])
            if b - a > MAX_ATOMS or (b > a and (a < 0 or b > N)):
                for k in MOL_KEYS:
                    out[k][s, g] = -1
                continue
            if b <= a:
                continue
            cls = v[s, a:b]
            valid = (cls >= 0) & (cls < K)
            el = np.asarray([elem_of_z[class_z[c]] if ok else 0 for c, ok in zip(cls, valid)], np.int64).reshape(-1)
            li = np.nonzero(valid)[0]
            c = pos[s, a:b].astype(np.float64)[li]
            R, e = lig_reach[el[li]], el[li]
            pts = points_of(c, R, dirs)
            free = ~occluded(pts, c, R, True)
            bound = free & ~occluded(pts, pc[pidx], pR[pidx])
            out['atom_free'][s, a + li] = free.sum(1)
            out['atom_bound'][s, a + li] = bound.sum(1)
            np.add.at(out['free'][s, g], e, free.sum(1))
            np.add.at(out['bound'][s, g], e, bound.sum(1))
            buried = np.zeros(Np, np.int64)
            if len(pidx) and len(li):
                buried[pidx] = (apo_exposed[pidx] & occluded(ppts[pidx], c, R)).sum(1)
            np.add.at(out['pocket_buried'][s, g], pel[pidx], buried[pidx])
            out['bits'][s, g] = pack_bits(buried > 0)
            if include is None or include[s][g]:
                out['pocket_buried_sum'][s] += buried
    return out


def torch_sasa_report(pos, v, ligand_ptr, class_z, protein_pos, protein_elem, ligand_reach, protein_reach, dirs, include=None,
                      return_atoms=True, return_bits=True, check=True):
    """sasa_report with capi.sasa_report's signature on CPU tensors: what the host tests patch the binding with"""
    import torch
    from targetdiff_amd import capi
    capi._sasa_inputs(pos, v, ligand_ptr, class_z, protein_pos, protein_elem, ligand_reach, protein_reach, dirs, include, check)
    r = sasa_report(pos.cpu().numpy(), v.cpu().numpy(), ligand_ptr.cpu().numpy(), class_z, protein_pos.cpu().numpy(),
                    protein_elem.cpu().numpy(), ligand_reach, protein_reach, dirs.cpu().numpy(),
                    None if include is None else include.cpu().numpy())
    out = {k: torch.from_numpy(r[k]) for k in KEYS}
    if not return_atoms:
        out['atom_free'] = out['atom_bound'] = None
    if not return_bits:
        out['bits'] = None
    return out


# ---- the case builder of the host and GPU tests
def build_case(seed, n_p, sizes, S=1, K=13, dead=True, spacing=3.5):
    """One pocket of ``n_p`` atoms and a pack of S frames of molecules of ``sizes``, points of a ball that the pocket and the ligands
    share, of the volume that gives the pocket and the largest molecule together about one atom per ``spacing``^3 cubic Angstrom: a
    sphere (reach about 3 A) then meets a few others, so that some of its points are buried and some exposed.  ``dead``: some protein
    atoms of element -1.  Returns a dict of numpy arrays: pos [S, N, 3] fp32, v [S, N] int64, ptr [B + 1] int32, ppos [n_p, 3] fp32,
    pelem [n_p] int32."""
    rng = np.random.default_rng(seed)
    N = int(sum(sizes))
    radius = max(3.0, spacing * (0.24 * (n_p + max(list(sizes) + [0]))) ** (1.0 / 3.0))

    def points(shape):
        x = rng.normal(size=shape + (3,))
        x *= (radius * rng.random(shape + (1,)) ** (1.0 / 3.0)) / np.linalg.norm(x, axis=-1, keepdims=True)
        return x.astype(np.float32)

    pelem = rng.choice(6, n_p, p=(0.1, 0.5, 0.15, 0.2, 0.03, 0.02)).astype(np.int32)
    if dead and n_p:
        pelem[rng.random(n_p) < 0.05] = -1
    return dict(pos=points((S, N)), v=rng.integers(0, K, (S, N)).astype(np.int64), ptr=np.cumsum([0] + list(sizes)).astype(np.int32),
                ppos=points((n_p,)), pelem=pelem)
