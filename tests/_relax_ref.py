"""Numpy float64 restatement of the rigid-body relaxation ("Pose relaxation"), written from the contract of
td_score_minimize in include/targetdiff_hip.h: the pairs and term values of tests/_score_ref.py, the roles of tests/_interactions_ref.py
at the input pose, the pose fp32(R(q) x0 + (c0 + t)) in the header's operation order, the per-pair slope f = dE/dd and the six gradient
components, each rounded to units of 2^-24 and summed as int64, and BFGS with an Armijo backtracking line search on the 6-vector.  Only
exp can differ from the kernel in an evaluation; the 6 x 6 algebra may differ in its last bits, so trajectories are not compared.  It
shares no code with targetdiff_amd.quality.  A local optimisation under this project's heuristic score, not AutoDock Vina's minimize;
rigid-body only: three translations and three rotations, no torsions."""
import numpy as np

import _interactions_ref as IR
import _pocket_ref as PR
import _score_ref as SR

MAX_STEPS, MAX_SHIFT, TRIALS, ARMIJO = 64, 3.0, 10, 1e-4
CONVERGED, OUT_OF_BUDGET, AT_CAP = 1, 2, 4
KEYS = ('protein_role', 'n_rot', 'pos', 'terms_in', 'terms', 'n_pairs', 'n_steps', 'n_evals', 'status', 'transform', 'grad_in')


def centroid(lpos, scored):
    """c0 [3] float64: the scored atoms summed in index order"""
    x = np.asarray(lpos, np.float64)[scored]
    return np.cumsum(x, axis=0)[-1] / float(len(x)) if len(x) else np.zeros(3)


def rotation(q):
    """[3, 3] of the unit quaternion (w, x, y, z), in the header's operation order"""
    w, x, y, z = (np.float64(a) for a in q)
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    return np.asarray([[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
                       [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
                       [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]], np.float64)


def pose64(x0, q, t, c0):
    """[n, 3] float64: ((R_k0 x0 + R_k1 y0) + R_k2 z0) + (c0 + t)_k, before the rounding to fp32"""
    R, c = rotation(q), np.asarray(c0, np.float64) + np.asarray(t, np.float64)
    x0 = np.asarray(x0, np.float64).reshape(-1, 3)
    return ((R[None, :, 0] * x0[:, 0:1] + R[None, :, 1] * x0[:, 1:2]) + R[None, :, 2] * x0[:, 2:3]) + c[None, :]


def pose(x0, q, t, c0):
    return pose64(x0, q, t, c0).astype(np.float32)


def transformed(lpos, scored, transform):
    """the pose that a transform [7] (q, t) of td_score_minimize gives the input molecule lpos [n, 3] fp32"""
    c0 = centroid(lpos, scored)
    return pose(np.asarray(lpos, np.float64) - c0, transform[:4], transform[4:], c0)


def pair_slope(d, hy, hb, weights):
    """[m] float64 f = dE/dd of the counted pairs: zero on the flat pieces, at a breakpoint the piece that the term value takes"""
    w = np.asarray(weights, np.float64)
    t, u = d * 2.0, (d - 3.0) / 2.0
    with np.errstate(over='ignore'):
        e1, e2 = np.exp(-(t * t)), np.exp(-(u * u))
    dg1, dg2 = (-4.0 * t) * e1, (-u) * e2
    drep = np.where(d < 0.0, t, 0.0)
    dhy = np.where(hy & (d < 1.5) & ~(d < 0.5), -1.0, 0.0)
    dhb = np.where(hb & (d < 0.0) & ~(d < -0.7), -1.0 / 0.7, 0.0)
    return (((w[0] * dg1 + w[1] * dg2) + w[2] * drep) + w[3] * dhy) + w[4] * dhb


def counted(lpos, lel, ppos, pelem, prole, cutoff, r=None):
    """(ligand index [m], protein index [m], r [m]) of the pairs that count, in the order of _score_ref.molecule_pairs"""
    if not len(lpos) or not len(ppos):
        z = np.zeros(0, np.int64)
        return z, z, np.zeros(0)
    r = PR.distances(lpos, ppos) if r is None else r
    count = (lel > 0)[:, None] & ((prole >= 0) & (np.asarray(pelem) != 0))[None, :] & (r < np.float64(cutoff))
    li, pj = np.nonzero(count)
    return li, pj, r[count]


def evaluate(lpos, lel, lrole, centre, ppos, pelem, prole, rsum, cutoff, weights):
    """One evaluation at the fp32 pose lpos [n, 3]: (terms [5] int64, grad [6] int64, pairs); the torque about ``centre`` [3] float64"""
    d, hy, hb = SR.molecule_pairs(lpos, lel, lrole, ppos, pelem, prole, rsum, cutoff)
    li, pj, r = counted(lpos, lel, ppos, pelem, prole, cutoff)
    assert len(li) == len(d)
    if not len(d):
        return np.zeros(5, np.int64), np.zeros(6, np.int64), 0
    terms = SR.fixed(SR.term_values(d, hy, hb)).sum(0)
    f = pair_slope(d, hy, hb, weights)
    xl, xp = lpos.astype(np.float64)[li], ppos.astype(np.float64)[pj]
    ok = r > 0.0
    with np.errstate(invalid='ignore', divide='ignore'):
        g = f[:, None] * ((xl - xp) / r[:, None])
    a = xl - np.asarray(centre, np.float64)[None, :]
    torque = np.stack([a[:, 1] * g[:, 2] - a[:, 2] * g[:, 1], a[:, 2] * g[:, 0] - a[:, 0] * g[:, 2], a[:, 0] * g[:, 1] - a[:, 1] * g[:, 0]], 1)
    comp = np.where(ok[:, None], np.concatenate([g, torque], 1), 0.0)
    return terms, SR.fixed(comp).sum(0), len(d)


def energy(terms, weights):
    """inter of integer terms [5]: (((w0 T0 + w1 T1) + w2 T2) + w3 T3) + w4 T4"""
    T, w = np.asarray(terms, np.float64) / SR.UNIT, np.asarray(weights, np.float64)
    return float((((w[0] * T[0] + w[1] * T[1]) + w[2] * T[2]) + w[3] * T[3]) + w[4] * T[4])


def unrounded(lpos64, lel, lrole, centre, ppos, pelem, prole, rsum, cutoff, weights):
    """The energy and its analytic gradient with nothing rounded to fp32 or to units of 2^-24, at the float64 pose lpos64 [n, 3]:
    (E, grad [6], the smallest distance of a pair's d to a breakpoint or of its r to the cutoff) -- what central differences are taken of"""
    xl_all, xp_all = np.asarray(lpos64, np.float64), np.asarray(ppos, np.float64)
    diff = xl_all[:, None, :] - xp_all[None, :, :]
    r = np.sqrt((diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2])
    li, pj, rc = counted(xl_all, lel, ppos, pelem, prole, cutoff, r)
    part = (lel > 0)[:, None] & ((prole >= 0) & (np.asarray(pelem) != 0))[None, :]
    rs = np.asarray(rsum, np.float64).reshape(8, 6)[lel[li], np.asarray(pelem)[pj]]
    d = rc - rs
    prb = np.asarray(prole)[pj]
    hy = ((lrole[li] & IR.HYDROPHOBIC) != 0) & ((prb & IR.HYDROPHOBIC) != 0)
    hb = (((lrole[li] & IR.DONOR) != 0) & ((prb & IR.ACCEPTOR) != 0)) | (((lrole[li] & IR.ACCEPTOR) != 0) & ((prb & IR.DONOR) != 0))
    w = np.asarray(weights, np.float64)
    E = float((SR.term_values(d, hy, hb) * w).sum())
    f = pair_slope(d, hy, hb, w)
    g = f[:, None] * (diff[li, pj] / rc[:, None])
    a = xl_all[li] - np.asarray(centre, np.float64)[None, :]
    grad = np.concatenate([g.sum(0), np.cross(a, g).sum(0)])
    margins = [np.abs(r[part] - cutoff).min()] if part.any() else [np.inf]
    margins += [np.abs(d - b).min() for b in (0.0,)] if len(d) else []
    margins += [np.abs(d[hy] - b).min() for b in (0.5, 1.5) if hy.any()] + [np.abs(d[hb] - b).min() for b in (-0.7,) if hb.any()]
    return E, grad, float(min(margins))


def moved(q, t, delta):
    """the state (q, t) after the step delta [6]: t + delta[:3]; the normalised quaternion (1, delta[3:] / 2) composed on the left and
    renormalised"""
    h = 0.5 * np.asarray(delta[3:], np.float64)
    nrm = np.sqrt(1.0 + (h[0] * h[0] + h[1] * h[1] + h[2] * h[2]))
    dw, dx, dy, dz = 1.0 / nrm, h[0] / nrm, h[1] / nrm, h[2] / nrm
    qw, qx, qy, qz = q
    n = np.asarray([dw * qw - dx * qx - dy * qy - dz * qz, dw * qx + dx * qw + dy * qz - dz * qy,
                    dw * qy - dx * qz + dy * qw + dz * qx, dw * qz + dx * qy - dy * qx + dz * qw], np.float64)
    return n / np.sqrt((n * n).sum()), np.asarray(t, np.float64) + np.asarray(delta[:3], np.float64)


def relax_molecule(lpos, lel, lrole, ppos, pelem, prole, rsum, weights, cutoff=8.0, max_steps=MAX_STEPS, max_evals=None, max_shift=MAX_SHIFT,
                   torque=True):
    """The relaxation of one molecule: lpos [n, 3] fp32, lel [n] element indices (-1 outside the table), lrole [n] the roles of the input
    pose; the pocket with its RESOLVED roles prole.  Returns a dict: pos [n, 3] fp32, terms_in, terms [5] int64, n_pairs, n_steps,
    n_evals, status, transform [7], grad_in [6] int64 and trace, the energies of the accepted states.  ``torque=False`` zeroes the
    rotational gradient: the translation-only optimiser that the planted-minimum conditions must tell from the real one."""
    max_evals = 4 * max_steps + 1 if max_evals is None else max_evals
    lpos = np.asarray(lpos, np.float32)
    scored = lel > 0
    c0 = centroid(lpos, scored)
    x0 = lpos.astype(np.float64) - c0
    r2 = (x0[scored, 0] * x0[scored, 0] + x0[scored, 1] * x0[scored, 1]) + x0[scored, 2] * x0[scored, 2]
    msq = float(np.cumsum(r2)[-1]) / len(r2) if len(r2) else 0.0
    hr = 1.0 / msq if msq > 0.0 else 1.0
    H0 = np.diag([1.0, 1.0, 1.0, hr, hr, hr])

    def at(q, t, x):
        terms, grad, pairs = evaluate(x, lel, lrole, c0 + t, ppos, pelem, prole, rsum, cutoff, weights)
        gr = grad.astype(np.float64) / SR.UNIT
        if not torque:
            gr[3:] = 0.0
        return terms, grad, pairs, energy(terms, weights), gr

    q, t = np.asarray([1.0, 0.0, 0.0, 0.0]), np.zeros(3)
    terms, grad_in, pairs, f0, g = at(q, t, lpos)
    terms_in, x, evals, steps, status, H, trace = terms, lpos, 1, 0, 0, H0.copy(), [f0]
    while True:
        if steps >= max_steps:
            status |= OUT_OF_BUDGET
            break
        p = -(H @ g)
        slope = float(g @ p)
        if not slope < 0.0:
            H = H0.copy()
            p = -(H @ g)
            slope = float(g @ p)
            if not slope < 0.0:
                status |= CONVERGED
                break
        alpha, found = 1.0, None
        for _ in range(TRIALS):
            if evals >= max_evals:
                status |= OUT_OF_BUDGET
                break
            qn, tn = moved(q, t, alpha * p)
            if not np.sqrt(tn[0] * tn[0] + tn[1] * tn[1] + tn[2] * tn[2]) <= max_shift:
                status |= AT_CAP
                alpha *= 0.5
                continue
            xn = pose(x0, qn, tn, c0)
            tr, _, pn, f1, gn = at(qn, tn, xn)
            evals += 1
            if f1 - f0 < ARMIJO * alpha * slope:
                found = (qn, tn, xn, tr, pn, f1, gn)
                break
            alpha *= 0.5
        if status & OUT_OF_BUDGET:
            break
        if found is None:
            status |= CONVERGED
            break
        s, y = alpha * p, found[6] - g
        q, t, x, terms, pairs, f0, g = found
        steps += 1
        trace.append(f0)
        sy = float(s @ y)
        if sy > 0.0 and steps < max_steps:
            Hy = H @ y
            r = 1.0 / sy
            H = H + ((1.0 + float(y @ Hy) * r) * r) * np.outer(s, s) - r * (np.outer(Hy, s) + np.outer(s, Hy))
    return dict(pos=x, terms_in=terms_in, terms=terms, n_pairs=pairs, n_steps=steps, n_evals=evals, status=status,
                transform=np.concatenate([q, t]), grad_in=grad_in, trace=trace)


def molecule_inputs(pos, cls, class_z):
    """(element indices, roles, scored) of one molecule at the pose pos [n, 3] fp32"""
    lel = SR.element_index(cls, class_z)
    return lel, IR.ligand_roles(pos, cls, class_z), lel > 0


def score_minimize(pos, v, ptr, class_z, class_aromatic, ppos, pelem, pkind, prole, n_kinds, rsum, weights=SR.WEIGHTS, cutoff=8.0,
                   hetero_cutoff=1.75, with_rotors=True, max_steps=MAX_STEPS, max_evals=None, max_shift=MAX_SHIFT):
    """numpy twin of capi.score_minimize: pos [S, N, 3] fp32, v [S, N], ptr [B + 1], the pocket as _score_ref.score_report takes it"""
    pos, v, ptr, ppos, pelem = np.asarray(pos, np.float32), np.asarray(v), np.asarray(ptr), np.asarray(ppos, np.float32), np.asarray(pelem)
    S, B = pos.shape[0], len(ptr) - 1
    pr = IR.protein_roles(ppos, pelem, pkind, prole, n_kinds, hetero_cutoff)
    out = dict(protein_role=pr, n_rot=np.zeros((S, B), np.int32) if with_rotors else None, pos=pos.copy(),
               terms_in=np.zeros((S, B, 5), np.int64), terms=np.zeros((S, B, 5), np.int64), n_pairs=np.zeros((S, B), np.int32),
               n_steps=np.zeros((S, B), np.int32), n_evals=np.zeros((S, B), np.int32), status=np.zeros((S, B), np.int32),
               transform=np.zeros((S, B, 7)), grad_in=np.zeros((S, B, 6), np.int64))
    out['transform'][..., 0] = 1.0
    for s in range(S):
        for g in range(B):
            a, b = int(ptr[g]), int(ptr[g + 1])
            if b - a > SR.MAX_ATOMS or (b > a and (a < 0 or b > pos.shape[1])):
                out['terms_in'][s, g] = out['terms'][s, g] = SR.INT64_MIN
                out['n_pairs'][s, g] = out['status'][s, g] = -1
                if with_rotors:
                    out['n_rot'][s, g] = -1
                continue
            lel, lrole, _ = molecule_inputs(pos[s, a:b], v[s, a:b], class_z)
            r = relax_molecule(pos[s, a:b], lel, lrole, ppos, pelem, pr, rsum, weights, cutoff, max_steps, max_evals, max_shift)
            if r['n_steps'] > 0:
                out['pos'][s, a:b] = r['pos']
            for k in ('terms_in', 'terms', 'n_pairs', 'n_steps', 'n_evals', 'status', 'transform', 'grad_in'):
                out[k][s, g] = r[k]
            if with_rotors:
                out['n_rot'][s, g] = SR.rotors(pos[s, a:b], v[s, a:b], class_z, class_aromatic)
    return out


def torch_score_minimize(pos, v, ligand_ptr, class_z, class_aromatic, protein_pos, protein_elem, protein_kind, protein_role, n_kinds, rsum,
                         weights, cutoff=8.0, hetero_cutoff=1.75, bond_ptr=None, bond_ring=None, max_steps=MAX_STEPS, max_evals=None,
                         max_shift=MAX_SHIFT, check=True):
    """score_minimize with capi.score_minimize's signature on CPU tensors: what the host tests patch the binding with"""
    import torch
    from targetdiff_amd import capi
    S, _, B, _, aro, _ = capi._bond_inputs(pos, v, ligand_ptr, class_z, class_aromatic, None, (), check)
    capi._score_inputs(pos, protein_pos, protein_elem, protein_kind, protein_role, n_kinds, rsum, cutoff, hetero_cutoff, bond_ptr, bond_ring,
                       S, B, check)
    w, max_steps, max_evals, max_shift = capi._relax_inputs(weights, max_steps, max_evals, max_shift)
    r = score_minimize(pos.cpu().numpy(), v.cpu().numpy(), ligand_ptr.cpu().numpy(), class_z, class_aromatic, protein_pos.cpu().numpy(),
                       protein_elem.cpu().numpy(), protein_kind.cpu().numpy(), protein_role.cpu().numpy(), int(n_kinds),
                       np.asarray(rsum, np.float64), w, float(cutoff), float(hetero_cutoff), bond_ptr is not None, max_steps, max_evals,
                       max_shift)
    return {k: (None if r[k] is None else torch.from_numpy(r[k])) for k in KEYS}
