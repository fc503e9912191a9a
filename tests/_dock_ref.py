"""Numpy float64 restatement of the docking search ("Docking search"), written on tests/_relax_ref.py from the contract
of td_score_dock in include/targetdiff_hip.h: per (molecule, chain) rounds of mutate-and-relax with caller-supplied uniforms, a Metropolis
rule on inter, the chain's best, and the selection of the chain with the lowest inter.  The mutation is written in the header's operation
order, so a chain's state after a mutation is the kernel's bit for bit; the local optimisation is _relax_ref's loop restated from a state
(q, t) (its 6 x 6 algebra may differ from the kernel's in its last bits, so trajectories are compared only at max_steps = 0).  It is a
rigid-body global search under this project's heuristic score, not AutoDock Vina's dock: three translations and three rotations, no
torsions."""
import numpy as np

import _interactions_ref as IR
import _relax_ref as RR
import _score_ref as SR

N_CHAINS, N_ROUNDS, AMPLITUDE, TEMPERATURE, DRAWS = 16, 16, 2.0, 1.2, 7
KEYS = RR.KEYS + ('best_chain', 'chain_terms', 'chain_transform', 'chain_accepts', 'chain_evals')
CLAMP = 1.0 - 2.0 ** -40


def mutated(q, t, u, amplitude, hr, max_shift):
    """The state (q, t) after the mutation by six uniforms u: (q [4], t [3], clamped).  Every product, sum, quotient and square root is
    rounded on its own, in the order of the header."""
    a, f = np.float64(amplitude), np.float64
    s = [f(2.0) * f(x) - f(1.0) for x in u[:6]]
    t = [f(t[k]) + a * s[k] for k in range(3)]
    root = np.sqrt(f(hr))
    h = [f(0.5) * ((a * s[3 + k]) * root) for k in range(3)]
    nrm = np.sqrt(f(1.0) + ((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]))
    dw, dx, dy, dz = f(1.0) / nrm, h[0] / nrm, h[1] / nrm, h[2] / nrm
    qw, qx, qy, qz = (f(x) for x in q)
    w = ((dw * qw - dx * qx) - dy * qy) - dz * qz
    x = ((dw * qx + dx * qw) + dy * qz) - dz * qy
    y = ((dw * qy - dx * qz) + dy * qw) + dz * qx
    z = ((dw * qz + dx * qy) - dy * qx) + dz * qw
    length = np.sqrt(((w * w + x * x) + y * y) + z * z)
    norm = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    clamped = bool(norm > f(max_shift))
    if clamped:
        scale = (f(max_shift) / norm) * f(CLAMP)
        t = [x_ * scale for x_ in t]
    return np.asarray([w / length, x / length, y / length, z / length], np.float64), np.asarray(t, np.float64), clamped


class Molecule:
    """What a workgroup stages of one molecule: the roles of the input pose, c0, x0, hr and the protein atoms within reach"""

    def __init__(self, lpos, lel, lrole, ppos, pelem, prole, rsum, weights, cutoff=8.0, max_shift=RR.MAX_SHIFT):
        self.lpos, self.lel, self.lrole = np.asarray(lpos, np.float32), lel, lrole
        self.rsum, self.weights, self.cutoff, self.max_shift = rsum, weights, cutoff, max_shift
        scored = lel > 0
        self.c0 = RR.centroid(self.lpos, scored)
        self.x0 = self.lpos.astype(np.float64) - self.c0
        r2 = (self.x0[scored, 0] * self.x0[scored, 0] + self.x0[scored, 1] * self.x0[scored, 1]) + self.x0[scored, 2] * self.x0[scored, 2]
        msq = float(np.cumsum(r2)[-1]) / len(r2) if len(r2) else 0.0
        self.hr = 1.0 / msq if msq > 0.0 else 1.0
        ppos, pelem, prole = np.asarray(ppos, np.float32), np.asarray(pelem), np.asarray(prole)
        if len(ppos) and len(r2):                                                # a superset of what any reachable pose can count
            reach = np.sqrt(r2.max()) + cutoff + max_shift + 0.1
            near = ((ppos.astype(np.float64) - self.c0) ** 2).sum(1) <= reach * reach
            ppos, pelem, prole = ppos[near], pelem[near], prole[near]
        self.ppos, self.pelem, self.prole = ppos, pelem, prole

    def at(self, q, t, x=None):
        """one evaluation at the state (q, t): (x fp32, terms, pairs, inter, gradient in float64, grad int64)"""
        x = RR.pose(self.x0, q, t, self.c0) if x is None else x
        terms, grad, pairs = RR.evaluate(x, self.lel, self.lrole, self.c0 + t, self.ppos, self.pelem, self.prole, self.rsum, self.cutoff,
                                         self.weights)
        return x, terms, pairs, RR.energy(terms, self.weights), grad.astype(np.float64) / SR.UNIT, grad

    def relax_from(self, q, t, max_steps, max_evals, x=None):
        """_relax_ref.relax_molecule's loop from the state (q, t), H0 fresh; ``x``: the input pose itself, for the identity state.  Returns
        a dict: q, t, pos, terms, n_pairs, inter, n_steps, n_evals, status, and terms_in / grad_in of the first evaluation."""
        H0 = np.diag([1.0, 1.0, 1.0, self.hr, self.hr, self.hr])
        q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
        x, terms, pairs, f0, g, grad_in = self.at(q, t, x)
        terms_in, evals, steps, status, H = terms, 1, 0, 0, H0.copy()
        while True:
            if steps >= max_steps:
                status |= RR.OUT_OF_BUDGET
                break
            p = -(H @ g)
            slope = float(g @ p)
            if not slope < 0.0:
                H = H0.copy()
                p = -(H @ g)
                slope = float(g @ p)
                if not slope < 0.0:
                    status |= RR.CONVERGED
                    break
            alpha, found = 1.0, None
            for _ in range(RR.TRIALS):
                if evals >= max_evals:
                    status |= RR.OUT_OF_BUDGET
                    break
                qn, tn = RR.moved(q, t, alpha * p)
                if not np.sqrt(tn[0] * tn[0] + tn[1] * tn[1] + tn[2] * tn[2]) <= self.max_shift:
                    status |= RR.AT_CAP
                    alpha *= 0.5
                    continue
                xn, tr, pn, f1, gn, _ = self.at(qn, tn)
                evals += 1
                if f1 - f0 < RR.ARMIJO * alpha * slope:
                    found = (qn, tn, xn, tr, pn, f1, gn)
                    break
                alpha *= 0.5
            if status & RR.OUT_OF_BUDGET:
                break
            if found is None:
                status |= RR.CONVERGED
                break
            s, y = alpha * p, found[6] - g
            q, t, x, terms, pairs, f0, g = found
            steps += 1
            sy = float(s @ y)
            if sy > 0.0 and steps < max_steps:
                Hy = H @ y
                r = 1.0 / sy
                H = H + ((1.0 + float(y @ Hy) * r) * r) * np.outer(s, s) - r * (np.outer(Hy, s) + np.outer(s, Hy))
        return dict(q=q, t=t, pos=x, terms=terms, n_pairs=pairs, inter=f0, n_steps=steps, n_evals=evals, status=status, terms_in=terms_in,
                    grad_in=grad_in)

    def chain(self, c, draws, n_rounds, amplitude=AMPLITUDE, temperature=TEMPERATURE, max_steps=RR.MAX_STEPS, max_evals=None):
        """Chain c with draws [n_rounds + 1, 7].  Returns a dict: the chain's best (q, t, terms, n_pairs, inter, status, pos), accepts,
        n_steps and n_evals summed over its rounds, ``first`` (round 0's result), ``margin``: the smallest |difference of energies| that
        a Metropolis or best-so-far decision turned on, and ``history``: the best inter after each round."""
        max_evals = 4 * max_steps + 1 if max_evals is None else max_evals
        q, t, e_cur = np.asarray([1.0, 0.0, 0.0, 0.0]), np.zeros(3), None
        best, accepts, steps, evals, margin, history, first = None, 0, 0, 0, np.inf, [], None
        for r in range(n_rounds + 1):
            u = np.asarray(draws[r], np.float64)
            if c == 0 and r == 0:
                res = self.relax_from(q, t, max_steps, max_evals, self.lpos)
            else:
                qm, tm, clamped = mutated(q, t, u, amplitude, self.hr, self.max_shift)
                res = self.relax_from(qm, tm, max_steps, max_evals)
                if clamped:
                    res['status'] |= RR.AT_CAP
            steps, evals, e = steps + res['n_steps'], evals + res['n_evals'], res['inter']
            if r == 0:
                accept, first = True, res
            else:
                with np.errstate(divide='ignore'):
                    threshold = e_cur - temperature * np.log(u[6])                # accepted when e < e_cur or u6 < exp((e_cur - e) / T)
                margin = min(margin, abs(threshold - e))
                accept = e < e_cur or u[6] < np.exp((e_cur - e) / temperature)
            if accept:
                q, t, e_cur, accepts = res['q'], res['t'], e, accepts + 1
            if best is not None:
                margin = min(margin, abs(e - best['inter']))
            if best is None or e < best['inter']:
                best = res
            history.append(best['inter'])
        return dict(best, accepts=accepts, n_steps=steps, n_evals=evals, first=first, margin=margin, history=history)


def dock_molecule(lpos, lel, lrole, ppos, pelem, prole, rsum, weights, draws, cutoff=8.0, max_steps=RR.MAX_STEPS, max_evals=None,
                  max_shift=RR.MAX_SHIFT, amplitude=AMPLITUDE, temperature=TEMPERATURE):
    """The search of one molecule with draws [C, R + 1, 7].  Returns a dict with td_score_dock's outputs for the molecule, ``chains`` (the
    dicts of Molecule.chain) and ``select_margin``, the gap in inter between the winner and the next chain."""
    draws = np.asarray(draws, np.float64)
    mol = Molecule(lpos, lel, lrole, ppos, pelem, prole, rsum, weights, cutoff, max_shift)
    chains = [mol.chain(c, draws[c], draws.shape[1] - 1, amplitude, temperature, max_steps, max_evals) for c in range(draws.shape[0])]
    e = np.asarray([RR.energy(ch['terms'], weights) for ch in chains])
    k = int(np.argmin(e))                                                        # the first of the lowest
    win, rest = chains[k], np.delete(e, k)
    return dict(pos=win['pos'], terms_in=chains[0]['first']['terms_in'], grad_in=chains[0]['first']['grad_in'], terms=win['terms'],
                n_pairs=win['n_pairs'], n_steps=sum(ch['n_steps'] for ch in chains), n_evals=sum(ch['n_evals'] for ch in chains),
                status=win['status'], transform=np.concatenate([win['q'], win['t']]), best_chain=k,
                chain_terms=np.stack([ch['terms'] for ch in chains]), chain_transform=np.stack([np.concatenate([ch['q'], ch['t']]) for ch in chains]),
                chain_accepts=np.asarray([ch['accepts'] for ch in chains], np.int32), chain_evals=np.asarray([ch['n_evals'] for ch in chains], np.int32),
                chains=chains, select_margin=float((rest - e[k]).min()) if len(rest) else np.inf)


def score_dock(pos, v, ptr, class_z, class_aromatic, ppos, pelem, pkind, prole, n_kinds, rsum, weights=SR.WEIGHTS, cutoff=8.0,
               hetero_cutoff=1.75, with_rotors=True, max_steps=RR.MAX_STEPS, max_evals=None, max_shift=RR.MAX_SHIFT, n_chains=N_CHAINS,
               n_rounds=N_ROUNDS, amplitude=AMPLITUDE, temperature=TEMPERATURE, draws=None):
    """numpy twin of capi.score_dock: pos [S, N, 3] fp32, v [S, N], ptr [B + 1], draws [S, B, C, R + 1, 7]; also ``margin`` and ``chain_pairs`` [S, B, C]"""
    pos, v, ptr, ppos, pelem = np.asarray(pos, np.float32), np.asarray(v), np.asarray(ptr), np.asarray(ppos, np.float32), np.asarray(pelem)
    S, B, C = pos.shape[0], len(ptr) - 1, int(n_chains)
    draws = np.asarray(draws, np.float64).reshape(S, B, C, int(n_rounds) + 1, DRAWS)
    pr = IR.protein_roles(ppos, pelem, pkind, prole, n_kinds, hetero_cutoff)
    out = dict(protein_role=pr, n_rot=np.zeros((S, B), np.int32) if with_rotors else None, pos=pos.copy(),
               terms_in=np.zeros((S, B, 5), np.int64), terms=np.zeros((S, B, 5), np.int64), n_pairs=np.zeros((S, B), np.int32),
               n_steps=np.zeros((S, B), np.int32), n_evals=np.zeros((S, B), np.int32), status=np.zeros((S, B), np.int32),
               transform=np.zeros((S, B, 7)), grad_in=np.zeros((S, B, 6), np.int64), best_chain=np.zeros((S, B), np.int32),
               chain_terms=np.zeros((S, B, C, 5), np.int64), chain_transform=np.zeros((S, B, C, 7)), chain_accepts=np.zeros((S, B, C), np.int32),
               chain_evals=np.zeros((S, B, C), np.int32), margin=np.full((S, B, C), np.inf), chain_pairs=np.zeros((S, B, C), np.int32))
    out['transform'][..., 0] = out['chain_transform'][..., 0] = 1.0
    for s in range(S):
        for g in range(B):
            a, b = int(ptr[g]), int(ptr[g + 1])
            if b - a > SR.MAX_ATOMS or (b > a and (a < 0 or b > pos.shape[1])):
                out['terms_in'][s, g] = out['terms'][s, g] = out['chain_terms'][s, g] = SR.INT64_MIN
                out['n_pairs'][s, g] = out['status'][s, g] = -1
                if with_rotors:
                    out['n_rot'][s, g] = -1
                continue
            lel, lrole, _ = RR.molecule_inputs(pos[s, a:b], v[s, a:b], class_z)
            r = dock_molecule(pos[s, a:b], lel, lrole, ppos, pelem, pr, rsum, weights, draws[s, g], cutoff, max_steps, max_evals, max_shift,
                              amplitude, temperature)
            out['pos'][s, a:b] = r['pos']
            for k in KEYS[3:]:
                out[k][s, g] = r[k]
            out['margin'][s, g] = [ch['margin'] for ch in r['chains']]
            out['chain_pairs'][s, g] = [ch['n_pairs'] for ch in r['chains']]
            if with_rotors:
                out['n_rot'][s, g] = SR.rotors(pos[s, a:b], v[s, a:b], class_z, class_aromatic)
    return out


def torch_score_dock(pos, v, ligand_ptr, class_z, class_aromatic, protein_pos, protein_elem, protein_kind, protein_role, n_kinds, rsum,
                     weights, cutoff=8.0, hetero_cutoff=1.75, bond_ptr=None, bond_ring=None, max_steps=RR.MAX_STEPS, max_evals=None,
                     max_shift=RR.MAX_SHIFT, n_chains=N_CHAINS, n_rounds=N_ROUNDS, amplitude=AMPLITUDE, temperature=TEMPERATURE, seed=0,
                     draws=None, check=True):
    """score_dock with capi.score_dock's signature on CPU tensors: what the host tests patch the binding with"""
    import torch
    from targetdiff_amd import capi
    S, _, B, _, aro, _ = capi._bond_inputs(pos, v, ligand_ptr, class_z, class_aromatic, None, (), check)
    capi._score_inputs(pos, protein_pos, protein_elem, protein_kind, protein_role, n_kinds, rsum, cutoff, hetero_cutoff, bond_ptr, bond_ring,
                       S, B, check)
    w, max_steps, max_evals, max_shift = capi._relax_inputs(weights, max_steps, max_evals, max_shift)
    n_chains, n_rounds, amplitude, temperature, draws = capi._dock_inputs(n_chains, n_rounds, amplitude, temperature, seed, draws, S, B,
                                                                          pos.device, check)
    r = score_dock(pos.cpu().numpy(), v.cpu().numpy(), ligand_ptr.cpu().numpy(), class_z, class_aromatic, protein_pos.cpu().numpy(),
                   protein_elem.cpu().numpy(), protein_kind.cpu().numpy(), protein_role.cpu().numpy(), int(n_kinds),
                   np.asarray(rsum, np.float64), w, float(cutoff), float(hetero_cutoff), bond_ptr is not None, max_steps, max_evals, max_shift,
                   n_chains, n_rounds, amplitude, temperature, draws.cpu().numpy())
    return {k: (None if r[k] is None else torch.from_numpy(np.asarray(r[k]))) for k in KEYS}
