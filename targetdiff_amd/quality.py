"""Sample quality on the GPU: the chemistry-free half of the reference's ``scripts/evaluate_diffusion.py`` (:75-87, :150-174).

    from targetdiff_amd import quality
    result = sample_diffusion_ligand(model, pocket, 100, ...)
    rep = quality.sample_quality(result)                      # the final poses, as evaluate_diffusion.py --eval_step -1
    curve = quality.sample_quality(result, eval_step='all')   # one row per frame of the trajectory, in one launch
    rep.summary()   # {'mol_stable': ..., 'atm_stable': ..., 'JSD_CC_2A': ..., 'JSD_All_12A': ..., 'atom_type_js': ...}

Three metrics, all arithmetic on positions and types (``td_quality_report``, csrc/quality.hip):

  * atom and molecule stability from a bond-length table (utils/evaluation/analyze.py ``check_stability``, hs=False);
  * the pair-distance profiles ``CC_2A`` and ``All_12A`` (utils/evaluation/eval_bond_length.py) and their Jensen-Shannon distances;
  * the atom-type Jensen-Shannon distance (utils/evaluation/eval_atom_type.py).

The kernel returns integers (bond counts, stable atoms, histogram counts, atoms per element); the fractions, the normalised
distributions and the Jensen-Shannon distances are float64 numpy on the host, formed in the reference's order.  The empirical
distributions the distances are taken against are data inside the reference's Python files and are not part of this package:
``reference_distributions()`` loads them when the reference is importable, a caller may pass arrays, and without either a report
carries the histograms and no distance.  Reconstruction, the bond-length profiles that need bonds, QED / SA and docking need a
chemistry toolkit and are not here.
"""
from __future__ import annotations

import numpy as np
import torch

from . import capi

ELEMENTS = capi.QUALITY_ELEMENTS                      # H C N O F P S Cl: the columns of the element counts
# atomic number per class index (utils/transforms.py MAP_INDEX_TO_ATOM_TYPE_ONLY / _AROMATIC; 13 = this project's NUM_LIGAND_CLASSES)
_CLASS_Z = {'basic': (1, 6, 7, 8, 9, 15, 16, 17),
            'add_aromatic': (1, 6, 6, 7, 7, 8, 8, 9, 15, 15, 16, 16, 17)}
PROFILE_NAMES = ('CC_2A', 'All_12A')
ATOM_TYPE_KEYS = (6, 7, 8, 9, 15, 16, 17)             # eval_atom_type.ATOM_TYPE_DISTRIBUTION's keys, in its order (no hydrogen)


def class_atomic_numbers(mode='add_aromatic'):
    """Atomic number of every ligand class: ``'basic'`` (8 classes), ``'add_aromatic'`` (13), or an explicit sequence."""
    if isinstance(mode, str):
        if mode not in _CLASS_Z:
            raise ValueError(f"atom_enc_mode {mode!r}: 'basic', 'add_aromatic' or an explicit sequence of atomic numbers")
        return _CLASS_Z[mode]
    z = tuple(int(x) for x in mode)
    bad = sorted(set(z) - set(ELEMENTS))
    if bad or not z:
        raise ValueError(f'atomic numbers {bad} are outside the bond-length table {ELEMENTS}')
    return z


def default_profiles():
    """The reference's two pair profiles as (z1, z2, cutoff, edges): C-C pairs below 2 A and all pairs below 12 A, 100 edges each."""
    return ((6, 6, 2.0, np.linspace(0, 2, 100)), (0, 0, 12.0, np.linspace(0, 12, 100)))


def jensenshannon(p, q):
    """scipy.spatial.distance.jensenshannon(p, q) (natural logarithm) in its order of operations: normalise both, m = (p + q) / 2,
    sum of rel_entr(p, m) plus sum of rel_entr(q, m), halve, square root.  float64 numpy on the host."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    p, q = p / np.sum(p, axis=0), q / np.sum(q, axis=0)
    m = (p + q) / 2.0

    def rel_entr(x, y):
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(x > 0, x * np.log(x / y), np.where(x == 0, 0.0, np.inf))

    js = np.sum(rel_entr(p, m), axis=0) + np.sum(rel_entr(q, m), axis=0)
    return np.sqrt(js / 2.0)


def reference_distributions():
    """{'CC_2A': [101], 'All_12A': [101], 'atom_type': [7]} from the reference's utils.evaluation when it is importable (inside that
    repository), else None.  The arrays are the reference's data; this package holds no copy."""
    try:
        from utils.evaluation import eval_atom_type, eval_bond_length_config as cfg
    except Exception:
        return None
    out = {k: np.asarray(cfg.PAIR_EMPIRICAL_DISTRIBUTIONS[k], dtype=np.float64) for k in PROFILE_NAMES}
    out['atom_type'] = np.asarray([eval_atom_type.ATOM_TYPE_DISTRIBUTION[z] for z in ATOM_TYPE_KEYS], dtype=np.float64)
    return out


def _fp32_positions(pos, device):
    """[S, N_l, 3] fp32 on ``device`` from one frame or a stack; float64 only when it is widened fp32 (the driver's results are)."""
    if not torch.is_tensor(pos):
        pos = torch.from_numpy(np.ascontiguousarray(pos))
    if pos.dtype == torch.float64:
        p32 = pos.to(torch.float32)
        if not torch.equal(p32.to(torch.float64), pos):
            raise ValueError('float64 positions must round-trip through fp32 exactly: the metric is defined on fp32 coordinates')
        pos = p32
    elif pos.dtype != torch.float32:
        raise ValueError(f'positions must be fp32 (or float64 holding fp32 values), got {pos.dtype}')
    if pos.dim() == 2:
        pos = pos[None]
    if pos.dim() != 3 or pos.shape[2] != 3:
        raise ValueError(f'positions must be [N_l, 3] or [S, N_l, 3] (got {tuple(pos.shape)})')
    return pos.to(device).contiguous()


def _pack(pos, v, batch_ligand, ligand_ptr, device):
    if device is None:
        device = pos.device if torch.is_tensor(pos) and pos.is_cuda else 'cuda'
    pos = _fp32_positions(pos, device)
    v = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).to(device=pos.device, dtype=torch.int64)
    if v.dim() == 1:
        v = v[None]
    v = v.contiguous()
    if (batch_ligand is None) == (ligand_ptr is None):
        raise ValueError('give batch_ligand or ligand_ptr, one of the two')
    if ligand_ptr is None:
        b = torch.as_tensor(batch_ligand).to('cpu', torch.int64)
        if tuple(b.shape) != (pos.shape[1],):
            raise ValueError(f'batch_ligand must be [{pos.shape[1]}] (got {tuple(b.shape)})')
        if b.numel() and (int(b.min()) < 0 or bool((b[1:] < b[:-1]).any())):
            raise ValueError('batch_ligand must be sorted and non-negative')
        B = int(b[-1]) + 1 if b.numel() else 0
        ligand_ptr = torch.zeros(B + 1, dtype=torch.int64)
        ligand_ptr[1:] = torch.cumsum(torch.bincount(b, minlength=B), 0)
    ligand_ptr = torch.as_tensor(ligand_ptr).to(device=pos.device, dtype=torch.int32).contiguous()
    return pos, v, ligand_ptr


def stability(pos, v, batch_ligand=None, ligand_ptr=None, atom_enc_mode='add_aromatic', return_nr_bonds=False, device=None):
    """check_stability of every molecule of one frame ``[N_l, 3]`` or of a stack ``[S, N_l, 3]`` (classes ``v`` alike; the molecules
    by a sorted ``batch_ligand`` [N_l] or by ``ligand_ptr`` [B + 1], shared by the frames).  Returns ``(mol_stable [S, B] bool,
    stable_atoms [S, B] int32)`` and, with ``return_nr_bonds``, ``nr_bonds [S, N_l] int32`` -- device tensors, the frame axis dropped
    for a single frame."""
    single = (pos.ndim if not torch.is_tensor(pos) else pos.dim()) == 2
    pos, v, ligand_ptr = _pack(pos, v, batch_ligand, ligand_ptr, device)
    r = capi.quality_report(pos, v, ligand_ptr, class_atomic_numbers(atom_enc_mode), (), None, return_nr_bonds)
    out = (r['mol_stable'].bool(), r['stable_atoms']) + ((r['nr_bonds'],) if return_nr_bonds else ())
    return tuple(t[0] for t in out) if single else out


def pair_profiles(pos, v, batch_ligand=None, ligand_ptr=None, atom_enc_mode='add_aromatic', profiles=None, include=None, device=None):
    """The raw integer pair-distance histograms ``[S, P, 128] int64`` (bin = numpy.searchsorted(edges, d); the bins past a profile's
    ``len(edges)`` stay 0) and the element counts ``[S, 8] int64`` over the molecules of ``include`` ([S, B] bool, default all);
    ``profiles``: a sequence of (z1, z2, cutoff, edges), default the reference's two."""
    pos, v, ligand_ptr = _pack(pos, v, batch_ligand, ligand_ptr, device)
    if include is not None:
        include = torch.as_tensor(include).to(device=pos.device, dtype=torch.bool).reshape(pos.shape[0], -1).contiguous()
    r = capi.quality_report(pos, v, ligand_ptr, class_atomic_numbers(atom_enc_mode), default_profiles() if profiles is None else profiles,
                            include, False)
    return r['hist'], r['counts']


class QualityReport:
    """Per frame (axis 0; one row for a single ``eval_step``): the integers of the kernel and what the reference forms from them.

    ``mol_stable`` / ``atm_stable`` [S]: stable molecules / number of samples and stable atoms / number of atoms, as
    evaluate_diffusion.py:150-151 forms them.  ``hist`` [S, P, 128] and ``counts`` [S, 8] cover the included molecules only."""

    def __init__(self, stable_mols, stable_atoms, n_samples, n_atoms, hist, counts, profiles, reference=None, names=None):
        self.stable_mols = np.asarray(stable_mols, dtype=np.int64)
        self.stable_atoms = np.asarray(stable_atoms, dtype=np.int64)
        self.n_samples, self.n_atoms = int(n_samples), int(n_atoms)
        self.hist, self.counts = np.asarray(hist, dtype=np.int64), np.asarray(counts, dtype=np.int64)
        self.profiles = tuple(profiles)
        self.names = tuple(names) if names is not None else (PROFILE_NAMES if len(self.profiles) == 2 else
                                                              tuple(f'profile{p}' for p in range(len(self.profiles))))
        self.reference = reference
        with np.errstate(divide='ignore', invalid='ignore'):
            self.mol_stable = self.stable_mols / float(self.n_samples) if self.n_samples else np.full(self.stable_mols.shape, np.nan)
            self.atm_stable = self.stable_atoms / float(self.n_atoms) if self.n_atoms else np.full(self.stable_atoms.shape, np.nan)

    @classmethod
    def merged(cls, reports):
        """The report of several pockets' samples together: every integer summed, frame by frame (the reference accumulates the
        same sums over its result files)."""
        reports = list(reports)
        first = reports[0]
        if any(r.hist.shape != first.hist.shape for r in reports):
            raise ValueError('reports of different frame counts or profiles do not merge')
        return cls(sum(r.stable_mols for r in reports), sum(r.stable_atoms for r in reports), sum(r.n_samples for r in reports),
                   sum(r.n_atoms for r in reports), sum(r.hist for r in reports), sum(r.counts for r in reports), first.profiles,
                   first.reference, first.names)

    @property
    def num_frames(self):
        return self.hist.shape[0]

    def distribution(self, name, frame=-1):
        """``counts / counts.sum()`` of a profile over its ``len(edges) + 1`` bins, or None when no pair entered."""
        p = self.names.index(name)
        h = self.hist[frame, p, :len(self.profiles[p][3]) + 1]
        return h / np.sum(h) if h.sum() > 0 else None

    def atom_type_distribution(self, frame=-1):
        """Frequencies of C N O F P S Cl over all counted atoms, hydrogen in the denominator (eval_atom_type.py:26-30)."""
        total = int(self.counts[frame].sum())
        if total == 0:
            return None
        return np.asarray([int(self.counts[frame, ELEMENTS.index(z)]) / total for z in ATOM_TYPE_KEYS])

    def js(self, frame=-1):
        """{'JSD_<profile>': ..., 'atom_type_js': ...} against the reference distributions; None where there is no reference
        distribution or nothing was counted."""
        out = {}
        ref = self.reference or {}
        for name in self.names:
            d = self.distribution(name, frame)
            out[f'JSD_{name}'] = float(jensenshannon(ref[name], d)) if d is not None and name in ref else None
        d = self.atom_type_distribution(frame)
        out['atom_type_js'] = float(jensenshannon(ref['atom_type'], d)) if d is not None and 'atom_type' in ref else None
        return out

    def summary(self, frame=-1):
        return dict(mol_stable=float(self.mol_stable[frame]), atm_stable=float(self.atm_stable[frame]), **self.js(frame))


def _trajectories(result):
    if isinstance(result, dict):
        return result['pred_ligand_pos_traj'], result['pred_ligand_v_traj']
    return result[2], result[3]


def sample_quality(result, eval_step=-1, include='all', atom_enc_mode='add_aromatic', reference=None, profiles=None, device='cuda'):
    """Quality of the samples of one pocket: ``result`` is the driver's 7-tuple (``sample_diffusion_ligand``) or a loaded
    ``result_{i}.pt`` dictionary.  ``eval_step``: a frame index as evaluate_diffusion.py's ``--eval_step`` (default -1, the final
    poses) or ``'all'`` for every frame of the trajectory (one row each: the curve along the chain).  The chosen frames of all samples
    go to the GPU as one pack -- samples along the molecule axis (they are of ragged size), frames along the frame axis -- and one launch.

    ``include``: which molecules enter the pair profiles and the element counts: ``'all'`` (default), ``'stable'`` (the molecules
    that are stable in that frame; stability runs first and its flags are the mask, two launches) or a bool array [frames, samples].
    The reference takes these two from reconstructed complete molecules only (evaluate_diffusion.py:136-137, "success_pair_dist"),
    which needs a chemistry toolkit and cannot be had here: with 'all' the numbers are those the reference would print if every
    sample reconstructed.  ``reference``: the empirical distributions ({'CC_2A', 'All_12A', 'atom_type'} arrays); default
    ``reference_distributions()``; without them the report has no Jensen-Shannon value.  Returns a ``QualityReport``."""
    pos_traj, v_traj = _trajectories(result)
    if len(pos_traj) != len(v_traj):
        raise ValueError('position and type trajectories of different length')
    if isinstance(eval_step, str):
        if eval_step != 'all':
            raise ValueError("eval_step is a frame index or 'all'")
        take = lambda a: np.asarray(a)
    else:
        take = lambda a: np.asarray(a)[int(eval_step)][None]
    pos = [take(p) for p in pos_traj]
    v = [take(x) for x in v_traj]
    sizes = [p.shape[1] for p in pos]
    S = pos[0].shape[0] if pos else 0
    if any(p.shape[0] != S for p in pos) or any(x.shape[:2] != p.shape[:2] for p, x in zip(pos, v)):
        raise ValueError('every sample needs the same number of frames, positions and types alike')
    ptr = torch.as_tensor(np.cumsum([0] + sizes), dtype=torch.int32)
    pos = np.concatenate(pos, axis=1) if pos else np.zeros((0, 0, 3), np.float32)
    v = np.concatenate(v, axis=1) if v else np.zeros((0, 0), np.int64)
    pos, v, ptr = _pack(pos, v, None, ptr, device)
    cz = class_atomic_numbers(atom_enc_mode)
    prof = default_profiles() if profiles is None else tuple(profiles)
    if isinstance(include, str):
        if include not in ('all', 'stable'):
            raise ValueError("include is 'all', 'stable' or a mask [frames, samples]")
        mask = None
    else:
        mask = torch.as_tensor(np.asarray(include)).to(device=pos.device, dtype=torch.bool).reshape(S, len(sizes)).contiguous()
    if isinstance(include, str) and include == 'stable':
        first = capi.quality_report(pos, v, ptr, cz, (), None, False)
        r = capi.quality_report(pos, v, ptr, cz, prof, first['mol_stable'].bool(), False, check=False)
        r['mol_stable'], r['stable_atoms'] = first['mol_stable'], first['stable_atoms']
    else:
        r = capi.quality_report(pos, v, ptr, cz, prof, mask, False)
    if reference is None:
        reference = reference_distributions()
    return QualityReport(r['mol_stable'].sum(1).cpu().numpy(), r['stable_atoms'].sum(1).cpu().numpy(), len(sizes), sum(sizes),
                         r['hist'].cpu().numpy(), r['counts'].cpu().numpy(), prof, reference)
