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
carries the histograms and no distance.

The bonds the table implies are kept too (``td_bond_graph`` / ``td_bond_list``, csrc/bonds.hip; DESIGN.md section 3, "Bond graph"):

    g = quality.bond_graph(pos, v, batch_ligand, return_fragments=True, return_bonds=True)    # bonds, fragments, rings per molecule
    con = quality.sample_connectivity(result, eval_step='all')    # complete fraction, fragments and bond-length profiles per frame
    rep = quality.sample_quality(result, include='complete')      # the reference's "success_*" restriction to one-piece molecules

and so are its rings (``td_ring_report``, csrc/rings.hip; DESIGN.md section 3, "Rings"): per bond the size of the smallest cycle
through it, per atom the smallest ring that holds it, per molecule the set of such sizes:

    g = quality.bond_graph(pos, v, batch_ligand, return_bonds=True, rings=True)    # g.bond_ring, g.atom_ring, g.ring_mask, ...
    rings = quality.sample_rings(result, eval_step='all')         # evaluate_diffusion.py's ring ratios (:26-32), per frame
    rings.ring_ratio(-1)    # {3: ..., 4: ..., ..., 9: ...}: the share of molecules that have a ring of that size

and fingerprints of that graph (``td_fingerprint`` / ``td_fingerprint_similarity``, csrc/fingerprint.hip; DESIGN.md section 3,
"Fingerprints and diversity"), for how different the samples of a pocket are from each other and how many are the same molecule twice:

    fp = quality.fingerprints(pos, v, batch_ligand)               # fp.fp_words [S, B, 32], fp.n_bits, fp.key
    div = quality.sample_diversity(result, reference_ligand=(ref_pos, ref_v))
    div.summary()   # {'diversity': ..., 'uniqueness': ..., 'mean_nearest': ..., 'ref_sim_mean': ..., 'ref_sim_median': ..., 'ref_sim_max': ...}

This is not RDKit's RDKFingerprint, which the reference's utils/evaluation/similarity.py uses: RDKit's is path-based with its own
invariants.  This one is a circular, Morgan-style fingerprint over this project's bond graph, whose orders come from the bond-length
table.  Its similarities are comparable between runs of this tool, not with published tables.

And the shape the bonds make (``td_geometry_report``, csrc/geometry.hip; DESIGN.md section 3, "Local geometry"): bond angles and
unsigned torsion angles binned per type, and internal clashes -- pairs more than 3 bonds apart that are closer than 0.7 times the sum
of their van der Waals radii, this project's own convention (not PoseBusters' bound, not a force field):

    geo = quality.sample_geometry(result, eval_step='all', reference=quality.geometry_reference(molfile.read_sdf('ligands.sdf')))
    geo.summary()   # {'clash_free': ..., 'mean_clashes': ..., 'CCC': {'count': ..., 'mean': ..., 'js': ...}, ...}

And where the poses sit in their pocket (``td_pocket_report``, csrc/pocket.hip; DESIGN.md section 3, "Pocket contacts"): contacts (a
ligand atom and a protein atom closer than 4 A), clashes with the protein (closer than the sum of the van der Waals radii minus 0.5 A)
and, with the pocket's known ligand, how many of its contacts a sample recovers -- conventions of this project, not a pose checker's:

    poc = quality.sample_pocket(result, eval_step='all', reference_ligand=(ref_pos, ref_v))    # result['data'] is the pocket
    poc.summary()   # {'pocket_clash_free': ..., 'mean_contacts': ..., 'buried_share': ..., 'no_contact': ..., 'ref_recovery_mean': ...}
    poc.contact_profile(), poc.contact_frequency()    # contacts by residue kind ('ASP.sc', 'GLY.bb', ...), and per protein atom

And what kind of contacts they are (``td_interaction_report``, csrc/interactions.hip; DESIGN.md section 3, "Pocket interactions"):
hydrogen bonds (a donor and an acceptor closer than 3.5 A, heavy atom to heavy atom, no angle) and hydrophobic contacts (closer than
4.5 A), counted, never scored.  The ligand's donors are inferred from the valence deficit the bond rule leaves -- a heuristic of this
project, not perceived chemistry:

    ia = quality.sample_interactions(result, eval_step='all', reference_ligand=(ref_pos, ref_v))
    ia.summary()   # {'mean_hbonds': ..., 'mean_donated': ..., 'mean_accepted': ..., 'mean_hydrophobic': ..., 'no_hbond': ..., ...}
    ia.kind_profile('donated'), ia.interaction_frequency()    # hydrogen bonds by residue kind, and per type and protein atom

And a docking-style score of the poses (``td_score_report``, csrc/score.hip; DESIGN.md section 3, "Docking-style score"): the five
Vina-style terms (two Gaussians, repulsion, hydrophobic, hydrogen bond) summed over the ligand - pocket heavy-atom pairs within 8 A,
weighted on the host and divided by 1 + 0.0585 rotatable bonds.  It runs on this project's heuristic typing -- no hydrogens are placed,
the roles come from valence deficits, there is no intramolecular term -- so it is NOT AutoDock Vina's number: comparable between runs
of this tool, not with published tables:

    sc = quality.sample_score(result, eval_step='all', reference_ligand=(ref_pos, ref_v))
    sc.summary()   # {'mean_score': ..., 'median_score': ..., 'best_score': ..., 'share_negative': ..., 'better_than_ref': ..., ...}

And how much of a pose's surface the pocket covers (``td_sasa_report``, csrc/sasa.hip; DESIGN.md section 3, "Solvent-accessible
surface"): Shrake-Rupley point counts of the ligand alone and in the pocket, areas formed on the host from Bondi-type radii plus a
1.4 A probe -- comparable between runs of this tool, not with published tables; of the pocket, a cut-out, only the buried area:

    sa = quality.sample_sasa(result, eval_step='all', reference_ligand=(ref_pos, ref_v))
    sa.summary()   # {'sasa_free': ..., 'sasa_bound': ..., 'sasa_buried': ..., 'sasa_buried_share': ..., 'pocket_buried_area': ..., ...}

Several reports of one result share its pack, its host checks and its bond graph (``SamplePack``; the ``sample_*`` functions build one each):

    pack = quality.SamplePack(result, eval_step='all')
    rep, con, rings = pack.quality('complete'), pack.connectivity('complete'), pack.rings('complete')    # one upload, one plain bond graph
    side = quality.PocketSide(result['data'])                       # the pocket decoded once and uploaded once
    poc, ia, sa, sc = pack.pocket(side), pack.interactions(side), pack.sasa(side), pack.score(side)

OpenBabel's reconstruction, valence repair, QED / SA and AutoDock Vina's own docking need a chemistry toolkit and are not here.
"""
from __future__ import annotations

import numpy as np
import torch

from . import capi

ELEMENTS = capi.QUALITY_ELEMENTS                      # H C N O F P S Cl: the columns of the element counts
# atomic number per class index (utils/transforms.py MAP_INDEX_TO_ATOM_TYPE_ONLY / _AROMATIC; 13 = this project's NUM_LIGAND_CLASSES)
_CLASS_Z = {'basic': (1, 6, 7, 8, 9, 15, 16, 17),
            'add_aromatic': (1, 6, 6, 7, 7, 8, 8, 9, 15, 15, 16, 16, 17)}
# aromatic classes (utils/transforms.py is_aromatic_from_index: the second of each (element, aromatic) pair of 'add_aromatic')
_CLASS_AROMATIC = {'basic': (False,) * 8, 'add_aromatic': tuple(c in (2, 4, 6, 9, 11) for c in range(13))}
PROFILE_NAMES = ('CC_2A', 'All_12A')
# eval_bond_length_config.BOND_TYPES, (z1 <= z2, category): C-C, C-N single / double / aromatic, C-O single / double
BOND_TYPES = ((6, 6, 1), (6, 6, 2), (6, 6, 4), (6, 7, 1), (6, 7, 2), (6, 7, 4), (6, 8, 1), (6, 8, 2))
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


def class_aromatic(mode='add_aromatic'):
    """One flag per ligand class: is it aromatic (utils/transforms.py ``is_aromatic_from_index``)?  ``'add_aromatic'``: classes 2, 4,
    6, 9 and 11; ``'basic'`` and an explicit sequence of atomic numbers: none."""
    if isinstance(mode, str):
        if mode not in _CLASS_AROMATIC:
            raise ValueError(f"atom_enc_mode {mode!r}: 'basic', 'add_aromatic' or an explicit sequence of atomic numbers")
        return _CLASS_AROMATIC[mode]
    return (False,) * len(class_atomic_numbers(mode))


def default_bond_profiles():
    """The reference's eight bond types as (z1, z2, category, edges), each over eval_bond_length_config.DISTANCE_BINS (formed here
    the way the reference forms them); there is no cutoff: the last bin takes every longer bond."""
    edges = np.arange(1.1, 1.7, 0.005)[:-1]
    return tuple((z1, z2, c, edges) for z1, z2, c in BOND_TYPES)


def bond_type_name(bond_type):
    """'6-6|4' for (6, 6, 4): eval_bond_length._bond_type_str"""
    return f'{bond_type[0]}-{bond_type[1]}|{bond_type[2]}'


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


def reference_bond_distributions():
    """{(z1, z2, category): [len(DISTANCE_BINS) + 1]} from the reference's eval_bond_length_config.EMPIRICAL_DISTRIBUTIONS when it is
    importable, else None.  The arrays are the reference's data; this package holds no copy."""
    try:
        from utils.evaluation import eval_bond_length_config as cfg
    except Exception:
        return None
    return {tuple(int(x) for x in k): np.asarray(d, dtype=np.float64) for k, d in cfg.EMPIRICAL_DISTRIBUTIONS.items()}


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


def _frame_mask(include, pos):
    """``include`` [S, B] as a bool mask on the device of ``pos`` [S, N_l, 3], or None for every molecule"""
    if include is None:
        return None
    return torch.as_tensor(include).to(device=pos.device, dtype=torch.bool).reshape(pos.shape[0], -1).contiguous()


def _reference_pack(reference_ligand, device):
    """``(pos [n, 3], v [n])`` of a known ligand as a pack of one frame of one molecule on ``device``"""
    rpos, rv = reference_ligand
    rpos, rv, rptr = _pack(rpos, rv, None, torch.tensor([0, len(rv)], dtype=torch.int32), device)
    if rpos.shape[0] != 1:
        raise ValueError('the reference ligand is one molecule: pos [n, 3], v [n]')
    return rpos, rv, rptr


def _radii(table, radii):
    """a copy of ``table`` ({atomic number: radius in Angstrom}) with the entries of ``radii`` in their place"""
    r = dict(table)
    for z, x in (radii or {}).items():
        if int(z) not in r or not float(x) >= 0.0:
            raise ValueError(f'radii are non-negative and keyed by the atomic numbers {tuple(sorted(r))} (got {z}: {x})')
        r[int(z)] = float(x)
    return r


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
    include = _frame_mask(include, pos)
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


class SamplePack:
    """The chosen frames of all samples of a result as one pack on ``device`` -- samples along the molecule axis (they are of ragged
    size), frames along the frame axis -- and what the reports of one result share: ``pos`` [S, N_l, 3], ``v`` [S, N_l], ``ligand_ptr``
    [B + 1], the ``sizes``, ``S``, the class table ``class_z`` and the ``aromatic`` flags of ``atom_enc_mode``.  ``result`` and
    ``eval_step`` as ``sample_quality``.  The pack is made and uploaded once; the host's look at it (the bindings' ``check``) runs
    once; the stability flags, the plain bond graph (the 'complete' flags and ``bond_ptr``) and ``bond_ring`` are computed when a
    report first needs them and kept.  The reports are its methods, so none can be taken with another frame, encoding or device."""

    def __init__(self, result, eval_step=-1, atom_enc_mode='add_aromatic', device='cuda'):
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
        self.pos, self.v, self.ligand_ptr = _pack(pos, v, None, ptr, device)
        self.sizes, self.S = sizes, S
        self.class_z, self.aromatic = class_atomic_numbers(atom_enc_mode), class_aromatic(atom_enc_mode)
        self._checked = self._sized = False
        self._stable = self._graph = self._bond_ring = self._ref = self.relaxed_pos = self.docked_pos = None

    @property
    def _args(self):
        return self.pos, self.v, self.ligand_ptr, self.class_z

    def _check(self, sized=True):
        """``check`` of the next binding call: the first call on the pack looks at it on the host, later ones do not.  The look of
        the bond graph's family (``sized``) also bounds the molecule sizes, which quality_report's does not: it runs once more when
        quality_report came first."""
        todo = not (self._sized if sized else self._checked)
        self._checked, self._sized = True, self._sized or sized
        return todo

    @property
    def stable(self):
        """[S, B] bool: the molecules that are stable in that frame, from one quality_report without profiles"""
        if self._stable is None:
            self._stable = capi.quality_report(*self._args, (), None, False, check=self._check(False))['mol_stable'].bool()
        return self._stable

    @property
    def graph(self):
        """the plain bond graph (no profiles, every molecule): ``n_fragments`` -- one fragment: 'complete' -- and ``bond_ptr``"""
        if self._graph is None:
            self._graph = capi.bond_graph(*self._args, self.aromatic, (), None, False, True, check=self._check())
        return self._graph

    @property
    def bond_ring(self):
        """[n_bonds] int16 in the order of ``graph['bond_ptr']``: the smallest ring through every bond, 0 for a bridge"""
        if self._bond_ring is None:
            bond_ptr = self.graph['bond_ptr']
            self._bond_ring = capi.ring_report(*self._args, self.aromatic, None, bond_ptr, False, check=self._check())['bond_ring']
        return self._bond_ring

    def mask(self, include, allowed=('all', 'complete')):
        """``include`` as a device mask [S, B] bool, or None for every molecule: ``'all'``, ``'stable'``, ``'complete'`` -- those of
        them that ``allowed`` names -- or a bool array [frames, samples]"""
        if isinstance(include, str):
            if include not in allowed:
                raise ValueError('include is ' + ', '.join(repr(a) for a in allowed) + ' or a mask [frames, samples]')
            if include == 'all':
                return None
            return self.stable if include == 'stable' else self.graph['n_fragments'] == 1
        return torch.as_tensor(np.asarray(include)).to(device=self.pos.device, dtype=torch.bool).reshape(self.S, len(self.sizes)).contiguous()

    def quality(self, include='all', reference=None, profiles=None):
        """``sample_quality`` of the pack"""
        prof = default_profiles() if profiles is None else tuple(profiles)
        mask = self.mask(include, ('all', 'stable', 'complete'))
        r = capi.quality_report(*self._args, prof, mask, False, check=self._check(False))    # stability does not depend on the mask
        if reference is None:
            reference = reference_distributions()
        return QualityReport(r['mol_stable'].sum(1).cpu().numpy(), r['stable_atoms'].sum(1).cpu().numpy(), len(self.sizes), sum(self.sizes),
                             r['hist'].cpu().numpy(), r['counts'].cpu().numpy(), prof, reference)

    def connectivity(self, include='all', reference=None, bond_profiles=None):
        """``sample_connectivity`` of the pack"""
        prof = default_bond_profiles() if bond_profiles is None else tuple(bond_profiles)
        mask = self.mask(include)
        r = capi.bond_graph(*self._args, self.aromatic, prof, mask, check=self._check())
        nf, big = r['n_fragments'].cpu().numpy().astype(np.int64), r['largest_fragment'].cpu().numpy().astype(np.float64)
        n = np.asarray(self.sizes, dtype=np.float64)
        share = np.divide(big, n[None], out=np.zeros_like(big), where=n[None] > 0)
        if reference is None:
            reference = reference_bond_distributions()
        return ConnectivityReport((nf == 1).sum(1), nf.sum(1), share.sum(1), len(self.sizes), int((n > 0).sum()), r['bond_hist'].cpu().numpy(),
                                  prof, reference)

    def _included(self, mask):
        return np.ones((self.S, len(self.sizes)), bool) if mask is None else mask.cpu().numpy().astype(bool)

    def rings(self, include='all'):
        """``sample_rings`` of the pack"""
        mask = self.mask(include)
        r = capi.ring_report(*self._args, self.aromatic, mask, None, False, check=self._check())
        inc = self._included(mask)
        n = np.asarray(self.sizes, dtype=np.float64)
        ring_atoms = r['n_ring_atoms'].cpu().numpy().astype(np.float64)
        share = np.divide(ring_atoms, n[None], out=np.zeros_like(ring_atoms), where=n[None] > 0)
        large = (r['ring_mask'].cpu().numpy() >> (RING_SIZES[-1] + 1)) != 0
        return RingReport(r['ring_hist'].cpu().numpy(), inc.sum(1), (large & inc).sum(1), np.where(inc, share, 0.0).sum(1),
                          (inc & (n[None] > 0)).sum(1), len(self.sizes))

    def diversity(self, include='all', radius=2, key_rounds=8, reference_ligand=None):
        """``sample_diversity`` of the pack"""
        mask = self.mask(include)
        fp = capi.fingerprint(*self._args, self.aromatic, radius, key_rounds, False, check=self._check())
        qw = qb = None
        if reference_ligand is not None:
            q = capi.fingerprint(*self._reference(reference_ligand), self.aromatic, radius, key_rounds, False)
            qw, qb = q['fp_words'][0].contiguous(), q['n_bits'][0].contiguous()
        r = capi.fingerprint_similarity(fp['fp_words'], fp['n_bits'], fp['key'], mask, qw, qb, False)
        inc = fp['n_bits'].cpu().numpy() >= 0
        if mask is not None:
            inc &= mask.cpu().numpy().astype(bool)
        first = r['first_equal'].cpu().numpy()
        distinct = (first == np.arange(len(self.sizes))[None]) & inc
        return DiversityReport.from_frames(inc.sum(1), np.where(inc, r['sim_sum'].cpu().numpy(), 0.0).sum(1), distinct.sum(1),
                                           np.where(inc, r['sim_max'].cpu().numpy(), 0.0).sum(1), len(self.sizes),
                                           None if qw is None else r['query_sim'][:, :, 0].cpu().numpy(), inc)

    def geometry(self, include='all', reference=None, profiles=None, clash_scale=0.7, radii=None):
        """``sample_geometry`` of the pack"""
        prof = default_geometry_profiles() if profiles is None else tuple(profiles)
        mask = self.mask(include)
        r = _geometry_call(*self._args, self.aromatic, prof, mask, clash_thresholds(clash_scale, radii), False, pack=self)
        inc = self._included(mask)
        clashes = r['n_clashes'].cpu().numpy().astype(np.int64)
        tot = lambda k: np.where(inc, r[k].cpu().numpy().astype(np.int64), 0).sum(1)
        return GeometryReport(inc.sum(1), (inc & (clashes == 0)).sum(1), np.where(inc, clashes, 0).sum(1), tot('n_crowded'), tot('n_degenerate'),
                              tot('n_angles'), tot('n_torsions'), r['hist'].cpu().numpy(), prof, len(self.sizes), reference)

    def _reference(self, reference_ligand):
        """the known ligand as the leading arguments of a binding call, packed once for the reports that share it.  Kept by the
        identity of the ``reference_ligand`` object: arrays changed in place between two reports are not packed again -- pass a new
        tuple for another ligand"""
        if self._ref is None or self._ref[0] is not reference_ligand:
            self._ref = (reference_ligand, _reference_pack(reference_ligand, self.pos.device) + (self.class_z,))
        return self._ref[1]

    def _side(self, data):
        return data if isinstance(data, PocketSide) else PocketSide(data, self.pos.device)

    def pocket(self, data, include='all', reference_ligand=None, contact_cutoff=4.0, clash_tolerance=0.5, kinds='residue'):
        """``sample_pocket`` of the pack; ``data``: the pocket every molecule of the pack is in (``pocket_of``), or its ``PocketSide``"""
        side = self._side(data)
        kind, names = side.kinds(kinds)
        mask = self.mask(include)
        pocket = (side.pos, side.elem, kind, len(names), contact_cutoff)
        ref_bits = ref_size = None
        if reference_ligand is not None:
            q = capi.pocket_report(*self._reference(reference_ligand), *pocket, None, None, None, False, True)
            ref_bits, ref_size = q['bits'][0, 0].contiguous(), int(q['n_pocket_atoms'][0, 0])
        r = capi.pocket_report(*self._args, *pocket, pocket_clash_thresholds(clash_tolerance), mask, ref_bits, False, False,
                               check=self._check())
        keys = ('n_contacts', 'n_contact_atoms', 'n_pocket_atoms', 'n_clashes', 'min_dist', 'n_ref_common', 'kind_hist', 'pocket_freq')
        raw = {k: r[k].cpu().numpy() for k in keys if r[k] is not None}
        return PocketReport.from_outputs(raw, self._included(mask), self.sizes, names, [n.endswith('.bb') for n in names] if kinds == 'residue'
                                         else None, ref_size)

    def interactions(self, data, include='all', reference_ligand=None, hbond_cutoff=3.5, hydrophobic_cutoff=4.5, hetero_cutoff=1.75):
        """``sample_interactions`` of the pack; ``data`` as ``pocket``"""
        side = self._side(data)
        kind, names = side.kinds()
        mask = self.mask(include)
        pocket = (side.pos, side.elem, kind, side.roles(), len(names), hbond_cutoff, hydrophobic_cutoff, hetero_cutoff)
        ref_bits = ref_sizes = None
        if reference_ligand is not None:
            q = capi.interaction_report(*self._reference(reference_ligand), *pocket, None, None, False, True)
            ref_bits = q['bits'][0, 0].contiguous()
            ref_sizes = _popcount(ref_bits.cpu().numpy())
        r = capi.interaction_report(*self._args, *pocket, mask, ref_bits, True, ref_bits is not None, check=self._check())
        keys = ('n_donated', 'n_accepted', 'n_hbonds', 'n_hydrophobic', 'n_hb_atoms', 'atom_role', 'n_ref_common', 'bits', 'kind_hist',
                'pocket_freq')
        raw = {k: r[k].cpu().numpy() for k in keys if r[k] is not None}
        return InteractionReport.from_outputs(raw, self._included(mask), self.sizes, names, ref_sizes)

    def _pose_setup(self, data, include, weights, rot_weight, cutoff, max_steps=None, max_shift=None):
        """What ``score``, ``relax`` and ``dock`` share, said once: the conventions for what is None, ``include`` as a mask and the
        pocket.  Returns (weights, rot_weight, mask, the pocket's arguments of the three bindings up to the radius sums, (cutoff, hetero
        cutoff), the optimiser's budget as keywords)."""
        weights = SCORE_WEIGHTS if weights is None else weights
        rot_weight = SCORE_ROT_WEIGHT if rot_weight is None else rot_weight
        side = self._side(data)
        kind, names = side.kinds()
        mask = self.mask(include)
        pocket = (side.pos, side.elem, kind, side.roles(), len(names), score_radius_sums())
        cutoffs = (SCORE_CUTOFF if cutoff is None else cutoff, DEFAULT_HETERO_CUTOFF)
        budget = dict(max_steps=RELAX_MAX_STEPS if max_steps is None else max_steps, max_shift=RELAX_MAX_SHIFT if max_shift is None else max_shift)
        return weights, rot_weight, mask, pocket, cutoffs, budget

    @property
    def _rotors(self):
        """the rotor inputs of the pack: ``bond_ptr`` of its plain bond graph and ``bond_ring``"""
        return self.graph['bond_ptr'], self.bond_ring

    def _reference_rotors(self, reference_ligand):
        """(the known ligand as ``_reference`` packs it, its rotor inputs): its own bond graph and ring sizes"""
        ref = self._reference(reference_ligand)
        bond_ptr = capi.bond_graph(*ref, self.aromatic, (), None, False, True)['bond_ptr']
        return ref, (bond_ptr, capi.ring_report(*ref, self.aromatic, None, bond_ptr, False)['bond_ring'])

    def score(self, data, include='all', reference_ligand=None, weights=None, rot_weight=None, cutoff=None):
        """``sample_score`` of the pack; ``data`` as ``pocket``.  The rotatable bonds are counted on the pack's bond graph and ring sizes."""
        weights, rot_weight, mask, pocket, cutoffs, _ = self._pose_setup(data, include, weights, rot_weight, cutoff)
        ref_score = None
        if reference_ligand is not None:
            ref, rotors = self._reference_rotors(reference_ligand)
            q = capi.score_report(*ref, self.aromatic, *pocket, *cutoffs, *rotors)
            if int(q['n_pairs'][0, 0]) >= 0:
                ref_score = float(score_energies(q['terms'].cpu().numpy(), q['n_rot'].cpu().numpy(), weights, rot_weight)[2][0, 0])
        r = capi.score_report(*self._args, self.aromatic, *pocket, *cutoffs, *self._rotors, check=self._check())
        heavy = _heavy_atoms(self.v.cpu().numpy(), self.class_z, self.sizes)
        return ScoreReport.from_outputs(_numpy(r, ('terms', 'n_pairs', 'n_rot')), self._included(mask), heavy, weights, rot_weight, ref_score)

    def relax(self, data, include='all', reference_ligand=None, weights=None, max_steps=None, max_shift=None, cutoff=None, rot_weight=None):
        """``sample_relax`` of the pack; ``data`` as ``pocket``.  The rotatable bonds are those of the input poses, counted on the pack's
        bond graph and ring sizes; the relaxed coordinates of the last call stay in ``relaxed_pos`` [S, N_l, 3] on the device."""
        weights, rot_weight, mask, pocket, cutoffs, budget = self._pose_setup(data, include, weights, rot_weight, cutoff, max_steps, max_shift)
        ref_scores = None
        if reference_ligand is not None:
            ref, rotors = self._reference_rotors(reference_ligand)
            q = capi.score_minimize(*ref, self.aromatic, *pocket, weights, *cutoffs, *rotors, **budget)
            if int(q['status'][0, 0]) >= 0:
                _, before, after, _ = _relax_scores(_numpy(q, _SCORES_RAW), weights, rot_weight)
                ref_scores = (float(before[0, 0]), float(after[0, 0]))
        r = capi.score_minimize(*self._args, self.aromatic, *pocket, weights, *cutoffs, *self._rotors, **budget, check=self._check())
        self.relaxed_pos = r['pos']
        raw = _numpy(r, ('pos', 'n_steps', 'n_evals') + _SCORES_RAW)
        return RelaxReport.from_outputs(raw, self._included(mask), self.pos.cpu().numpy(), self.sizes, weights, rot_weight, ref_scores)

    def dock(self, data, include='all', reference_ligand=None, weights=None, n_chains=None, n_rounds=None, seed=0, max_steps=None,
             max_shift=None, cutoff=None, rot_weight=None):
        """``sample_dock`` of the pack, which must hold a single frame (ValueError otherwise: one launch would hold S B n_chains
        long-lived workgroups); ``data`` as ``pocket``.  The relaxation alone runs beside the search, for the score it is compared with;
        the docked coordinates of the last call stay in ``docked_pos`` [1, N_l, 3] on the device.  The known ligand's draws are seeded
        by ``seed`` too."""
        _single_frame(None, self.S)
        weights, rot_weight, mask, pocket, cutoffs, budget = self._pose_setup(data, include, weights, rot_weight, cutoff, max_steps, max_shift)
        search = dict(budget, n_chains=DOCK_CHAINS if n_chains is None else n_chains, n_rounds=DOCK_ROUNDS if n_rounds is None else n_rounds, seed=seed)
        ref_score = None
        if reference_ligand is not None:
            ref, rotors = self._reference_rotors(reference_ligand)
            q = capi.score_dock(*ref, self.aromatic, *pocket, weights, *cutoffs, *rotors, **search)
            if int(q['status'][0, 0]) >= 0:
                ref_score = float(_relax_scores(_numpy(q, _SCORES_RAW), weights, rot_weight)[2][0, 0])
        rotors = self._rotors
        r_min = capi.score_minimize(*self._args, self.aromatic, *pocket, weights, *cutoffs, *rotors, **budget, check=self._check())
        r = capi.score_dock(*self._args, self.aromatic, *pocket, weights, *cutoffs, *rotors, **search, check=self._check())
        self.docked_pos = r['pos']
        return DockReport.from_outputs(_numpy(r, _DOCK_RAW), _numpy(r_min, _SCORES_RAW), self._included(mask), self.pos.cpu().numpy(), self.sizes,
                                       weights, rot_weight, ref_score)

    def sasa(self, data, include='all', reference_ligand=None, probe=1.4, points=96):
        """``sample_sasa`` of the pack; ``data`` as ``pocket``"""
        side = self._side(data)
        mask = self.mask(include)
        lr, pr = sasa_reaches(probe)
        dirs = torch.from_numpy(sasa_directions(points)).to(self.pos.device)
        pocket = (side.pos, side.kinds('element')[0], lr, pr, dirs)
        ref = None
        if reference_ligand is not None:
            q = capi.sasa_report(*self._reference(reference_ligand), *pocket, None, False, True)
            ref = {k: q[k][0, 0].cpu().numpy() for k in ('free', 'bound', 'pocket_buried', 'bits')}
        self._check()
        # the pack's host look runs with every call: the kernel's cull is proved for the coordinates that look admits
        r = capi.sasa_report(*self._args, *pocket, mask, False, ref is not None, check=True)
        raw = {k: r[k].cpu().numpy() for k in ('free', 'bound', 'pocket_buried', 'bits', 'pocket_buried_sum') if r[k] is not None}
        return SasaReport.from_outputs(raw, self._included(mask), lr, pr, points, float(probe), ref)


def sample_quality(result, eval_step=-1, include='all', atom_enc_mode='add_aromatic', reference=None, profiles=None, device='cuda'):
    """Quality of the samples of one pocket: ``result`` is the driver's 7-tuple (``sample_diffusion_ligand``) or a loaded
    ``result_{i}.pt`` dictionary.  ``eval_step``: a frame index as evaluate_diffusion.py's ``--eval_step`` (default -1, the final
    poses) or ``'all'`` for every frame of the trajectory (one row each: the curve along the chain).  The chosen frames of all samples
    go to the GPU as one pack -- samples along the molecule axis (they are of ragged size), frames along the frame axis -- and one launch.

    ``include``: which molecules enter the pair profiles and the element counts: ``'all'`` (default), ``'stable'`` (the molecules
    that are stable in that frame; stability runs first and its flags are the mask, two launches), ``'complete'`` (the molecules
    whose bond graph is one fragment in that frame; the bond graph runs first) or a bool array [frames, samples].
    The reference takes these two from reconstructed complete molecules only (evaluate_diffusion.py:136-137, "success_pair_dist"):
    'complete' is that restriction with this project's bond graph in the place of OpenBabel's reconstruction; with 'all' the
    numbers are those the reference would print if every sample reconstructed.  ``reference``: the empirical distributions ({'CC_2A', 'All_12A', 'atom_type'} arrays); default
    ``reference_distributions()``; without them the report has no Jensen-Shannon value.  Returns a ``QualityReport``."""
    return SamplePack(result, eval_step, atom_enc_mode, device).quality(include, reference, profiles)


class BondGraph:
    """The bond graph of S frames of B molecules (``bond_graph``).  Device tensors, frame axis first: ``n_bonds``, ``n_fragments``,
    ``largest_fragment``, ``rings`` [S, B] int32 (rings = n_bonds - n_atoms + n_fragments, the cyclomatic number), ``complete``
    [S, B] bool (one fragment), ``bond_hist`` [S, P, 128] int64 over the included molecules, ``ligand_ptr`` [B + 1]; optional:
    ``fragment`` [S, N_l] int32 (per atom, the smallest molecule-local index of its component) and the bond list in ascending
    (frame, molecule, i, j) order: ``bond_ptr`` [S * B + 1] int64, ``bond_atoms`` [nb, 2] int32 (indices along the atom axis),
    ``bond_order`` / ``bond_category`` [nb] uint8, ``bond_length`` [nb] float64.  With ``rings=True``: ``ring_mask`` [S, B] int64
    (bit min(k, 31): some bond's smallest ring has k atoms), ``n_ring_bonds`` / ``n_ring_atoms`` [S, B] int32, ``atom_ring`` [S, N_l]
    int32 (the smallest ring that holds the atom, 0: none) and, beside the bond list, ``bond_ring`` [nb] int16 (atoms of the smallest
    cycle through the bond, 0: a bridge) and ``ring_category`` [nb] uint8 (the category, 4 only inside a ring of 5 or 6)."""

    def __init__(self, r, ligand_ptr, profiles, bonds=None, rings=None):
        self.n_bonds, self.n_fragments, self.largest_fragment = r['n_bonds'], r['n_fragments'], r['largest_fragment']
        self.bond_hist, self.fragment, self.bond_ptr = r['bond_hist'], r['fragment'], r['bond_ptr']
        self.ligand_ptr, self.profiles = ligand_ptr, tuple(profiles)
        self.n_atoms = ligand_ptr[1:] - ligand_ptr[:-1]
        self.complete = self.n_fragments == 1
        self.rings = self.n_bonds - self.n_atoms[None] + self.n_fragments
        bonds = bonds or {}
        self.bond_atoms, self.bond_order = bonds.get('bond_atoms'), bonds.get('bond_order')
        self.bond_category, self.bond_length = bonds.get('bond_category'), bonds.get('bond_length')
        rings = rings or {}
        self.ring_mask, self.n_ring_bonds, self.n_ring_atoms = rings.get('ring_mask'), rings.get('n_ring_bonds'), rings.get('n_ring_atoms')
        self.atom_ring, self.bond_ring, self.ring_category = rings.get('atom_ring'), rings.get('bond_ring'), rings.get('bond_category')

    def molecule_bonds(self, frame, molecule):
        """(atoms [k, 2] molecule-local, order [k], category [k], length [k]) of one molecule of one frame, as numpy; of a graph with
        rings also (ring size [k], ring-aware category [k])"""
        if self.bond_atoms is None:
            raise ValueError('the bond list was not asked for (return_bonds=True)')
        B = self.n_bonds.shape[1]
        frame = frame % self.n_bonds.shape[0]
        a, b = (int(x) for x in self.bond_ptr[frame * B + molecule:frame * B + molecule + 2])
        l0 = int(self.ligand_ptr[molecule])
        out = (self.bond_atoms[a:b].cpu().numpy() - l0, self.bond_order[a:b].cpu().numpy(), self.bond_category[a:b].cpu().numpy(),
               self.bond_length[a:b].cpu().numpy())
        if self.bond_ring is not None:
            out += (self.bond_ring[a:b].cpu().numpy(), self.ring_category[a:b].cpu().numpy())
        return out


def bond_graph(pos, v, batch_ligand=None, ligand_ptr=None, atom_enc_mode='add_aromatic', bond_profiles=None, include=None,
               return_fragments=False, return_bonds=False, rings=False, device=None):
    """The bond graph of every molecule of one frame ``[N_l, 3]`` or of a stack ``[S, N_l, 3]`` (arguments as ``stability``): a pair
    is bonded when the bond-length table gives it an order > 0; fragments are the connected components.  ``bond_profiles``: a sequence
    of (z1, z2, category, edges), default the reference's eight bond types; ``include`` [S, B] restricts ``bond_hist`` and nothing
    else.  ``rings``: also the ring sizes (one more launch, ``td_ring_report``), per bond when ``return_bonds`` is given too.
    Molecules of more than 512 atoms are refused.  Returns a ``BondGraph`` (the frame axis is kept for a single frame)."""
    pos, v, ligand_ptr = _pack(pos, v, batch_ligand, ligand_ptr, device)
    include = _frame_mask(include, pos)
    prof = default_bond_profiles() if bond_profiles is None else tuple(bond_profiles)
    cz, aro = class_atomic_numbers(atom_enc_mode), class_aromatic(atom_enc_mode)
    r = capi.bond_graph(pos, v, ligand_ptr, cz, aro, prof, include, return_fragments, return_bonds)
    bonds = capi.bond_list(pos, v, ligand_ptr, cz, aro, r['bond_ptr'], check=False) if return_bonds else None
    ring = capi.ring_report(pos, v, ligand_ptr, cz, aro, None, r['bond_ptr'], check=False) if rings else None
    return BondGraph(r, ligand_ptr, prof, bonds, ring)


class ConnectivityReport:
    """Per frame (axis 0): how many samples are one piece, and the bond-length profiles of the included molecules.

    ``complete`` [S] = complete molecules / samples (evaluate_diffusion.py:154), ``mean_fragments`` [S], ``mean_largest_share`` [S]
    (atoms of the largest fragment / atoms, averaged over the non-empty samples); ``bond_hist`` [S, P, 128] int64."""

    def __init__(self, n_complete, sum_fragments, sum_share, n_samples, n_nonempty, bond_hist, profiles, reference=None):
        self.n_complete, self.sum_fragments = np.asarray(n_complete, dtype=np.int64), np.asarray(sum_fragments, dtype=np.int64)
        self.sum_share = np.asarray(sum_share, dtype=np.float64)
        self.n_samples, self.n_nonempty = int(n_samples), int(n_nonempty)
        self.bond_hist, self.profiles, self.reference = np.asarray(bond_hist, dtype=np.int64), tuple(profiles), reference
        self.bond_types = tuple((int(z1), int(z2), int(c)) for z1, z2, c, _ in self.profiles)
        nan = np.full(self.n_complete.shape, np.nan)
        self.complete = self.n_complete / float(self.n_samples) if self.n_samples else nan
        self.mean_fragments = self.sum_fragments / float(self.n_samples) if self.n_samples else nan
        self.mean_largest_share = self.sum_share / float(self.n_nonempty) if self.n_nonempty else nan

    @classmethod
    def merged(cls, reports):
        reports = list(reports)
        first = reports[0]
        if any(r.bond_hist.shape != first.bond_hist.shape for r in reports):
            raise ValueError('reports of different frame counts or profiles do not merge')
        return cls(sum(r.n_complete for r in reports), sum(r.sum_fragments for r in reports), sum(r.sum_share for r in reports),
                   sum(r.n_samples for r in reports), sum(r.n_nonempty for r in reports), sum(r.bond_hist for r in reports),
                   first.profiles, first.reference)

    @property
    def num_frames(self):
        return self.bond_hist.shape[0]

    def distribution(self, bond_type, frame=-1):
        """``counts / counts.sum()`` of a bond type over its ``len(edges) + 1`` bins (eval_bond_length.get_distribution), or None
        when no such bond was seen (the reference's profile has no such key then)."""
        p = self.bond_types.index(tuple(bond_type))
        h = self.bond_hist[frame, p, :len(self.profiles[p][3]) + 1]
        return h / np.sum(h) if h.sum() > 0 else None

    def js(self, frame=-1):
        """{'JSD_6-6|1': ...} over the profiles, as eval_bond_length.eval_bond_length_profile names them: None where there is no
        reference distribution or no bond of that type."""
        ref = self.reference or {}
        out = {}
        for t in self.bond_types:
            d = self.distribution(t, frame)
            out['JSD_' + bond_type_name(t)] = float(jensenshannon(ref[t], d)) if d is not None and t in ref else None
        return out

    def summary(self, frame=-1):
        return dict(complete=float(self.complete[frame]), mean_fragments=float(self.mean_fragments[frame]),
                    mean_largest_share=float(self.mean_largest_share[frame]), **self.js(frame))


def sample_connectivity(result, eval_step=-1, include='all', atom_enc_mode='add_aromatic', reference=None, bond_profiles=None,
                        device='cuda'):
    """Connectivity of the samples of one pocket (``result``, ``eval_step`` and the packing as ``sample_quality``): per frame the
    complete fraction, the mean number of fragments, the mean share of atoms in the largest fragment and the bond-length
    distributions with their Jensen-Shannon distances.  ``include``: which molecules enter the bond-length histograms: ``'all'``
    (default), ``'complete'`` (two launches: the first call's flags are the mask) or a bool array [frames, samples].  ``reference``:
    {(z1, z2, category): distribution}; default ``reference_bond_distributions()``.  Returns a ``ConnectivityReport``."""
    return SamplePack(result, eval_step, atom_enc_mode, device).connectivity(include, reference, bond_profiles)


_i64, _f64 = (lambda a: np.asarray(a, dtype=np.int64)), (lambda a: np.asarray(a, dtype=np.float64))
# the kinds of a report's fields as (how a constructor argument is taken, how ``merged`` combines it): summed over the reports; carried
# from the first; a per-pocket map, kept only for a single report; a sum that exists only with a reference ligand; a per-molecule array
# [S, B, ...], joined along the molecule axis
_FIELD_KINDS = {'per_mol': (np.asarray, 'mol'), 'i64': (_i64, 'sum'), 'f64': (_f64, 'sum'), 'int_sum': (int, 'sum'), 'int_carried': (int, 'carried'), 'tuple': (tuple, 'carried'),
                'value': (lambda x: x, 'carried'), 'flags': (lambda a: np.asarray(a, dtype=bool), 'carried'), 'map': (_i64, 'map'),
                'ref_i64': (_i64, 'ref'), 'ref_f64': (_f64, 'ref')}


class _SumReport:
    """What the per-frame reports that are sums over molecules share.  A class names its ``FIELDS`` once, (name, kind) in the order of
    its constructor's arguments (``_FIELD_KINDS``; the last ``OPTIONAL`` of them default to None and stay None), what must agree for
    two reports to merge (``_merge_key``) and the ``MISMATCH`` message.  From that: the converting constructor, ``merged``,
    ``num_frames``, ``_mean`` and the ``key:\tvalue`` lines of the summary."""
    FIELDS, OPTIONAL, MISMATCH = (), 0, ''

    def __init__(self, *args, **kw):
        names = [name for name, _ in self.FIELDS]
        if len(args) > len(names) or not set(kw) <= set(names[len(args):]):
            raise TypeError(f'{type(self).__name__}({", ".join(names)})')
        given = dict(zip(names, args), **kw)
        missing = [name for name in names[:len(names) - self.OPTIONAL] if name not in given]
        if missing:
            raise TypeError(f'{type(self).__name__}() needs {", ".join(missing)}')
        for name, kind in self.FIELDS:
            x = given.get(name)
            setattr(self, name, None if x is None else _FIELD_KINDS[kind][0](x))

    @classmethod
    def merged(cls, reports):
        """Several pockets together: every sum added, frame by frame; the reference values become means over the pockets that have
        one (the reference's tables average a per-pocket number).  A per-pocket map belongs to one pocket: the merged report of several
        has none."""
        reports = list(reports)
        first = reports[0]
        if any(r._merge_key() != first._merge_key() for r in reports):
            raise ValueError(cls.MISMATCH)
        tot = lambda name: sum(getattr(r, name) for r in reports)
        how = {'sum': tot, 'carried': lambda name: getattr(first, name), 'map': lambda name: getattr(first, name) if len(reports) == 1 else None,
               'ref': lambda name: None if first.sum_ref is None else tot(name),
               'mol': lambda name: np.concatenate([getattr(r, name) for r in reports], axis=1)}
        return cls(*(how[_FIELD_KINDS[kind][1]](name) for name, kind in cls.FIELDS))

    @property
    def num_frames(self):
        return getattr(self, self.FIELDS[0][0]).shape[0]

    @staticmethod
    def _mean(total, count):
        return float(total) / int(count) if int(count) else float('nan')

    def lines(self, frame=-1):
        """the summary as printed lines"""
        return [f'{k}:\t{x:.4f}' if x == x else f'{k}:\tNone' for k, x in self.summary(frame).items()]


RING_SIZES = tuple(range(3, 10))                      # evaluate_diffusion.py print_ring_ratio: range(3, 10)


class RingReport(_SumReport):
    """Per frame (axis 0): which ring sizes the included molecules have.  ``ring_hist`` [S, 32] int64: entry k > 0 counts the
    included molecules in which some bond's smallest ring has k atoms (31: 31 or more), entry 0 those without any ring; ``n_included``
    [S]; ``n_large`` [S] the included molecules with a ring of more than 9 atoms; ``sum_atom_share`` [S] the sum over the included
    non-empty molecules (``n_nonempty`` [S]) of atoms in rings / atoms.  A ring here is the smallest cycle through some bond: not a
    smallest set of smallest rings ("Rings")."""

    FIELDS = (('ring_hist', 'i64'), ('n_included', 'i64'), ('n_large', 'i64'), ('sum_atom_share', 'f64'), ('n_nonempty', 'i64'), ('n_samples', 'int_sum'))
    MISMATCH = 'reports of different frame counts do not merge'

    def _merge_key(self):
        return self.ring_hist.shape

    def _share(self, count, frame):
        n = int(self.n_included[frame])
        return int(count) / n if n else float('nan')

    def ring_ratio(self, frame=-1):
        """{3: ..., ..., 9: ...}: molecules with a ring of that size / included molecules (print_ring_ratio's n_mol / len)"""
        return {k: self._share(self.ring_hist[frame, k], frame) for k in RING_SIZES}

    def no_ring(self, frame=-1):
        return self._share(self.ring_hist[frame, 0], frame)

    def large_ring(self, frame=-1):
        return self._share(self.n_large[frame], frame)

    def ring_atom_share(self, frame=-1):
        n = int(self.n_nonempty[frame])
        return float(self.sum_atom_share[frame]) / n if n else float('nan')

    def summary(self, frame=-1):
        return dict(**{f'ring_{k}': x for k, x in self.ring_ratio(frame).items()}, no_ring=self.no_ring(frame),
                    large_ring=self.large_ring(frame), ring_atom_share=self.ring_atom_share(frame))


def sample_rings(result, eval_step=-1, include='all', atom_enc_mode='add_aromatic', device='cuda'):
    """Rings of the samples of one pocket (``result``, ``eval_step`` and the packing as ``sample_quality``): per frame the share of
    molecules that have a ring of 3 .. 9 atoms as the reference's print_ring_ratio forms it, the share without any ring, the share
    with a ring of more than 9 atoms and the mean share of atoms in rings.  ``include``: the molecules that are counted: ``'all'``
    (default), ``'complete'`` (one fragment in that frame; the bond graph runs first and its flags are the mask) or a bool array
    [frames, samples].  Returns a ``RingReport``."""
    return SamplePack(result, eval_step, atom_enc_mode, device).rings(include)


class Fingerprints:
    """The fingerprints of S frames of B molecules (``fingerprints``).  Device tensors, frame axis first: ``fp_words`` [S, B, 32] int64
    (word w, bit k: fingerprint bit 64 w + k of 2048), ``n_bits`` [S, B] int32 (the set bits), ``key`` [S, B] int64 (equal for molecules
    that colour refinement does not tell apart), ``atom_key`` [S, N_l] int64 or None (an atom's id after the key's rounds: atoms of one
    molecule with equal values are topologically alike; 0 for an atom of no class), ``ligand_ptr`` [B + 1]."""

    def __init__(self, r, ligand_ptr, radius, key_rounds):
        self.fp_words, self.n_bits, self.key, self.atom_key = r['fp_words'], r['n_bits'], r['key'], r['atom_key']
        self.ligand_ptr, self.radius, self.key_rounds = ligand_ptr, int(radius), int(key_rounds)

    def similarity(self, include=None, query=None, return_common=False):
        """capi.fingerprint_similarity of these fingerprints: ``include`` [S, B] bool or None; ``query``: a one-frame ``Fingerprints``
        whose molecules are the query set (the pocket's known ligand, a training set).  Returns its dict of device tensors."""
        if include is not None:
            include = torch.as_tensor(include).to(device=self.n_bits.device, dtype=torch.bool).reshape(self.n_bits.shape).contiguous()
        qw = qb = None
        if query is not None:
            if query.fp_words.shape[0] != 1 or (query.radius, query.key_rounds) != (self.radius, self.key_rounds):
                raise ValueError('the query set is one frame of fingerprints made with the same radius and key_rounds')
            qw, qb = query.fp_words[0].contiguous(), query.n_bits[0].contiguous()
        return capi.fingerprint_similarity(self.fp_words, self.n_bits, self.key, include, qw, qb, return_common)


def fingerprints(pos, v, batch_ligand=None, ligand_ptr=None, atom_enc_mode='add_aromatic', radius=2, key_rounds=8, return_atom_keys=False,
                 device=None):
    """The fingerprint and the key of every molecule of one frame ``[N_l, 3]`` or of a stack ``[S, N_l, 3]`` (arguments as
    ``bond_graph``), on exactly the bonds of ``bond_graph``.  Per atom an id from (atomic number, aromatic class, degree, valence),
    refined ``radius`` times (0 .. 4) with the ids of the bonded atoms and the bonds' categories; every id of every round sets one of
    2048 bits.  ``key``: a hash of the multiset of ids after ``key_rounds`` rounds (``radius`` .. 16): equal keys mean that
    Weisfeiler-Lehman colour refinement with these invariants does not tell the molecules apart -- not a canonical form: the skeletons
    of decalin and bicyclopentyl get equal keys.  This is not RDKit's RDKFingerprint: it is a circular, Morgan-style fingerprint over
    this project's bond graph, whose orders come from the bond-length table; its similarities are comparable between runs of this tool,
    not with published tables.  Molecules of more than 512 atoms are refused.  Returns a ``Fingerprints`` (the frame axis is kept)."""
    pos, v, ligand_ptr = _pack(pos, v, batch_ligand, ligand_ptr, device)
    r = capi.fingerprint(pos, v, ligand_ptr, class_atomic_numbers(atom_enc_mode), class_aromatic(atom_enc_mode), radius, key_rounds,
                         return_atom_keys)
    return Fingerprints(r, ligand_ptr, radius, key_rounds)


class DiversityReport(_SumReport):
    """Per frame (axis 0): how different the included samples of a pocket are from each other, as sums over pockets.

    Of one pocket with m included molecules: ``diversity`` = 1 - (sum of sim_sum) / (m (m - 1)), one minus the mean Tanimoto similarity
    over the ordered pairs (nan for m < 2); ``uniqueness`` = distinct keys / m (nan for m = 0); ``mean_nearest`` = the mean of sim_max,
    the similarity to the most similar other sample (nan for m < 2); with a reference ligand ``ref_sim_mean`` / ``ref_sim_median`` /
    ``ref_sim_max`` of the similarity to it (nan for m = 0).  A merged report gives the mean over the pockets that have a value: the
    convention of the reference's tables, which average a per-pocket number.  Kept for that: ``sum_diversity`` and ``n_diversity``
    (pockets with m >= 2), ``sum_nearest``, ``sum_uniqueness`` and ``n_unique`` (pockets with m >= 1), ``sum_ref`` [S, 3] and
    ``n_ref``; beside them the plain totals ``n_included``, ``n_distinct`` [S] and ``n_samples``.  The fingerprint is this project's
    own (``fingerprints``), not RDKit's: the values compare between runs of this tool, not with published tables."""

    FIELDS = (('sum_diversity', 'f64'), ('n_diversity', 'i64'), ('sum_nearest', 'f64'), ('sum_uniqueness', 'f64'), ('n_unique', 'i64'),
              ('n_included', 'i64'), ('n_distinct', 'i64'), ('n_samples', 'int_sum'), ('sum_ref', 'ref_f64'), ('n_ref', 'ref_i64'))
    OPTIONAL, MISMATCH = 2, 'reports of different frame counts, or with and without a reference ligand, do not merge'

    def _merge_key(self):
        return self.sum_diversity.shape, self.sum_ref is None

    @classmethod
    def from_frames(cls, n_included, sum_sim, n_distinct, sum_max, n_samples, ref_sim=None, included=None):
        """One pocket: ``n_included`` (m), the sums of sim_sum and sim_max over the included molecules and the number of distinct
        keys, each [S]; ``ref_sim`` [S, B] with ``included`` [S, B]: the similarity of every molecule to the reference ligand."""
        m = np.asarray(n_included, dtype=np.int64)
        mf = m.astype(np.float64)
        two, one = m >= 2, m >= 1
        safe = lambda den: np.where(den > 0, den, 1.0)
        diversity = np.where(two, 1.0 - np.asarray(sum_sim, dtype=np.float64) / safe(mf * (mf - 1.0)), 0.0)
        nearest = np.where(two, np.asarray(sum_max, dtype=np.float64) / safe(mf), 0.0)
        unique = np.where(one, np.asarray(n_distinct, dtype=np.float64) / safe(mf), 0.0)
        sum_ref = n_ref = None
        if ref_sim is not None:
            ref_sim, included = np.asarray(ref_sim, dtype=np.float64), np.asarray(included, dtype=bool)
            sum_ref = np.zeros((len(m), 3))
            for s in range(len(m)):
                x = ref_sim[s][included[s]]
                if x.size:
                    sum_ref[s] = (x.sum() / x.size, np.median(x), x.max())
            n_ref = one.astype(np.int64)
        return cls(diversity, two.astype(np.int64), nearest, unique, one.astype(np.int64), m, n_distinct, n_samples, sum_ref, n_ref)

    def diversity(self, frame=-1):
        return self._mean(self.sum_diversity[frame], self.n_diversity[frame])

    def mean_nearest(self, frame=-1):
        return self._mean(self.sum_nearest[frame], self.n_diversity[frame])

    def uniqueness(self, frame=-1):
        return self._mean(self.sum_uniqueness[frame], self.n_unique[frame])

    def reference_similarity(self, frame=-1):
        """{'ref_sim_mean', 'ref_sim_median', 'ref_sim_max'} or {} without a reference ligand"""
        if self.sum_ref is None:
            return {}
        return {k: self._mean(self.sum_ref[frame, c], self.n_ref[frame]) for c, k in enumerate(('ref_sim_mean', 'ref_sim_median', 'ref_sim_max'))}

    def summary(self, frame=-1):
        return dict(diversity=self.diversity(frame), uniqueness=self.uniqueness(frame), mean_nearest=self.mean_nearest(frame),
                    **self.reference_similarity(frame))


def sample_diversity(result, eval_step=-1, include='all', radius=2, key_rounds=8, reference_ligand=None, atom_enc_mode='add_aromatic',
                     device='cuda'):
    """Diversity of the samples of one pocket (``result``, ``eval_step`` and the packing as ``sample_quality``): per frame one minus the
    mean pairwise Tanimoto similarity of the samples' fingerprints, the share of distinct keys (uniqueness) and the mean similarity to
    the nearest other sample.  ``include``: the molecules that are compared, as ``sample_rings``: ``'all'`` (default), ``'complete'``
    (one fragment in that frame; the bond graph runs first and its flags are the mask) or a bool array [frames, samples].
    ``reference_ligand``: ``(pos [n, 3], v [n])`` of a known ligand, fingerprinted through the same kernel: the report then also holds
    the mean, median and largest similarity of the included samples to it (the reference's tanimoto_sim_N_to_1).  ``radius`` and
    ``key_rounds`` as ``fingerprints``.  Two launches (three with ``'complete'``).  The fingerprint is this project's own, not RDKit's:
    the numbers compare between runs of this tool, not with published tables.  Returns a ``DiversityReport``."""
    return SamplePack(result, eval_step, atom_enc_mode, device).diversity(include, radius, key_rounds, reference_ligand)


# ---- local geometry (``td_geometry_report``, csrc/geometry.hip; DESIGN.md section 3, "Local geometry")
# van der Waals radii in Angstrom (Bondi's, the usual table) of H C N O F P S Cl: an internal clash is a pair more than 3 bonds apart
# that is closer than clash_scale * (r_i + r_j).  This project's own convention: not PoseBusters' distance-geometry bound, not a force field.
GEOMETRY_RADII = {1: 1.2, 6: 1.7, 7: 1.55, 8: 1.52, 9: 1.47, 15: 1.8, 16: 1.8, 17: 1.75}
ANGLE_TYPES = ((6, 6, 6), (6, 6, 7), (6, 6, 8), (6, 7, 6), (6, 8, 6), (7, 6, 7))
TORSION_TYPES = (((6, 6, 6, 6), 'chain'), ((6, 6, 6, 6), 'ring'), ((6, 6, 6, 7), 'any'), ((6, 6, 6, 8), 'any'), ((6, 6, 7, 6), 'any'),
                 ((6, 6, 8, 6), 'chain'))
_SYMBOL = {0: '*', 1: 'H', 6: 'C', 7: 'N', 8: 'O', 9: 'F', 15: 'P', 16: 'S', 17: 'Cl'}
_RING_CODE = {None: 'any', 0: 'any', 1: 'chain', 2: 'ring', 'any': 'any', 'chain': 'chain', 'ring': 'ring'}


def default_geometry_profiles():
    """The default angle and torsion types as (kind, elements, category, ring, edges in degrees): the angles C-C-C, C-C-N, C-C-O,
    C-N-C, C-O-C and N-C-N (the centre in the middle) in 2 degree bins over 0 .. 180 (edges 2, 4, ..., 178), and the torsions C-C-C-C
    with the central bond outside a ring and inside one, C-C-C-N, C-C-C-O, C-C-N-C and C-C-O-C outside a ring, in 5 degree bins."""
    a, t = np.arange(2.0, 180.0, 2.0), np.arange(5.0, 180.0, 5.0)
    return tuple(('angle', z, 0, 'any', a) for z in ANGLE_TYPES) + tuple(('torsion', z, 0, ring, t) for z, ring in TORSION_TYPES)


def geometry_profile_name(profile):
    """'CCN' for the angle (6, 6, 7), 'CCCC|ring' for a torsion inside a ring, 'CCNC|2' with a category, '*' for any element"""
    _, z, category, ring, _ = profile
    name = ''.join(_SYMBOL[int(x)] for x in z)
    if int(category):
        name += f'|{int(category)}'
    return name if _RING_CODE[ring] == 'any' else f'{name}|{_RING_CODE[ring]}'


def clash_thresholds(clash_scale=0.7, radii=None):
    """[8, 8] float64 over H C N O F P S Cl: ``clash_scale * (r_i + r_j)``; ``radii``: {atomic number: radius in Angstrom} over
    ``GEOMETRY_RADII`` (missing elements keep the default), or None"""
    r = _radii(GEOMETRY_RADII, radii)
    rr = np.asarray([r[z] for z in ELEMENTS], dtype=np.float64)
    if not float(clash_scale) >= 0.0:
        raise ValueError(f'clash_scale is non-negative (got {clash_scale})')
    return np.float64(clash_scale) * (rr[:, None] + rr[None, :])


def _cosine_profiles(profiles):
    """Profiles with ascending edges in degrees (0 .. 180) as the binding's profiles with ascending cosine edges: numpy.cos of the
    edges in float64, once, reversed.  The kernel's bin k of m edges is bin m - k by ascending angle."""
    out = []
    for kind, z, category, ring, edges in profiles:
        e = np.asarray(edges, dtype=np.float64).reshape(-1)
        if e.size == 0 or not np.isfinite(e).all() or bool((e[1:] <= e[:-1]).any()) or e[0] < 0.0 or e[-1] > 180.0:
            raise ValueError('the edges of a geometry profile are degrees in 0 .. 180, strictly ascending')
        out.append((kind, tuple(int(x) for x in z), int(category), _RING_CODE[ring], np.cos(np.radians(e))[::-1].copy()))
    return out


def _geometry_call(pos, v, ptr, cz, aro, profiles, mask, thr, return_atom_clash, check=True, pack=None):
    """capi.geometry_report under profiles in degrees, the histograms flipped back to ascending angle; when a profile filters on the
    ring it takes ``bond_ptr`` and ``bond_ring`` from ``pack`` (a ``SamplePack`` of these arrays), and without one the bond graph and
    the ring report run first"""
    cosp = _cosine_profiles(profiles)
    bond_ptr = bond_ring = None
    ring = any(p[3] != 'any' for p in cosp)
    if pack is not None:
        if ring:
            bond_ptr, bond_ring = pack.graph['bond_ptr'], pack.bond_ring
        check = pack._check()
    elif ring:
        bond_ptr = capi.bond_graph(pos, v, ptr, cz, aro, (), None, False, True, check=check)['bond_ptr']
        bond_ring = capi.ring_report(pos, v, ptr, cz, aro, None, bond_ptr, False, check=False)['bond_ring']
        check = False
    r = capi.geometry_report(pos, v, ptr, cz, aro, cosp, mask, thr, bond_ptr, bond_ring, return_atom_clash, check=check)
    hist = torch.zeros_like(r['hist'])
    for p, prof in enumerate(cosp):
        m = len(prof[4])
        hist[:, p, :m + 1] = r['hist'][:, p, :m + 1].flip(-1)
    r['hist'] = hist
    return r


class Geometry:
    """The local geometry of S frames of B molecules (``geometry``).  Device tensors, frame axis first: ``n_angles``, ``n_torsions``
    (the non-degenerate ones, whatever the profiles), ``n_degenerate`` (angles and torsions whose cosine is 0 / 0), ``n_crowded`` (atoms
    of more than 8 bonds: the centre of no angle, the end of no central bond), ``n_clashes`` [S, B] int32, ``clash_free`` [S, B] bool,
    ``atom_clash`` [S, N_l] int32 (the clashes an atom takes part in), ``hist`` [S, P, 128] int64 over the included molecules, by
    ascending angle: bin b of a profile with edges e holds e[b - 1] <= angle < e[b]; ``profiles``, ``names``, ``ligand_ptr``."""

    def __init__(self, r, ligand_ptr, profiles):
        self.n_angles, self.n_torsions, self.n_degenerate, self.n_crowded = r['n_angles'], r['n_torsions'], r['n_degenerate'], r['n_crowded']
        self.n_clashes, self.atom_clash, self.hist = r['n_clashes'], r['atom_clash'], r['hist']
        self.clash_free = self.n_clashes == 0
        self.ligand_ptr, self.profiles = ligand_ptr, tuple(profiles)
        self.names = tuple(geometry_profile_name(p) for p in self.profiles)


def geometry(pos, v, batch_ligand=None, ligand_ptr=None, atom_enc_mode='add_aromatic', profiles=None, include=None, clash_scale=0.7,
             radii=None, device=None):
    """Bond angles, torsions and internal clashes of every molecule of one frame ``[N_l, 3]`` or of a stack ``[S, N_l, 3]`` (arguments
    as ``bond_graph``), on exactly the bonds of ``bond_graph``.

    Angle (i, j, k): j the centre, i < k bonded to it.  Torsion (i, j, k, l): the central bond j < k, i on j, l on k, all four
    different; the unsigned angle 0 .. 180 degrees, so mirror images histogram alike.  An atom of more than 8 bonds (a collapsed cloud)
    is the centre of no angle and the end of no central bond.  The kernel bins by the cosine in float64; no acos runs on the device.
    ``profiles``: a sequence of (kind, elements, category, ring, edges): 'angle' with 3 atomic numbers (the centre in the middle, the
    ends in either order) or 'torsion' with 4 (as given or reversed), 0 for any element; the central bond's category 1 .. 4 or 0 for
    any, and ring 'any', 'chain' (the central bond is in no ring) or 'ring' -- both for torsions only; ascending edges in **degrees**.
    Default ``default_geometry_profiles()``.  The edges become cosines once, by numpy.cos in float64, and the histogram comes back by
    ascending angle: bin b holds edges[b - 1] <= angle < edges[b], and an angle whose cosine equals numpy.cos(numpy.radians(edge))
    exactly lands in the bin that starts at that edge.  A ring filter costs two more launches (``td_bond_graph``, ``td_ring_report``).
    ``include`` [S, B] restricts ``hist`` and nothing else.

    Internal clash: a pair of atoms of one molecule more than 3 bonds apart (other fragments included) that is closer than
    ``clash_scale * (r_i + r_j)``, with the van der Waals radii H 1.2, C 1.7, N 1.55, O 1.52, F 1.47, P 1.8, S 1.8, Cl 1.75 A
    (``radii``: {atomic number: radius} to change some).  This is this project's own convention: it is not PoseBusters'
    distance-geometry bound and not a force field.  Molecules of more than 512 atoms are refused.  Returns a ``Geometry``."""
    pos, v, ligand_ptr = _pack(pos, v, batch_ligand, ligand_ptr, device)
    include = _frame_mask(include, pos)
    prof = default_geometry_profiles() if profiles is None else tuple(profiles)
    r = _geometry_call(pos, v, ligand_ptr, class_atomic_numbers(atom_enc_mode), class_aromatic(atom_enc_mode), prof, include,
                       clash_thresholds(clash_scale, radii), True)
    return Geometry(r, ligand_ptr, prof)


class GeometryReport:
    """Per frame (axis 0), over the included molecules (``n_included`` [S] of ``n_samples``): ``n_clash_free`` and ``sum_clashes``
    [S], ``n_crowded``, ``n_degenerate``, ``n_angles``, ``n_torsions`` [S], and ``hist`` [S, P, 128] int64 by ascending angle under
    ``profiles`` (edges in degrees; ``names``).  ``reference``: {name: counts or a distribution over the profile's bins}, as
    ``geometry_reference`` makes it, or None.  The clash rule and the radii are this project's own convention (``geometry``)."""

    def __init__(self, n_included, n_clash_free, sum_clashes, n_crowded, n_degenerate, n_angles, n_torsions, hist, profiles, n_samples,
                 reference=None):
        i64 = lambda a: np.asarray(a, dtype=np.int64)
        self.n_included, self.n_clash_free, self.sum_clashes = i64(n_included), i64(n_clash_free), i64(sum_clashes)
        self.n_crowded, self.n_degenerate, self.n_angles, self.n_torsions = i64(n_crowded), i64(n_degenerate), i64(n_angles), i64(n_torsions)
        self.hist, self.profiles, self.n_samples, self.reference = i64(hist), tuple(profiles), int(n_samples), reference
        self.names = tuple(geometry_profile_name(p) for p in self.profiles)

    @classmethod
    def merged(cls, reports):
        """Several pockets together: every integer summed, frame by frame"""
        reports = list(reports)
        first = reports[0]
        if any(r.hist.shape != first.hist.shape or r.names != first.names for r in reports):
            raise ValueError('reports of different frame counts or profiles do not merge')
        tot = lambda name: sum(getattr(r, name) for r in reports)
        return cls(tot('n_included'), tot('n_clash_free'), tot('sum_clashes'), tot('n_crowded'), tot('n_degenerate'), tot('n_angles'),
                   tot('n_torsions'), tot('hist'), first.profiles, tot('n_samples'), first.reference)

    @property
    def num_frames(self):
        return self.hist.shape[0]

    def _per_molecule(self, count, frame):
        n = int(self.n_included[frame])
        return int(count) / n if n else float('nan')

    def clash_free(self, frame=-1):
        """included molecules without an internal clash / included molecules"""
        return self._per_molecule(self.n_clash_free[frame], frame)

    def mean_clashes(self, frame=-1):
        return self._per_molecule(self.sum_clashes[frame], frame)

    def counts(self, name, frame=-1):
        """the counts of a profile over its ``len(edges) + 1`` bins"""
        p = self.names.index(name)
        return self.hist[frame, p, :len(self.profiles[p][4]) + 1]

    def count(self, name, frame=-1):
        return int(self.counts(name, frame).sum())

    def distribution(self, name, frame=-1):
        h = self.counts(name, frame)
        return h / np.sum(h) if h.sum() > 0 else None

    def bin_centres(self, name):
        """the middle of every bin in degrees, the outer bins running to 0 and to 180"""
        e = np.asarray(self.profiles[self.names.index(name)][4], dtype=np.float64)
        e = np.concatenate([[0.0], e, [180.0]])
        return (e[:-1] + e[1:]) / 2.0

    def mean_angle(self, name, frame=-1):
        """the mean angle in degrees from the bin centres, nan when nothing was counted"""
        h = self.counts(name, frame)
        return float(np.sum(h * self.bin_centres(name)) / h.sum()) if h.sum() > 0 else float('nan')

    def js(self, frame=-1):
        """{'JSD_<name>': ...}: the Jensen-Shannon distance of every profile to the reference's; None where there is no reference
        distribution or nothing was counted"""
        ref = self.reference or {}
        out = {}
        for name in self.names:
            d = self.distribution(name, frame)
            q = ref.get(name)
            ok = d is not None and q is not None and len(q) == len(d) and np.sum(q) > 0
            out['JSD_' + name] = float(jensenshannon(np.asarray(q, dtype=np.float64), d)) if ok else None
        return out

    def summary(self, frame=-1):
        out = dict(clash_free=self.clash_free(frame), mean_clashes=self.mean_clashes(frame), crowded_atoms=int(self.n_crowded[frame]),
                   degenerate=int(self.n_degenerate[frame]), angles=int(self.n_angles[frame]), torsions=int(self.n_torsions[frame]))
        js = self.js(frame)
        for name in self.names:
            out[name] = dict(count=self.count(name, frame), mean=self.mean_angle(name, frame), js=js['JSD_' + name])
        return out

    def lines(self, frame=-1):
        """the report as printed lines"""
        s = self.summary(frame)
        out = [f"clash_free:\t{s['clash_free']:.4f}", f"mean_clashes:\t{s['mean_clashes']:.4f}", f"crowded_atoms:\t{s['crowded_atoms']}",
               f"degenerate:\t{s['degenerate']}", f"angles:\t{s['angles']}", f"torsions:\t{s['torsions']}"]
        for p, name in enumerate(self.names):
            kind = 'angle' if len(self.profiles[p][1]) == 3 else 'torsion'
            js = 'None' if s[name]['js'] is None else f"{s[name]['js']:.4f}"
            out.append(f"{kind} {name}:\tcount {s[name]['count']}\tmean {s[name]['mean']:.2f}\tJSD {js}")
        return out


def sample_geometry(result, eval_step=-1, include='all', reference=None, profiles=None, clash_scale=0.7, radii=None,
                    atom_enc_mode='add_aromatic', device='cuda'):
    """Local geometry of the samples of one pocket (``result``, ``eval_step`` and the packing as ``sample_quality``): per frame the
    share of molecules without an internal clash, the mean number of clashes, the crowded-atom and degenerate counts, and per profile
    the count, the mean angle and -- with ``reference`` ({name: counts}, of ``geometry_reference``) -- the Jensen-Shannon distance.
    ``include``: the molecules that are counted, as ``sample_rings``: ``'all'``, ``'complete'`` or a bool array [frames, samples].
    ``profiles``, ``clash_scale`` and ``radii`` as ``geometry``, whose conventions these are.  Returns a ``GeometryReport``."""
    return SamplePack(result, eval_step, atom_enc_mode, device).geometry(include, reference, profiles, clash_scale, radii)


def geometry_reference(molecules, profiles=None, atom_enc_mode='add_aromatic', device='cuda'):
    """The reference distributions of ``sample_geometry`` from known ligands, through the same kernel and so under the same bond rule
    (a reference made under another rule would not be comparable; no empirical distribution is part of this package).  ``molecules``:
    a list of ``(pos [n, 3], v [n])``, or of records of ``molfile.read_sdf`` (taken through ``molfile.ligand_classes``, atoms of
    elements outside the table left out).  Returns {name: counts [len(edges) + 1] int64} over ``profiles``."""
    from . import molfile
    prof = default_geometry_profiles() if profiles is None else tuple(profiles)
    mols = [molfile.ligand_classes(m, atom_enc_mode, drop_unknown=True) if isinstance(m, dict) else m for m in molecules]
    mols = [(np.asarray(p, dtype=np.float32).reshape(-1, 3), np.asarray(c, dtype=np.int64).reshape(-1)) for p, c in mols]
    if not mols:
        raise ValueError('a geometry reference needs at least one molecule')
    ptr = torch.as_tensor(np.cumsum([0] + [len(c) for _, c in mols]), dtype=torch.int32)
    pos, v, ptr = _pack(np.concatenate([p for p, _ in mols]), np.concatenate([c for _, c in mols]), None, ptr, device)
    r = _geometry_call(pos, v, ptr, class_atomic_numbers(atom_enc_mode), class_aromatic(atom_enc_mode), prof, None, None, False)
    hist = r['hist'][0].cpu().numpy()
    return {geometry_profile_name(p): hist[k, :len(p[4]) + 1].copy() for k, p in enumerate(prof)}


# ---- pocket contacts (``td_pocket_report``, csrc/pocket.hip; DESIGN.md section 3, "Pocket contacts")
# A contact is a ligand atom and a protein atom closer than 4 A; a protein clash is such a pair closer than the sum of their van der
# Waals radii minus 0.5 A.  Both numbers are conventions of this project, stated here and not measured: the cutoff is the usual one of
# contact fingerprints, the tolerance keeps hydrogen-bonded heavy atoms (N-O near 2.8 A against 3.07 A of radii) from counting as clashes.
DEFAULT_CONTACT_CUTOFF = 4.0
DEFAULT_CLASH_TOLERANCE = 0.5
POCKET_RADII = {**GEOMETRY_RADII, 34: 1.90}           # geometry's radii and Se


def pocket_kinds(feat, by='residue', hydrogens=False):
    """``(elem [n] int32, kind [n] int32, names)`` of the protein feature ``[n, 27]`` (workloads.featurize_protein: 6 element bits over
    H C N O S Se, 20 residue bits, the backbone bit).  ``elem``: the index of the element bit, -1 for a row without one.  ``kind``: by
    ``'residue'`` 2 * residue + backbone, 40 kinds named ``ALA.sc``, ``ALA.bb``, ... (-1 for a row without a residue bit); by
    ``'element'`` the element index, 6 kinds.  A protein hydrogen gets kind -1 unless ``hydrogens``: pockets are usually stored
    without hydrogens, and one stored with them would otherwise count every contact twice over.  An atom of kind -1 or element -1
    takes part in no contact and no clash."""
    return _kinds(_decode_features(feat), by, hydrogens)


def _decode_features(feat):
    """``(elem [n] int32, residue [n], backbone [n] bool)`` of the protein feature ``[n, 27]``: the index of the element bit and of the
    residue bit, -1 for a row without one, and the backbone bit.  The one decode that ``pocket_kinds`` and ``pocket_roles`` read."""
    from . import workloads
    f = feat.detach().cpu().numpy() if torch.is_tensor(feat) else np.asarray(feat)
    ne, na = len(workloads.PROTEIN_ELEMENTS), len(workloads.AA_NAMES)
    if f.ndim != 2 or f.shape[1] != ne + na + 1:
        raise ValueError(f'the protein feature is [n, {ne + na + 1}] (got {tuple(f.shape)})')
    f = f != 0
    elem = np.where(f[:, :ne].any(1), f[:, :ne].argmax(1), -1).astype(np.int32)
    return elem, np.where(f[:, ne:ne + na].any(1), f[:, ne:ne + na].argmax(1), -1), f[:, ne + na]


def _kinds(decoded, by, hydrogens):
    """``pocket_kinds`` of a decoded feature"""
    from . import workloads
    elem, aa, bb = decoded
    if by == 'residue':
        kind = np.where(aa >= 0, 2 * aa + bb, -1).astype(np.int32)
        names = tuple(f'{aa}.{part}' for aa in workloads.AA_NAMES for part in ('sc', 'bb'))
    elif by == 'element':
        kind, names = elem.copy(), ('H', 'C', 'N', 'O', 'S', 'Se')
    else:
        raise ValueError(f"kinds are by 'residue' or by 'element' (got {by!r})")
    if not hydrogens:
        kind[elem == 0] = -1
    return elem, kind, names


def pocket_clash_thresholds(tolerance=DEFAULT_CLASH_TOLERANCE, radii=None):
    """[8, 6] float64, ligand element over H C N O F P S Cl by protein element over H C N O S Se: ``r_l + r_p - tolerance`` with
    geometry's van der Waals radii and Se 1.90 A; ``radii``: {atomic number: radius in Angstrom} to change some.  The tolerance is a
    convention (``DEFAULT_CLASH_TOLERANCE``), not a measurement."""
    from . import workloads
    r = _radii(POCKET_RADII, radii)
    if not np.isfinite(float(tolerance)):
        raise ValueError(f'the clash tolerance is finite (got {tolerance})')
    rl = np.asarray([r[z] for z in ELEMENTS], dtype=np.float64)
    rp = np.asarray([r[z] for z in workloads.PROTEIN_ELEMENTS], dtype=np.float64)
    return (rl[:, None] + rp[None, :]) - np.float64(tolerance)


def pocket_of(data):
    """``(pos [N_p, 3], feat [N_p, 27])`` of the pocket ``data``: a workloads.Pocket (``pos``, ``feat``), an object or a dictionary
    with ``protein_pos`` and ``protein_atom_feature`` (what a result file's ``'data'`` is), or such a pair itself"""
    get = (lambda k: data.get(k)) if isinstance(data, dict) else (lambda k: getattr(data, k, None))
    if isinstance(data, (tuple, list)) and len(data) == 2:
        pos, feat = data
    else:
        pos, feat = get('protein_pos'), get('protein_atom_feature')
        if pos is None or feat is None:
            pos, feat = get('pos'), get('feat')
    if pos is None or feat is None:
        raise ValueError('no pocket: it is a workloads.Pocket, an object with protein_pos and protein_atom_feature, or (pos, feat)')
    return pos, feat


def _pocket_data(result, who):
    """the pocket a result dictionary carries, for ``sample_<who>``; the driver's bare 7-tuple carries none"""
    data = result.get('data') if isinstance(result, dict) else None
    if data is None:
        raise ValueError(f"the result carries no pocket: sample_{who} needs a result dictionary with its 'data' (results.result_dict), "
                         f'or use SamplePack.{who}(data)')
    return data


class PocketSide:
    """The protein side of the pocket reports, said once: the pocket ``data`` (``pocket_of``) decoded once and its positions uploaded
    once to ``device``.  ``pos`` [N_p, 3] fp32 and ``elem`` [N_p] int32 are device tensors; ``kinds(by, hydrogens)`` gives ``(kind [N_p]
    int32 on the device, names)`` as ``pocket_kinds`` -- by ``'element'`` the element index that the surface report takes --, and
    ``roles(hydrogens)`` the table of ``pocket_roles``; both are made when a report first asks and kept.  ``SamplePack.pocket``,
    ``.interactions`` and ``.sasa`` take one in the place of ``data``, so that several reports of one result file share it."""

    def __init__(self, data, device='cuda'):
        pos, feat = pocket_of(data)
        self._decoded = _decode_features(feat)
        pos = _fp32_positions(pos, device)
        n = len(self._decoded[0])
        if pos.shape[0] != 1 or pos.shape[1] != n:
            raise ValueError(f'protein positions must be [{n}, 3] (got {tuple(pos.shape[1:]) if pos.shape[0] == 1 else tuple(pos.shape)})')
        self.pos = pos[0].contiguous()
        self.elem = torch.from_numpy(self._decoded[0]).to(self.pos.device)
        self._kept = {}

    def _keep(self, key, make):
        if key not in self._kept:
            self._kept[key] = make()
        return self._kept[key]

    def kinds(self, by='residue', hydrogens=False):
        def make():
            _, kind, names = _kinds(self._decoded, by, hydrogens)
            return torch.from_numpy(kind).to(self.pos.device), names
        return self._keep((by, bool(hydrogens)), make)

    def roles(self, hydrogens=False):
        return self._keep(('role', bool(hydrogens)), lambda: torch.from_numpy(_roles(self._decoded, hydrogens)).to(self.pos.device))


class PocketContacts:
    """The contacts of S frames of B molecules with one pocket (``pocket_contacts``).  Device tensors, frame axis first: ``n_contacts``,
    ``n_contact_atoms`` (the buried atoms), ``n_pocket_atoms``, ``n_clashes``, ``n_clash_atoms`` [S, B] int32, ``clash_free`` [S, B]
    bool, ``min_dist`` [S, B] float64 (+inf without pairs), ``n_ref_common`` [S, B] int32 or None, ``atom_contacts`` / ``atom_clash``
    [S, N_l] int32, ``bits`` [S, B, W] int64 or None (bit j & 63 of word j >> 6: the molecule contacts protein atom j), and over the
    included molecules ``kind_hist`` [S, 8, n_kinds] int64 (ligand element over H C N O F P S Cl by protein kind, ``names``) and
    ``pocket_freq`` [S, N_p] int32; ``protein_elem`` / ``protein_kind`` [N_p] int32, ``ligand_ptr``."""

    def __init__(self, r, ligand_ptr, protein_elem, protein_kind, names):
        for k, t in r.items():
            setattr(self, k, t)
        self.clash_free = None if r['n_clashes'] is None else r['n_clashes'] == 0
        self.ligand_ptr, self.protein_elem, self.protein_kind, self.names = ligand_ptr, protein_elem, protein_kind, tuple(names)


def pocket_contacts(protein_pos, protein_feat, pos, v, batch_ligand=None, ligand_ptr=None, atom_enc_mode='add_aromatic',
                    contact_cutoff=DEFAULT_CONTACT_CUTOFF, clash_tolerance=DEFAULT_CLASH_TOLERANCE, radii=None, kinds='residue',
                    hydrogens=False, include=None, ref_bits=None, return_bits=False, device=None):
    """Contacts and clashes of every molecule of one frame ``[N_l, 3]`` or of a stack ``[S, N_l, 3]`` (arguments as ``bond_graph``)
    with the pocket ``protein_pos`` [N_p, 3], ``protein_feat`` [N_p, 27], both in the frame of ``pos``; every molecule is in that one
    pocket.  A pair is a ligand atom and a protein atom that takes part (``pocket_kinds``: no hydrogens unless ``hydrogens``); its
    distance is the bond rule's float64 distance.  Contact: d < ``contact_cutoff`` (default 4 A).  Clash: d < r_l + r_p -
    ``clash_tolerance`` (default 0.5 A; ``pocket_clash_thresholds``; None: no clash pass).  Both defaults are this project's
    conventions, not measurements, and not a pose checker's.  ``include`` [S, B] restricts ``kind_hist`` and ``pocket_freq`` and
    nothing else; ``ref_bits`` [W] int64: the contact words of a known ligand (``bits`` of a call on it), for ``n_ref_common``.
    Molecules of more than 512 atoms are refused.  Returns a ``PocketContacts`` (the frame axis is kept)."""
    pos, v, ligand_ptr = _pack(pos, v, batch_ligand, ligand_ptr, device)
    side = PocketSide((protein_pos, protein_feat), pos.device)
    (kind, names), elem = side.kinds(kinds, hydrogens), side.elem
    include = _frame_mask(include, pos)
    if ref_bits is not None:
        ref_bits = torch.as_tensor(ref_bits).to(device=pos.device).contiguous()
    thr = None if clash_tolerance is None else pocket_clash_thresholds(clash_tolerance, radii)
    r = capi.pocket_report(pos, v, ligand_ptr, class_atomic_numbers(atom_enc_mode), side.pos, elem, kind, len(names), contact_cutoff, thr,
                           include, ref_bits, True, return_bits)
    return PocketContacts(r, ligand_ptr, elem, kind, names)


def _reference_recovery(common, touched, ref_size, included):
    """How a pocket's molecules recover the protein atoms a known ligand marks: ``common`` [S, B] the marked atoms a molecule hits,
    ``touched`` [S, B] the atoms it hits, ``ref_size`` the marked atoms.  Returns (``sum_ref`` [S, 4], ``n_ref`` [S]): per frame the
    mean, the median and the largest recovery common / ref_size and the mean Tanimoto common / (touched + ref_size - common) over the
    included molecules, and 1 where the frame has them (a reference that marks nothing, or an empty set, gives none)."""
    inc = np.asarray(included, dtype=bool)
    S = inc.shape[0]
    sum_ref, n_ref = np.zeros((S, 4)), np.zeros(S, np.int64)
    common, touched = np.asarray(common, dtype=np.float64), np.asarray(touched, dtype=np.float64)
    for s in range(S):
        if int(ref_size) > 0 and inc[s].any():
            rec = common[s][inc[s]] / float(ref_size)
            tan = common[s][inc[s]] / (touched[s][inc[s]] + float(ref_size) - common[s][inc[s]])
            sum_ref[s] = (rec.sum() / rec.size, np.median(rec), rec.max(), tan.sum() / tan.size)
            n_ref[s] = 1
    return sum_ref, n_ref


class PocketReport(_SumReport):
    """Per frame (axis 0), over the included molecules (``n_included`` [S] of ``n_samples``): ``n_clash_free``, ``sum_clashes``,
    ``sum_contacts``, ``n_no_contact`` [S] int64; ``sum_buried`` [S], the sum of buried atoms / atoms over the ``n_nonempty`` [S]
    non-empty ones; ``sum_min_dist`` [S] over the ``n_min_dist`` [S] molecules that have a pair; ``kind_hist`` [S, 8, n_kinds] int64
    with ``names`` and ``backbone`` (one flag per kind, or None when the kinds do not tell); ``pocket_freq`` [S, N_p] int64, the
    pocket's contact map, or None for a report merged from several pockets.  With a reference ligand ``sum_ref`` [S, 4] -- per pocket
    the mean, the median and the largest recovery n_ref_common / |ref| and the mean Tanimoto n_common / (n_pocket_atoms + |ref| -
    n_common) -- over the ``n_ref`` [S] pockets that have them: a reference that touches nothing gives no value, and the summary NaN.
    The cutoff and the clash rule are this project's conventions (``pocket_contacts``)."""

    FIELDS = (('n_included', 'i64'), ('n_clash_free', 'i64'), ('sum_clashes', 'i64'), ('sum_contacts', 'i64'), ('n_no_contact', 'i64'),
              ('sum_buried', 'f64'), ('n_nonempty', 'i64'), ('sum_min_dist', 'f64'), ('n_min_dist', 'i64'), ('kind_hist', 'i64'), ('names', 'tuple'),
              ('backbone', 'flags'), ('n_samples', 'int_sum'), ('pocket_freq', 'map'), ('sum_ref', 'ref_f64'), ('n_ref', 'ref_i64'))
    OPTIONAL, MISMATCH = 3, 'reports of different frame counts or kinds, or with and without a reference ligand, do not merge'

    def _merge_key(self):
        return self.kind_hist.shape, self.names, self.sum_ref is None

    @classmethod
    def from_outputs(cls, raw, included, sizes, names, backbone=None, ref_size=None):
        """One pocket: ``raw`` the numpy outputs of capi.pocket_report (n_contacts, n_contact_atoms, n_pocket_atoms, n_clashes,
        min_dist, kind_hist, pocket_freq and, with a reference of ``ref_size`` contacted atoms, n_ref_common), ``included`` [S, B]
        bool, ``sizes`` [B]"""
        inc = np.asarray(included, dtype=bool)
        n = np.asarray(sizes, dtype=np.float64)
        con, clashes = np.asarray(raw['n_contacts'], dtype=np.int64), np.asarray(raw['n_clashes'], dtype=np.int64)
        buried, md = np.asarray(raw['n_contact_atoms'], dtype=np.float64), np.asarray(raw['min_dist'], dtype=np.float64)
        share = np.divide(buried, n[None], out=np.zeros_like(buried), where=n[None] > 0)
        has = inc & np.isfinite(md)
        sum_ref = n_ref = None
        if ref_size is not None:
            sum_ref, n_ref = _reference_recovery(raw['n_ref_common'], raw['n_pocket_atoms'], ref_size, inc)
        return cls(inc.sum(1), (inc & (clashes == 0)).sum(1), np.where(inc, clashes, 0).sum(1), np.where(inc, con, 0).sum(1),
                   (inc & (con == 0)).sum(1), np.where(inc, share, 0.0).sum(1), (inc & (n[None] > 0)).sum(1), np.where(has, md, 0.0).sum(1),
                   has.sum(1), raw['kind_hist'], names, backbone, len(n), raw['pocket_freq'], sum_ref, n_ref)

    def clash_free(self, frame=-1):
        """included molecules without a protein clash / included molecules"""
        return self._mean(self.n_clash_free[frame], self.n_included[frame])

    def mean_clashes(self, frame=-1):
        return self._mean(self.sum_clashes[frame], self.n_included[frame])

    def mean_contacts(self, frame=-1):
        return self._mean(self.sum_contacts[frame], self.n_included[frame])

    def buried_share(self, frame=-1):
        """the mean of atoms with a contact / atoms over the included non-empty molecules"""
        return self._mean(self.sum_buried[frame], self.n_nonempty[frame])

    def no_contact(self, frame=-1):
        """the share of included molecules that touch nothing: poses that left the pocket"""
        return self._mean(self.n_no_contact[frame], self.n_included[frame])

    def mean_min_dist(self, frame=-1):
        return self._mean(self.sum_min_dist[frame], self.n_min_dist[frame])

    def contact_profile(self, frame=-1):
        """{kind name: share of the contact pairs}, or None when there is no contact"""
        h = self.kind_hist[frame].sum(0)
        return {k: float(x) / float(h.sum()) for k, x in zip(self.names, h)} if h.sum() > 0 else None

    def backbone_share(self, frame=-1):
        """the share of the contact pairs whose protein atom is of the backbone; nan without contacts or when the kinds do not tell"""
        h = self.kind_hist[frame].sum(0)
        return self._mean(h[self.backbone].sum(), h.sum()) if self.backbone is not None else float('nan')

    def contact_frequency(self, frame=-1):
        """[N_p]: the share of the included molecules that contact each protein atom; None for a report of several pockets"""
        if self.pocket_freq is None:
            return None
        n = int(self.n_included[frame])
        return self.pocket_freq[frame] / float(n) if n else np.full(self.pocket_freq.shape[1], np.nan)

    def reference_recovery(self, frame=-1):
        """{'ref_recovery_mean', 'ref_recovery_median', 'ref_recovery_max', 'ref_tanimoto'} or {} without a reference ligand"""
        if self.sum_ref is None:
            return {}
        keys = ('ref_recovery_mean', 'ref_recovery_median', 'ref_recovery_max', 'ref_tanimoto')
        return {k: self._mean(self.sum_ref[frame, c], self.n_ref[frame]) for c, k in enumerate(keys)}

    def summary(self, frame=-1):
        return dict(pocket_clash_free=self.clash_free(frame), pocket_mean_clashes=self.mean_clashes(frame),
                    mean_contacts=self.mean_contacts(frame), buried_share=self.buried_share(frame), no_contact=self.no_contact(frame),
                    mean_min_dist=self.mean_min_dist(frame), backbone_share=self.backbone_share(frame), **self.reference_recovery(frame))

    def lines(self, frame=-1, top=5):
        """the report as printed lines: the summary, then the ``top`` kinds of the contact profile"""
        out = super().lines(frame)
        prof = self.contact_profile(frame) or {}
        for k, x in sorted(prof.items(), key=lambda kx: (-kx[1], kx[0]))[:top]:
            if x > 0:
                out.append(f'contacts {k}:\t{x:.4f}')
        return out


def sample_pocket(result, eval_step=-1, include='all', reference_ligand=None, contact_cutoff=DEFAULT_CONTACT_CUTOFF,
                  clash_tolerance=DEFAULT_CLASH_TOLERANCE, kinds='residue', atom_enc_mode='add_aromatic', device='cuda'):
    """Pocket contacts of the samples of one pocket (``result`` a loaded ``result_{i}.pt`` dictionary, whose ``'data'`` is the pocket;
    ``eval_step`` and the packing as ``sample_quality``): per frame the share of molecules without a protein clash, the mean numbers of
    clashes and contacts, the buried share, the share of poses that touch nothing, the mean smallest distance, the contact profile by
    residue kind and the pocket's contact map; with ``reference_ligand`` ``(pos [n, 3], v [n])``, run through the same kernel, the
    recovery of its contacts.  ``include`` as ``sample_rings``.  The cutoff and the clash rule are conventions (``pocket_contacts``).
    A result without a pocket (the driver's bare 7-tuple) is refused.  Returns a ``PocketReport``."""
    return SamplePack(result, eval_step, atom_enc_mode, device).pocket(_pocket_data(result, 'pocket'), include, reference_ligand, contact_cutoff, clash_tolerance, kinds)


# ---- typed pocket interactions (``td_interaction_report``, csrc/interactions.hip; DESIGN.md section 3, "Pocket interactions")
# Counts of hydrogen bonds and hydrophobic contacts; no energy and no score.  The roles are conventions of this project: the ligand's
# donors are inferred from the valence deficit of N and O under the bond rule (the sampler places no hydrogens), a heuristic and not
# perceived chemistry; the protein's come from a residue table; a hydrogen bond is a donor - acceptor pair of heavy atoms closer than
# 3.5 A with no angle criterion, a hydrophobic contact a pair of hydrophobic atoms closer than 4.5 A.
ROLE_DONOR, ROLE_ACCEPTOR, ROLE_HYDROPHOBIC = capi.ROLE_DONOR, capi.ROLE_ACCEPTOR, capi.ROLE_HYDROPHOBIC
ROLE_NAMES = {ROLE_DONOR: 'donor', ROLE_ACCEPTOR: 'acceptor', ROLE_HYDROPHOBIC: 'hydrophobic'}
INTERACTION_NAMES = ('donated', 'accepted', 'hydrophobic')      # type 0: the ligand donates; 1: the ligand accepts; 2: hydrophobic
DEFAULT_HBOND_CUTOFF = 3.5
DEFAULT_HYDROPHOBIC_CUTOFF = 4.5
DEFAULT_HETERO_CUTOFF = 1.75                          # between a C-N / C-O bond and the nearest non-bonded pair


def pocket_roles(feat, hydrogens=False):
    """[n] int32 of the protein feature ``[n, 27]`` (``pocket_kinds``): the donor / acceptor bits of every protein atom by residue,
    element and backbone bit.  Backbone N: DONOR, except PRO.  Backbone O: ACCEPTOR.  Side-chain O of SER, THR, TYR: DONOR | ACCEPTOR;
    any other O (ASP, GLU, ASN, GLN, a terminal OXT): ACCEPTOR.  Side-chain N of ARG, LYS, ASN, GLN, TRP: DONOR; of HIS: DONOR |
    ACCEPTOR.  C, S, Se, H: 0 (which carbons are hydrophobic the device decides).  -1, an atom that takes part nowhere: a row without
    an element bit or without a residue bit, and a hydrogen unless ``hydrogens``."""
    return _roles(_decode_features(feat), hydrogens)


def _roles(decoded, hydrogens):
    """``pocket_roles`` of a decoded feature"""
    from . import workloads
    elem, aa, bb = decoded
    of = lambda *names: np.isin(aa, [workloads.AA_NAMES.index(x) for x in names])
    N, O = elem == workloads.PROTEIN_ELEMENTS.index(7), elem == workloads.PROTEIN_ELEMENTS.index(8)
    role = np.zeros(len(elem), np.int32)
    role[N & bb & ~of('PRO')] = ROLE_DONOR
    role[N & ~bb & of('ARG', 'LYS', 'ASN', 'GLN', 'TRP')] = ROLE_DONOR
    role[N & ~bb & of('HIS')] = ROLE_DONOR | ROLE_ACCEPTOR
    role[O] = ROLE_ACCEPTOR
    role[O & ~bb & of('SER', 'THR', 'TYR')] = ROLE_DONOR | ROLE_ACCEPTOR
    role[(elem < 0) | (aa < 0)] = -1
    if not hydrogens:
        role[elem == workloads.PROTEIN_ELEMENTS.index(1)] = -1
    return role


class Interactions:
    """The typed interactions of S frames of B molecules with one pocket (``pocket_interactions``).  Device tensors, frame axis first:
    ``protein_role`` [N_p] int32 (the table's bits with the hydrophobic bit resolved, -1: takes no part); ``n_donated``, ``n_accepted``,
    ``n_hbonds``, ``n_hydrophobic`` (pairs), ``n_hb_atoms``, ``n_donors``, ``n_acceptors``, ``n_hydrophobic_atoms`` (ligand atoms)
    [S, B] int32; ``n_ref_common`` [S, B, 3] int32 or None; ``atom_role``, ``atom_hbonds``, ``atom_hydrophobic`` [S, N_l] int32;
    ``bits`` [S, B, 3, W] int64 or None (per type, bit j & 63 of word j >> 6: the molecule hits protein atom j); over the included
    molecules ``kind_hist`` [S, 3, n_kinds] int64 (type by protein kind, ``names``) and ``pocket_freq`` [S, 3, N_p] int32;
    ``protein_elem`` / ``protein_kind`` [N_p] int32, ``ligand_ptr``.  The types: ``INTERACTION_NAMES``."""

    def __init__(self, r, ligand_ptr, protein_elem, protein_kind, names):
        for k, t in r.items():
            setattr(self, k, t)
        self.ligand_ptr, self.protein_elem, self.protein_kind, self.names = ligand_ptr, protein_elem, protein_kind, tuple(names)


def pocket_interactions(protein_pos, protein_feat, pos, v, batch_ligand=None, ligand_ptr=None, atom_enc_mode='add_aromatic',
                        hbond_cutoff=DEFAULT_HBOND_CUTOFF, hydrophobic_cutoff=DEFAULT_HYDROPHOBIC_CUTOFF,
                        hetero_cutoff=DEFAULT_HETERO_CUTOFF, kinds='residue', hydrogens=False, include=None, ref_bits=None,
                        return_bits=False, device=None):
    """Hydrogen bonds and hydrophobic contacts of every molecule of one frame ``[N_l, 3]`` or of a stack ``[S, N_l, 3]`` (arguments as
    ``bond_graph``) with the pocket ``protein_pos`` [N_p, 3], ``protein_feat`` [N_p, 27] (as ``pocket_contacts``).  Ligand roles: on
    the bond graph, DONOR an N or O with at least one hydrogen, bonded or implied by its valence deficit (3 - val for N, 2 - val for O);
    ACCEPTOR an O, or an N without hydrogens and val <= 3; HYDROPHOBIC a C without a bonded N or O, F, Cl.  Protein roles:
    ``pocket_roles``, and HYDROPHOBIC a carbon without a protein N or O closer than ``hetero_cutoff``.  Ligand donates / accepts:
    d < ``hbond_cutoff`` between heavy atoms, no angle; hydrophobic: d < ``hydrophobic_cutoff``; d the bond rule's float64 distance.
    All of it is this project's convention, a heuristic and not perceived chemistry, and not a docking score.  ``include`` [S, B]
    restricts ``kind_hist`` and ``pocket_freq`` and nothing else; ``ref_bits`` [3, W] int64: the words of a known ligand (``bits`` of
    a call on it), for ``n_ref_common``.  Molecules of more than 512 atoms are refused.  Returns an ``Interactions``."""
    pos, v, ligand_ptr = _pack(pos, v, batch_ligand, ligand_ptr, device)
    side = PocketSide((protein_pos, protein_feat), pos.device)
    (kind, names), elem = side.kinds(kinds, hydrogens), side.elem
    include = _frame_mask(include, pos)
    if ref_bits is not None:
        ref_bits = torch.as_tensor(ref_bits).to(device=pos.device).contiguous()
    r = capi.interaction_report(pos, v, ligand_ptr, class_atomic_numbers(atom_enc_mode), side.pos, elem, kind, side.roles(hydrogens), len(names), hbond_cutoff,
                                hydrophobic_cutoff, hetero_cutoff, include, ref_bits, True, return_bits)
    return Interactions(r, ligand_ptr, elem, kind, names)


def _popcount(words):
    """the set bits of int64 words, summed over the last axis"""
    w = np.ascontiguousarray(words)
    return np.unpackbits(w.view(np.uint8).reshape(w.shape + (8,)), axis=-1).sum((-1, -2)).astype(np.int64)


class InteractionReport(_SumReport):
    """Per frame (axis 0), over the included molecules (``n_included`` [S] of ``n_samples``): ``sum_hbonds``, ``sum_donated``,
    ``sum_accepted``, ``sum_hydrophobic`` [S] int64, the pairs; ``n_no_hbond`` [S], the molecules without a hydrogen bond;
    ``sum_hb_atoms`` of the ``sum_polar_atoms`` [S] ligand atoms that are donor or acceptor; ``kind_hist`` [S, 3, n_kinds] int64 with
    ``names``; ``pocket_freq`` [S, 3, N_p] int64, the pocket's interaction map, or None for a report merged from several pockets.
    With a reference ligand ``sum_ref`` [S, 3, 4] -- per pocket and type the mean, the median and the largest recovery n_ref_common /
    |ref| and the mean Tanimoto n_common / (n_hit + |ref| - n_common) -- over the ``n_ref`` [S, 3] pockets that have them: a
    reference without an interaction of a type gives no value there, and the summary NaN.  The roles and the cutoffs are this
    project's conventions (``pocket_interactions``)."""

    FIELDS = (('n_included', 'i64'), ('sum_hbonds', 'i64'), ('sum_donated', 'i64'), ('sum_accepted', 'i64'), ('sum_hydrophobic', 'i64'),
              ('n_no_hbond', 'i64'), ('sum_hb_atoms', 'i64'), ('sum_polar_atoms', 'i64'), ('kind_hist', 'i64'), ('names', 'tuple'),
              ('n_samples', 'int_sum'), ('pocket_freq', 'map'), ('sum_ref', 'ref_f64'), ('n_ref', 'ref_i64'))
    OPTIONAL, MISMATCH = 3, PocketReport.MISMATCH

    def _merge_key(self):
        return self.kind_hist.shape, self.names, self.sum_ref is None

    @classmethod
    def from_outputs(cls, raw, included, sizes, names, ref_sizes=None):
        """One pocket: ``raw`` the numpy outputs of capi.interaction_report (n_donated, n_accepted, n_hbonds, n_hydrophobic,
        n_hb_atoms, atom_role, kind_hist, pocket_freq and, with a reference of ``ref_sizes`` [3] protein atoms hit per type,
        n_ref_common and bits), ``included`` [S, B] bool, ``sizes`` [B]"""
        inc = np.asarray(included, dtype=bool)
        S = inc.shape[0]
        ptr = np.cumsum([0] + [int(n) for n in sizes])
        polar = (np.asarray(raw['atom_role']) & (ROLE_DONOR | ROLE_ACCEPTOR)) != 0
        run = np.concatenate([np.zeros((S, 1), np.int64), np.cumsum(polar, axis=1, dtype=np.int64)], axis=1)
        n_polar = run[:, ptr[1:]] - run[:, ptr[:-1]]                                # [S, B]
        tot = lambda x: np.where(inc, np.asarray(x, dtype=np.int64), 0).sum(1)
        hbonds = np.asarray(raw['n_hbonds'], dtype=np.int64)
        sum_ref = n_ref = None
        if ref_sizes is not None:
            common, hit = np.asarray(raw['n_ref_common']), _popcount(raw['bits'])
            per_type = [_reference_recovery(common[..., t], hit[..., t], ref_sizes[t], inc) for t in range(3)]
            sum_ref, n_ref = (np.stack(x, axis=1) for x in zip(*per_type))
        return cls(inc.sum(1), tot(hbonds), tot(raw['n_donated']), tot(raw['n_accepted']), tot(raw['n_hydrophobic']), (inc & (hbonds == 0)).sum(1),
                   tot(raw['n_hb_atoms']), tot(n_polar), raw['kind_hist'], names, len(sizes), raw['pocket_freq'], sum_ref, n_ref)

    def mean_hbonds(self, frame=-1):
        """hydrogen bonds per included molecule; a pair that donates and accepts at once counts once"""
        return self._mean(self.sum_hbonds[frame], self.n_included[frame])

    def mean_donated(self, frame=-1):
        return self._mean(self.sum_donated[frame], self.n_included[frame])

    def mean_accepted(self, frame=-1):
        return self._mean(self.sum_accepted[frame], self.n_included[frame])

    def mean_hydrophobic(self, frame=-1):
        return self._mean(self.sum_hydrophobic[frame], self.n_included[frame])

    def no_hbond(self, frame=-1):
        """the share of included molecules without a hydrogen bond"""
        return self._mean(self.n_no_hbond[frame], self.n_included[frame])

    def polar_in_hbond(self, frame=-1):
        """the share of the ligands' donor or acceptor atoms that take part in a hydrogen bond; nan without such atoms"""
        return self._mean(self.sum_hb_atoms[frame], self.sum_polar_atoms[frame])

    def kind_profile(self, kind, frame=-1):
        """{kind name: share of the pairs of the type} (``kind`` an index or a name of ``INTERACTION_NAMES``), or None without pairs"""
        t = INTERACTION_NAMES.index(kind) if isinstance(kind, str) else int(kind)
        h = self.kind_hist[frame, t]
        return {k: float(x) / float(h.sum()) for k, x in zip(self.names, h)} if h.sum() > 0 else None

    def interaction_frequency(self, frame=-1):
        """[3, N_p]: the share of the included molecules that hit each protein atom, per type; None for a report of several pockets"""
        if self.pocket_freq is None:
            return None
        n = int(self.n_included[frame])
        return self.pocket_freq[frame] / float(n) if n else np.full(self.pocket_freq.shape[1:], np.nan)

    def reference_recovery(self, frame=-1):
        """{'ref_<type>_recovery_mean', '..._recovery_median', '..._recovery_max', 'ref_<type>_tanimoto'} per type, or {} without a
        reference ligand"""
        if self.sum_ref is None:
            return {}
        keys = ('recovery_mean', 'recovery_median', 'recovery_max', 'tanimoto')
        return {f'ref_{name}_{k}': self._mean(self.sum_ref[frame, t, c], self.n_ref[frame, t]) for t, name in enumerate(INTERACTION_NAMES)
                for c, k in enumerate(keys)}

    def summary(self, frame=-1):
        return dict(mean_hbonds=self.mean_hbonds(frame), mean_donated=self.mean_donated(frame), mean_accepted=self.mean_accepted(frame),
                    mean_hydrophobic=self.mean_hydrophobic(frame), no_hbond=self.no_hbond(frame), polar_in_hbond=self.polar_in_hbond(frame),
                    **self.reference_recovery(frame))

    def lines(self, frame=-1, top=3):
        """the report as printed lines: the summary, then per type the ``top`` residue kinds"""
        out = super().lines(frame)
        for name in INTERACTION_NAMES:
            prof = self.kind_profile(name, frame) or {}
            for k, x in sorted(prof.items(), key=lambda kx: (-kx[1], kx[0]))[:top]:
                if x > 0:
                    out.append(f'{name} {k}:\t{x:.4f}')
        return out


def sample_interactions(result, eval_step=-1, include='all', reference_ligand=None, hbond_cutoff=DEFAULT_HBOND_CUTOFF,
                        hydrophobic_cutoff=DEFAULT_HYDROPHOBIC_CUTOFF, hetero_cutoff=DEFAULT_HETERO_CUTOFF, atom_enc_mode='add_aromatic',
                        device='cuda'):
    """Typed pocket interactions of the samples of one pocket (``result`` a loaded ``result_{i}.pt`` dictionary, whose ``'data'`` is
    the pocket; ``eval_step`` and the packing as ``sample_quality``): per frame the mean hydrogen bonds per molecule and their donated /
    accepted split, the mean hydrophobic contacts, the share of molecules without a hydrogen bond, the share of polar ligand atoms in
    one, the residue kinds per type and the pocket's interaction map; with ``reference_ligand`` ``(pos [n, 3], v [n])``, run through
    the same kernel, the recovery of its interactions per type.  ``include`` as ``sample_rings``.  The roles and cutoffs are
    conventions (``pocket_interactions``).  A result without a pocket is refused.  Returns an ``InteractionReport``."""
    return SamplePack(result, eval_step, atom_enc_mode, device).interactions(_pocket_data(result, 'interactions'), include, reference_ligand,
                                                                             hbond_cutoff, hydrophobic_cutoff, hetero_cutoff)


# ---- docking-style score (``td_score_report``, csrc/score.hip; DESIGN.md section 3, "Docking-style score")
# A Vina-style score on this project's heuristic typing: the functional form and the weights are those of the AutoDock Vina paper
# (Trott & Olson 2010), but no hydrogens are placed, the donor / acceptor / hydrophobic roles are those of ``pocket_interactions`` (valence
# deficits and a residue table), the radii are one per element, and there is no intramolecular term.  It is NOT AutoDock Vina's number:
# comparable between runs of this tool, not with published tables.  The kernel returns the five unweighted term sums as integers in
# units of 2^-24; the weights and the rotor normalisation are applied here, so a caller may re-weight without a rebuild.
SCORE_TERM_NAMES = capi.SCORE_TERM_NAMES              # gauss1, gauss2, repulsion, hydrophobic, hbond
SCORE_WEIGHTS = (-0.035579, -0.005156, 0.840245, -0.035069, -0.587439)
SCORE_ROT_WEIGHT = 0.0585
SCORE_CUTOFF = 8.0
SCORE_LIGAND_RADII = (0.0, 1.9, 1.8, 1.7, 1.5, 2.1, 2.0, 1.8)      # H C N O F P S Cl; H never takes part
SCORE_PROTEIN_RADII = (0.0, 1.9, 1.8, 1.7, 2.0, 2.0)               # H C N O S Se


def score_radius_sums(ligand_radii=None, protein_radii=None):
    """[8, 6] float64, ligand element over H C N O F P S Cl by protein element over H C N O S Se: ``R_l + R_p`` of
    ``SCORE_LIGAND_RADII`` and ``SCORE_PROTEIN_RADII`` or of the tables given.  The H row and column hold 1: hydrogens never take part,
    so the entries are never read, and the entry point admits only sums in (0, 6]."""
    rl = np.asarray(SCORE_LIGAND_RADII if ligand_radii is None else ligand_radii, dtype=np.float64)
    rp = np.asarray(SCORE_PROTEIN_RADII if protein_radii is None else protein_radii, dtype=np.float64)
    if rl.shape != (8,) or rp.shape != (6,):
        raise ValueError('the radii are [8] over H C N O F P S Cl and [6] over H C N O S Se')
    rs = rl[:, None] + rp[None, :]
    rs[0, :] = 1.0
    rs[:, 0] = 1.0
    return rs


def score_energies(terms, n_rot, weights=SCORE_WEIGHTS, rot_weight=SCORE_ROT_WEIGHT):
    """``(terms, inter, score)`` as float64 numpy of the integer ``terms`` [..., 5] of td_score_report and ``n_rot`` [...] (None: no
    rotors): the terms / 2^24, ``inter`` = weights . terms, ``score`` = inter / (1 + rot_weight n_rot)"""
    t = np.asarray(terms, dtype=np.float64) / float(1 << capi.SCORE_FRAC_BITS)
    w = np.asarray(weights, dtype=np.float64)
    if w.shape != (capi.SCORE_TERMS,):
        raise ValueError(f'the weights are {capi.SCORE_TERMS}: {", ".join(SCORE_TERM_NAMES)}')
    inter = (t * w).sum(-1)
    rot = np.zeros(inter.shape) if n_rot is None else np.asarray(n_rot, dtype=np.float64)
    return t, inter, inter / (1.0 + np.float64(rot_weight) * rot)


def _heavy_atoms(v, class_z, sizes):
    """[S, B] int64: per molecule the atoms with a class in the table and an element other than H; ``v`` [S, N_l] numpy"""
    z = np.asarray(class_z, dtype=np.int64)
    v = np.asarray(v)
    ok = (v >= 0) & (v < len(z))
    heavy = ok & (z[np.where(ok, v, 0)] != 1)
    ptr = np.cumsum([0] + [int(n) for n in sizes])
    run = np.concatenate([np.zeros((v.shape[0], 1), np.int64), np.cumsum(heavy, axis=1, dtype=np.int64)], axis=1)
    return run[:, ptr[1:]] - run[:, ptr[:-1]]


def _pose_inputs(protein_pos, protein_feat, pos, v, batch_ligand, ligand_ptr, atom_enc_mode, ligand_radii, protein_radii, hydrogens, rotors,
                 device, single_frame=False):
    """What ``pocket_score``, ``pocket_relax`` and ``pocket_dock`` open with, as they pass it to the bindings: (the pack with the class
    tables, the pocket up to the radius sums, (bond_ptr, bond_ring)).  With ``rotors`` this runs ``td_bond_graph`` and
    ``td_ring_report`` -- the host's look at the pack is the bond graph's --, otherwise both are None."""
    pos, v, ligand_ptr = _pack(pos, v, batch_ligand, ligand_ptr, device)
    if single_frame:
        _single_frame(None, pos.shape[0])
    side = PocketSide((protein_pos, protein_feat), pos.device)
    (kind, names), elem = side.kinds('residue', hydrogens), side.elem
    cz, aro = class_atomic_numbers(atom_enc_mode), class_aromatic(atom_enc_mode)
    bond_ptr = bond_ring = None
    if rotors:
        bond_ptr = capi.bond_graph(pos, v, ligand_ptr, cz, aro, (), None, False, True)['bond_ptr']
        bond_ring = capi.ring_report(pos, v, ligand_ptr, cz, aro, None, bond_ptr, False, check=False)['bond_ring']
    pocket = (side.pos, elem, kind, side.roles(hydrogens), len(names), score_radius_sums(ligand_radii, protein_radii))
    return (pos, v, ligand_ptr, cz, aro), pocket, (bond_ptr, bond_ring)


def _numpy(r, keys):
    """``keys`` of a binding's dict of device tensors as numpy; None stays None"""
    return {k: None if r[k] is None else r[k].cpu().numpy() for k in keys}


def _reference_rows(inc, score, ref):
    """(``sum_ref`` [S, len(ref) + 1], ``n_ref`` [S]) of one pocket: for every frame with an included molecule (``inc`` [S, B]) the
    known ligand's values ``ref`` and the share of the included molecules whose ``score`` [S, B] is below the last of them; (None,
    None) without ``ref``"""
    if ref is None:
        return None, None
    S = inc.shape[0]
    sum_ref, n_ref = np.zeros((S, len(ref) + 1)), np.zeros(S, np.int64)
    for s in range(S):
        if inc[s].any():
            sum_ref[s] = (*ref, float((score[s][inc[s]] < ref[-1]).sum()) / float(inc[s].sum()))
            n_ref[s] = 1
    return sum_ref, n_ref


class _PoseReport(_SumReport):
    """What ``ScoreReport``, ``RelaxReport`` and ``DockReport`` share beyond ``_SumReport``: ``n_included`` first and ``sum_ref`` /
    ``n_ref`` last among the ``FIELDS``, the statistics over a per-molecule score column -- a class's ``_of(frame, ...)`` gives the
    scored molecules' values of the column that the arguments after ``frame`` choose, by default its final one -- and ``reference``
    from the names ``REF_KEYS`` of the columns of ``sum_ref``."""
    OPTIONAL, MISMATCH = 2, 'the reports differ in their frames or in whether they have a reference ligand'
    REF_KEYS = ()

    def _merge_key(self):
        return self.n_included.shape, self.sum_ref is None

    @staticmethod
    def _mean_of(x):
        return float(x.sum()) / x.size if x.size else float('nan')

    def mean_score(self, frame=-1, *column, **kw):
        return self._mean_of(self._of(frame, *column, **kw))

    def median_score(self, frame=-1, *column, **kw):
        x = self._of(frame, *column, **kw)
        return float(np.median(x)) if x.size else float('nan')

    def best_score(self, frame=-1, *column, **kw):
        """the lowest score of the frame"""
        x = self._of(frame, *column, **kw)
        return float(x.min()) if x.size else float('nan')

    def share_negative(self, frame=-1):
        return self._mean((self._of(frame) < 0.0).sum(), self.n_included[frame])

    def reference(self, frame=-1):
        """``REF_KEYS`` with their values (means over the pockets of a merged report), or {} without a reference ligand"""
        if self.sum_ref is None:
            return {}
        return {k: self._mean(self.sum_ref[frame, c], self.n_ref[frame]) for c, k in enumerate(self.REF_KEYS)}


class Score:
    """The docking-style score of S frames of B molecules with one pocket (``pocket_score``).  ``protein_role`` [N_p] int32 on the
    device; numpy, frame axis first: ``terms`` [S, B, 5] float64 (the unweighted sums, ``SCORE_TERM_NAMES``), ``n_pairs`` [S, B] int32,
    ``n_rot`` [S, B] int32 or None, ``heavy_atoms`` [S, B], ``inter`` = weights . terms, ``score`` = inter / (1 + rot_weight n_rot) and
    ``efficiency`` = score / heavy atoms (NaN without heavy atoms) [S, B] float64; ``raw_terms`` [S, B, 5] int64, the kernel's integers.
    A molecule the kernel refused (n_pairs = -1) has NaN in the float outputs.  Not AutoDock Vina's number (``pocket_score``)."""

    def __init__(self, r, ligand_ptr, heavy, weights, rot_weight):
        self.protein_role, self.ligand_ptr = r['protein_role'], ligand_ptr
        self.raw_terms, self.n_pairs = r['terms'].cpu().numpy(), r['n_pairs'].cpu().numpy()
        self.n_rot = None if r['n_rot'] is None else r['n_rot'].cpu().numpy()
        self.heavy_atoms = heavy
        bad = self.n_pairs < 0
        self.terms, self.inter, self.score = score_energies(np.where(bad[..., None], 0, self.raw_terms), self.n_rot, weights, rot_weight)
        self.terms[bad], self.inter[bad], self.score[bad] = np.nan, np.nan, np.nan
        self.efficiency = np.divide(self.score, heavy, out=np.full(self.score.shape, np.nan), where=heavy > 0)


def pocket_score(protein_pos, protein_feat, pos, v, batch_ligand=None, ligand_ptr=None, atom_enc_mode='add_aromatic', weights=SCORE_WEIGHTS,
                 rot_weight=SCORE_ROT_WEIGHT, cutoff=SCORE_CUTOFF, hetero_cutoff=DEFAULT_HETERO_CUTOFF, ligand_radii=None, protein_radii=None,
                 hydrogens=False, rotors=True, device=None):
    """A Vina-style score of every molecule of one frame ``[N_l, 3]`` or of a stack ``[S, N_l, 3]`` (arguments as ``bond_graph``) in
    the pocket ``protein_pos`` [N_p, 3], ``protein_feat`` [N_p, 27] (as ``pocket_contacts``).  Pairs: ligand heavy atoms with protein
    heavy atoms that take part, at a bond-rule distance r < ``cutoff`` (8 A); surface distance d = r - R_l - R_p (``score_radius_sums``).
    Terms: gauss1 exp(-(2 d)^2), gauss2 exp(-((d - 3) / 2)^2), repulsion d^2 for d < 0, hydrophobic (1 below 0.5 A, linear to 0 at
    1.5 A, between HYDROPHOBIC atoms) and hbond (1 below -0.7 A, linear to 0 at 0, donor with acceptor), the roles those of
    ``pocket_interactions``.  ``inter`` = ``weights`` . terms and ``score`` = inter / (1 + ``rot_weight`` n_rot); a rotatable bond has
    order 1, lies in no ring and has two bonded heavy atoms at each end (amides and bonds next to a triple bond are not excluded: a
    convention).  This runs ``td_bond_graph`` and ``td_ring_report`` for the rotors (``rotors=False``: none, score = inter), then
    ``td_score_report``.  This is NOT AutoDock Vina's number: no hydrogens are placed, the roles are a valence-deficit heuristic and
    there is no intramolecular term; it compares between runs of this tool, not with published tables.  Molecules of more than 512
    atoms are refused.  Returns a ``Score``."""
    pack, pocket, rotor_graph = _pose_inputs(protein_pos, protein_feat, pos, v, batch_ligand, ligand_ptr, atom_enc_mode, ligand_radii,
                                             protein_radii, hydrogens, rotors, device)
    r = capi.score_report(*pack, *pocket, cutoff, hetero_cutoff, *rotor_graph, check=not rotors)
    _, v, ligand_ptr, cz, _ = pack
    sizes = ligand_ptr.cpu().to(torch.int64).diff().tolist()
    return Score(r, ligand_ptr, _heavy_atoms(v.cpu().numpy(), cz, sizes), weights, rot_weight)


class ScoreReport(_PoseReport):
    """Per frame (axis 0), over the included molecules that the kernel scored (``n_included`` [S] of ``n_samples``; a molecule with
    n_pairs = -1 is excluded everywhere): ``sum_inter`` [S] and ``sum_terms`` [S, 5] float64, the weighted terms; ``sum_rotors`` and
    ``sum_pairs`` [S] int64; ``n_no_pairs`` [S], the poses with no pair inside the cutoff; ``sum_efficiency`` [S] over the
    ``n_efficiency`` [S] molecules with heavy atoms; ``scores`` [S, B] float64 with ``scored`` [S, B] bool, the per-molecule values that
    the median and the best need (joined along the molecule axis by ``merged``).  With a reference ligand ``sum_ref`` [S, 2] -- per
    pocket the reference's score and the share of molecules with a score below it, the reference's "high affinity" -- over the
    ``n_ref`` [S] pockets that have them.  Not AutoDock Vina's number (``pocket_score``)."""

    FIELDS = (('n_included', 'i64'), ('sum_inter', 'f64'), ('sum_terms', 'f64'), ('sum_rotors', 'i64'), ('sum_pairs', 'i64'),
              ('n_no_pairs', 'i64'), ('sum_efficiency', 'f64'), ('n_efficiency', 'i64'), ('scores', 'per_mol'), ('scored', 'per_mol'),
              ('n_samples', 'int_sum'), ('sum_ref', 'ref_f64'), ('n_ref', 'ref_i64'))
    REF_KEYS = ('ref_score', 'better_than_ref')         # the known ligand's score and the share of molecules that score below it

    @classmethod
    def from_outputs(cls, raw, included, heavy, weights=SCORE_WEIGHTS, rot_weight=SCORE_ROT_WEIGHT, ref_score=None):
        """One pocket: ``raw`` the numpy outputs of capi.score_report (terms, n_pairs, n_rot), ``included`` [S, B] bool, ``heavy``
        [S, B] the heavy atoms; ``ref_score``: the known ligand's score or None"""
        n_pairs = np.asarray(raw['n_pairs'], dtype=np.int64)
        inc = np.asarray(included, dtype=bool) & (n_pairs >= 0)
        n_rot = np.zeros_like(n_pairs) if raw.get('n_rot') is None else np.asarray(raw['n_rot'], dtype=np.int64)
        terms, inter, score = score_energies(np.where(inc[..., None], raw['terms'], 0), np.where(inc, n_rot, 0), weights, rot_weight)
        heavy = np.asarray(heavy, dtype=np.int64)
        has = inc & (heavy > 0)
        eff = np.divide(score, heavy, out=np.zeros(score.shape), where=has)
        tot = lambda x: np.where(inc, x, 0).sum(1)
        return cls(inc.sum(1), tot(inter), np.where(inc[..., None], terms * np.asarray(weights, dtype=np.float64), 0.0).sum(1), tot(n_rot),
                   tot(n_pairs), (inc & (n_pairs == 0)).sum(1), np.where(has, eff, 0.0).sum(1), has.sum(1), np.where(inc, score, np.nan), inc,
                   inc.shape[1], *_reference_rows(inc, score, None if ref_score is None else (ref_score,)))

    def _of(self, frame):
        return self.scores[frame][self.scored[frame]]

    def summary(self, frame=-1):
        n = self.n_included[frame]
        return dict(mean_score=self.mean_score(frame), median_score=self.median_score(frame), best_score=self.best_score(frame),
                    share_negative=self.share_negative(frame), mean_inter=self._mean(self.sum_inter[frame], n),
                    **{f'mean_{name}': self._mean(self.sum_terms[frame, t], n) for t, name in enumerate(SCORE_TERM_NAMES)},
                    mean_rotors=self._mean(self.sum_rotors[frame], n), mean_efficiency=self._mean(self.sum_efficiency[frame], self.n_efficiency[frame]),
                    mean_pairs=self._mean(self.sum_pairs[frame], n), no_pairs=self._mean(self.n_no_pairs[frame], n), **self.reference(frame))


def sample_score(result, eval_step=-1, include='all', reference_ligand=None, weights=SCORE_WEIGHTS, rot_weight=SCORE_ROT_WEIGHT,
                 cutoff=SCORE_CUTOFF, atom_enc_mode='add_aromatic', device='cuda'):
    """The docking-style score of the samples of one pocket (``result`` a loaded ``result_{i}.pt`` dictionary, whose ``'data'`` is the
    pocket; ``eval_step`` and the packing as ``sample_quality``): per frame the mean, the median and the best score, the share of
    negative scores, the weighted terms, the rotatable bonds, the score per heavy atom and the poses with no pair inside the cutoff;
    with ``reference_ligand`` ``(pos [n, 3], v [n])``, run through the same kernel, its score and the share of samples that score
    below it (the reference's "high affinity").  ``include`` as ``sample_rings``.  A Vina-style score on this project's heuristic
    typing, NOT AutoDock Vina's number (``pocket_score``): comparable between runs of this tool, not with published tables.  A result
    without a pocket is refused.  Returns a ``ScoreReport``."""
    return SamplePack(result, eval_step, atom_enc_mode, device).score(_pocket_data(result, 'score'), include, reference_ligand, weights,
                                                                      rot_weight, cutoff)


# ---- pose relaxation (``td_score_minimize``, csrc/relax.hip; DESIGN.md section 3, "Pose relaxation")
# The pose of every molecule after a local optimisation of ``inter`` over rigid motions, by one persistent workgroup per molecule: the
# reference's ``vina_score`` / ``vina_min`` pair on this project's typing.  It is a local optimisation under this project's heuristic
# score, not AutoDock Vina's ``minimize``, and it is rigid-body only: three translations and three rotations, no torsions.  No global
# search (``vina_dock``), no intramolecular term, no hydrogens.
RELAX_MAX_STEPS, RELAX_MAX_SHIFT = capi.RELAX_MAX_STEPS, capi.RELAX_MAX_SHIFT


def _moved(pos_in, pos_out, sizes):
    """[S, B] float64: per molecule the RMSD between two sets of coordinates [S, N_l, 3] (numpy), 0 for an empty molecule"""
    d2 = ((np.asarray(pos_out, dtype=np.float64) - np.asarray(pos_in, dtype=np.float64)) ** 2).sum(-1)
    ptr = np.cumsum([0] + [int(n) for n in sizes])
    run = np.concatenate([np.zeros((d2.shape[0], 1)), np.cumsum(d2, axis=1)], axis=1)
    n = np.asarray(sizes, dtype=np.float64)[None, :]
    return np.sqrt(np.divide(run[:, ptr[1:]] - run[:, ptr[:-1]], n, out=np.zeros((d2.shape[0], len(sizes))), where=n > 0))


def _relax_scores(raw, weights, rot_weight):
    """(bad [S, B], score before, score after, the shift of the centre) of the numpy outputs of capi.score_minimize; the rotatable
    bonds are the input pose's for both scores"""
    bad = np.asarray(raw['status']) < 0
    n_rot = None if raw.get('n_rot') is None else np.where(bad, 0, raw['n_rot'])
    before = score_energies(np.where(bad[..., None], 0, raw['terms_in']), n_rot, weights, rot_weight)[2]
    after = score_energies(np.where(bad[..., None], 0, raw['terms']), n_rot, weights, rot_weight)[2]
    return bad, before, after, np.sqrt((np.asarray(raw['transform'], dtype=np.float64)[..., 4:] ** 2).sum(-1))


_SCORES_RAW = ('terms_in', 'terms', 'n_rot', 'status', 'transform')         # what _relax_scores reads
_RELAXED_RAW = ('terms_in', 'terms', 'n_pairs', 'n_steps', 'n_evals', 'status', 'transform')


class _Pose:
    """what ``Relaxed`` and ``Docked`` share: the conversion of the raw outputs of capi.score_minimize / score_dock"""

    def _take(self, r, pos_in, ligand_ptr, more):
        """Sets ``pos``, ``protein_role`` and ``ligand_ptr``, as numpy ``raw_terms_in`` / ``raw_terms``, the rest of ``_RELAXED_RAW``, the
        keys ``more`` and ``n_rot`` under their own names, and ``rmsd``.  Returns the numpy outputs as a dict."""
        self.pos, self.protein_role, self.ligand_ptr = r['pos'], r['protein_role'], ligand_ptr
        raw = _numpy(r, _RELAXED_RAW + more + ('n_rot',))
        self.raw_terms_in, self.raw_terms = raw['terms_in'], raw['terms']
        for k in tuple(raw)[2:]:
            setattr(self, k, raw[k])
        self.rmsd = _moved(pos_in.cpu().numpy(), self.pos.cpu().numpy(), ligand_ptr.cpu().to(torch.int64).diff().tolist())
        return raw


class Relaxed(_Pose):
    """The rigid-body relaxation of S frames of B molecules in one pocket (``pocket_relax``).  ``pos`` [S, N_l, 3] fp32 on the device,
    the relaxed poses; numpy, frame axis first: ``raw_terms_in`` / ``raw_terms`` [S, B, 5] int64 (the kernel's integers at the input and
    at the relaxed pose), ``n_pairs``, ``n_steps``, ``n_evals``, ``status`` [S, B] int32 (bits ``capi.RELAX_CONVERGED``,
    ``RELAX_OUT_OF_BUDGET``, ``RELAX_AT_CAP``), ``n_rot`` [S, B] int32 of the input pose or None, ``transform`` [S, B, 7] float64 (unit
    quaternion, shift of the centre), ``grad_in`` [S, B, 6] int64, and ``score_in`` / ``score`` [S, B] float64 = inter / (1 + rot_weight
    n_rot) before and after, ``rmsd`` [S, B] the RMSD moved over all atoms and ``shift`` [S, B] the shift of the centre.  A molecule the
    kernel refused (status -1) has NaN scores.  A local optimisation under this
    project's heuristic score, not AutoDock Vina's ``minimize``; rigid-body only: three translations and three rotations, no torsions
    (``pocket_relax``)."""

    def __init__(self, r, pos_in, ligand_ptr, weights, rot_weight):
        raw = self._take(r, pos_in, ligand_ptr, ('grad_in',))
        bad, self.score_in, self.score, self.shift = _relax_scores(raw, weights, rot_weight)
        self.score_in[bad], self.score[bad] = np.nan, np.nan


def pocket_relax(protein_pos, protein_feat, pos, v, batch_ligand=None, ligand_ptr=None, atom_enc_mode='add_aromatic', weights=SCORE_WEIGHTS,
                 rot_weight=SCORE_ROT_WEIGHT, cutoff=SCORE_CUTOFF, hetero_cutoff=DEFAULT_HETERO_CUTOFF, max_steps=RELAX_MAX_STEPS,
                 max_evals=None, max_shift=RELAX_MAX_SHIFT, ligand_radii=None, protein_radii=None, hydrogens=False, rotors=True, device=None):
    """The pose of every molecule of one frame ``[N_l, 3]`` or of a stack ``[S, N_l, 3]`` (arguments as ``pocket_score``) after a local
    optimisation of ``inter`` = ``weights`` . terms of ``pocket_score`` over rigid motions of the molecule in the pocket: BFGS with a
    backtracking line search on three translations and three rotations, at most ``max_steps`` accepted steps and ``max_evals``
    evaluations (None: 4 max_steps + 1), the centre never more than ``max_shift`` Angstrom from where it was; one persistent workgroup
    per molecule (``td_score_minimize``), with the roles and the rotatable bonds of the input pose.  It is a local optimisation under this
    project's heuristic score, not AutoDock Vina's ``minimize``, and it is rigid-body only: three translations and three rotations, no
    torsions; no global search, no intramolecular term, no hydrogens.  Returns a ``Relaxed``."""
    pack, pocket, rotor_graph = _pose_inputs(protein_pos, protein_feat, pos, v, batch_ligand, ligand_ptr, atom_enc_mode, ligand_radii,
                                             protein_radii, hydrogens, rotors, device)
    r = capi.score_minimize(*pack, *pocket, weights, cutoff, hetero_cutoff, *rotor_graph, max_steps, max_evals, max_shift, check=not rotors)
    return Relaxed(r, pack[0], pack[2], weights, rot_weight)


class RelaxReport(_PoseReport):
    """Per frame (axis 0), over the included molecules that the kernel relaxed (``n_included`` [S] of ``n_samples``; a molecule with
    status -1 is excluded everywhere): ``scores_in`` and ``scores`` [S, B] float64 with ``scored`` [S, B] bool, the per-molecule scores
    before and after (the reference's ``vina_score`` / ``vina_min`` pair on this typing; joined along the molecule axis by ``merged``);
    ``sum_rmsd`` and ``sum_shift`` [S] float64, the RMSD moved and the shift of the centre; ``n_converged``, ``n_out_of_budget``,
    ``n_at_cap`` [S], the molecules with each status bit; ``sum_steps``, ``sum_evals`` [S] int64.  With a reference ligand relaxed through
    the same kernel ``sum_ref`` [S, 3] -- per pocket its score before and after and the share of molecules whose minimised score is
    below its minimised score -- over the ``n_ref`` [S] pockets that have them.  A local optimisation under this
    project's heuristic score, not AutoDock Vina's ``minimize``; rigid-body only: three translations and three rotations, no torsions
    (``pocket_relax``)."""

    FIELDS = (('n_included', 'i64'), ('scores_in', 'per_mol'), ('scores', 'per_mol'), ('scored', 'per_mol'), ('sum_rmsd', 'f64'),
              ('sum_shift', 'f64'), ('n_converged', 'i64'), ('n_out_of_budget', 'i64'), ('n_at_cap', 'i64'), ('sum_steps', 'i64'),
              ('sum_evals', 'i64'), ('n_samples', 'int_sum'), ('sum_ref', 'ref_f64'), ('n_ref', 'ref_i64'))
    # the known ligand's score before and after its own relaxation and the share of molecules whose minimised score is below its
    # minimised score
    REF_KEYS = ('ref_score', 'ref_score_min', 'better_than_ref_min')

    @classmethod
    def from_outputs(cls, raw, included, pos_in, sizes, weights=SCORE_WEIGHTS, rot_weight=SCORE_ROT_WEIGHT, ref_scores=None):
        """One pocket: ``raw`` the numpy outputs of capi.score_minimize (pos, terms_in, terms, n_rot, n_steps, n_evals, status,
        transform), ``included`` [S, B] bool, ``pos_in`` [S, N_l, 3] the input poses, ``sizes`` the molecules' atom counts;
        ``ref_scores``: the known ligand's (score, minimised score) or None"""
        bad, before, after, shift = _relax_scores(raw, weights, rot_weight)
        inc = np.asarray(included, dtype=bool) & ~bad
        status = np.asarray(raw['status'], dtype=np.int64)
        rmsd = _moved(pos_in, raw['pos'], sizes)
        tot = lambda x: np.where(inc, x, 0).sum(1)
        return cls(inc.sum(1), np.where(inc, before, np.nan), np.where(inc, after, np.nan), inc, tot(rmsd), tot(shift),
                   tot((status & capi.RELAX_CONVERGED) != 0), tot((status & capi.RELAX_OUT_OF_BUDGET) != 0),
                   tot((status & capi.RELAX_AT_CAP) != 0), tot(np.asarray(raw['n_steps'], dtype=np.int64)),
                   tot(np.asarray(raw['n_evals'], dtype=np.int64)), inc.shape[1], *_reference_rows(inc, after, ref_scores))

    def _of(self, frame, after=True):
        return (self.scores if after else self.scores_in)[frame][self.scored[frame]]

    def mean_gain(self, frame=-1):
        """the mean of score before - score after"""
        return self._mean_of(self._of(frame, False) - self._of(frame, True))

    def summary(self, frame=-1):
        n = self.n_included[frame]
        return dict(mean_score=self.mean_score(frame, False), median_score=self.median_score(frame, False),
                    best_score=self.best_score(frame, False), mean_score_min=self.mean_score(frame), median_score_min=self.median_score(frame),
                    best_score_min=self.best_score(frame), mean_gain=self.mean_gain(frame), share_negative_min=self.share_negative(frame),
                    mean_rmsd=self._mean(self.sum_rmsd[frame], n), mean_shift=self._mean(self.sum_shift[frame], n),
                    converged=self._mean(self.n_converged[frame], n), out_of_budget=self._mean(self.n_out_of_budget[frame], n),
                    at_cap=self._mean(self.n_at_cap[frame], n), mean_steps=self._mean(self.sum_steps[frame], n),
                    mean_evals=self._mean(self.sum_evals[frame], n), **self.reference(frame))


def sample_relax(result, eval_step=-1, include='all', reference_ligand=None, weights=SCORE_WEIGHTS, rot_weight=SCORE_ROT_WEIGHT,
                 max_steps=RELAX_MAX_STEPS, max_shift=RELAX_MAX_SHIFT, cutoff=SCORE_CUTOFF, atom_enc_mode='add_aromatic', device='cuda'):
    """The rigid-body relaxation of the samples of one pocket (``result``, ``eval_step``, ``include`` and the packing as
    ``sample_score``): per frame the mean, the median and the best score before and after (the reference's ``vina_score`` / ``vina_min``
    pair, on this typing), the mean gain, the share of negative scores after, the mean RMSD moved and shift of the centre, the shares
    converged, out of budget and at the cap, the mean steps and evaluations; with ``reference_ligand`` ``(pos [n, 3], v [n])``, relaxed
    through the same kernel, its two scores and the share of samples whose minimised score is below its minimised score.  It is a local
    optimisation under this project's heuristic score, not AutoDock Vina's ``minimize``, and it is rigid-body only: three translations
    and three rotations, no torsions (``pocket_relax``).  A result without a pocket is refused.  Returns a ``RelaxReport``."""
    return SamplePack(result, eval_step, atom_enc_mode, device).relax(_pocket_data(result, 'relax'), include, reference_ligand, weights,
                                                                      max_steps, max_shift, cutoff, rot_weight)


# ---- docking search (``td_score_dock``, csrc/relax.hip; DESIGN.md section 3, "Docking search")
# The best pose that independent Monte-Carlo chains of mutate-and-relax rounds find for every molecule, one persistent workgroup per
# (molecule, chain): the reference's ``vina_dock`` next to ``vina_score`` and ``vina_min``, on this project's typing.  It is a rigid-body
# global search under this project's heuristic score, not AutoDock Vina's ``dock``: three translations and three rotations, no torsions.
# No intramolecular term, no hydrogens; the search box is the ball of ``max_shift`` around the input centroid.
DOCK_CHAINS, DOCK_ROUNDS, DOCK_AMPLITUDE, DOCK_TEMPERATURE = capi.DOCK_CHAINS, capi.DOCK_ROUNDS, capi.DOCK_AMPLITUDE, capi.DOCK_TEMPERATURE
DOCK_AGREE = 0.5                                      # a chain agrees with the winner when its best inter is within this of the winner's
_DOCK_RAW = ('pos', 'terms_in', 'terms', 'n_rot', 'n_steps', 'n_evals', 'status', 'transform', 'best_chain', 'chain_terms')


def _single_frame(eval_step, S=None):
    """the docking search takes one frame: refuse a stack, and say why"""
    if eval_step == 'all' or (S is not None and S != 1):
        raise ValueError("the docking search takes a single frame, not eval_step='all' or a stack: one launch would hold S B n_chains "
                         'long-lived workgroups')


def _dock_scores(raw, raw_min, weights, rot_weight):
    """(bad [S, B], score before, score after the relaxation, score after the search, the share of chains whose best inter is within
    DOCK_AGREE of the winner's) of the numpy outputs of capi.score_dock and, for the middle one, of capi.score_minimize"""
    bad, before, docked, _ = _relax_scores(raw, weights, rot_weight)
    minimised = _relax_scores(raw_min, weights, rot_weight)[2]
    inter = score_energies(np.where(bad[..., None, None], 0, raw['chain_terms']), None, weights, rot_weight)[1]        # [S, B, C]
    won = np.take_along_axis(inter, np.asarray(raw['best_chain'], dtype=np.int64)[..., None], -1)
    return bad, before, minimised, docked, (inter <= won + DOCK_AGREE).sum(-1) / float(inter.shape[-1])


class Docked(_Pose):
    """The docking search of one frame of B molecules in one pocket (``pocket_dock``).  ``pos`` [1, N_l, 3] fp32 on the device, the
    docked poses; numpy, frame axis first: ``raw_terms_in`` / ``raw_terms`` [1, B, 5] int64 (the kernel's integers at the input and at
    the docked pose), ``n_pairs``, ``n_steps``, ``n_evals`` (summed over the chains), ``status`` [1, B] int32, ``n_rot`` [1, B] int32 of
    the input pose or None, ``transform`` [1, B, 7] float64, ``best_chain`` [1, B] int32, ``chain_terms`` [1, B, C, 5] int64,
    ``chain_transform`` [1, B, C, 7], ``chain_accepts``, ``chain_evals`` [1, B, C] int32, and ``score_in`` / ``score_min`` / ``score``
    [1, B] float64 = inter / (1 + rot_weight n_rot) of the input pose, after the relaxation alone and after the search, ``rmsd`` [1, B]
    the RMSD moved over all atoms, ``agree`` [1, B] the share of chains whose best inter is within ``DOCK_AGREE`` of the winner's.  A
    molecule the kernel refused (status -1) has NaN scores.  A rigid-body global search under this project's heuristic score, not
    AutoDock Vina's ``dock``: three translations and three rotations, no torsions (``pocket_dock``)."""

    def __init__(self, r, r_min, pos_in, ligand_ptr, weights, rot_weight):
        raw = self._take(r, pos_in, ligand_ptr, ('best_chain', 'chain_terms', 'chain_transform', 'chain_accepts', 'chain_evals'))
        self.draws = r.get('draws')
        bad, self.score_in, self.score_min, self.score, self.agree = _dock_scores(raw, _numpy(r_min, _SCORES_RAW), weights, rot_weight)
        for x in (self.score_in, self.score_min, self.score):
            x[bad] = np.nan


def pocket_dock(protein_pos, protein_feat, pos, v, batch_ligand=None, ligand_ptr=None, atom_enc_mode='add_aromatic', weights=SCORE_WEIGHTS,
                rot_weight=SCORE_ROT_WEIGHT, cutoff=SCORE_CUTOFF, hetero_cutoff=DEFAULT_HETERO_CUTOFF, n_chains=DOCK_CHAINS, n_rounds=DOCK_ROUNDS,
                amplitude=DOCK_AMPLITUDE, temperature=DOCK_TEMPERATURE, seed=0, draws=None, max_steps=RELAX_MAX_STEPS, max_evals=None,
                max_shift=RELAX_MAX_SHIFT, ligand_radii=None, protein_radii=None, hydrogens=False, rotors=True, device=None):
    """The best pose of every molecule of ONE frame ``[N_l, 3]`` (arguments as ``pocket_relax``; a stack is refused: one launch would
    hold S B n_chains long-lived workgroups) that ``n_chains`` independent Monte-Carlo chains of ``n_rounds`` + 1 rounds find: each round
    a random rigid move (up to ``amplitude`` Angstrom per axis and a turn to match) followed by ``pocket_relax``'s local optimisation
    (``max_steps`` and ``max_evals`` per round), accepted by a Metropolis rule at ``temperature``; chain 0 starts with the plain
    relaxation, so the result is never worse than ``pocket_relax``'s.  One persistent workgroup per (molecule, chain)
    (``td_score_dock``); the uniforms are ``draws`` or torch.rand seeded by ``seed``.  It is a rigid-body global search under this project's
    heuristic score, not AutoDock Vina's ``dock``: three translations and three rotations, no torsions.  No intramolecular term, no
    hydrogens; the search box is the ball of ``max_shift`` around the input centroid.  Returns a ``Docked``."""
    pack, pocket, rotor_graph = _pose_inputs(protein_pos, protein_feat, pos, v, batch_ligand, ligand_ptr, atom_enc_mode, ligand_radii,
                                             protein_radii, hydrogens, rotors, device, single_frame=True)
    args = (*pack, *pocket, weights, cutoff, hetero_cutoff, *rotor_graph, max_steps, max_evals, max_shift)
    r_min = capi.score_minimize(*args, check=not rotors)
    r = capi.score_dock(*args, n_chains, n_rounds, amplitude, temperature, seed, draws, check=not rotors)
    return Docked(r, r_min, pack[0], pack[2], weights, rot_weight)


class DockReport(_PoseReport):
    """Per frame (axis 0; the search takes one frame), over the included molecules that the kernel searched (``n_included`` [S] of
    ``n_samples``; a molecule with status -1 is excluded everywhere): ``scores_in``, ``scores_min`` and ``scores`` [S, B] float64 with
    ``scored`` [S, B] bool, the per-molecule scores of the input pose, after the relaxation alone and after the search (the reference's
    ``vina_score`` / ``vina_min`` / ``vina_dock`` on this typing; joined along the molecule axis by ``merged``); ``sum_rmsd`` [S] the RMSD
    from the input; ``sum_agree`` [S] the share of chains whose best inter is within ``DOCK_AGREE`` of the winner's, a convergence
    indicator; ``sum_evals`` [S] int64.  With a reference ligand run through the same kernel ``sum_ref`` [S, 2] -- per pocket its docked
    score and the share of molecules whose docked score is below it -- over the ``n_ref`` [S] pockets that have them.  A rigid-body global
    search under this project's heuristic score, not AutoDock Vina's ``dock``: three translations and three rotations, no torsions
    (``pocket_dock``)."""

    FIELDS = (('n_included', 'i64'), ('scores_in', 'per_mol'), ('scores_min', 'per_mol'), ('scores', 'per_mol'), ('scored', 'per_mol'),
              ('sum_rmsd', 'f64'), ('sum_agree', 'f64'), ('sum_evals', 'i64'), ('n_samples', 'int_sum'), ('sum_ref', 'ref_f64'), ('n_ref', 'ref_i64'))
    # the known ligand's score after its own search and the share of molecules whose docked score is below it
    REF_KEYS = ('ref_score_dock', 'better_than_ref_dock')

    @classmethod
    def from_outputs(cls, raw, raw_min, included, pos_in, sizes, weights=SCORE_WEIGHTS, rot_weight=SCORE_ROT_WEIGHT, ref_score=None):
        """One pocket: ``raw`` the numpy outputs of capi.score_dock (pos, terms_in, terms, n_rot, n_evals, status, transform, best_chain,
        chain_terms), ``raw_min`` those of capi.score_minimize on the same pack (terms_in, terms, n_rot, status, transform), ``included``
        [S, B] bool, ``pos_in`` [S, N_l, 3] the input poses, ``sizes`` the molecules' atom counts; ``ref_score``: the known ligand's docked
        score or None"""
        bad, before, minimised, docked, agree = _dock_scores(raw, raw_min, weights, rot_weight)
        inc = np.asarray(included, dtype=bool) & ~bad
        rmsd = _moved(pos_in, raw['pos'], sizes)
        tot = lambda x: np.where(inc, x, 0).sum(1)
        return cls(inc.sum(1), np.where(inc, before, np.nan), np.where(inc, minimised, np.nan), np.where(inc, docked, np.nan), inc, tot(rmsd),
                   tot(agree), tot(np.asarray(raw['n_evals'], dtype=np.int64)), inc.shape[1],
                   *_reference_rows(inc, docked, None if ref_score is None else (ref_score,)))

    def _of(self, frame, which='dock'):
        return {'in': self.scores_in, 'min': self.scores_min, 'dock': self.scores}[which][frame][self.scored[frame]]

    def mean_gain(self, frame=-1):
        """the mean of score after the relaxation alone - score after the search"""
        return self._mean_of(self._of(frame, 'min') - self._of(frame, 'dock'))

    def summary(self, frame=-1):
        n = self.n_included[frame]
        out = {}
        for which, tag in (('in', ''), ('min', '_min'), ('dock', '_dock')):
            out.update({f'mean_score{tag}': self.mean_score(frame, which), f'median_score{tag}': self.median_score(frame, which),
                        f'best_score{tag}': self.best_score(frame, which)})
        return dict(out, mean_gain_dock=self.mean_gain(frame), share_negative_dock=self.share_negative(frame),
                    mean_rmsd_dock=self._mean(self.sum_rmsd[frame], n), chains_agree=self._mean(self.sum_agree[frame], n),
                    mean_evals_dock=self._mean(self.sum_evals[frame], n), **self.reference(frame))


def sample_dock(result, eval_step=-1, include='all', reference_ligand=None, weights=SCORE_WEIGHTS, rot_weight=SCORE_ROT_WEIGHT,
                n_chains=DOCK_CHAINS, n_rounds=DOCK_ROUNDS, seed=0, max_steps=RELAX_MAX_STEPS, max_shift=RELAX_MAX_SHIFT, cutoff=SCORE_CUTOFF,
                atom_enc_mode='add_aromatic', device='cuda'):
    """The docking search of the samples of one pocket at ONE frame (``result``, ``include`` and the packing as ``sample_relax``;
    ``eval_step='all'`` raises ValueError: one launch would hold S B n_chains long-lived workgroups): the mean, the median and the best
    score of the input poses, after the relaxation alone and after the search (the reference's ``vina_score`` / ``vina_min`` /
    ``vina_dock``, on this typing), the mean gain over the relaxation, the share of negative docked scores, the mean RMSD from the input,
    the mean share of chains that agree with the winner (a convergence indicator), the mean evaluations; with ``reference_ligand``
    ``(pos [n, 3], v [n])``, run through the same kernel, its docked score and the share of samples whose docked score is below it.  It
    is a rigid-body global search under this project's heuristic score, not AutoDock Vina's ``dock``: three translations and three
    rotations, no torsions (``pocket_dock``).  A result without a pocket is refused.  Returns a ``DockReport``."""
    _single_frame(eval_step)
    return SamplePack(result, eval_step, atom_enc_mode, device).dock(_pocket_data(result, 'dock'), include, reference_ligand, weights, n_chains,
                                                                     n_rounds, seed, max_steps, max_shift, cutoff, rot_weight)


# ---- solvent-accessible surface (``td_sasa_report``, csrc/sasa.hip; DESIGN.md section 3, "Solvent-accessible surface")
# Shrake-Rupley point counting: every atom carries ``SASA_POINTS`` test points on the sphere of its van der Waals radius plus the probe
# radius, and a point is exposed when no other such sphere holds it.  The kernel counts points; the areas are formed here, in float64,
# as 4 pi R^2 n / P per element.  Conventions and limits: Bondi-type radii on heavy atoms with no united-atom correction, so the areas
# compare between runs of this tool and not with published tables; a stored pocket is a cut-out whose rim is exposed only because the
# rest of the protein is missing, so of the pocket only the **buried** area is reported (the apo-exposed counts are a raw output); at 96
# points one point is about 1 % of a sphere.
SASA_PROBE = 1.4
SASA_POINTS = 96
SASA_POLAR = (2, 3)                                   # N and O: their index is the same over H C N O F P S Cl and over H C N O S Se


def sasa_directions(points=SASA_POINTS):
    """[P, 3] float64 unit vectors on the golden-section spiral: z_k = 1 - (2 k + 1) / P, r = sqrt(1 - z^2), phi = k pi (3 - sqrt 5).
    The only trigonometry of the report: the kernel and its restatement both read these bits."""
    P = int(points)
    if not 1 <= P <= capi.SASA_MAX_POINTS:
        raise ValueError(f'1 .. {capi.SASA_MAX_POINTS} points per sphere (got {points})')
    k = np.arange(P, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / np.float64(P)
    r = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def sasa_reaches(probe=SASA_PROBE, radii=None):
    """([8], [6]) float64: the expanded radius ``r + probe`` of the ligand's elements H C N O F P S Cl and of the protein's H C N O S Se,
    with geometry's van der Waals radii and Se 1.90 A; ``radii``: {atomic number: radius in Angstrom} to change some"""
    from . import workloads
    r = _radii(POCKET_RADII, radii)
    if not (np.isfinite(float(probe)) and float(probe) >= 0.0):
        raise ValueError(f'the probe radius is finite and >= 0 (got {probe})')
    rl = np.asarray([r[z] for z in ELEMENTS], dtype=np.float64) + np.float64(probe)
    rp = np.asarray([r[z] for z in workloads.PROTEIN_ELEMENTS], dtype=np.float64) + np.float64(probe)
    if not ((rl > 0.0).all() and (rp > 0.0).all()):
        raise ValueError('every radius plus the probe must be > 0')
    return rl, rp


def sasa_areas(counts, reach, points):
    """[..., 3] float64 (total, polar, apolar) in square Angstrom of point counts [..., E] by element: 4 pi R_e^2 n_e / P each, N and O
    polar, every other element apolar"""
    reach = np.asarray(reach, dtype=np.float64)
    a = np.asarray(counts, dtype=np.float64) * ((4.0 * np.pi) * reach * reach / np.float64(points))
    polar = np.zeros(len(reach), bool)
    polar[list(SASA_POLAR)] = True
    return np.stack([a.sum(-1), a[..., polar].sum(-1), a[..., ~polar].sum(-1)], axis=-1)


def _buried_share(free_area, buried_area):
    """buried / free, 0 where nothing is free"""
    return np.divide(buried_area, free_area, out=np.zeros_like(free_area), where=free_area > 0)


class Sasa:
    """The surface of S frames of B molecules, alone and in one pocket (``pocket_sasa``).  Device tensors, frame axis first: ``free``,
    ``bound`` [S, B, 8] int32 (exposed points by ligand element H C N O F P S Cl), ``pocket_buried`` [S, B, 6] int32 (apo-exposed pocket
    points the molecule covers, by protein element), ``atom_free`` / ``atom_bound`` [S, N_l] int32, ``bits`` [S, B, W] int64 or None
    (bit j & 63 of word j >> 6: the molecule buries a point of protein atom j), ``pocket_free`` [N_p] int32 and ``pocket_mask`` [N_p, 4]
    int64 (the pocket alone; at a cut-out's rim an artefact), ``pocket_buried_sum`` [S, N_p] int64 over the included molecules.
    Areas in square Angstrom, float64 [S, B]: ``free_area``, ``bound_area``, ``buried_area`` = free - bound, ``pocket_buried_area``,
    and ``buried_share`` = buried / free (0 where nothing is free).  ``ligand_reach``, ``protein_reach``, ``points``, ``protein_elem``,
    ``ligand_ptr``."""

    def __init__(self, r, ligand_ptr, protein_elem, ligand_reach, protein_reach, points):
        for k, t in r.items():
            setattr(self, k, t)
        self.ligand_ptr, self.protein_elem, self.points = ligand_ptr, protein_elem, int(points)
        self.ligand_reach, self.protein_reach = ligand_reach, protein_reach
        free, bound = r['free'].cpu().numpy().astype(np.int64), r['bound'].cpu().numpy().astype(np.int64)
        dev = r['free'].device
        area = lambda counts, reach: sasa_areas(counts, reach, points)[..., 0]
        fa, ba, bu = area(free, ligand_reach), area(bound, ligand_reach), area(free - bound, ligand_reach)
        self.free_area, self.bound_area, self.buried_area = (torch.from_numpy(x).to(dev) for x in (fa, ba, bu))
        self.pocket_buried_area = torch.from_numpy(area(r['pocket_buried'].cpu().numpy(), protein_reach)).to(dev)
        self.buried_share = torch.from_numpy(_buried_share(fa, bu)).to(dev)


def pocket_sasa(protein_pos, protein_feat, pos, v, batch_ligand=None, ligand_ptr=None, atom_enc_mode='add_aromatic', probe=SASA_PROBE,
                points=SASA_POINTS, radii=None, hydrogens=False, include=None, return_bits=False, device=None):
    """Solvent-accessible surface of every molecule of one frame ``[N_l, 3]`` or of a stack ``[S, N_l, 3]`` (arguments as
    ``bond_graph``), alone and inside the pocket ``protein_pos`` [N_p, 3], ``protein_feat`` [N_p, 27], both in the frame of ``pos``.
    ``probe``: the probe radius (default 1.4 A, water); ``points``: test points per sphere (default 96, 1 .. 256); ``radii`` as
    ``sasa_reaches``.  Protein hydrogens take no part unless ``hydrogens`` (``pocket_kinds``).  ``include`` [S, B] restricts
    ``pocket_buried_sum`` and nothing else.  Molecules of more than 512 atoms and coordinates beyond 1e5 A are refused.  Returns a
    ``Sasa`` (the frame axis is kept)."""
    pos, v, ligand_ptr = _pack(pos, v, batch_ligand, ligand_ptr, device)
    side = PocketSide((protein_pos, protein_feat), pos.device)
    elem = side.kinds('element', hydrogens)[0]
    include = _frame_mask(include, pos)
    lr, pr = sasa_reaches(probe, radii)
    dirs = torch.from_numpy(sasa_directions(points)).to(pos.device)
    r = capi.sasa_report(pos, v, ligand_ptr, class_atomic_numbers(atom_enc_mode), side.pos, elem, lr, pr, dirs, include, True, return_bits)
    return Sasa(r, ligand_ptr, elem, lr, pr, points)


class SasaReport(_SumReport):
    """Per frame (axis 0), over the included molecules (``n_included`` [S] of ``n_samples``), areas in square Angstrom: ``sum_free``,
    ``sum_bound``, ``sum_buried`` [S, 3] float64, the ligands' surface alone, in the pocket and their difference, each as (total, polar,
    apolar; polar is N and O); ``sum_share`` [S], the sum of buried / free (0 for a molecule with nothing free); ``n_nothing`` [S], the
    molecules of whose surface the pocket covers no point; ``sum_pocket`` [S, 3], the pocket's apo-exposed surface the ligands cover;
    ``pocket_buried_sum`` [S, N_p] int64, the covered points per protein atom, or None for a report merged from several pockets.  With
    a reference ligand ``sum_own`` [S, 5] -- its own free, bound and buried area, buried share and covered pocket area, from the same
    kernel -- and ``sum_ref`` [S, 4] -- the mean, the median and the largest recovery of the protein atoms it buries and the mean
    Tanimoto, as ``PocketReport`` forms them for contacts -- over the ``n_own`` / ``n_ref`` [S] pockets that have them.  The radii, the
    probe and the point count are conventions (``pocket_sasa``); of the pocket only buried area is reported."""

    FIELDS = (('n_included', 'i64'), ('sum_free', 'f64'), ('sum_bound', 'f64'), ('sum_buried', 'f64'), ('sum_share', 'f64'), ('n_nothing', 'i64'),
              ('sum_pocket', 'f64'), ('n_samples', 'int_sum'), ('points', 'int_carried'), ('probe', 'value'), ('pocket_buried_sum', 'map'), ('sum_own', 'ref_f64'),
              ('n_own', 'ref_i64'), ('sum_ref', 'ref_f64'), ('n_ref', 'ref_i64'))
    OPTIONAL = 6
    MISMATCH = 'reports of different frame counts, point counts or probes, or with and without a reference ligand, do not merge'

    def _merge_key(self):
        return self.sum_free.shape, self.points, self.probe, self.sum_ref is None

    @classmethod
    def from_outputs(cls, raw, included, ligand_reach, protein_reach, points, probe=None, ref=None):
        """One pocket: ``raw`` the numpy outputs of capi.sasa_report (free, bound, pocket_buried, pocket_buried_sum and, with a
        reference, bits), ``included`` [S, B] bool; ``ref``: the same outputs of the reference ligand's own call, one frame of one
        molecule (free [8], bound [8], pocket_buried [6], bits [W])"""
        inc = np.asarray(included, dtype=bool)
        S, B = inc.shape
        free, bound = np.asarray(raw['free'], dtype=np.int64), np.asarray(raw['bound'], dtype=np.int64)
        fa, ba, bu = (sasa_areas(x, ligand_reach, points) for x in (free, bound, free - bound))
        pa = sasa_areas(raw['pocket_buried'], protein_reach, points)
        share = _buried_share(fa[..., 0], bu[..., 0])
        tot = lambda a: np.where(inc[..., None], a, 0.0).sum(1)
        sum_own = n_own = sum_ref = n_ref = None
        if ref is not None:
            rf, rb = np.asarray(ref['free'], dtype=np.int64), np.asarray(ref['bound'], dtype=np.int64)
            own_f, own_b, own_u = (sasa_areas(x, ligand_reach, points)[0] for x in (rf, rb, rf - rb))
            own = (own_f, own_b, own_u, float(_buried_share(np.asarray([own_f]), np.asarray([own_u]))[0]),
                   sasa_areas(ref['pocket_buried'], protein_reach, points)[0])
            sum_own, n_own = np.tile(np.asarray(own, dtype=np.float64), (S, 1)), np.ones(S, np.int64)
            bits, rbits = np.asarray(raw['bits']), np.asarray(ref['bits'])
            sum_ref, n_ref = _reference_recovery(_popcount(bits & rbits[None, None]), _popcount(bits), int(_popcount(rbits)), inc)
        return cls(inc.sum(1), tot(fa), tot(ba), tot(bu), np.where(inc, share, 0.0).sum(1), (inc & ((free - bound).sum(-1) == 0)).sum(1),
                   tot(pa), B, points, probe, raw['pocket_buried_sum'], sum_own, n_own, sum_ref, n_ref)

    def free_area(self, frame=-1, part=0):
        """mean surface of an included molecule alone; ``part`` 0 total, 1 polar, 2 apolar"""
        return self._mean(self.sum_free[frame, part], self.n_included[frame])

    def bound_area(self, frame=-1, part=0):
        """mean surface of an included molecule that stays exposed inside the pocket"""
        return self._mean(self.sum_bound[frame, part], self.n_included[frame])

    def buried_area(self, frame=-1, part=0):
        """mean surface of an included molecule that the pocket covers: free - bound"""
        return self._mean(self.sum_buried[frame, part], self.n_included[frame])

    def buried_share(self, frame=-1):
        """the mean of buried / free over the included molecules (0 for a molecule with nothing free)"""
        return self._mean(self.sum_share[frame], self.n_included[frame])

    def pocket_buried_area(self, frame=-1):
        """mean apo-exposed surface of the pocket that an included molecule covers"""
        return self._mean(self.sum_pocket[frame, 0], self.n_included[frame])

    def pocket_buried_polar_share(self, frame=-1):
        """the share of that covered pocket surface that belongs to N and O; nan when nothing is covered"""
        return float(self.sum_pocket[frame, 1]) / float(self.sum_pocket[frame, 0]) if self.sum_pocket[frame, 0] > 0 else float('nan')

    def buries_nothing(self, frame=-1):
        """the share of included molecules of whose surface the pocket covers no point: poses that left the pocket"""
        return self._mean(self.n_nothing[frame], self.n_included[frame])

    def pocket_map(self, frame=-1):
        """[N_p]: the covered points of each protein atom per included molecule; None for a report of several pockets"""
        if self.pocket_buried_sum is None:
            return None
        n = int(self.n_included[frame])
        return self.pocket_buried_sum[frame] / float(n) if n else np.full(self.pocket_buried_sum.shape[1], np.nan)

    def reference(self, frame=-1):
        """the known ligand's own numbers and the recovery of the protein atoms it buries, or {} without a reference ligand"""
        if self.sum_ref is None:
            return {}
        own = ('ref_sasa_free', 'ref_sasa_bound', 'ref_sasa_buried', 'ref_sasa_buried_share', 'ref_pocket_buried_area')
        keys = ('ref_recovery_mean', 'ref_recovery_median', 'ref_recovery_max', 'ref_tanimoto')
        return {**{k: self._mean(self.sum_own[frame, c], self.n_own[frame]) for c, k in enumerate(own)},
                **{k: self._mean(self.sum_ref[frame, c], self.n_ref[frame]) for c, k in enumerate(keys)}}

    def summary(self, frame=-1):
        out = dict(sasa_free=self.free_area(frame), sasa_bound=self.bound_area(frame), sasa_buried=self.buried_area(frame),
                   sasa_buried_share=self.buried_share(frame))
        for part, name in ((1, 'polar'), (2, 'apolar')):
            out.update({f'sasa_free_{name}': self.free_area(frame, part), f'sasa_bound_{name}': self.bound_area(frame, part),
                        f'sasa_buried_{name}': self.buried_area(frame, part)})
        out.update(pocket_buried_area=self.pocket_buried_area(frame), pocket_buried_polar_share=self.pocket_buried_polar_share(frame),
                   buries_nothing=self.buries_nothing(frame), **self.reference(frame))
        return out


def sample_sasa(result, eval_step=-1, include='all', reference_ligand=None, probe=SASA_PROBE, points=SASA_POINTS,
                atom_enc_mode='add_aromatic', device='cuda'):
    """Solvent-accessible surface of the samples of one pocket (``result`` a loaded ``result_{i}.pt`` dictionary, whose ``'data'`` is
    the pocket; ``eval_step`` and the packing as ``sample_quality``): per frame the mean surface of a molecule alone and in the pocket,
    the buried area and share with their polar (N, O) and apolar parts, the pocket surface the molecule covers and its polar share, and
    the share of poses the pocket does not cover at all; with ``reference_ligand`` ``(pos [n, 3], v [n])``, run through the same
    kernel, its own numbers and the recovery of the protein atoms it buries.  ``include`` as ``sample_rings``.  The radii, the probe
    and the point count are conventions (``pocket_sasa``).  A result without a pocket is refused.  Returns a ``SasaReport``."""
    return SamplePack(result, eval_step, atom_enc_mode, device).sasa(_pocket_data(result, 'sasa'), include, reference_ligand, probe, points)
