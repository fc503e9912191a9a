"""The chemistry-free half of the reference's scripts/evaluate_diffusion.py (:54-87, :150-174) on the GPU:

    python tools/evaluate_samples.py --sample_path DIR [--eval_step -1|all] [--atom_enc_mode add_aromatic] [--eval_num_examples N]

Reads the ``result_{i}.pt`` files a sampling driver wrote (tools/batch_sample.py, or the reference's scripts/sample_diffusion.py),
sorted as the reference sorts them, and prints under the reference's names: ``mol_stable`` and ``atm_stable``, the pair-distance
Jensen-Shannon distances ``JSD_CC_2A`` and ``JSD_All_12A`` and ``Atom type JS``.  The pair profiles and the atom types are taken over
``--include all`` samples (default), the ``stable`` ones or the ``complete`` ones (one fragment of the bond graph of
quality.bond_graph; the reference takes them over the molecules OpenBabel reconstructs in one piece).  ``--connectivity`` adds, from
that bond graph, ``complete``, ``mean_fragments``, ``mean_largest_share`` and the reference's eight bond-length Jensen-Shannon
distances (``JSD_6-6|1`` ...; ``--reference_npz`` may carry them as ``bond_types`` [8, 3] and ``bond_distributions`` [8, bins]).
``--rings`` adds the reference's ring ratios (evaluate_diffusion.py print_ring_ratio, ``ring size: k ratio: x.xxx`` for k = 3 .. 9)
from the ring sizes of quality.sample_rings -- the smallest cycle through some bond, not a toolkit's ring set -- over ``--include
all`` or ``complete`` samples, and the shares of molecules without a ring and with a ring of more than 9 atoms.  ``--diversity`` adds
``diversity`` (one minus the mean pairwise Tanimoto similarity of a pocket's samples, averaged over the pockets as the reference's
tables do), ``uniqueness`` (distinct molecules / samples) and ``mean_nearest`` from quality.sample_diversity, over ``--include all`` or
``complete`` samples, and with a known ligand -- ``--reference_sdf FILE`` (the first record, heavy atoms, elements of the table) or
arrays ``ligand_pos`` [n, 3] and ``ligand_v`` [n] in ``--reference_npz`` -- the mean, median and largest similarity of the samples to
it.  ``--geometry`` adds the local geometry of quality.sample_geometry over ``--include all`` or ``complete`` samples: the share of
molecules without an internal clash (a pair more than 3 bonds apart and closer than 0.7 times the sum of the van der Waals radii: this
project's own convention, not PoseBusters' bound and not a force field), the mean number of clashes, the crowded-atom and degenerate
counts, and per angle and torsion type the count, the mean angle and -- with ``--reference_sdf FILE``, of which every record then makes
up the reference (quality.geometry_reference: the same kernel, the same bond rule) -- the Jensen-Shannon distance.
``--pocket [--contact_cutoff X] [--clash_tolerance X]`` adds the contacts of the samples with their pocket (quality.sample_pocket; the
pocket is the file's ``data``), over ``--include all`` or ``complete`` samples: the share of molecules without a protein clash (a ligand
atom and a protein atom closer than the sum of their van der Waals radii minus 0.5 A), the mean numbers of clashes and of contacts
(pairs closer than 4 A), the buried share, the share of poses that touch nothing, the mean smallest distance, the share of contacts
with the backbone and the most frequent residue kinds -- conventions of this project, not a pose checker's -- and, with the known
ligand of ``--reference_sdf`` / ``--reference_npz``, how many of its contacts the samples recover.
``--interactions [--hbond_cutoff X] [--hydrophobic_cutoff X]`` adds the typed interactions with the pocket (quality.sample_interactions),
over ``--include all`` or ``complete`` samples: the mean hydrogen bonds per molecule (a ligand donor or acceptor and a protein acceptor
or donor closer than 3.5 A, heavy atom to heavy atom, no angle) with the donated / accepted split, the mean hydrophobic contacts
(hydrophobic atoms closer than 4.5 A), the share of molecules without a hydrogen bond, the share of polar ligand atoms in one and the
most frequent residue kinds per type -- the ligand's donors are inferred from the valence deficit, a heuristic of this project and not
perceived chemistry, and nothing here is a docking score (``--score`` is this tool's) -- and, with the known ligand, the recovery of
its interactions per type.
``--sasa [--probe 1.4] [--sasa_points 96]`` adds the solvent-accessible surface of the samples alone and in their pocket
(quality.sample_sasa: Shrake-Rupley point counts, areas in square Angstrom), over ``--include all`` or ``complete`` samples: the mean
free, bound and buried area of a molecule with the polar (N, O) and apolar parts, the buried share, the pocket surface a molecule
covers and its polar share, the share of poses the pocket does not cover at all and, with the known ligand, its own numbers and the
recovery of the protein atoms it buries.  Bondi-type radii on heavy atoms without a united-atom correction: the areas compare between
runs of this tool, not with published tables; the stored pocket is a cut-out, so of the pocket only buried area is reported; at 96
points one point is about 1 % of a sphere.
``--score [--score_cutoff 8.0]`` adds a docking-style score of the samples in their pocket (quality.sample_score), over ``--include all``
or ``complete`` samples: the mean, the median and the best score, the share of negative scores, the weighted terms (two Gaussians,
repulsion, hydrophobic, hydrogen bond) summed over the heavy-atom pairs closer than the cutoff, the mean rotatable bonds, the score per
heavy atom, the share of poses with no pair inside the cutoff and, with the known ligand run through the same kernel, its score and
the share of samples that score below it (the reference's "high affinity").  It is a Vina-style score on this project's heuristic typing
-- no hydrogens are placed, the roles come from valence deficits, there is no intramolecular term -- and NOT AutoDock Vina's number:
it compares between runs of this tool, not with published tables.  QED and SA are still not here.
``--minimize [--min_steps 64] [--max_shift 3.0]`` adds the same score after a rigid-body relaxation of every sample in its pocket
(quality.sample_relax: one persistent GPU workgroup per molecule, BFGS with a backtracking line search), alongside ``--score``: the
mean, the median and the best score before and after (the reference's ``vina_score`` / ``vina_min`` pair, on this typing), the mean
gain, the share of negative scores after, the mean RMSD moved and shift of the centre, the shares converged, out of budget and at
the cap, the mean steps and evaluations and, with the known ligand relaxed through the same kernel, its two scores and the share of
samples whose minimised score is below its minimised score.  It is a local optimisation under this project's heuristic score, not
AutoDock Vina's ``minimize``, and it is rigid-body only: three translations and three rotations, no torsions; no global search
(``vina_dock``), no intramolecular term, no hydrogens.
``--dock [--dock_chains 16] [--dock_rounds 16] [--dock_seed 0]`` adds the score after a docking search of every sample in its pocket
(quality.sample_dock: one persistent GPU workgroup per (molecule, chain); independent Monte-Carlo chains of random rigid moves, each
followed by ``--minimize``'s relaxation and a Metropolis rule), alongside ``--score``: the mean, the median and the best score of the
input poses, after the relaxation alone and after the search (the reference's ``vina_score`` / ``vina_min`` / ``vina_dock``, on this
typing), the mean gain over the relaxation, the share of negative docked scores, the mean RMSD from the input, the mean share of chains
that agree with the winner, the mean evaluations and, with the known ligand run through the same kernel, its docked score and the share
of samples whose docked score is below it.  The final poses only: ``--eval_step all`` is refused.  It is a rigid-body global search
under this project's heuristic score, not
AutoDock Vina's ``dock``: three translations and three rotations, no torsions; no intramolecular term, no hydrogens, and the search
box is the ball of ``--max_shift`` around the input centroid.
The fingerprint is this project's own circular one over its bond graph, not RDKit's RDKFingerprint: the numbers compare between
runs of this tool, not with published tables.  The Jensen-Shannon distances need the reference's empirical distributions: they are
loaded from ``utils.evaluation`` when the tool runs inside the reference repository (or with it on PYTHONPATH), or from
``--reference_npz FILE`` with arrays CC_2A, All_12A and atom_type (a file that holds a reference ligand may leave them out); without
them the three lines print None.

Writes ``DIR/eval_results/quality.json``: the numbers above, the raw histograms and element counts, and with ``--eval_step all`` the
per-frame curve (``curve``: one entry per frame of the trajectory).  With seeded random weights the numbers say nothing about chemistry.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from glob import glob

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from targetdiff_amd import molfile, quality  # noqa: E402


def result_files(sample_path, eval_num_examples=None):
    """scripts/evaluate_diffusion.py:55-58"""
    files = glob(os.path.join(sample_path, '*result_*.pt'))
    files = sorted(files, key=lambda x: int(os.path.basename(x)[:-3].split('_')[-1]))
    return files if eval_num_examples is None else files[:eval_num_examples]


def print_dict(d):
    """scripts/evaluate_diffusion.py:18-23"""
    for k, v in d.items():
        print(f'{k}:\t{v:.4f}' if v is not None else f'{k}:\tNone')


def nan_none(d):
    """a summary with None in the place of NaN, as JSON wants it"""
    return {k: (None if x != x else x) for k, x in d.items()}


METHODS = {'minimize': 'relax'}                       # the flags whose SamplePack method has another name


def pocket_sections(args):
    """The reports against the pocket that ``args`` asks for, as (flag -- also the name of the SamplePack method and of the JSON
    section, but for ``METHODS`` --, report class, the method's arguments after the reference ligand, extra JSON fields of the merged
    report)"""
    scoring = dict(weights=dict(zip(quality.SCORE_TERM_NAMES, quality.SCORE_WEIGHTS)), rot_weight=quality.SCORE_ROT_WEIGHT)
    every = (
        ('pocket', quality.PocketReport, (args.contact_cutoff, args.clash_tolerance),
         lambda r: dict(contact_cutoff=args.contact_cutoff, clash_tolerance=args.clash_tolerance, contact_profile=r.contact_profile(-1),
                        kind_hist=dict(zip(r.names, r.kind_hist[-1].sum(0).tolist())))),
        ('interactions', quality.InteractionReport, (args.hbond_cutoff, args.hydrophobic_cutoff),
         lambda r: dict(hbond_cutoff=args.hbond_cutoff, hydrophobic_cutoff=args.hydrophobic_cutoff,
                        kind_hist={t: dict(zip(r.names, r.kind_hist[-1, k].tolist())) for k, t in enumerate(quality.INTERACTION_NAMES)})),
        ('sasa', quality.SasaReport, (args.probe, args.sasa_points), lambda r: dict(probe=args.probe, points=args.sasa_points)),
        ('score', quality.ScoreReport, (None, None, args.score_cutoff),
         lambda r: dict(score_cutoff=args.score_cutoff, **scoring)),
        ('minimize', quality.RelaxReport, (None, args.min_steps, args.max_shift, args.score_cutoff),
         lambda r: dict(score_cutoff=args.score_cutoff, max_steps=args.min_steps, max_shift=args.max_shift, **scoring)),
        ('dock', quality.DockReport, (None, args.dock_chains, args.dock_rounds, args.dock_seed, args.min_steps, args.max_shift, args.score_cutoff),
         lambda r: dict(score_cutoff=args.score_cutoff, n_chains=args.dock_chains, n_rounds=args.dock_rounds, seed=args.dock_seed,
                        amplitude=quality.DOCK_AMPLITUDE, temperature=quality.DOCK_TEMPERATURE, max_steps=args.min_steps, max_shift=args.max_shift,
                        **scoring)))
    return [section for section in every if getattr(args, section[0])]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--sample_path', type=str, required=True)
    ap.add_argument('--eval_step', type=str, default='-1', help="a frame index (default -1: the final poses) or 'all'")
    ap.add_argument('--eval_num_examples', type=int, default=None)
    ap.add_argument('--atom_enc_mode', type=str, default='add_aromatic')
    ap.add_argument('--include', type=str, default='all', choices=['all', 'stable', 'complete'])
    ap.add_argument('--connectivity', action='store_true', help='also the bond graph: complete fraction, fragments, bond-length profiles')
    ap.add_argument('--rings', action='store_true', help='also the ring ratios: the share of molecules with a ring of 3 .. 9 atoms')
    ap.add_argument('--diversity', action='store_true', help='also diversity, uniqueness and the similarity to a reference ligand '
                    "(this project's circular fingerprint, not RDKit's)")
    ap.add_argument('--geometry', action='store_true', help='also bond angles, torsions and internal clashes (a convention of this '
                    'project, not a pose checker)')
    ap.add_argument('--pocket', action='store_true', help='also the contacts and clashes with the pocket (the result file\'s data; a '
                    'convention of this project, not a pose checker)')
    ap.add_argument('--contact_cutoff', type=float, default=quality.DEFAULT_CONTACT_CUTOFF, help='--pocket: a contact is a pair closer than this')
    ap.add_argument('--clash_tolerance', type=float, default=quality.DEFAULT_CLASH_TOLERANCE,
                    help='--pocket: a clash is a pair closer than the sum of the van der Waals radii minus this')
    ap.add_argument('--interactions', action='store_true', help='also the hydrogen bonds and hydrophobic contacts with the pocket (the '
                    "result file's data; counts under this project's role heuristic, not a score)")
    ap.add_argument('--hbond_cutoff', type=float, default=quality.DEFAULT_HBOND_CUTOFF,
                    help='--interactions: a hydrogen bond is a donor - acceptor pair of heavy atoms closer than this')
    ap.add_argument('--hydrophobic_cutoff', type=float, default=quality.DEFAULT_HYDROPHOBIC_CUTOFF,
                    help='--interactions: a hydrophobic contact is a pair of hydrophobic atoms closer than this')
    ap.add_argument('--sasa', action='store_true', help='also the solvent-accessible surface alone and in the pocket (the result '
                    "file's data; this project's radii, comparable between runs of this tool only)")
    ap.add_argument('--probe', type=float, default=quality.SASA_PROBE, help='--sasa: the probe radius in Angstrom')
    ap.add_argument('--sasa_points', type=int, default=quality.SASA_POINTS, help='--sasa: test points per sphere, 1 .. 256')
    ap.add_argument('--score', action='store_true', help="also a docking-style score of the samples in their pocket (the result file's "
                    "data): a Vina-style score on this project's heuristic typing, NOT AutoDock Vina's number -- comparable between runs "
                    'of this tool, not with published tables')
    ap.add_argument('--score_cutoff', type=float, default=quality.SCORE_CUTOFF, help='--score: a pair counts when it is closer than this')
    ap.add_argument('--minimize', action='store_true', help="also the score after a rigid-body relaxation of every sample in its pocket: a "
                    "local optimisation under this project's heuristic score, not AutoDock Vina's minimize; rigid-body only: three "
                    'translations and three rotations, no torsions')
    ap.add_argument('--min_steps', type=int, default=quality.RELAX_MAX_STEPS, help='--minimize: accepted steps at most')
    ap.add_argument('--max_shift', type=float, default=quality.RELAX_MAX_SHIFT, help='--minimize, --dock: the centre of a molecule moves at most '
                    'this far, in Angstrom')
    ap.add_argument('--dock', action='store_true', help="also the score after a docking search of every sample in its pocket: a rigid-body "
                    "global search under this project's heuristic score, not AutoDock Vina's dock: three translations and three rotations, "
                    'no torsions')
    ap.add_argument('--dock_chains', type=int, default=quality.DOCK_CHAINS, help='--dock: independent Monte-Carlo chains per molecule, 1 .. 64')
    ap.add_argument('--dock_rounds', type=int, default=quality.DOCK_ROUNDS, help='--dock: mutate-and-relax rounds per chain after the first, 0 .. 256')
    ap.add_argument('--dock_seed', type=int, default=0, help='--dock: the seed of the uniforms')
    ap.add_argument('--reference_sdf', type=str, default=None, help='--diversity, --pocket, --interactions, --sasa, --score, --minimize, --dock: a known ligand, the first V2000 record of '
                    'FILE; --geometry: known ligands, every record of FILE')
    ap.add_argument('--reference_npz', type=str, default=None)
    ap.add_argument('--device', type=str, default='cuda')
    args = ap.parse_args(argv)
    eval_step = 'all' if args.eval_step == 'all' else int(args.eval_step)

    reference = bond_reference = reference_ligand = geometry_reference = None
    if args.reference_sdf is not None:
        records = molfile.read_sdf(args.reference_sdf)
        mol = records[0]
        if args.geometry:
            geometry_reference = quality.geometry_reference(records, atom_enc_mode=args.atom_enc_mode, device=args.device)
        reference_ligand = molfile.ligand_classes(mol, args.atom_enc_mode, drop_unknown=True)
        if len(reference_ligand[1]) != len(mol['symbols']):
            print(f"reference ligand: {len(mol['symbols']) - len(reference_ligand[1])} atoms of elements outside the table left out")
    if args.reference_npz is not None:
        with np.load(args.reference_npz) as z:
            if 'ligand_pos' in z.files and reference_ligand is None:
                reference_ligand = (z['ligand_pos'].astype(np.float32), z['ligand_v'].astype(np.int64))
            if 'CC_2A' in z.files or 'ligand_pos' not in z.files:
                reference = {k: z[k] for k in ('CC_2A', 'All_12A', 'atom_type')}
            if 'bond_types' in z.files:
                bond_reference = {tuple(int(x) for x in t): d for t, d in zip(z['bond_types'], z['bond_distributions'])}
    files = result_files(args.sample_path, args.eval_num_examples)
    if not files:
        raise SystemExit(f'no result_*.pt under {args.sample_path}')
    print(f'Load generated data done! {len(files)} examples in total.')
    reports, connectivity, rings, diversity, geometry = [], [], [], [], []
    sections = pocket_sections(args)
    against_pocket = {flag: [] for flag, _, _, _ in sections}
    graph_include = 'complete' if args.include == 'complete' else 'all'     # 'stable' restricts the pair profiles and atom types only
    for name in files:
        result = torch.load(name, map_location='cpu', weights_only=False)
        pack = quality.SamplePack(result, eval_step, args.atom_enc_mode, args.device)
        if args.connectivity:
            connectivity.append(pack.connectivity(graph_include, bond_reference))
        if args.rings:
            rings.append(pack.rings(graph_include))
        if args.diversity:
            diversity.append(pack.diversity(graph_include, reference_ligand=reference_ligand))
        if args.geometry:
            geometry.append(pack.geometry(graph_include, geometry_reference))
        side = None                                                             # the file's pocket, decoded and uploaded once
        for flag, _, extra, _ in sections:
            if not isinstance(result, dict) or result.get('data') is None:
                raise SystemExit(f'{name} carries no pocket (no data): --{flag} needs the files of a sampling driver')
            try:
                side = side or quality.PocketSide(result['data'], args.device)
                against_pocket[flag].append(getattr(pack, METHODS.get(flag, flag))(side, graph_include, reference_ligand, *extra))
            except ValueError as e:
                if flag not in ('sasa', 'dock'):
                    raise
                raise SystemExit(f'--{flag}: {e}')
        reports.append(pack.quality(args.include, reference))
    rep = quality.QualityReport.merged(reports)
    print(f'Evaluate done! {rep.n_samples} samples in total.')

    def frame(s):
        js = rep.js(s)
        return dict(mol_stable=float(rep.mol_stable[s]), atm_stable=float(rep.atm_stable[s]), JSD_CC_2A=js['JSD_CC_2A'],
                    JSD_All_12A=js['JSD_All_12A'], atom_type_js=js['atom_type_js'])

    last = frame(-1)
    print_dict({k: last[k] for k in ('mol_stable', 'atm_stable')})
    print_dict({k: last[k] for k in ('JSD_CC_2A', 'JSD_All_12A')})
    print('Atom type JS: %.4f' % last['atom_type_js'] if last['atom_type_js'] is not None else 'Atom type JS: None')
    out = dict(num_examples=len(files), num_samples=rep.n_samples, num_atoms=rep.n_atoms, eval_step=eval_step, include=args.include,
               atom_enc_mode=args.atom_enc_mode, **last,
               hist={n: rep.hist[-1, p, :len(rep.profiles[p][3]) + 1].tolist() for p, n in enumerate(rep.names)},
               element_counts=dict(zip(('H', 'C', 'N', 'O', 'F', 'P', 'S', 'Cl'), rep.counts[-1].tolist())))
    if eval_step == 'all':
        out['curve'] = [frame(s) for s in range(rep.num_frames)]
    if args.connectivity:
        con = quality.ConnectivityReport.merged(connectivity)
        last_con = con.summary(-1)
        print_dict(last_con)
        out['connectivity'] = dict(last_con, bond_hist={quality.bond_type_name(t): con.bond_hist[-1, p, :len(con.profiles[p][3]) + 1].tolist()
                                                        for p, t in enumerate(con.bond_types)})
        if eval_step == 'all':
            out['connectivity']['curve'] = [con.summary(s) for s in range(con.num_frames)]
    if args.rings:
        ring = quality.RingReport.merged(rings)
        for k, x in ring.ring_ratio(-1).items():
            print(f'ring size: {k} ratio: {x:.3f}')
        print_dict({k: x for k, x in ring.summary(-1).items() if not k.startswith('ring_') or k == 'ring_atom_share'})
        out['rings'] = dict(ring.summary(-1), ring_hist=ring.ring_hist[-1].tolist(), num_included=int(ring.n_included[-1]))
        if eval_step == 'all':
            out['rings']['curve'] = [ring.summary(s) for s in range(ring.num_frames)]
    if args.diversity:
        div = quality.DiversityReport.merged(diversity)
        last_div = nan_none(div.summary(-1))
        print_dict(last_div)
        out['diversity'] = dict(last_div, num_included=int(div.n_included[-1]), num_distinct=int(div.n_distinct[-1]))
        if eval_step == 'all':
            out['diversity']['curve'] = [nan_none(div.summary(s)) for s in range(div.num_frames)]
    if args.geometry:
        geo = quality.GeometryReport.merged(geometry)
        print('\n'.join(geo.lines(-1)))
        scalar = lambda x: None if isinstance(x, float) and x != x else x
        flat = lambda d: {k: ({q: scalar(y) for q, y in x.items()} if isinstance(x, dict) else scalar(x)) for k, x in d.items()}
        out['geometry'] = dict(flat(geo.summary(-1)), num_included=int(geo.n_included[-1]),
                               hist={n: geo.counts(n, -1).tolist() for n in geo.names})
        if eval_step == 'all':
            out['geometry']['curve'] = [flat(geo.summary(s)) for s in range(geo.num_frames)]
    for flag, report_class, _, fields in sections:
        total = report_class.merged(against_pocket[flag])
        print('\n'.join(total.lines(-1)))
        out[flag] = dict(nan_none(total.summary(-1)), num_included=int(total.n_included[-1]), **fields(total))
        if eval_step == 'all':
            out[flag]['curve'] = [nan_none(total.summary(s)) for s in range(total.num_frames)]
    result_path = os.path.join(args.sample_path, 'eval_results')
    os.makedirs(result_path, exist_ok=True)
    with open(os.path.join(result_path, 'quality.json'), 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', os.path.join(result_path, 'quality.json'))
    return out


if __name__ == '__main__':
    main()
