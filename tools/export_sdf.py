"""Sampled ligands as SD files, without a chemistry toolkit:

    python tools/export_sdf.py --sample_path DIR --out DIR [--eval_step -1] [--only-complete] [--largest-fragment] [--ring-aromatic]
                                [--unique] [--clash-free] [--pocket-clash-free] [--min-hbonds N]
                                [--min-buried-share X] [--max-score X] [--sort-by-score] [--relaxed | --docked]

Reads the ``result_{i}.pt`` files a sampling driver wrote (sorted as tools/evaluate_samples.py sorts them), takes the frame
``--eval_step`` of every sample (default -1: the final poses), builds the bond graph on the GPU (quality.bond_graph: bonds from the
bond-length table, fragments as connected components) and writes ``OUT/result_{i}.sdf`` with one V2000 record per sample: element
symbols from the class table, the bond type from the bond's category (1 / 2 / 3, 4 = aromatic: both atoms of aromatic classes and
order 1 or 2; DESIGN.md section 3, "Bond graph" -- a convention, not perceived chemistry; no hydrogens are added).
``--ring-aromatic`` writes the ring-aware category instead (quality.bond_graph(rings=True); DESIGN.md section 3, "Rings"): type 4 only
for a bond that also lies in a ring of 5 or 6 atoms, its order otherwise, so no atom outside a ring carries an aromatic bond.
``--only-complete`` writes only the samples that are one fragment; ``--largest-fragment`` writes of every sample its largest fragment.
``--unique`` writes, of the samples with equal keys (quality.fingerprints: not told apart by colour refinement of the bond graph;
DESIGN.md section 3, "Fingerprints and diversity"), only the first.  It applies after ``--only-complete`` has chosen the samples, and
the keys are of the whole molecule, also under ``--largest-fragment``: two samples whose largest fragments agree and whose small
fragments differ are both written.
``--clash-free`` writes only the samples without an internal clash (quality.geometry: no pair of atoms more than 3 bonds apart closer
than 0.7 times the sum of their van der Waals radii; DESIGN.md section 3, "Local geometry" -- this project's convention, not a pose
checker's); it applies before ``--unique`` chooses among what is left.
``--pocket-clash-free`` writes only the samples without a clash with the protein (quality.pocket_contacts on the file's pocket: no
ligand atom closer to a protein atom than the sum of their van der Waals radii minus 0.5 A; DESIGN.md section 3, "Pocket contacts" --
again a convention); it combines with ``--clash-free`` and applies before ``--unique`` too.
``--min-hbonds N`` writes only the samples with at least N hydrogen bonds to the protein (quality.pocket_interactions on the file's
pocket: donor - acceptor pairs of heavy atoms closer than 3.5 A, the ligand's donors inferred from the valence deficit; DESIGN.md
section 3, "Pocket interactions" -- a heuristic count, not a score); it combines with the two above and applies before ``--unique``.
``--min-buried-share X`` writes only the samples of whose solvent-accessible surface the pocket covers at least the share X
(quality.pocket_sasa on the file's pocket: buried / free area by Shrake-Rupley point counting with this project's radii and a 1.4 A
probe; DESIGN.md section 3, "Solvent-accessible surface"); it combines with the three above and applies before ``--unique``.
``--max-score X`` writes only the samples whose docking-style score is at most X (quality.pocket_score on the file's pocket: a
Vina-style score on this project's heuristic typing -- no hydrogens, roles from valence deficits, no intramolecular term -- and NOT
AutoDock Vina's number; DESIGN.md section 3, "Docking-style score"); it combines with the four above and applies before ``--unique``.
``--sort-by-score`` writes the samples of a file best (lowest) score first.  With either, every record carries a ``> <score>`` data item.
``--relaxed`` writes the coordinates after a rigid-body relaxation of every sample in the file's pocket (quality.pocket_relax; DESIGN.md
section 3, "Pose relaxation") and a ``> <score_min>`` data item next to ``> <score>``, the score before.  The bonds, the filters and the
order are those of the sampled poses: a rigid motion changes no bond.  It is a local optimisation under this project's heuristic score,
not AutoDock Vina's ``minimize``, and it is rigid-body only: three translations and three rotations, no torsions.
``--docked [--dock_chains 16] [--dock_rounds 16] [--dock_seed 0]`` writes the coordinates after a docking search of every sample in the
file's pocket instead (quality.pocket_dock; DESIGN.md section 3, "Docking search") and ``> <score_min>`` and ``> <score_dock>`` data items
next to ``> <score>``: the score after the relaxation alone and after the search.  It is a rigid-body global search under this project's
heuristic score, not AutoDock Vina's ``dock``: three translations and three rotations, no torsions.
Prints one line per file and returns the counts.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

from targetdiff_amd import molfile, quality  # noqa: E402
from evaluate_samples import result_files  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--sample_path', type=str, required=True)
    ap.add_argument('--out', type=str, required=True)
    ap.add_argument('--eval_step', type=int, default=-1)
    ap.add_argument('--eval_num_examples', type=int, default=None)
    ap.add_argument('--atom_enc_mode', type=str, default='add_aromatic')
    ap.add_argument('--only-complete', action='store_true')
    ap.add_argument('--largest-fragment', action='store_true')
    ap.add_argument('--ring-aromatic', action='store_true', help='bond type 4 only inside a ring of 5 or 6 atoms')
    ap.add_argument('--unique', action='store_true', help='of the samples with equal keys only the first; the keys are of the whole '
                    'molecule (also with --largest-fragment), taken after --only-complete')
    ap.add_argument('--clash-free', action='store_true', help='only the samples without an internal clash')
    ap.add_argument('--pocket-clash-free', action='store_true', help="only the samples without a clash with the protein (the file's data)")
    ap.add_argument('--min-hbonds', type=int, default=None, help="only the samples with at least N hydrogen bonds to the protein (the "
                    "file's data; this project's role heuristic)")
    ap.add_argument('--min-buried-share', type=float, default=None, help="only the samples with at least this share of their "
                    "solvent-accessible surface covered by the pocket (the file's data; 0 .. 1)")
    ap.add_argument('--max-score', type=float, default=None, help="only the samples with a docking-style score of at most this (the file's "
                    "data; a Vina-style score on this project's heuristic typing, NOT AutoDock Vina's number)")
    ap.add_argument('--sort-by-score', action='store_true', help='the samples of a file best (lowest) docking-style score first')
    ap.add_argument('--relaxed', action='store_true', help="the coordinates after a rigid-body relaxation in the file's pocket, with a "
                    "score_min data item: a local optimisation under this project's heuristic score, not AutoDock Vina's minimize; "
                    'rigid-body only: three translations and three rotations, no torsions')
    ap.add_argument('--docked', action='store_true', help="the coordinates after a docking search in the file's pocket, with score_min and "
                    "score_dock data items: a rigid-body global search under this project's heuristic score, not AutoDock Vina's dock: "
                    'three translations and three rotations, no torsions')
    ap.add_argument('--dock_chains', type=int, default=quality.DOCK_CHAINS, help='--docked: independent Monte-Carlo chains per molecule')
    ap.add_argument('--dock_rounds', type=int, default=quality.DOCK_ROUNDS, help='--docked: mutate-and-relax rounds per chain after the first')
    ap.add_argument('--dock_seed', type=int, default=0, help='--docked: the seed of the uniforms')
    ap.add_argument('--device', type=str, default='cuda')
    args = ap.parse_args(argv)
    if args.relaxed and args.docked:
        raise SystemExit('--relaxed and --docked both write coordinates: choose one')
    if args.min_buried_share is not None and not 0.0 <= args.min_buried_share <= 1.0:
        raise SystemExit(f'--min-buried-share is a share, 0 .. 1 (got {args.min_buried_share})')
    files = result_files(args.sample_path, args.eval_num_examples)
    if not files:
        raise SystemExit(f'no result_*.pt under {args.sample_path}')
    os.makedirs(args.out, exist_ok=True)
    out = {}
    for name in files:
        result = torch.load(name, map_location='cpu', weights_only=False)
        pack = quality.SamplePack(result, args.eval_step, args.atom_enc_mode, args.device)
        pos, v, ptr, sizes = pack.pos, pack.v, pack.ligand_ptr, pack.sizes
        g = quality.bond_graph(pos, v, ligand_ptr=ptr, atom_enc_mode=args.atom_enc_mode, bond_profiles=(), return_fragments=True,
                               return_bonds=True, rings=args.ring_aromatic, device=args.device)
        select = chosen = clash_free = pocket_clash_free = enough_hbonds = buried_enough = None
        if args.only_complete:
            chosen = g.complete[0]
        if args.clash_free:
            clash_free = quality.geometry(pos, v, ligand_ptr=ptr, atom_enc_mode=args.atom_enc_mode, profiles=(), device=args.device).clash_free[0]
            chosen = clash_free if chosen is None else chosen & clash_free
            select = clash_free.cpu().numpy()
        if args.pocket_clash_free:
            if not isinstance(result, dict) or result.get('data') is None:
                raise SystemExit(f'{name} carries no pocket (no data): --pocket-clash-free needs the files of a sampling driver')
            pocket_clash_free = quality.pocket_contacts(*quality.pocket_of(result['data']), pos, v, ligand_ptr=ptr,
                                                        atom_enc_mode=args.atom_enc_mode, device=args.device).clash_free[0]
            chosen = pocket_clash_free if chosen is None else chosen & pocket_clash_free
            select = pocket_clash_free.cpu().numpy() & (True if select is None else select)
        if args.min_hbonds is not None:
            if not isinstance(result, dict) or result.get('data') is None:
                raise SystemExit(f'{name} carries no pocket (no data): --min-hbonds needs the files of a sampling driver')
            enough_hbonds = quality.pocket_interactions(*quality.pocket_of(result['data']), pos, v, ligand_ptr=ptr,
                                                        atom_enc_mode=args.atom_enc_mode, device=args.device).n_hbonds[0] >= args.min_hbonds
            chosen = enough_hbonds if chosen is None else chosen & enough_hbonds
            select = enough_hbonds.cpu().numpy() & (True if select is None else select)
        if args.min_buried_share is not None:
            if not isinstance(result, dict) or result.get('data') is None:
                raise SystemExit(f'{name} carries no pocket (no data): --min-buried-share needs the files of a sampling driver')
            buried_enough = quality.pocket_sasa(*quality.pocket_of(result['data']), pos, v, ligand_ptr=ptr, atom_enc_mode=args.atom_enc_mode,
                                                device=args.device).buried_share[0] >= args.min_buried_share
            chosen = buried_enough if chosen is None else chosen & buried_enough
            select = buried_enough.cpu().numpy() & (True if select is None else select)
        score = good_score = None
        if args.max_score is not None or args.sort_by_score:
            if not isinstance(result, dict) or result.get('data') is None:
                raise SystemExit(f'{name} carries no pocket (no data): --max-score and --sort-by-score need the files of a sampling driver')
            score = quality.pocket_score(*quality.pocket_of(result['data']), pos, v, ligand_ptr=ptr, atom_enc_mode=args.atom_enc_mode,
                                         device=args.device).score[0]
        if args.max_score is not None:
            good_score = torch.from_numpy(score <= args.max_score).to(pos.device)
            chosen = good_score if chosen is None else chosen & good_score
            select = good_score.cpu().numpy() & (True if select is None else select)
        relaxed = None
        if args.relaxed:
            if not isinstance(result, dict) or result.get('data') is None:
                raise SystemExit(f'{name} carries no pocket (no data): --relaxed needs the files of a sampling driver')
            relaxed = quality.pocket_relax(*quality.pocket_of(result['data']), pos, v, ligand_ptr=ptr, atom_enc_mode=args.atom_enc_mode,
                                           device=args.device)
            score = relaxed.score_in[0] if score is None else score
        if args.docked:
            if not isinstance(result, dict) or result.get('data') is None:
                raise SystemExit(f'{name} carries no pocket (no data): --docked needs the files of a sampling driver')
            relaxed = quality.pocket_dock(*quality.pocket_of(result['data']), pos, v, ligand_ptr=ptr, atom_enc_mode=args.atom_enc_mode,
                                          n_chains=args.dock_chains, n_rounds=args.dock_rounds, seed=args.dock_seed, device=args.device)
            score = relaxed.score_in[0] if score is None else score
        if args.unique:
            fp = quality.fingerprints(pos, v, ligand_ptr=ptr, atom_enc_mode=args.atom_enc_mode, device=args.device)
            first = fp.similarity(include=None if chosen is None else chosen[None])['first_equal'][0].cpu().numpy()
            select = (first == np.arange(len(sizes))) & (True if select is None else select)
        mols = molfile.molecules_from_graph(g, pos if relaxed is None else relaxed.pos, v, args.atom_enc_mode, 0, args.only_complete, args.largest_fragment,
                                            categories=g.ring_category if args.ring_aromatic else None, select=select)
        if score is not None:
            of = lambda m: float(score[int(m['name'].rsplit('_', 1)[1])])          # molecules_from_graph names them sample_{g}
            for m in mols:
                m['properties']['score'] = f'{of(m):.4f}'
                if relaxed is not None:
                    after = relaxed.score_min if args.docked else relaxed.score
                    m['properties']['score_min'] = f"{float(after[0][int(m['name'].rsplit('_', 1)[1])]):.4f}"
                if args.docked:
                    m['properties']['score_dock'] = f"{float(relaxed.score[0][int(m['name'].rsplit('_', 1)[1])]):.4f}"
            if args.sort_by_score:
                mols.sort(key=of)
        stem = os.path.basename(name)[:-3]
        path = os.path.join(args.out, stem + '.sdf')
        n = molfile.write_sdf(path, mols)
        complete = int(g.complete[0].sum())
        print(f'{path}: {n} of {len(sizes)} samples written, {complete} complete')
        out[stem] = dict(path=path, written=n, samples=len(sizes), complete=complete)
        if clash_free is not None:
            out[stem]['clash_free'] = int(clash_free.sum())
        if pocket_clash_free is not None:
            out[stem]['pocket_clash_free'] = int(pocket_clash_free.sum())
        if enough_hbonds is not None:
            out[stem]['min_hbonds'] = int(enough_hbonds.sum())
        if buried_enough is not None:
            out[stem]['min_buried_share'] = int(buried_enough.sum())
        if good_score is not None:
            out[stem]['max_score'] = int(good_score.sum())
    return out


if __name__ == '__main__':
    main()
