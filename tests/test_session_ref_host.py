"""What the geometries of tests/_session_ref.py promise (CPU only), so that tests/test_gpu_session_graph.py cannot quietly lose its
point: the lattices really hold protein rows that are clean only because a tie at the k-th neighbour goes to the protein atom, the size
matrix really holds every (protein, ligand) pair, and the expectation code agrees with a census taken from distances alone."""
import pytest
import torch

import _session_ref as S


@pytest.fixture(scope='module', params=range(len(S.LATTICE_CASES)), ids=lambda i: 'x'.join(map(str, S.LATTICE_CASES[i][0])) + f'-r{S.LATTICE_CASES[i][1]}')
def lattice(request):
    grid, rad, k, n_prot, n_lig = S.LATTICE_CASES[request.param]
    batch = S.Batch([S.vacancy_lattice(grid, rad)])
    return batch, k, n_prot, n_lig, S.merge_census(batch, k)


def test_lattice_counts_and_exact_coordinates(lattice):
    batch, k, n_prot, n_lig, _ = lattice
    assert batch.n_prot == [n_prot] and batch.n_lig == [n_lig]
    # even integers (A): every difference and every d2 is an exact fp32 integer -- and nothing was centred
    assert torch.equal(batch.x, torch.round(batch.x / 2.0) * 2.0) and float(batch.x.min()) == 0.0
    assert S.min_pair_d2(batch) == 4.0            # no coincident points: nearest sites are one grid step apart


def test_lattice_holds_tie_only_clean_rows(lattice):
    batch, k, _, _, census = lattice
    kinds = [kind for kind, _ in census.values()]
    assert kinds.count('tie') >= 1, 'no protein row is clean only by the tie rule'
    assert kinds.count('dirty') >= 1
    assert sum(1 for kind, has_k in census.values() if kind == 'clean' and has_k) >= 1


def test_lattice_expectation_agrees_with_the_census(lattice):
    """the table-based dirty set (what the GPU test compares with) == the distance-based census: a 'tie' row is clean"""
    batch, k, _, _, census = lattice
    dirty, reach, levels = S.row_lists(S.neighbour_table(batch, 'knn', k), batch.mask)
    want = {i for i, (kind, _) in census.items() if kind == 'dirty'} | {i for i in range(batch.N) if batch.mask[i]}
    assert dirty == want
    assert dirty <= reach and all(a <= b for a, b in zip(levels, levels[1:])) and len(levels) == S.HOP_LEVELS
    assert len(reach) < batch.N                   # some rows keep their cached layer-1 output


def test_lattice_table_of_the_issue():
    """dirty protein rows / rows clean only by the tie, as recorded when the cases were chosen"""
    want = [(97, 18), (86, 15), (53, 6), (136, 9), (104, 20)]
    for (grid, rad, k, _, _), (n_dirty, n_tie) in zip(S.LATTICE_CASES, want):
        batch = S.Batch([S.vacancy_lattice(grid, rad)])
        kinds = [kind for kind, _ in S.merge_census(batch, k).values()]
        assert (kinds.count('dirty'), kinds.count('tie')) == (n_dirty, n_tie), (grid, rad, k)


def test_shifted_lattice_ligand_stays_exact_and_apart():
    """the teleport sequence's other placements: out of the grid by whole grid steps, and back inside on odd coordinates (between the
    sites: exact integer d2, never on a protein atom; d2 = 3 mod 8 there, so no ties -- those are placement A's business)"""
    g = S.vacancy_lattice((10, 6, 5), 2.5)
    far = S.Batch([S.moved(g, (1000.0, 0.0, 0.0))])
    assert S.min_ligand_protein_d2(far) > 900.0 ** 2
    kinds = [kind for kind, _ in S.merge_census(far, 32).values()]
    assert kinds.count('dirty') == 0
    inside = S.Batch([S.moved(g, (11.0, 1.0, -1.0))])
    assert S.min_ligand_protein_d2(inside) == 3.0            # (1, 1, 1) A from the nearest site
    kinds = [kind for kind, _ in S.merge_census(inside, 32).values()]
    assert kinds.count('dirty') >= 1 and kinds.count('clean') >= 1


def test_size_matrix_holds_every_pair_and_every_branch():
    pairs = set()
    for b in range(6):
        batch = S.size_matrix_batch(b)
        pairs |= set(zip(batch.n_prot, batch.n_lig))
        assert sorted(batch.n_lig) == S.LIGAND_SIZES          # one key per lane, two, and the passes above 128 in every batch
        assert min(batch.n_prot) < 32 <= max(batch.n_prot)
        assert S.min_pair_d2(batch) > 0.0
    assert pairs == {(p, l) for p in S.PROTEIN_SIZES for l in S.LIGAND_SIZES} and (20, 40) in pairs
    # protein rows of both kinds at every k of the default graph (batch 0 holds the 100-atom protein with rim ligands)
    batch = S.size_matrix_batch(0)
    for k in (5, 16, 32):
        kinds = [kind for kind, _ in S.merge_census(batch, k).values()]
        assert kinds.count('dirty') >= 1 and kinds.count('clean') >= 1, k


def test_general_batch_sizes():
    batch = S.general_batch()
    assert {65, 129, 200} <= set(batch.n_lig) and (20, 65) in set(zip(batch.n_prot, batch.n_lig))
    assert S.min_pair_d2(batch) > 0.0


def test_row_lists_on_a_hand_made_table():
    """0, 1, 2, 3 protein, 4 ligand.  Row 1 holds the ligand; row 2 holds row 1; row 3 holds row 2; row 0 holds row 3."""
    table = torch.tensor([[3, -1], [4, 0], [1, 0], [2, 0], [1, -1]])
    mask = torch.tensor([False, False, False, False, True])
    dirty, reach, levels = S.row_lists(table, mask, levels=3)
    assert dirty == {1, 4}
    assert reach == {1, 2, 4}
    assert levels == [{4, 1}, {4, 1, 0}, {4, 1, 0, 3}]


def test_batches_hold_rows_decided_by_the_last_static_key():
    """protein rows that are dirty only through a ligand atom between their (k-1)-th and k-th protein neighbour: a merge threshold
    taken one neighbour too near would call them clean (default graph: size-matrix batches and lattices; general merge: its batch)"""
    for k in (5, 16, 32):
        assert len(S.rows_decided_by_the_last_static_key(S.size_matrix_batch(0), k)) >= 1, k
    grid, rad, k, _, _ = S.LATTICE_CASES[4]
    assert len(S.rows_decided_by_the_last_static_key(S.Batch([S.vacancy_lattice(grid, rad)]), k)) >= 1
    batch = S.general_batch()
    for k in (33, 48, 64, 32):            # (32: the protein rows of `hybrid`)
        assert len(S.rows_decided_by_the_last_static_key(batch, k)) >= 1, k


def test_batches_hold_rows_with_a_ligand_atom_of_a_later_pass():
    """ligand atoms number 128 and later of a graph (129, 175, 200 ligand atoms) are in some protein row's k nearest: a merge that
    stops after its first pass of 128 loses them"""
    for b in range(6):
        batch = S.size_matrix_batch(b)
        for k in (5, 16, 32):
            assert len(S.rows_holding_a_late_ligand_atom(batch, S.neighbour_table(batch, 'knn', k))) >= 1, (b, k)
    grid, rad, k, _, _ = S.LATTICE_CASES[4]
    batch = S.Batch([S.vacancy_lattice(grid, rad)])
    assert len(S.rows_holding_a_late_ligand_atom(batch, S.neighbour_table(batch, 'knn', k))) >= 1
