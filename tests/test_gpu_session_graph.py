"""The sampling session's neighbour merge and row lists (knn_merge_body, knn_merge_general_kernel, step_lists_kernel and the separate
list kernels, csrc/graph.hip) on geometry that decides every branch they have.  Needs an MI355X: ``-m gpu``.

Everything here is integer work, so nothing has a tolerance.  After every ``sess.forward`` the same four checks run (``_Case.step``):

1. the stateless neighbour table == the table of oracle/shims.py (k-NN: as is; hybrid: row sets);
2. session outputs == stateless outputs, ``torch.equal``;
3. ``row_counts()`` / ``forward_reach_rows()`` == what a plain CPU walk over the shims table gives (tests/_session_ref.py);
4. 2 and 3 again with the separate list kernels (``session_step_lists = 0``) and in a session with per-graph static tables
   (``session_share_pockets = 0``).  Both switches exist for the default graph (k-NN, k <= 32) only: the session of a general graph
   (k of 33 .. 64, hybrid) always takes its row lists from the one launch and keeps its tables per node, so there check 4 is the
   same session called a second time, which exercises only the per-step reset of its flags and counters; rows going from dirty
   back to clean on a general graph are the business of the k = 48 and hybrid teleport cases.

Once per geometry family and graph mode the stateless forward itself is held to the oracle restatement (TOL_X / TOL_H of
tests/_tol.py), so that "stateless" is anchored on lattice input too.

Branches reached (tests/test_session_ref_host.py pins that the inputs really hold them): the second ligand key per lane (64 .. 127
ligand atoms), the passes above 128 ligand atoms, fewer than k protein atoms with more than k atoms in all, a ligand atom at exactly
the k-th protein neighbour's d2 (it must lose: lattices), clean -> dirty -> clean across calls (teleports), shared pocket tables
whose replicas take different merge branches, a too small neighbour-search hint, and a graph too large for the row-list kernel's
LDS flags.  Which of these kill which one-line mutant of graph.hip: EXPERIMENTS.md.
"""
import pytest
import torch

import _session_ref as S
from _tol import TOL_X, TOL_H, close

pytestmark = pytest.mark.gpu

KEYS = ('pred_ligand_pos', 'pred_ligand_v', 'final_ligand_h')


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


def _cfg(mode, k):
    from oracle import weights
    return dict(weights.DEFAULT_MODEL_CONFIG, cutoff_mode=mode, knn=k)


@pytest.fixture(scope='module')
def natives(state_dict):
    """one native model per graph mode, made on first use"""
    _dev()                                  # no device: skip before anything is built
    from targetdiff_amd.models import ScorePosNet3D
    made = {}

    def get(mode, k):
        if (mode, k) not in made:
            m = ScorePosNet3D(_cfg(mode, k), S.PROTEIN_FEAT_DIM, S.LIGAND_CLASSES)
            assert not m.load_state_dict(state_dict, strict=False).unexpected_keys
            m = m.to(_dev()).eval()
            made[(mode, k)] = (m, m._native(_dev()))
        return made[(mode, k)][1]
    return get


def _row_sets(table):
    return [sorted(int(j) for j in r if j >= 0) for r in table.tolist()]


class _Case:
    """One batch layout (protein blocks, ligand sizes) with a session sharing pocket tables and, on the default graph, one that does
    not; ``step`` takes the ligand placement of the call."""

    def __init__(self, nat, mode, k, batch, hint=0, caching=True):
        from targetdiff_amd import capi
        self.nat, self.mode, self.k, self.hint, self.caching = nat, mode, k, hint, caching
        self.default_graph = mode == 'knn' and k <= 32
        self.dev = dev = _dev()
        self.ppos, self.pv = batch.ppos.to(dev), batch.pv.to(dev)
        self.pptr, self.lptr = batch.pptr.to(dev), batch.lptr.to(dev)
        assert nat.get_option('session_share_pockets') == 1 and nat.get_option('session_step_lists') == 1      # shipped defaults
        self.shared = capi.NativeSession(nat, self.ppos, self.pv, self.pptr, self.lptr, batch.Nl, hint)
        if not self.default_graph:
            self.passes = (('session', self.shared, 1), ('session, called again', self.shared, 1))
            return
        nat.set_option('session_share_pockets', 0)
        try:
            self.own = capi.NativeSession(nat, self.ppos, self.pv, self.pptr, self.lptr, batch.Nl, hint)
        finally:
            nat.set_option('session_share_pockets', 1)
        assert self.own.shared_static_tables() is None
        self.passes = (('shared tables', self.shared, 1), ('separate list kernels', self.shared, 0), ('own tables', self.own, 1),
                       ('own tables, separate list kernels', self.own, 0))

    def stateless_table(self, batch):
        x, node_ptr = batch.x.to(self.dev), batch.node_ptr.to(self.dev)
        if self.mode == 'knn' and self.k <= 32:
            return self.nat.knn(x, node_ptr, self.k, self.hint).cpu().long()
        width = self.k if self.mode == 'knn' else max(batch.n_lig) - 1 + self.k
        return self.nat.graph_build(x, batch.mask.to(self.dev), node_ptr, width, self.hint).cpu().long()

    def step(self, batch, what='', table_from_gpu=False):
        """the four checks on this placement of the ligands; returns the stateless outputs"""
        nat = self.nat
        # 1. the stateless table
        got_table = self.stateless_table(batch)
        if table_from_gpu:
            table = got_table
        else:
            table = S.neighbour_table(batch, self.mode, self.k)
            if self.mode == 'knn':
                assert torch.equal(got_table, table), (what, 'stateless table')
            else:
                assert _row_sets(got_table) == _row_sets(table), (what, 'stateless table')
        want_counts = S.expected_counts(batch, self.mode, self.k, table=table) if self.caching else ((batch.N, batch.N, []), None)
        # 2. - 4.
        lpos, lv = batch.lpos.to(self.dev), batch.lv.to(self.dev)
        want = nat.model_forward(self.ppos, self.pv, self.pptr, lpos, lv, self.lptr, max_graph_nodes=self.hint, want_final_h=False)
        for name, sess, lists in self.passes:
            nat.set_option('session_step_lists', lists)
            try:
                got = sess.forward(lpos, lv)
            finally:
                nat.set_option('session_step_lists', 1)
            for key in KEYS:
                assert torch.equal(got[key], want[key]), (what, name, key, float((got[key] - want[key]).abs().max()))
            assert (sess.row_counts(), sess.forward_reach_rows()) == want_counts, (what, name)
        return want, want_counts


def _oracle_anchor(state_dict, case, batch):
    from oracle import restatement as R
    want = R.model_forward(state_dict, _cfg(case.mode, case.k), batch.ppos, batch.pv, batch.batch_protein, batch.lpos, batch.lv,
                           batch.batch_ligand)
    got = case.nat.model_forward(case.ppos, case.pv, case.pptr, batch.lpos.to(case.dev), batch.lv.to(case.dev), case.lptr)
    close(got['pred_ligand_pos'], want['pred_ligand_pos'], TOL_X)
    close(got['pred_ligand_v'], want['pred_ligand_v'], TOL_H)
    close(got['final_h'], want['final_h'], TOL_H)


# ------------------------------------------------------------------------------------------ size matrix on clouds
@pytest.mark.parametrize('b', range(6))
@pytest.mark.parametrize('k', [5, 16, 32])
def test_size_matrix_default_graph(natives, k, b):
    """Protein sizes {5, 20, 31, 32, 33, 100} x ligand sizes {1, 40, 63, 64, 65, 127, 128, 129, 200}, nine graphs to a batch: every
    batch mixes the rank merge on one and on two ligand keys per lane with the passes above 128 ligand atoms, and protein blocks
    below k (every ligand atom a candidate, the surplus dropped at rank >= k: (20, 40) is in batch 0) with blocks above it."""
    batch = S.size_matrix_batch(b)
    _Case(natives('knn', k), 'knn', k, batch).step(batch)


@pytest.mark.parametrize('mode,k', [('knn', 33), ('knn', 48), ('knn', 64), ('hybrid', 32)])
def test_size_subset_general_merge(natives, mode, k):
    """knn_merge_general_kernel (k of 33 .. 64, and the protein rows of `hybrid`) on 65, 129 and 200 ligand atoms, with protein
    blocks of 5 .. 100 atoms: fewer static keys than k, exactly as many, more."""
    batch = S.general_batch()
    _Case(natives(mode, k), mode, k, batch).step(batch)


# ------------------------------------------------------------------------------------------ lattices: ties at the threshold
@pytest.mark.parametrize('case', range(len(S.LATTICE_CASES)), ids=lambda i: 'x'.join(map(str, S.LATTICE_CASES[i][0])) + f'-r{S.LATTICE_CASES[i][1]}-k{S.LATTICE_CASES[i][2]}')
def test_vacancy_lattice_ties_go_to_the_protein_atom(natives, case):
    """Every d2 is an exact integer; 6 .. 20 protein rows per lattice have a ligand atom at exactly their k-th protein neighbour's d2
    and must stay clean (the ligand index is the higher one), 53 .. 136 are dirty.  Two lattices in a batch (the second a replica
    of the first: a shared pocket whose table rows are rebased)."""
    grid, rad, k, n_prot, n_lig = S.LATTICE_CASES[case]
    g = S.vacancy_lattice(grid, rad)
    batch = S.Batch([g, dict(g, lv=(g['lv'] + 1) % S.LIGAND_CLASSES)])
    assert batch.n_prot == [n_prot] * 2 and batch.n_lig == [n_lig] * 2
    _, (counts, _) = _Case(natives('knn', k), 'knn', k, batch).step(batch)
    assert counts[1] < batch.N                       # (clean rows exist: the counts above were compared with equality)


@pytest.mark.parametrize('mode,k', [('knn', 32), ('knn', 48), ('hybrid', 32)])
@pytest.mark.parametrize('family', ['lattice', 'cloud'])
def test_stateless_forward_vs_oracle_on_these_geometries(natives, state_dict, family, mode, k):
    """what the session is compared with, held to the restatement on uncentred lattice / cloud input (TOL_X, TOL_H)"""
    if family == 'lattice':
        batch = S.Batch([S.vacancy_lattice((10, 6, 5), 2.0)])
    else:
        batch = S.Batch([S.cloud(100, 40, S.INSIDE, 1), S.cloud(20, 40, S.RIM, 2), S.cloud(33, 1, S.INSIDE, 3)])
    case = _Case(natives(mode, k), mode, k, batch)
    _oracle_anchor(state_dict, case, batch)
    case.step(batch)


# ------------------------------------------------------------------------------------------ far ligand
@pytest.mark.parametrize('mode,k,prot', [('knn', 32, (33, 100)), ('knn', 5, (33, 100)), ('knn', 48, (49, 100)), ('hybrid', 32, (33, 100))])
def test_far_ligand_leaves_every_protein_row_clean(natives, mode, k, prot):
    """ligands 1000 A away, every graph with at least k + 1 protein atoms: only the ligand rows are dirty, nothing else is reached"""
    graphs = [S.cloud(p, nl, S.FAR, seed=77 * p + nl) for p in prot for nl in (1, 65, 129)]
    batch = S.Batch(graphs)
    _, (counts, reach) = _Case(natives(mode, k), mode, k, batch).step(batch)
    assert counts[1] == batch.Nl and reach == batch.Nl


# ------------------------------------------------------------------------------------------ teleports in one session
def _teleport(natives, mode, k, placements):
    a = placements[0]
    case = _Case(natives(mode, k), mode, k, a)
    outs, counts = [], []
    for name, batch in zip('ABCA', placements + [a]):
        o, c = case.step(batch, what=name)
        outs.append({key: o[key].clone() for key in KEYS})
        counts.append(c)
    for key in KEYS:
        assert torch.equal(outs[3][key], outs[0][key]), key
    assert counts[3] == counts[0]
    return counts


@pytest.mark.parametrize('mode,k', [('knn', 32), ('knn', 48), ('hybrid', 32)])
def test_teleport_sequence_cloud(natives, mode, k):
    """A (inside) -> B (1000 A away) -> C (inside, other side) -> A: rows dirty at one call and clean at the next come back from the
    cache (static neighbour row, gate row, layer-0 / 1 / 2 outputs); the fourth call equals the first bit for bit"""
    sizes = [(100, 40), (100, 129), (64, 65), (20, 64), (100, 1)]
    graphs = [S.cloud(p, nl, (0.0, 0.0, 0.0), seed=31 * p + nl) for p, nl in sizes]
    place = lambda c: S.Batch([S.moved(g, c) for g in graphs])
    a = place((4.0, 0.0, 0.0))
    counts = _teleport(natives, mode, k, [a, place(S.FAR), place((-4.0, 2.0, 0.0))])
    assert a.Nl < counts[0][0][1] < a.N and a.Nl < counts[2][0][1] < a.N          # A and C: dirty and clean protein rows


@pytest.mark.parametrize('mode,k', [('knn', 32), ('knn', 48), ('hybrid', 32)])
def test_teleport_sequence_lattice(natives, mode, k):
    """the same on lattices (ties at A): B is the ligand 500 grid steps out of the grid, C the ligand moved to odd coordinates
    on the other side of the grid (between the sites, never on one)"""
    graphs = [(S.vacancy_lattice((10, 6, 5), 2.5), (11.0, 1.0, -1.0)), (S.vacancy_lattice((14, 7, 6), 3.7), (15.0, 1.0, -1.0)),
              (S.vacancy_lattice((14, 7, 6), 4.2), (15.0, -1.0, 1.0))]
    a = S.Batch([g for g, _ in graphs])
    b = S.Batch([S.moved(g, (1000.0, 0.0, 0.0)) for g, _ in graphs])
    c = S.Batch([S.moved(g, shift) for g, shift in graphs])
    _teleport(natives, mode, k, [a, b, c])


# ------------------------------------------------------------------------------------------ shared pockets
@pytest.mark.parametrize('k', [16, 32])
def test_shared_pockets_with_different_merge_branches(natives, k):
    """graphs 0 - 2: one 100-atom pocket with 1 / 65 / 129 ligand atoms (one key per lane, two, the passes); graph 3: another pocket of
    100 atoms; graph 4: the first pocket again, its ligand far away (every row restored through the rebase)"""
    p1, p2 = S.cloud(100, 1, S.INSIDE, seed=5), S.cloud(100, 40, S.RIM, seed=6)
    with_pocket = lambda g, p: dict(g, ppos=p['ppos'], pv=p['pv'])
    graphs = [p1, with_pocket(S.cloud(100, 65, S.RIM, seed=7), p1), with_pocket(S.cloud(100, 129, S.INSIDE, seed=8), p1), p2,
              with_pocket(S.cloud(100, 30, S.FAR, seed=9), p1)]
    batch = S.Batch(graphs)
    case = _Case(natives('knn', k), 'knn', k, batch)
    assert case.shared.shared_static_tables() == (200, 2)
    case.step(batch, what='first')
    # the ligands swap regimes: the far one comes in, the others leave
    batch2 = S.Batch([S.moved(g, (1000.0, 0.0, 0.0)) for g in graphs[:4]] + [S.moved(graphs[4], (-995.0, 0.0, 0.0))])
    case.step(batch2, what='swapped')
    case.step(batch, what='back')


# ------------------------------------------------------------------------------------------ neighbour-search hint
@pytest.mark.parametrize('mode,k', [('knn', 32), ('knn', 48)])
def test_neighbour_search_hint_only_costs_time(natives, mode, k):
    """max_graph_nodes = 0 (unknown), exact, and too small (100 / 300 for a 400-node graph: the search loops in passes of
    64 x {4, 6, 11, 17} candidates): same bits, same counts"""
    batch = S.Batch([S.cloud(300, 100, S.RIM, seed=11), S.cloud(100, 40, S.INSIDE, seed=12)])
    ref = None
    for hint in (0, 400, 100, 300):
        want, counts = _Case(natives(mode, k), mode, k, batch, hint=hint).step(batch, what=f'hint {hint}')
        if ref is None:
            ref = ({key: want[key].clone() for key in KEYS}, counts)
        for key in KEYS:
            assert torch.equal(want[key], ref[0][key]), (hint, key)
        assert counts == ref[1]


# ------------------------------------------------------------------------------------------ largest graph
def _large_batch():
    n = 12300
    return S.Batch([S.cloud(n, 20, S.INSIDE, seed=13, sigma_prot=4.0 * (n / 100.0) ** (1.0 / 3.0)), S.cloud(100, 40, S.RIM, seed=14)])


def test_largest_graph_takes_the_separate_list_kernels_by_itself(natives):
    """12,300 + 20 nodes in one graph: 4 flag bytes per node no longer fit the row-list kernel's 48 KiB of LDS (12,288 nodes), so the
    library falls back to compact_dirty / forward_reach / expand_hop / expand_level / compact_levels without being told to.  The
    expected counts come from the STATELESS table read back from the GPU: a 12k x 12k distance matrix of oracle/shims.py does not
    fit a test (the stateless search is held to shims at every other size in this file and in test_knn_bit_exact)."""
    batch = _large_batch()
    assert max(batch.sizes) > 12288
    _Case(natives('knn', 32), 'knn', 32, batch).step(batch, table_from_gpu=True)


def test_largest_graph_general_session_is_plain(natives):
    """k = 48 on the same batch: the session of a general graph needs the row-list kernel, so it keeps the layout only (every row
    recomputed): session == stateless"""
    batch = _large_batch()
    _Case(natives('knn', 48), 'knn', 48, batch, caching=False).step(batch, table_from_gpu=True)
