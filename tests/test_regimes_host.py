"""The conditions that keep tests/test_gpu_input_regimes.py honest, on the CPU: the regimes of tests/_regime_ref.py are what their names say, the
float64 reference is finite and sees the same edges as the fp32 one, and the comparison rule rejects an error of three times the fp32
restatement's own."""
import math

import pytest
import torch

import _regime_ref as G
from _tol import TOL_FWD, maxdiff
from oracle import restatement as R

CASE_GRAPH = [pytest.param(c, g, id=f'{G.case_id(c)}-{g}') for c in G.CASES for g in G.GRAPHS]


def test_case_list():
    assert len(G.CASES) == len(set(G.CASES)) == 16 and G.PACK.N == 158
    assert {c[0] for c in G.CASES if c[1:] == ('cloud', 1)} == set(G.FEATURES)
    assert {c[1] for c in G.CASES if c[0] == 'unit' and c[2] == 1} == set(G.GEOMETRIES)
    assert {c for c in G.CASES if c[2] != 1} == {(f, g, s) for s in (30, 300) for f, g in (('unit', 'cloud'), ('unit', 'coincident'), ('mixed', 'cloud'))}


@pytest.mark.parametrize('case,graph', CASE_GRAPH)
def test_references_finite_on_one_graph(case, graph):
    """fp32 and float64 restatement outputs finite, on an identical neighbour table; the table has the rows the pack was chosen for"""
    r = G.refine_reference(case, graph)
    for name in ('f32', 'f64', 'f32_fix', 'f64_fix'):
        assert bool(torch.isfinite(r[name]['h']).all()) and bool(torch.isfinite(r[name]['x']).all()), (case, graph, name)
    assert bool(torch.isfinite(r['f64_ew']).all()) and r['f64']['h'].dtype == torch.float64
    assert torch.equal(r['f32_nbr'], r['f64_nbr'])
    deg = (r['f64_nbr'] >= 0).sum(1)
    assert int(deg[0]) == int(deg[1]) == 1 and set(deg[2:7].tolist()) == {4}                     # single in-edge; fewer than k: pads
    assert int(deg[list(G.PACK.protein_rows(G.BIG))].min()) == {'knn32': 32, 'knn48': 48, 'hybrid': 32}[graph]
    assert int(deg[list(G.PACK.ligand_rows(G.BIG))].max()) == {'knn32': 32, 'knn48': 48, 'hybrid': 11 + 32}[graph]
    assert int(deg[list(G.PACK.ligand_rows(4))].max()) == {'knn32': 32, 'knn48': 44, 'hybrid': 39 + 5}[graph]


@pytest.mark.parametrize('graph', list(G.GRAPHS))
def test_far_has_no_ligand_edge_inside_the_gaussians(graph):
    r = G.refine_reference(('unit', 'far', 1), graph)
    d = G.edge_lengths(r['x'], r['f64_nbr'])[list(G.PACK.ligand_rows(G.BIG))]
    assert float(d[~d.isnan()].min()) > G.LAST_CENTRE
    near = G.edge_lengths(G.geometry('cloud'), G.refine_reference(('unit', 'cloud', 1), graph)['f64_nbr'])
    assert float(near[~near.isnan()].min()) < 1.0                                                 # and the cloud does


@pytest.mark.parametrize('graph', list(G.GRAPHS))
def test_coincident_has_zero_length_edges_of_every_type_pair(graph):
    r = G.refine_reference(('unit', 'coincident', 1), graph)
    nbr = r['f64_nbr']
    d = G.edge_lengths(r['x'], nbr)
    etype = R.edge_types(nbr, G.PACK.mask)
    zero = (d == 0) & (nbr >= 0)
    assert {int(t) for t in etype[zero]} == {0, 1, 2, 3}
    for a, b in G.coincident_pairs():
        assert bool(zero[a][nbr[a] == b].all()) and int((nbr[a] == b).sum()) == 1 and int((nbr[b] == a).sum()) == 1, (a, b)
    x = r['x']                                                                                    # the duplicates are exact in fp32
    assert all(torch.equal(x[a], x[b]) for a, b in G.coincident_pairs())


def test_lattice_ties_and_offset():
    x = G.geometry('lattice')
    assert torch.equal(x * 4, (x * 4).round())                                                    # multiples of 0.75 / 3 -> exact
    r = G.refine_reference(('unit', 'lattice', 1), 'knn32')
    d = G.edge_lengths(x, r['f64_nbr'])[list(G.PACK.ligand_rows(G.BIG))]
    assert all(2 * len(set(row[~row.isnan()].tolist())) <= 32 for row in d)                       # 32 edges, at most 16 distinct lengths
    assert float(G.geometry('offset').min()) > 450.0


def test_sharp_logits_underflow_fp32_exp():
    """s = 300: a row whose float64 logits spread further than 88 (exp(-88) is the smallest normal fp32), on every graph; s = 1 is flat"""
    for graph in G.GRAPHS:
        for s, want in ((1, False), (300, True)):
            r = G.refine_reference(('unit', 'cloud', s), graph)
            lg, q = G.layer0_logits(r['sd'], r['cfg'], r['h'], r['x'], r['f64_nbr'], G.PACK.mask)
            hi = torch.where(lg.isnan(), torch.full_like(lg, -math.inf), lg).amax(1)
            lo = torch.where(lg.isnan(), torch.full_like(lg, math.inf), lg).amin(1)
            assert bool(((hi - lo) > 88.0).any()) == want, (graph, s, float((hi - lo).max()))
            if s == 300:
                assert 400.0 < float(q.abs().max()) < 500.0


def test_zero_rows_query_is_the_bias_path():
    r = G.refine_reference(('zero', 'cloud', 1), 'knn32')
    rows = G.zero_rows()
    assert len(rows) >= 53 and bool((r['h'][rows] == 0).all()) and bool((r['h'][[i for i in range(G.PACK.N) if i not in rows]] != 0).any(1).all())
    _, q = G.layer0_logits(r['sd'], r['cfg'], r['h'], r['x'], r['f64_nbr'], G.PACK.mask)
    q0 = R._mlp(r['sd'], 'refine_net.base_block.0.x2h_layers.0.hq_func', torch.zeros(1, 128, dtype=torch.float64), torch.float64)
    assert torch.equal(q[rows], q[rows[:1]].expand(len(rows), -1)) and maxdiff(q[rows[0]], q0[0]) < 1e-12 and float(q0.abs().max()) > 0.5
    assert {0, 1} <= set(rows)                                                                    # both rows of the (1, 1) graph


def test_mixed_decades_all_present():
    groups = G.decade_groups(G.features('mixed'))
    assert set(groups) == set(range(-6, 4)) and all(len(rows) >= 5 for rows, _ in groups.values())
    assert set(G.decade_groups(G.features('zero'))) == {None, 0}


@pytest.mark.parametrize('case', [('unit', 'cloud', 1), ('mixed', 'cloud', 1), ('large', 'cloud', 1), ('unit', 'cloud', 300)], ids=G.case_id)
def test_rule_is_not_vacuous(case):
    """The fp32 restatement passes its own rule; a result 3 r64 + TOL_FWD away from it in one element (of the group with the smallest rows, where
    the inputs are grouped) does not."""
    from _tol import MARGINS
    r = G.refine_reference(case, 'knn32')
    recorded = len(MARGINS)
    for key in ('h', 'x'):
        h_in = r['h'] if key == 'h' and case[0] in G.GROUPED else None
        f32, f64 = r['f32'][key], r['f64'][key]
        G.check(f32, f32, f64, ('self', key), h_in=h_in)
        if h_in is None:
            rows, extra = torch.arange(f64.shape[0]), 0.0
        else:
            rows, gmax = min(G.decade_groups(h_in).values(), key=lambda g: g[1])
            extra = 2.0 ** -22 * gmax
        r64 = maxdiff(f32[rows], f64[rows])
        bad = f64.clone()
        bad[rows[0], 0] += 3.0 * r64 + TOL_FWD + extra
        with pytest.raises(AssertionError, match='tolerance'):
            G.check(bad, f32, f64, ('perturbed', key), h_in=h_in)
    nan = r['f32']['h'].clone()
    nan[5, 5] = float('nan')
    with pytest.raises(AssertionError, match='not finite'):
        G.check(nan, r['f32']['h'], r['f64']['h'], 'nan')
    del MARGINS[recorded:]                 # the comparisons made to fail here are not margins of the suite


@pytest.mark.parametrize('geom', G.GEOMETRIES)
@pytest.mark.parametrize('feat', G.EGNN_FEATURES)
def test_egnn_references_finite_on_one_graph(feat, geom):
    r = G.egnn_reference(feat, geom)
    for name in ('f32', 'f64'):
        assert bool(torch.isfinite(r[name]['h']).all()) and bool(torch.isfinite(r[name]['x']).all()), (feat, geom, name)
    assert torch.equal(r['f32_nbr'], r['f64_nbr'])
    assert float(r['f64']['h'].abs().max()) < 1e4


@pytest.mark.parametrize('geom', G.GEOMETRIES[1:])
def test_model_references_finite(geom):
    r = G.model_reference(geom)
    assert all(bool(torch.isfinite(r[n][k]).all()) for n in ('f32', 'f64') for k in ('pred_ligand_pos', 'pred_ligand_v', 'final_h'))
    if geom == 'offset':
        assert float(r['f64']['pred_ligand_pos'].min()) > 400.0         # nothing centred the positions
