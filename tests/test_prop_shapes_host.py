"""Affinity predictor over its supported range, CPU side (tests/_prop_shapes_ref.py cases): the float64 restatement reproduces the real
reference's float64 outputs and gradient projections (tests/golden/prop_shapes.npz, tools/make_golden_prop_shapes.py), so the GPU tests
are judged against the reference's arithmetic; the fp32 reference's own distance r from float64 leaves the GPU bound at TOL_GRAD; and
every case still has the property it is in the table for."""
import json

import numpy as np
import pytest
import torch

import _prop_grad_ref as PG
import _prop_ref as P
import _prop_shapes_ref as S
from conftest import load_golden

NAMES = list(S.CASES)
TOL_F64 = 1e-10


@pytest.fixture(scope='module')
def golden():
    return load_golden('prop_shapes.npz')


def _rel(a, b, scale):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) / scale


def test_fixture_holds_every_case_and_nothing_else(golden):
    entries = {'keys', 'loss', 'norm', 'proj', 'r', 'crc', 'out'}
    assert {k.split('/')[0] for k in golden} == set(NAMES)
    for name in NAMES:
        have = {k.split('/', 1)[1] for k in golden if k.startswith(name + '/')}
        assert have == (entries - {'out'} if name in S.LARGE else entries), name
        assert golden[f'{name}/proj'].shape == (len(json.loads(str(golden[f'{name}/keys']))), PG.NDIR)


@pytest.mark.parametrize('name', NAMES)
def test_restatement_matches_reference(name, golden):
    """Outputs, loss, and every parameter's gradient norm and 16 projections, float64 against float64."""
    case, cfg, sd32, inp, out_kind, y, enc, up = S.load(name)
    assert int(golden[f'{name}/crc']) == int(S.inputs_crc(inp, enc)), 'the case table no longer gives the inputs the fixture was made from'
    loss, out, grads = S.restate_grads(name)
    if name not in S.LARGE:
        ref = golden[f'{name}/out']
        assert out.shape == ref.shape
        assert _rel(out.numpy(), ref, max(1.0, float(np.max(np.abs(ref))))) < TOL_F64
    scale = float((out.abs() * torch.as_tensor(np.abs(up), dtype=torch.float64)).sum()) if up is not None else abs(float(golden[f'{name}/loss']))
    assert _rel(loss.item(), golden[f'{name}/loss'], max(1.0, scale)) < TOL_F64
    keys, norm, proj = S.summarize(case, grads)
    assert keys == json.loads(str(golden[f'{name}/keys']))
    for i, k in enumerate(keys):
        n = float(golden[f'{name}/norm'][i])
        if n == 0.0:                       # no gradient in the reference (no edge, no protein atom, ...): none in the restatement
            assert float(grads[k].abs().max()) == 0.0, k
            continue
        assert abs(norm[i] - n) / n < TOL_F64, k
        assert _rel(proj[i], golden[f'{name}/proj'][i], n) < TOL_F64, k


@pytest.mark.parametrize('name', NAMES)
def test_fp32_reference_distance_keeps_the_bound(name, golden):
    """r <= TOL_GRAD / 2: the GPU bound max(TOL_GRAD, 2 r) is TOL_GRAD for every case but the gain-3 one."""
    r = float(golden[f'{name}/r'])
    print(f'{name}: fp32 reference vs float64, r = {r:.3e}')
    assert r > 0.0
    if name in S.GAIN_CASES:
        assert r < 1e-3
    else:
        assert r <= S.TOL_GRAD / 2


@pytest.mark.parametrize('name', NAMES)
def test_no_relu_kink_beyond_what_the_table_records(name):
    """The seed rule of _prop_shapes_ref (KINK_WINDOW): flipping a ReLU that is within fp32 rounding of zero moves no gradient by more
    than TOL_GRAD / 4 of its tensor's max |g|, or by what KINK_RESIDUAL records for the case."""
    e, where, near = S.kink_exposure(name)
    print(f'{name}: {near} ReLU units within {S.KINK_WINDOW:.1e} of zero, largest exposure {e:.3e} ({where})')
    assert e <= S.KINK_RESIDUAL.get(name, S.TOL_GRAD / 4)


# ------------------------------------------------------------------------------------------ the cases keep their properties
def _sizes(case):
    return [n_p + n_l for n_p, n_l in case.complexes]


def test_table_covers_what_it_is_for():
    C = S.CASES
    fan = {c.knn: c for n, c in C.items() if n.startswith('fan_')}
    assert set(fan) == {1, 5, 15, 16, 17, 33, 47, 63, 64} and {c.layers for c in fan.values()} == {1, 2, 3}
    for k, c in fan.items():
        n = _sizes(c)
        assert min(n) < k + 1 and k + 1 in n and max(n) > k + 1
    assert {c.layers for n, c in C.items() if n.startswith('layers_')} == {1, 2, 7}
    assert all(c.knn == 48 for n, c in C.items() if n.startswith('layers_'))
    rows = [c for n, c in C.items() if n.startswith('rows_')]
    assert sorted(sum(_sizes(c)) for c in rows) == [1, 2, 3, 4, 5, 15, 16, 17, 32] and {len(c.complexes) for c in rows} == {1, 2, 5}
    assert C['rows_n1'].complexes == ((1, 0),)
    n16 = _sizes(C['rows_n16'])
    assert n16[0] == n16[2] == n16[4] == 1
    assert any(n_l == 0 < n_p for c in rows for n_p, n_l in c.complexes) and any(n_p == 0 < n_l for c in rows for n_p, n_l in c.complexes)
    assert (0, 0) in C['rows_n17'].complexes[1:-1]
    wid = [c for n, c in C.items() if n.startswith('widths_')]
    for i in range(3):
        assert {c.widths[i] for c in wid} == {0, 1, 3, 17, 65}
    assert {c.widths[3] for c in wid} == {1, 2, 5} and all(c.loss == 'up' and c.kind == 'enc' for c in wid)
    ks = [K for c in wid for K in (P.LIGAND_FEAT_DIM + c.widths[0], 256 + c.widths[1], 256 + c.widths[2])]
    assert any(K % 4 for K in ks) and any(K % 64 for K in ks) and P.PROTEIN_FEAT_DIM % 4
    nk = lambda n: sum(_sizes(C[n])) * C[n].knn
    assert nk('red_1024') == 1024 and nk('red_1025') == 1025
    assert 65536 < nk('red_cap') < 65536 + 1024 and sum(_sizes(C['red_cap'])) % 4 and C['red_cap'].knn == 64
    assert sum(_sizes(C['red_scan1025'])) == 1025 and sum(_sizes(C['red_scan2049'])) == 2049
    assert 16384 < sum(_sizes(C['red_grid'])) < 16384 + 16 and sum(_sizes(C['red_grid'])) % 4
    assert all(C[n].layers == 1 for n in C if n.startswith('red_')) and all(C[n].knn == 4 for n in ('red_scan1025', 'red_scan2049', 'red_grid'))
    # the workspace-reuse test runs these two through one model
    assert S.spec('rows_n1') == S.spec('red_cap') and C['rows_n1'].knn == C['red_cap'].knn == 64


@pytest.mark.parametrize('name', ['hub_k1', 'hub_k64'])
def test_hub_is_in_every_neighbour_list(name):
    n = sum(S.CASES[name].complexes[0])
    nbr = S.restate(name)['nbr'][:n]
    assert n == {'hub_k1': 13, 'hub_k64': 221}[name]
    others = np.delete(np.arange(n), S.HUB_AT)
    assert all(S.HUB_AT in nbr[i] for i in others), 'the hub is not a neighbour of every other node of its complex'
    assert int((nbr == S.HUB_AT).sum()) == n - 1


@pytest.mark.parametrize('k', [5, 48])
def test_geometry_cases(k):
    inp = S.load(f'lattice_k{k}')[3]
    x = np.concatenate([inp['protein_pos'][inp['batch_protein'] == 0], inp['ligand_pos'][inp['batch_ligand'] == 0]]).astype(np.float64)
    assert len(x) == 64 and len(np.unique(x, axis=0)) == 64 and set(np.unique(x)) == {0.0, 1.5, 3.0, 4.5}
    inp = S.load(f'coincident_k{k}')[3]
    assert np.array_equal(inp['ligand_pos'][0], inp['protein_pos'][3]) and np.array_equal(inp['ligand_pos'][5], inp['ligand_pos'][2])
    r = S.restate(f'coincident_k{k}')
    assert r['nbr'][40, 0] == 3 and r['nbr'][3, 0] == 40 and r['nbr'][42, 0] == 45 and r['nbr'][45, 0] == 42      # d = 0 comes first
    r = S.restate(f'sparse_k{k}')
    assert r['rbf'].numel() > 0 and float(r['rbf'].max()) < 1e-30
    inp = S.load(f'sparse_k{k}')[3]
    for b in (0, 1):
        x = np.concatenate([inp['protein_pos'][inp['batch_protein'] == b], inp['ligand_pos'][inp['batch_ligand'] == b]]).astype(np.float64)
        d = np.linalg.norm(x[:, None] - x[None], axis=-1) + 1e9 * np.eye(len(x))
        assert d.min() >= 12.0


def test_softplus_case_straddles_the_threshold():
    z = S.restate('ssp_gain3')['out_pre']
    assert bool((z > 20).any()) and bool((z < 20).any())
    # and not only far from it: torch's softplus switches to the identity above 20, where log1p(exp(z)) - z is 2e-9
    assert int(((z > 0) & (z < 20)).sum()) > 0 and int(((z > 20) & (z < 200)).sum()) > 0
    print(f'out_block.0 pre-activations: {int((z > 20).sum())} above 20, {int((z < 20).sum())} below, range {float(z.min()):.1f} .. {float(z.max()):.1f}')


def test_permutations_are_what_they_say():
    case, cfg, sd32, inp, out_kind, y, enc, up = S.load('widths_3_17_65_o5')
    mixed, e = S.interleaved(inp, enc)
    assert not np.array_equal(mixed['batch_protein'], inp['batch_protein'])
    a = P.restate(sd32, cfg, inp, None, enc['ligand'], enc['node'], enc['graph'])
    b = P.restate(sd32, cfg, mixed, None, e['ligand'], e['node'], e['graph'])
    assert torch.equal(a['out'], b['out']) and torch.equal(a['h_layers'], b['h_layers'])          # the same composed batch
    shuf, e = S.shuffled(inp, enc)
    c = P.restate(sd32, cfg, shuf, None, e['ligand'], e['node'], e['graph'])
    assert P.rel_err(c['out'], a['out']) < TOL_F64 and not np.array_equal(c['order'], a['order'])
