"""Binding-affinity predictor on the GPU, forward and backward, over its whole supported range: every case of tests/_prop_shapes_ref.py
(fan-in 1..64 with partial edge blocks, 1..7 layers, N from 1 to 16,386, complexes of one node / without ligand / without protein /
without any atom, enc_* widths and output widths that are no multiple of 4, split-K chunk boundaries and cap, the reverse-adjacency
scan and a 220-entry hub, lattice / coincident / far-apart geometry, softplus on both sides of its threshold) against the float64
restatement run on the CPU here, which tests/test_prop_shapes_host.py ties to the real reference.

Per case: the k-NN table exactly; out and every layer's h at TOL_PROP (relative, as tests/test_gpu_prop.py); every parameter's
gradient element by element, relative to that tensor's max |g|, at max(TOL_GRAD, 2 r) (r = the fp32 reference's own distance from
float64, tests/golden/prop_shapes.npz; the rule of test_gpu_prop_train.test_gradient_parity) -- a tensor whose float64 gradient is
identically zero must be exactly zero; bit-identical reruns; and, for batches of two or more complexes, two permutations of the atoms:
  interleaved  complexes mixed, every complex's atoms in their order: the composed batch is the same, so every bit must be
  shuffled     `unsorted` of test_gpu_prop_train.py, which also reorders the atoms inside a complex: the rows of a complex, the order
               of its sums and the index deciding a k-NN tie change with it, so it is held to the float64 restatement of the
               shuffled batch at the same bounds, not to the sorted run's bits.
"""
import numpy as np
import pytest
import torch

import _prop_ref as P
import _prop_shapes_ref as S
from _tol import close
from conftest import load_golden
from targetdiff_amd import prop
from test_gpu_prop import TOL_PROP, rel_close
from test_gpu_prop_train import TOL_GRAD, TOL_LOSS

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAMES = list(S.CASES)
assert TOL_GRAD == S.TOL_GRAD


@pytest.fixture(scope='module')
def golden():
    return load_golden('prop_shapes.npz')


def build(case, sd32):
    m = S.build_model(case, prop)
    m.load_state_dict(sd32, strict=True)
    return m.to(DEV)


def args_of(case, inp, out_kind, enc):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    a = [t(inp[k]) for k in ('protein_pos', 'protein_feat', 'ligand_pos', 'ligand_feat', 'batch_protein', 'batch_ligand')] + [t(out_kind)]
    if case.kind == 'enc':
        a += [t(enc.get('ligand')), t(enc.get('node')), t(enc.get('graph'))]
    return a


def run(m, case, inp, out_kind, y, enc, up):
    """One plain forward with the extras and one differentiable forward + backward: dict(out, h_layers, final_h, nbr, loss, grads)."""
    a = args_of(case, inp, out_kind, enc)
    out, extra = m(*a, return_extra=True)
    m.zero_grad(set_to_none=True)
    diff = m(*a, differentiable=True)
    assert torch.equal(out, diff.detach()), 'differentiable=True changed the forward'
    if up is not None:
        loss = (diff * torch.from_numpy(up).to(DEV)).sum()
    else:
        loss = torch.nn.functional.mse_loss(diff.view(-1), torch.from_numpy(y).to(DEV))
    loss.backward()
    return dict(out=out, loss=loss.detach(), grads={k: p.grad.detach().clone() for k, p in m.named_parameters()}, **extra)


def same_bits(a, b, what, extras=True):
    for k in ('out', 'loss') + (('h_layers', 'final_h', 'nbr') if extras else ()):
        assert torch.equal(a[k], b[k]), f'{what}: {k} differs'
    for k in a['grads']:
        assert torch.equal(a['grads'][k], b['grads'][k]), f'{what}: d{k} differs'


def against_float64(got, name, order, bound, inp, cfg, sd32, out_kind, enc, up):
    """nbr exactly; out, per-layer h, loss and every gradient against the float64 restatement of the batch in `order`."""
    inp, enc = S.PERMUTATIONS[order](inp, enc)
    fwd = P.restate(sd32, cfg, inp, output_kind=out_kind, enc_ligand=enc.get('ligand'), enc_node=enc.get('node'), enc_graph=enc.get('graph'))
    loss64, out64, g64 = S.restate_grads(name, order)
    assert torch.equal(got['nbr'].cpu().long(), torch.from_numpy(fwd['nbr'])), f'{name} {order}: k-NN table differs from knn_table'
    assert got['out'].shape == out64.shape
    worst_fwd = rel_close(got['out'], out64, TOL_PROP, f'{name} {order} out')
    for l in range(fwd['h_layers'].shape[0]):
        worst_fwd = max(worst_fwd, rel_close(got['h_layers'][l], fwd['h_layers'][l], TOL_PROP, f'{name} {order} h of layer {l}'))
    worst, zero = 0.0, []
    for k, ref in g64.items():
        h = got['grads'][k].double().cpu()
        s = float(ref.abs().max())
        if s == 0.0:
            zero.append(k)
            assert torch.equal(h, torch.zeros_like(h)), f'{name} {order}: d{k} is identically zero in float64, not on the GPU'
            continue
        worst = max(worst, close(h / s, ref / s, bound, f'{name} {order} d{k}'))
    print(f'{name} {order}: forward {worst_fwd:.3e} (TOL_PROP {TOL_PROP:.0e}); worst gradient element / max|g| = {worst:.3e} '
          f'(bound {bound:.2e}); {len(zero)} tensors exactly zero; loss {got["loss"].item():.6g} vs {loss64.item():.6g}')
    scale = float((out64.abs() * torch.from_numpy(np.abs(up)).double()).sum()) if up is not None else abs(loss64.item())
    close(torch.tensor(got['loss'].item(), dtype=torch.float64), loss64, TOL_LOSS * max(1.0, scale), f'{name} {order} loss')


@pytest.mark.parametrize('name', NAMES)
def test_case(name, golden):
    """Measured on an MI355X: every id passes, the largest difference / tolerance 0.72 (hub_k64, d edge_inf.0.bias), layers_7_k48 0.27,
    the forward at most 0.07 of TOL_PROP.

    A case can only meet TOL_GRAD if no ReLU that matters sits within fp32 rounding of zero: one such unit evaluated on the other side
    moves one row of a weight gradient by that edge's whole term (seen at 1.2e-4 .. 4.3e-4 on seeds the rule below now refuses, each
    traced on the CPU to single edges with pre-activations 0.04 .. 1.3 unit roundoffs from zero).  The seeds are therefore chosen on
    the CPU (_prop_shapes_ref: ORDERS, KINK_WINDOW): the reference's fp32 run must stay within TOL_GRAD / 2 of float64 under nine
    different orders of its sums."""
    case, cfg, sd32, inp, out_kind, y, enc, up = S.load(name)
    bound = max(TOL_GRAD, 2 * float(golden[f'{name}/r']))
    m = build(case, sd32)
    first = run(m, case, inp, out_kind, y, enc, up)
    against_float64(first, name, 'sorted', bound, inp, cfg, sd32, out_kind, enc, up)
    same_bits(first, run(m, case, inp, out_kind, y, enc, up), f'{name}: rerun')
    if len(case.complexes) >= 2:
        mixed, e = S.interleaved(inp, enc)
        same_bits(first, run(m, case, mixed, out_kind, y, e, up), f'{name}: complexes interleaved')
        shuf, e = S.shuffled(inp, enc)
        against_float64(run(m, case, shuf, out_kind, y, e, up), name, 'shuffled', bound, inp, cfg, sd32, out_kind, enc, up)


def test_workspace_reuse():
    """One td_prop handle: the split-K cap case (1,030 nodes, 65,920 edges), the lone one-node complex, the cap case again.  Padded
    slots and the cnt / rptr / ridx buffers must not depend on what the call before left behind: every call gives the bits of a
    freshly built model."""
    big, tiny = S.load('red_cap'), S.load('rows_n1')
    case, sd32 = big[0], big[2]
    m = build(case, sd32)
    m(*args_of(case, big[3], big[4], big[6]))
    handle = m._native
    for step, (c, cfg, _, inp, out_kind, y, enc, up) in enumerate((big, tiny, big)):
        got = run(m, case, inp, out_kind, y, enc, up)
        assert m._native is handle, 'a new td_prop handle was built'
        same_bits(got, run(build(case, sd32), case, inp, out_kind, y, enc, up), f'call {step} ({c.name}) on a used handle vs a fresh model')
