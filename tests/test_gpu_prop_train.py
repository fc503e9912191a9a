"""Binding-affinity predictor training on the GPU (td_prop_forward_train / td_prop_backward / td_prop_set_weights through
PropPredNet(Enc).get_loss and forward(differentiable=True)).

Gradient parity: every parameter's HIP gradient against float64 autograd of the restatement (_prop_ref.restate, run on the CPU here),
element by element at full size, each error relative to that tensor's max |g|; the bound is max(TOL_GRAD, 2 r), r = the reference's
own fp32 distance from float64 for the fixture (tools/make_golden_prop_grad.py).  Also: the fixtures' projections, bit-identical
forward outputs and reruns, pack linearity, Adam steps against a float64 Adam, the on-device weight refresh and get_loss's noise.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import _prop_grad_ref as PG
import _prop_ref as P
from _tol import close
from conftest import load_golden
from targetdiff_amd import capi, prop

pytestmark = pytest.mark.gpu

TOL_GRAD = 1e-4
TOL_LOSS = 2e-5          # relative, as TOL_PROP of the forward (tests/test_gpu_prop.py); for sum(out * U), relative to sum |out * U|
DEV = 'cuda:0'
CASES = list(PG.CASES)


def build(kind, sd32):
    cfg = PG.model_config(kind)
    if cfg is None:
        m = prop.PropPredNet(P.MODEL_CONFIG, P.PROTEIN_FEAT_DIM, P.LIGAND_FEAT_DIM)
    else:
        m = prop.PropPredNetEnc(cfg, P.PROTEIN_FEAT_DIM, P.LIGAND_FEAT_DIM, cfg['enc_ligand_dim'], cfg['enc_node_dim'],
                                cfg['enc_graph_dim'], cfg['enc_feature_type'], output_dim=1)
    m.load_state_dict(sd32, strict=True)
    return m.to(DEV)


def args_of(m, inp, out_kind, enc, use_kind=True):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    a = [t(inp[k]) for k in ('protein_pos', 'protein_feat', 'ligand_pos', 'ligand_feat', 'batch_protein', 'batch_ligand')]
    a.append(t(out_kind) if use_kind else None)
    if isinstance(m, prop.PropPredNetEnc):
        a += [t(enc.get('ligand')), t(enc.get('node')), t(enc.get('graph'))]
    return a


def hip_loss(m, inp, out_kind, y, enc, up):
    out = m(*args_of(m, inp, out_kind, enc, up is None), differentiable=True)
    if up is not None:
        return (out * torch.from_numpy(up).to(DEV)).sum(), out
    return torch.nn.functional.mse_loss(out.view(-1), torch.from_numpy(y).to(DEV)), out


def hip_grads(m, inp, out_kind, y, enc, up):
    m.zero_grad(set_to_none=True)
    loss, out = hip_loss(m, inp, out_kind, y, enc, up)
    loss.backward()
    return loss.detach(), out.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def unsorted(inp):
    r = np.random.RandomState(13)
    pp, lp = r.permutation(len(inp['batch_protein'])), r.permutation(len(inp['batch_ligand']))
    return dict(protein_pos=inp['protein_pos'][pp], protein_feat=inp['protein_feat'][pp], batch_protein=inp['batch_protein'][pp],
                ligand_pos=inp['ligand_pos'][lp], ligand_feat=inp['ligand_feat'][lp], batch_ligand=inp['batch_ligand'][lp])


@pytest.mark.parametrize('name,order', [(c, 'sorted') for c in CASES] + [('prop_grad_kind', 'unsorted')])
def test_gradient_parity(name, order):
    g, kind, cfg, sd32, inp, out_kind, y, enc, up = PG.load_case(name, load_golden)
    if order == 'unsorted':
        inp = unsorted(inp)
    bound = max(TOL_GRAD, 2 * float(g['r']))
    m = build(kind, sd32)
    loss, out, gh = hip_grads(m, inp, out_kind, y, enc, up)
    loss64, out64, g64 = PG.restate_grads(sd32, cfg, inp, out_kind, y, enc, up)
    worst = 0.0
    top = max(float(ref.abs().max()) for ref in g64.values())
    for k, ref in g64.items():
        h = gh[k].double().cpu()
        # a tensor whose every unit is dead (ReLU off on every edge: the gain-3 weights) has no gradient: measured against the
        # largest |g| of the model instead
        s = float(ref.abs().max()) or top
        d = close(h / s, ref / s, bound, f'{name} {order} d{k}')
        worst = max(worst, d)
        if order == 'sorted':
            n = float(g[f'f64/norm/{k}']) or float(np.sqrt(h.numel())) * top
            pr = (PG.directions(k, h.shape) @ h.reshape(-1)).numpy()
            close(torch.from_numpy(pr / n), torch.from_numpy(g[f'f64/proj/{k}'] / n), bound, f'{name} proj d{k}')
    print(f'{name} {order}: worst element error / max|g| = {worst:.3e} (bound {bound:.2e}); loss {loss.item():.6g} vs {loss64.item():.6g}')
    scale = float((out64.view(-1) * torch.from_numpy(up).double().view(-1)).abs().sum()) if up is not None else abs(loss64.item())
    close(torch.tensor(loss.item(), dtype=torch.float64), loss64, TOL_LOSS * max(1.0, scale), f'{name} loss')


@pytest.mark.parametrize('name', CASES)
def test_differentiable_forward_equals_plain_forward_and_reruns_are_identical(name):
    g, kind, cfg, sd32, inp, out_kind, y, enc, up = PG.load_case(name, load_golden)
    m = build(kind, sd32)
    a = args_of(m, inp, out_kind, enc, up is None)
    plain = m(*a)
    diff = m(*a, differentiable=True)
    assert diff.requires_grad and not plain.requires_grad
    assert torch.equal(plain, diff.detach()), 'differentiable=True changed the forward'
    _, _, g1 = hip_grads(m, inp, out_kind, y, enc, up)
    _, _, g2 = hip_grads(m, inp, out_kind, y, enc, up)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), f'rerun changed d{k}'


def test_pack_linearity():
    """The gradient of a pack's summed output equals the sum of the per-complex gradients (66 mixed complexes)."""
    cx = []
    for s in range(66):
        if s % 3 == 0:
            cx.append(P.complex_1h36(seed=s, jitter=0.3))
        elif s % 3 == 1:
            cx.append(P.synthetic_complex(400 + s, 60 + s, 6 + s % 9, 8.0))
        else:
            cx.append(P.synthetic_complex(500 + s, 16 + s % 12, 4 + s % 5, 5.0))
    sd32 = P.make_state_dict(PG.spec_for('net'), 2030)
    m = build('net', sd32)
    kind = np.array([1 + s % 3 for s in range(len(cx))], np.int64)
    w = np.random.RandomState(3).normal(size=len(cx)).astype(np.float32)
    up = lambda ww: ww.reshape(-1, 1)

    def grads(inp, kk, ww):
        m.zero_grad(set_to_none=True)
        out = m(*args_of(m, inp, kk, {}), differentiable=True)
        (out * torch.from_numpy(up(ww)).to(DEV)).sum().backward()
        return {k: p.grad.double().cpu() for k, p in m.named_parameters()}
    whole = grads(P.batch_of(cx), kind, w)
    parts = [grads(P.batch_of([c]), kind[b:b + 1], w[b:b + 1]) for b, c in enumerate(cx)]
    for k in whole:
        tot = sum(p[k] for p in parts)
        s = float(tot.abs().max()) or 1.0
        close(whole[k] / s, tot / s, TOL_GRAD, f'pack d{k}')


def _batch(inp, kind, y, dev=DEV):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in inp.items()}
    return types.SimpleNamespace(protein_pos=t['protein_pos'], protein_atom_feature=t['protein_feat'], ligand_pos=t['ligand_pos'],
                                 ligand_atom_feature_full=t['ligand_feat'], protein_element_batch=t['batch_protein'],
                                 ligand_element_batch=t['batch_ligand'], kind=torch.from_numpy(kind).to(dev),
                                 y=torch.from_numpy(y).to(dev))


TOL_ADAM = 5e-2          # per tensor: |(p5 - p0)_HIP - (p5 - p0)_float64|_2 / |(p5 - p0)_float64|_2
TOL_ADAM_LOSS = 1e-4     # relative, the loss of every step (an MSE: twice the relative error of out - y, out ~ 100 here)


def test_adam_steps_track_float64():
    g, kind, cfg, sd32, inp, out_kind, y, enc, up = PG.load_case('prop_grad_kind', load_golden)
    m = build(kind, sd32)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4, betas=(0.99, 0.999))
    batch = _batch(inp, out_kind, y)
    sd64 = {k: v.detach().double().requires_grad_(PG.is_param(k)) for k, v in sd32.items()}
    p64 = [v for k, v in sd64.items() if PG.is_param(k)]
    opt64 = torch.optim.Adam(p64, lr=1e-4, betas=(0.99, 0.999))
    for step in range(5):
        opt.zero_grad()
        loss = m.get_loss(batch, pos_noise_std=0.0)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 10)
        opt.step()
        opt64.zero_grad()
        loss64, _ = PG.restate_loss(sd64, cfg, inp, out_kind, y, enc)
        loss64.backward()
        torch.nn.utils.clip_grad_norm_(p64, 10)
        opt64.step()
        close(torch.tensor(loss.item(), dtype=torch.float64), loss64.detach(), TOL_ADAM_LOSS * abs(loss64.item()), f'Adam step {step} loss')
    worst = 0.0
    for k, p in m.named_parameters():
        d64 = sd64[k].detach() - sd32[k].double()
        dh = p.detach().double().cpu() - sd32[k].double()
        rel = float((dh - d64).norm() / d64.norm()) if float(d64.norm()) > 0 else float(dh.norm())
        worst = max(worst, rel)
        close(torch.tensor(rel), torch.tensor(0.0), TOL_ADAM, f'Adam 5 steps {k}')
    print(f'Adam, 5 steps: worst per-tensor relative distance of the parameter change {worst:.3e}')


def test_training_lowers_the_loss():
    g, kind, cfg, sd32, inp, out_kind, y, enc, up = PG.load_case('prop_grad_kind', load_golden)
    m = build(kind, sd32)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4, betas=(0.99, 0.999))
    batch = _batch(inp, out_kind, y)
    losses = []
    for _ in range(100):
        opt.zero_grad()
        loss = m.get_loss(batch, pos_noise_std=0.0)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 10)
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        final = m.get_loss(batch, pos_noise_std=0.0).item()
    print(f'100 Adam steps on one batch: loss {losses[0]:.4g} -> {final:.4g}')
    assert final < losses[0]


def test_weight_refresh_on_device():
    g, kind, cfg, sd32, inp, out_kind, y, enc, up = PG.load_case('prop_grad_enc_all', load_golden)
    m = build(kind, sd32)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    a = args_of(m, inp, out_kind, enc)
    loss = torch.nn.functional.mse_loss(m(*a, differentiable=True).view(-1), torch.from_numpy(y).to(DEV))
    loss.backward()
    handle = m._native
    opt.step()
    after = m(*a)
    assert m._native is handle, 'optimizer.step() made a new td_prop handle'
    fresh = build(kind, {k: v.detach().cpu() for k, v in m.state_dict().items()})
    assert torch.equal(after, fresh(*a)), 'the re-packed weights differ from a freshly built model'
    assert not torch.equal(after, build(kind, sd32)(*a))


def test_get_loss_draws_reference_order_noise():
    g, kind, cfg, sd32, inp, out_kind, y, enc, up = PG.load_case('prop_grad_kind', load_golden)
    m = build(kind, sd32)
    batch = _batch(inp, out_kind, y)
    torch.cuda.manual_seed(1234)
    loss, pred = m.get_loss(batch, pos_noise_std=0.1, return_pred=True)
    torch.cuda.manual_seed(1234)
    pn = torch.randn_like(batch.protein_pos) * 0.1
    ln = torch.randn_like(batch.ligand_pos) * 0.1
    want = m(batch.protein_pos + pn, batch.protein_atom_feature, batch.ligand_pos + ln, batch.ligand_atom_feature_full,
             batch.protein_element_batch, batch.ligand_element_batch, batch.kind)
    assert torch.equal(pred.detach(), want)
    assert torch.equal(loss.detach(), torch.nn.functional.mse_loss(want.view(-1), batch.y))
    with torch.no_grad():
        l2 = m.get_loss(batch, pos_noise_std=0.0)
    assert not l2.requires_grad


def test_backward_refuses_foreign_tapes():
    g, kind, cfg, sd32, inp, out_kind, y, enc, up = PG.load_case('prop_grad_kind', load_golden)
    m = build(kind, sd32)
    a = args_of(m, inp, out_kind, enc)
    m(*a)
    native = m._native
    op, bp = prop._sort_by_complex(a[4])
    ol, bl = prop._sort_by_complex(a[5])
    pptr, lptr = capi.graph_ptr(bp.contiguous(), 3), capi.graph_ptr(bl.contiguous(), 3)
    out, tape = native.forward_train(a[0][op].contiguous(), a[1][op].contiguous(), pptr, a[2][ol].contiguous(), a[3][ol].contiguous(),
                                     lptr, output_kind=a[6])
    rec, ws, (Np, Nl, B) = tape
    gout = torch.ones_like(out)
    with pytest.raises(RuntimeError, match='recorded at'):
        native.backward((rec, ws, (Np, Nl, B - 1)), gout)
    other = build(kind, sd32)
    other(*a)
    with pytest.raises(RuntimeError, match='another td_prop handle'):
        other._native.backward(tape, gout)
    grad = torch.empty(native.num_weights() + 1, device=DEV)
    lib = capi.load_library()
    assert lib.td_prop_backward(native.handle, ctypes.byref(rec), Np, Nl, B, gout.data_ptr(), grad.data_ptr(), grad.numel(), None) == -1
    small = lib.td_prop_train_workspace_bytes(native.handle, Np, Nl, B) - 1
    assert lib.td_prop_forward_train(native.handle, a[0].data_ptr(), a[1].data_ptr(), pptr.data_ptr(), Np, a[2].data_ptr(),
                                     a[3].data_ptr(), lptr.data_ptr(), Nl, B, None, None, None, None, 0, out.data_ptr(),
                                     ws.data_ptr(), small, ctypes.byref(capi.TdPropTape()), None) == -2
    native.set_weights(torch.cat([m.state_dict()[k].reshape(-1) for k in m._flat_keys()]).to(DEV))
    with pytest.raises(RuntimeError, match='weights changed'):
        native.backward(tape, gout)
    with pytest.raises(RuntimeError, match='expected'):
        native.set_weights(torch.zeros(5, device=DEV))
