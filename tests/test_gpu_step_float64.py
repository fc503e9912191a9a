"""The diffusion-step kernels (csrc/misc.hip) and the likelihood kernels (csrc/likelihood.hip) through capi against the float64 restatement of
tests/_step_ref.py, over its cases: graphs of 1, 63, 64, 65, 130, 0 and 7 atoms, time steps at both ends of the schedule, logits saturated to
a log-softmax of -300, the perfect prediction, coordinates 30 times out, uniform draws at the ends of [0, 1) and an exact tie, 13, 16 and 2
classes, program rows of every kind, known atoms, the head's softplus on both sides of its threshold.  Needs an MI355X: ``-m gpu``.

The rule (tests/_step_ref.py): |HIP - float64| <= max(floor, 2 x |fp32 restatement - float64|) per output; sampled types
equal the float64 argmax wherever its top-two margin exceeds 1e-4.  tests/test_step_ref_host.py shows on the CPU that the cases are what they
claim, that the restatement reproduces the recordings of the real reference, and that the rule rejects every planted defect.  With
tests/test_gpu_step_variants.py holding the session and graph forms bit-equal to the stateless call, the float64 result carries to every form."""
import os

import pytest
import torch

import _step_ref as S

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
_HANDLES = {}
FIGURES = bool(os.environ.get('TD_STEP_FIGURES'))          # print r64 / d64 / bound of every comparison (the table of EXPERIMENTS.md; run with -s)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


def _native(C, mean_type='C0'):
    """a one-layer handle of C classes, cached for the module"""
    from targetdiff_amd import capi
    if (C, mean_type) not in _HANDLES:
        dev = _dev()
        sched = {k: v.numpy() for k, v in S.schedules().items()}
        with torch.cuda.device(dev):
            _HANDLES[(C, mean_type)] = capi.NativeModel(S.native_config(C, mean_type), S.state_dict(C), sched, device=dev)
    return _HANDLES[(C, mean_type)]


def _lptr(nat, dev):
    ptr = nat.graph_ptr(S.BATCH.to(dev), S.B)
    assert ptr.cpu().tolist() == S.PTR            # the empty graph in the middle included
    return ptr


def _figure(case, op, out, r64, d64, bound):
    if FIGURES:
        print(f'FIG {case} {op} {out} r64 {r64:.3e} d64 {d64:.3e} bound {bound:.3e}')


def _order(figs):
    d64, r64, bound = figs
    return r64, d64, bound


def _report(case, op, rows):
    for out, ok, d, r64, bound, why in rows:
        _figure(S.case_id(case), op, out, r64, d, bound)


def _posterior(case, form, dev, in_place=False):
    kw, mean_type, _ = S.posterior_call(case, form)
    C = case[1]
    nat = _native(C, mean_type)
    d = {k: v.to(dev).contiguous() for k, v in kw.items()}
    d['t'] = d['t'].int()
    out = dict(log_v0=torch.full((S.N, C), float('nan'), device=dev), log_post=torch.full((S.N, C), float('nan'), device=dev))
    if in_place:
        out.update(pos_next=d['ligand_pos'], v_next=d['ligand_v'])
    else:
        out.update(pos_next=torch.full((S.N, 3), float('nan'), device=dev), v_next=torch.full((S.N,), -1, dtype=torch.int64, device=dev))
    t = d.pop('t')
    pos, v = nat.posterior_step(t, _lptr(nat, dev), **d, **out)
    assert pos.data_ptr() == out['pos_next'].data_ptr() and v.data_ptr() == out['v_next'].data_ptr()
    if not in_place:            # the inputs stay as they were
        assert torch.equal(d['ligand_pos'].cpu(), kw['ligand_pos']) and torch.equal(d['ligand_v'].cpu(), kw['ligand_v'])
    return dict(pos=pos.cpu(), v=v.cpu(), log_v0=out['log_v0'].cpu(), log_post=out['log_post'].cpu())


def _renoise(case, op, dev, in_place=False):
    i = S.inputs(case)
    C = case[1]
    nat = _native(C)
    po = op.endswith('_pos_only')
    row = S.program_rows()[op[len('renoise_'):-len('_pos_only')] if po else op[len('renoise_'):]][0].to(dev)
    pos_in, v_in = i['x_t'].to(dev), i['v_t'].to(dev)
    out = {} if po else dict(log_v0=torch.full((S.N, C), float('nan'), device=dev), log_q=torch.full((S.N, C), float('nan'), device=dev))
    if in_place:
        out.update(pos_next=pos_in, v_next=v_in)
    pos, v = nat.renoise_step(row, pos_in, v_in, i['noise'].to(dev), None if po else i['uniform'].to(dev), **out)
    got = dict(pos=pos.cpu(), v=v.cpu())
    if not po:
        got.update(log_v0=out['log_v0'].cpu(), log_post=out['log_q'].cpu())
    return got


@pytest.mark.parametrize('case', S.CASE_IDS, ids=S.case_id)
def test_posterior_step_vs_float64(case):
    """td_posterior_step plain, with known atoms, with a shift of x0, with model_mean_type 'noise', and with a program row of 1 level, of 130
    levels and of the last slot, each with and without known atoms: pos_next, log_v0 and log_post by the rule, v_next by the margin rule."""
    dev = _dev()
    for form in S.FORMS:
        op = f'posterior_{form}'
        got = _posterior(case, form, dev)
        assert bool((got['v'] >= 0).all()) and bool((got['v'] < case[1]).all())
        _report(case, op, S.judge(op, case, got, asserting=True))
        f64 = S.reference(op, case, F64)
        if 'fixed' in form:          # a known atom of a step that ends on clean data is its known state, bit for bit
            i = S.inputs(case)
            k = f64['forced']
            assert torch.equal(got['pos'][k], i['x0'][k]) and torch.equal(got['v'][k], i['v0'][k])


@pytest.mark.parametrize('case', S.CASE_IDS, ids=S.case_id)
def test_renoise_step_vs_float64(case):
    """td_renoise_step over 1 level (rho next to 1) and from level 0 to 999, with the type draw and without (pos_only: the types stay)"""
    dev = _dev()
    for op in S.RENOISE_OPS:
        got = _renoise(case, op, dev)
        _report(case, op, S.judge(op, case, got, asserting=True))
        if op.endswith('_pos_only'):
            assert torch.equal(got['v'], S.inputs(case)['v_t'])


@pytest.mark.parametrize('case', S.CASE_IDS, ids=S.case_id)
def test_perturb_vs_float64(case):
    """perturb_kernel on its own: x_t by the rule, v_t by the margin rule, per-graph time steps across an empty graph"""
    dev = _dev()
    i = S.inputs(case)
    nat = _native(case[1])
    pos_t, v_t = nat.perturb(i['t'].int().to(dev), _lptr(nat, dev), i['x0'].to(dev), i['v0'].to(dev), i['noise'].to(dev), i['uniform'].to(dev))
    _report(case, 'perturb', S.judge('perturb', case, dict(pos=pos_t.cpu(), v=v_t.cpu()), asserting=True))


@pytest.mark.parametrize('case', S.CASE_IDS, ids=S.case_id)
def test_likelihood_kernels_vs_float64(case):
    """likelihood_terms_kernel and likelihood_prior_kernel called directly on the case's predictions, no network in front: per graph,
    |x - f64| / max(|f64|, 1e-2) by the rule, floor 2e-6 (for kl_v, on graphs where it is small, one fp32 ulp of ln K if that is more:
    _step_ref.floor_of).  The empty graph gives exactly 0; where the prediction is perfect the KL terms are also held in absolute terms (they
    cancel to 0): floor 2e-8, the relative floor at its smallest denominator."""
    dev = _dev()
    i = S.inputs(case)
    nat = _native(case[1])
    lptr = _lptr(nat, dev)
    D = lambda k: i[k].to(dev)
    empty = S.SIZES.index(0)
    kp, kv = nat.likelihood_terms(i['t'].int().to(dev), lptr, D('x0'), D('x_t'), D('v0'), D('v_t'), D('pred_pos'), D('pred_v'))
    got = dict(kl_pos=kp.cpu(), kl_v=kv.cpu())
    _report(case, 'likelihood_terms', S.judge('likelihood_terms', case, got, asserting=True))
    assert float(got['kl_pos'][empty]) == 0 and float(got['kl_v'][empty]) == 0
    if 'perfect' in case[0]:
        f32, f64 = S.reference('likelihood_terms', case, F32), S.reference('likelihood_terms', case, F64)
        kl = i['t'] > 0
        for out in ('kl_pos', 'kl_v'):
            r64 = S.distance(f32[out][kl], f64[out][kl])
            bound = max(S.FLOOR['kl'] * S.KL_DEN, S.FACTOR * r64)
            d64 = S.close(got[out][kl], f64[out][kl], bound, f'{S.case_id(case)} perfect {out} absolute')
            _figure(S.case_id(case), 'likelihood_terms_perfect_abs', out, r64, d64, bound)
    kp, kv = nat.likelihood_prior(lptr, D('x0'), D('v0'))
    got = dict(kl_pos=kp.cpu(), kl_v=kv.cpu())
    _report(case, 'likelihood_prior', S.judge('likelihood_prior', case, got, asserting=True))
    assert float(got['kl_pos'][empty]) == 0 and float(got['kl_v'][empty]) == 0


@pytest.mark.parametrize('C', S.CLASSES)
def test_head_and_embedding_vs_float64(C):
    """td_v_inference on 1, 7, 8, 9 and 330 free-standing rows whose pre-activations reach from -100 to 100 (the softplus threshold crossed, one
    row all zero): by the rule over all rows of the call (floor TOL_FWD), and again per group of rows of one scale (floor: _step_ref.head_floor),
    so that the rows of large scale do not set the bound of the small ones.  td_embed_ligand on the same row counts, its node-indicator column
    exactly 1."""
    dev = _dev()
    nat = _native(C)
    sd = S.state_dict(C)
    h, grp = S.head_rows(C)
    f32, f64 = S.v_inference(sd, h, F32), S.v_inference(sd, h, F64)
    for n in S.HEAD_ROWS:
        got = nat.v_inference(h[:n].contiguous().to(dev))
        _figure(f'head-C{C}', 'v_inference', f'n{n}', *_order(S.check(got, f32[:n], f64[:n], S.FLOOR['fwd'], f'v_inference C{C} n{n}')))
        _figure(f'head-C{C}', 'v_inference_grouped', f'n{n}',
                *_order(S.check(got, f32[:n], f64[:n], S.head_floor, f'v_inference C{C} n{n}', groups=grp[:n])))
        v = torch.arange(n) % C
        e = nat.embed_ligand(v.to(dev))
        assert e.shape == (n, 128) and bool((e[:, 127] == 1).all())
        _figure(f'head-C{C}', 'embed_ligand', f'n{n}',
                *_order(S.check(e, S.embed_ligand(sd, v, F32), S.embed_ligand(sd, v, F64), S.FLOOR['fwd'], f'embed_ligand C{C} n{n}')))


@pytest.mark.parametrize('case', [('sat30', 13), ('all0', 2)], ids=S.case_id)
def test_in_place_forms_are_bit_identical(case):
    """pos_next = ligand_pos and v_next = ligand_v, the form the session uses: every output equals the out-of-place call's bit for bit"""
    dev = _dev()
    for form in S.FORMS:
        a, b = _posterior(case, form, dev), _posterior(case, form, dev, in_place=True)
        for k in a:
            assert torch.equal(a[k], b[k]), (form, k)
    for op in S.RENOISE_OPS:
        a, b = _renoise(case, op, dev), _renoise(case, op, dev, in_place=True)
        for k in a:
            assert torch.equal(a[k], b[k]), (op, k)
