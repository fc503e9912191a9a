"""Pocket-clash guidance on the MI355X (``-m gpu``; DESIGN.md section 3, "Clash guidance").  The yardstick is the float64 torch statement
of the rule in tests/_guidance_ref.py; the reference has no such mode.

  1. the shift and the report of one ragged pack (protein sizes 1, tile - 1, tile, tile + 77; ligand sizes 0, 1, 5, 37; an atom on a
     protein atom, an atom just outside every radius, atoms above the cap) against float64.  Tolerance per graph, computed at run time:
     8 x the error the plain fp32 torch closed form makes against float64 on the same input, floor 1e-6 A -- another summation order
     costs a small multiple of a plain fp32 evaluation's error, never an order of magnitude.  Pair counts are exact (the pack keeps
     every d_ij 1e-4 A away from sigma_j).
     The reference-side figures are in EXPERIMENTS.md, "Clash guidance"; each case prints its measured margin before it asserts.
  2. determinism: the same call twice, a graph alone and inside the pack: torch.equal;
  3. the guided posterior step bit for bit: a given shift == the unguided step fed fl32(pred_pos + shift); with / without known atoms,
     with / without a program row, at t = 0; a NULL shift and w = 0 == td_posterior_step; model_mean_type 'noise' against the float64
     rule at TOL_X;
  4. sampling: session == stateless, graph replay == launch by launch, both == forward -> clash_shift -> guided posterior composed from
     the public pieces, torch.equal; known atoms' trajectory == the unguided run's; renoise slots are the unguided rule; set / remove /
     set inside one session;
  5. ``guidance=None`` changes nothing;
  6. the batching driver, and ``clash_report`` of its final poses against float64.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import _guidance_ref as GR
from _tol import TOL_X, close
from oracle import draws, weights
from targetdiff_amd import capi, guidance as G, workloads
from targetdiff_amd.guidance import ClashGuidance
from targetdiff_amd.schedule import RENOISE, TimeProgram

pytestmark = pytest.mark.gpu

FLOOR = 1e-6            # A (and A^2 for the energy): the floor of the run-time tolerance
T_SMALL = 5             # levels of the sampling tests' model: five steps end at t = 0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


_CACHE = {}


def _pack(dev):
    """the kernel test's pack and its float64 / fp32 torch references, computed once"""
    if 'pack' not in _CACHE:
        pk = GR.make_pack(capi.CLASH_TILE)
        pk['dev'] = dict(protein=pk['protein'].to(dev), sigma=pk['sigma'].to(dev), x=pk['x'].to(dev),
                         pptr=torch.tensor(pk['pptr'], dtype=torch.int32, device=dev), lptr=torch.tensor(pk['lptr'], dtype=torch.int32, device=dev))
        pk['ref'] = {}
        for w, cap in [(1.0, 0.0), (0.5, pk['max_shift'])]:
            a = (pk['protein'], pk['sigma'], pk['pptr'], pk['x'], pk['lptr'], w, cap)
            pk['ref'][(w, cap)] = (GR.per_graph(GR.shift_closed, *a), GR.per_graph(GR.shift_closed, *a, dtype=torch.float32))
        a = (pk['protein'], pk['sigma'], pk['pptr'], pk['x'], pk['lptr'])
        pk['rep'] = (GR.per_graph(GR.report, *a), GR.per_graph(GR.report, *a, dtype=torch.float32))
        _CACHE['pack'] = pk
    return _CACHE['pack']


def _model(mean_type='C0'):
    key = ('model', mean_type)
    if key not in _CACHE:
        from targetdiff_amd.models import ScorePosNet3D
        m = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG, num_diffusion_timesteps=T_SMALL, model_mean_type=mean_type), 27, 13)
        assert not m.load_state_dict(weights.make_state_dict(2021), strict=False).unexpected_keys
        _CACHE[key] = m.to(_dev()).eval()
    return _CACHE[key]


POCKETS = [(101, 60, 3.0, 9.0), (102, 45, 3.0, 8.0), (103, 38, 3.0, 8.0)]
SIZES = [9, 7, 5]


def _batch(dev):
    if 'batch' not in _CACHE:
        b = workloads.pack_samples([workloads.synthetic_pocket(*p) for p in POCKETS], 1, SIZES)
        g = torch.Generator().manual_seed(77)
        init_pos, init_v = workloads.init_ligand(b, generator=g)
        n = init_pos.shape[0]
        mask = torch.zeros(n, dtype=torch.bool)
        mask[[1, 4, 10, 17]] = True
        cen = torch.stack([b.protein_pos[b.protein_element_batch == k].mean(0) for k in range(3)])
        fixed_pos = cen[b.ligand_element_batch] + 1.2 * torch.randn(n, 3, generator=g)
        fixed_v = torch.randint(0, 13, (n,), generator=g)
        sigma = 3.5 + 1.5 * torch.rand(b.protein_pos.shape[0], generator=g)
        _CACHE['batch'] = (b.to(dev), init_pos.to(dev), init_v.to(dev),
                           dict(fixed_mask=mask.to(dev), fixed_pos=fixed_pos.to(dev), fixed_v=fixed_v.to(dev)), sigma.to(dev))
    return _CACHE['batch']


def _args(dev):
    b, init_pos, init_v, _, _ = _batch(dev)
    return (b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch, init_pos, init_v, b.ligand_element_batch)


def _same(a, b, what):
    for k in ('pos_traj', 'v_traj', 'v0_traj', 'vt_traj'):
        assert len(a[k]) == len(b[k]), (what, k)
        for s, (x, y) in enumerate(zip(a[k], b[k])):
            assert torch.equal(x, y), f'{what}: {k} differs at step {s}'
    assert torch.equal(a['pos'], b['pos']) and torch.equal(a['v'], b['v']), what


def _on_side_stream(dev, fn):
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        out = fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    return out


# ------------------------------------------------------------------------------------------ 1. shift and report against float64
def test_pack_keeps_its_promises():
    """(CPU arithmetic) the float64 reference sees no d_ij within 1e-4 A of sigma_j, and the three special atoms are what they claim"""
    pk = _pack(_dev())
    assert min(GR.per_graph(GR.min_gap, pk['protein'], pk['sigma'], pk['pptr'], pk['x'], pk['lptr'])) > 1e-4
    sp = pk['special']
    assert torch.equal(pk['x'][sp['coincident']], pk['protein'][sp['coincident_protein']])
    assert sp['coincident_protein'] - pk['pptr'][3] >= capi.CLASH_TILE                         # ... of the second tile
    raw64 = torch.cat(pk['ref'][(1.0, 0.0)][0])
    assert torch.equal(raw64[sp['outside']], torch.zeros(3, dtype=torch.float64))
    n = raw64.norm(dim=-1)
    assert float(n[sp['capped']]) > 2 * pk['max_shift'] and int((n > 2 * pk['max_shift']).sum()) >= 5 and int((n > 1.0).sum()) < n.numel()
    assert [c for c, _, _ in pk['rep'][0]] == [c for c, _, _ in pk['rep'][1]]
    assert sum(c for c, _, _ in pk['rep'][0]) > 3 * pk['x'].shape[0]                               # several partners per atom


@pytest.mark.parametrize('w,capped', [(1.0, False), (0.5, True)])
def test_shift_against_float64(w, capped):
    dev = _dev()
    pk = _pack(dev)
    d = pk['dev']
    cap = pk['max_shift'] if capped else 0.0
    got = capi.clash_shift(d['protein'], d['sigma'], d['pptr'], d['lptr'], d['x'], w, cap).cpu()
    r64, r32 = pk['ref'][(w, cap)]
    lp = pk['lptr']
    for g in range(4):
        if lp[g + 1] == lp[g]:
            continue
        err32 = float((r32[g].double() - r64[g]).abs().max())
        tol = max(8 * err32, FLOOR)
        assert tol <= TOL_X, f'graph {g}: tolerance {tol:.2e} above TOL_X: shrink the inputs'
        diff = close(got[lp[g]:lp[g + 1]], r64[g], tol, f'shift, w = {w}, max_shift = {cap}, graph {g}')
        print(f'shift w={w} cap={cap} graph {g}: |kernel - f64| = {diff:.3e}, |fp32 torch - f64| = {err32:.3e}, tolerance {tol:.3e}')
    sp = pk['special']
    assert torch.equal(got[sp['outside']], torch.zeros(3))                                   # exactly zero, not small
    assert bool(torch.isfinite(got).all())
    if capped:
        n = got.double().norm(dim=-1)
        assert float(n.max()) <= cap * (1 + 4e-7) and abs(float(n[sp['capped']]) - cap) <= 4e-7 * cap


def test_report_against_float64():
    dev = _dev()
    pk = _pack(dev)
    d = pk['dev']
    count, energy, min_dist = (t.cpu() for t in capi.clash_report(d['protein'], d['sigma'], d['pptr'], d['lptr'], d['x']))
    assert count.dtype == torch.int32 and energy.dtype == min_dist.dtype == torch.float32
    r64, r32 = pk['rep']
    assert count.tolist() == [c for c, _, _ in r64]                                          # exact
    for g in range(4):
        (_, e64, m64), (_, e32, m32) = r64[g], r32[g]
        if not np.isfinite(m64):
            assert float(min_dist[g]) == float('inf') and float(energy[g]) == 0.0
            continue
        tol_e, tol_m = max(8 * abs(e32 - e64), FLOOR), max(8 * abs(m32 - m64), FLOOR)
        de = close(energy[g:g + 1], [e64], tol_e, f'energy, graph {g}')
        dm = close(min_dist[g:g + 1], [m64], tol_m, f'min distance, graph {g}')
        print(f'report graph {g}: |dE| = {de:.3e} (fp32 torch {abs(e32 - e64):.3e}, tolerance {tol_e:.3e}), |d min| = {dm:.3e} '
              f'(fp32 torch {abs(m32 - m64):.3e}, tolerance {tol_m:.3e})')
    assert float(min_dist[3]) == 0.0                                                          # the coincident atom


def test_single_pair_ends_at_the_contact_distance():
    dev = _dev()
    p = torch.tensor([[1.0, -2.0, 0.5]], device=dev)
    x = p + 0.5 * torch.tensor([[0.6, 0.0, -0.8]], device=dev)
    ptr = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    s = torch.tensor([3.0], device=dev)
    x1 = x + capi.clash_shift(p, s, ptr, ptr, x, 1.0, 0.0)
    # fp32: the distance 0.5 and the direction carry half an ulp each; 3 A x 2^-23 x a few
    close((x1 - p).double().norm(dim=-1), [3.0], 2e-6, 'one pair, w = 1, no cap')


# ------------------------------------------------------------------------------------------ 2. determinism
def test_same_bits_twice_and_alone_versus_in_the_pack():
    dev = _dev()
    pk = _pack(dev)
    d = pk['dev']
    run = lambda: capi.clash_shift(d['protein'], d['sigma'], d['pptr'], d['lptr'], d['x'], 0.5, pk['max_shift'])
    a = run()
    assert torch.equal(a, run())
    rep = capi.clash_report(d['protein'], d['sigma'], d['pptr'], d['lptr'], d['x'])
    for u, v in zip(rep, capi.clash_report(d['protein'], d['sigma'], d['pptr'], d['lptr'], d['x'])):
        assert torch.equal(u, v)
    pp, lp = pk['pptr'], pk['lptr']
    for g in (1, 2, 3):
        prot, sig, x = d['protein'][pp[g]:pp[g + 1]].contiguous(), d['sigma'][pp[g]:pp[g + 1]].contiguous(), d['x'][lp[g]:lp[g + 1]].contiguous()
        p1 = torch.tensor([0, prot.shape[0]], dtype=torch.int32, device=dev)
        l1 = torch.tensor([0, x.shape[0]], dtype=torch.int32, device=dev)
        assert torch.equal(capi.clash_shift(prot, sig, p1, l1, x, 0.5, pk['max_shift']), a[lp[g]:lp[g + 1]]), f'graph {g} alone'
        for u, v in zip(capi.clash_report(prot, sig, p1, l1, x), rep):
            assert torch.equal(u, v[g:g + 1]), f'graph {g} alone'


def test_argument_errors():
    dev = _dev()
    pk = _pack(dev)
    d = pk['dev']
    a = (d['protein'], d['sigma'], d['pptr'], d['lptr'], d['x'])
    with pytest.raises(RuntimeError, match='weight must be >= 0'):
        capi.clash_shift(*a, -1.0, 0.0)
    with pytest.raises(RuntimeError, match='max_shift must be >= 0'):
        capi.clash_shift(*a, 1.0, -0.5)
    bad = d['sigma'].clone()
    bad[5] = 0.0
    with pytest.raises(ValueError, match='radius'):
        capi.clash_shift(d['protein'], bad, d['pptr'], d['lptr'], d['x'])
    with pytest.raises(ValueError):
        capi.clash_shift(d['protein'], d['sigma'][:-1], d['pptr'], d['lptr'], d['x'])
    with pytest.raises(ValueError):                                                  # offsets that do not end at N_l
        capi.clash_shift(d['protein'], d['sigma'], d['pptr'], d['lptr'] + 1, d['x'])
    with pytest.raises(ValueError):
        G.clash_shift(d['protein'], torch.zeros(d['protein'].shape[0], dtype=torch.int64, device=dev), d['x'],
                      torch.zeros(d['x'].shape[0], dtype=torch.int64, device=dev), radius=3.0, weight=-1.0)


# ------------------------------------------------------------------------------------------ 3. the guided posterior step
def _step_inputs(dev, t_value, seed):
    b, _, _, fixed, _ = _batch(dev)
    g = torch.Generator().manual_seed(seed)
    Nl, C, B = sum(SIZES), 13, 3
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    lptr = torch.tensor(np.cumsum([0] + SIZES), dtype=torch.int32, device=dev)
    t = torch.full((B,), t_value, dtype=torch.int32, device=dev)
    return dict(t=t, lptr=lptr, pos=2 * r(Nl, 3), v=torch.randint(0, C, (Nl,), generator=g).to(dev), pred_pos=2 * r(Nl, 3), pred_v=r(Nl, C),
                noise=r(Nl, 3), uniform=torch.rand(Nl, C, generator=g).to(dev), shift=0.7 * r(Nl, 3), fixed=fixed)


def _post(native, i, pred_pos, **kw):
    Nl, C = i['pos'].shape[0], 13
    l0, lp = torch.empty(Nl, C, device=i['pos'].device), torch.empty(Nl, C, device=i['pos'].device)
    pos, v = native.posterior_step(i['t'], i['lptr'], i['pos'], i['v'], pred_pos, i['pred_v'], i['noise'], i['uniform'], log_v0=l0,
                                   log_post=lp, **kw)
    return pos, v, l0, lp


@pytest.mark.parametrize('t_value', [T_SMALL - 2, 0])
@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('prog', [False, True])
def test_guided_posterior_is_the_unguided_step_on_the_shifted_prediction(t_value, mask, prog):
    dev = _dev()
    m = _model()
    native = m._native(dev)
    i = _step_inputs(dev, t_value, 300 + t_value)
    kw = dict(i['fixed']) if mask else {}
    if prog:
        levels = [T_SMALL - 1, T_SMALL - 2, 0, -1]
        p = TimeProgram.from_levels(T_SMALL, levels)
        slot = 1 if t_value == T_SMALL - 2 else 2                                     # 3 -> 0 (two levels at once), 0 -> clean data
        kw['prog_row'] = torch.from_numpy(p.tables(m)).to(dev)[slot].contiguous()
    shifted = i['pred_pos'] + i['shift']                                              # one rounded fp32 add per element
    want = _post(native, i, shifted, **kw)
    got = _post(native, i, i['pred_pos'], x0_shift=i['shift'], **kw)
    for name, a, b in zip(('pos', 'v', 'log_v0', 'log_post'), got, want):
        assert torch.equal(a, b), f'{name}: t = {t_value}, mask = {mask}, program row = {prog}'
    plain = _post(native, i, i['pred_pos'], **kw)
    assert not torch.equal(plain[0], got[0])                                          # the shift does reach the step
    if mask:
        mk = i['fixed']['fixed_mask']
        assert torch.equal(plain[0][mk], got[0][mk]) and torch.equal(plain[1][mk], got[1][mk])        # known atoms ignore it


def _guided_raw(native, i, shift_ptr):
    """td_posterior_step_guided through ctypes, so that a NULL shift can be passed"""
    Nl, C, dev = i['pos'].shape[0], 13, i['pos'].device
    pos, v = torch.empty_like(i['pos']), torch.empty_like(i['v'])
    l0, lp = torch.empty(Nl, C, device=dev), torch.empty(Nl, C, device=dev)
    P = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = native.lib.td_posterior_step_guided(native.handle, P(i['t']), None, P(i['lptr']), Nl, 3, P(i['pos']), P(i['v']), P(i['pred_pos']),
                                             P(i['pred_v']), P(i['noise']), P(i['uniform']), P(pos), P(v), P(l0), P(lp), None, None, None,
                                             shift_ptr, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, native.lib.td_last_error()
    return pos, v, l0, lp


def test_null_shift_and_zero_weight_are_the_unguided_step():
    dev = _dev()
    native = _model()._native(dev)
    i = _step_inputs(dev, 2, 311)
    want = _post(native, i, i['pred_pos'])
    for name, a, b in zip(('pos', 'v', 'log_v0', 'log_post'), _guided_raw(native, i, None), want):
        assert torch.equal(a, b), f'NULL shift: {name}'
    b, _, _, _, sigma = _batch(dev)
    pptr = capi.graph_ptr(b.protein_element_batch, 3)
    ppos = b.protein_pos.clone()
    native.center_pos(ppos, pptr, None, i['lptr'])          # the pockets sit up to 20 A off the origin, the predictions around it
    zero = capi.clash_shift(ppos, sigma, pptr, i['lptr'], i['pred_pos'], 0.0, 1.0)
    assert float(capi.clash_shift(ppos, sigma, pptr, i['lptr'], i['pred_pos'], 1.0, 0.0).abs().max()) > 0      # (w = 1 would move them)
    assert float(zero.abs().max()) == 0.0
    for name, a, b in zip(('pos', 'v', 'log_v0', 'log_post'), _post(native, i, i['pred_pos'], x0_shift=zero), want):
        assert torch.equal(a, b), f'w = 0: {name}'


def test_guided_posterior_with_noise_mean_type_against_float64():
    dev = _dev()
    m = _model('noise')
    native = m._native(dev)
    t_value = 3
    i = _step_inputs(dev, t_value, 322)
    out = i['pos'] + 0.5 * i['pred_pos']                                              # the network's output: x_t + eps
    got, _, _, _ = _post(native, i, out, x0_shift=i['shift'])
    f = lambda name: float(getattr(m, name)[t_value])                                  # the model's fp32 table entries, as the kernel reads them
    xt, o, sh, nz = (x.double().cpu() for x in (i['pos'], out, i['shift'], i['noise']))
    x0 = f('sqrt_recip_alphas_cumprod') * xt - f('sqrt_recipm1_alphas_cumprod') * (o - xt)
    want = f('posterior_mean_c0_coef') * (x0 + sh) + f('posterior_mean_ct_coef') * xt + np.exp(0.5 * f('posterior_logvar')) * nz
    close(got, want, TOL_X, "guided step, model_mean_type 'noise'")
    plain, _, _, _ = _post(native, i, out)
    assert float((plain - got).abs().max()) > 0.01


# ------------------------------------------------------------------------------------------ 4. sampling paths
def _guid(dev):
    return ClashGuidance(radius=_batch(dev)[4], weight=1.0, max_shift=1.0)


def _run(dev, base=4100, **kw):
    m = _model(kw.pop('mean_type', 'C0'))
    return m.sample_diffusion(*_args(dev), center_pos_mode='protein', noise_source=draws.Source(base, dev), **kw)


def _manual(dev, g, base=4100, fixed=None):
    """forward -> clash_shift -> guided posterior from the public pieces, T_SMALL unit steps down to clean data"""
    m = _model()
    native = m._native(dev)
    ppos, pv, bp, lpos, lv, bl = _args(dev)
    ppos, lpos, lv = ppos.clone(), lpos.clone(), lv.clone()
    pptr, lptr = capi.graph_ptr(bp, 3), capi.graph_ptr(bl, 3)
    offset = native.center_pos(ppos, pptr, lpos, lptr)
    kw = {}
    if fixed is not None:
        fpos = fixed['fixed_pos'].clone() - offset[bl]
        fpos[~fixed['fixed_mask']] = 0.0
        fv = torch.where(fixed['fixed_mask'], fixed['fixed_v'], torch.zeros_like(fixed['fixed_v']))
        kw = dict(fixed_mask=fixed['fixed_mask'], fixed_pos=fpos, fixed_v=fv)
        a = m.alphas_cumprod[T_SMALL - 1].detach().float().cpu()
        lpos[fixed['fixed_mask']] = float(a.sqrt()) * fpos[fixed['fixed_mask']] + float((1.0 - a).sqrt()) * lpos[fixed['fixed_mask']]
    src = draws.Source(base, dev)
    sigma = g.radii(ppos.shape[0], dev)
    traj, moved = [], 0.0
    for s, t in enumerate(range(T_SMALL - 1, -1, -1)):
        noise, uniform = src(s, 'noise', lpos), src(s, 'uniform', torch.empty(lpos.shape[0], 13))
        preds = native.model_forward(ppos, pv, pptr, lpos, lv, lptr, want_final_h=False)
        shift = G.clash_shift(ppos, bp, preds['pred_ligand_pos'], bl, radius=g, weight=g.weight, max_shift=g.max_shift)
        moved = max(moved, float(shift.abs().max()))
        lpos, lv = native.posterior_step(torch.full((3,), t, dtype=torch.int32, device=dev), lptr, lpos, lv, preds['pred_ligand_pos'],
                                         preds['pred_ligand_v'], noise, uniform, x0_shift=shift, **kw)
        traj.append((lpos + offset[bl]).cpu())
    return traj, lv, moved


def test_session_graph_eager_stateless_and_manual_composition_are_identical():
    dev = _dev()
    g = _guid(dev)

    def run(use_graph, use_session=True):
        s = _model().begin_sampling(*_args(dev), center_pos_mode='protein', noise_source=draws.Source(4100, dev), use_graph=use_graph,
                                    use_session=use_session, guidance=g)
        replayed = []
        while not s.done:
            s.step()
            replayed.append(bool(s.session.last_step_was_graph()) if s.session is not None else False)
        return s.finish(), replayed
    eager, rep_e = run(False)
    assert not any(rep_e) and len(eager['pos_traj']) == T_SMALL
    graph, rep_g = _on_side_stream(dev, lambda: run(True))
    assert rep_g == [False] + [True] * (T_SMALL - 1)                                  # td_session_step_graph reports 1 from the second step on
    stateless, _ = run(None, use_session=False)
    _same(eager, graph, 'guided: launch by launch vs captured hipGraph')
    _same(eager, stateless, 'guided: session vs stateless')
    traj, lv, moved = _manual(dev, g)
    assert moved > 0.1, 'the guidance never moved an atom: the test would show nothing'
    for s in range(T_SMALL):
        assert torch.equal(traj[s], eager['pos_traj'][s]), f'manual composition: positions differ at step {s}'
    assert torch.equal(lv, eager['v'])
    plain = _run(dev, num_steps=None, use_graph=False)
    assert not torch.equal(plain['pos'], eager['pos'])                                # guided and unguided runs do differ


def test_known_atoms_follow_the_unguided_trajectory():
    dev = _dev()
    fixed = _batch(dev)[3]
    mk = fixed['fixed_mask'].cpu()
    for kw in (dict(use_graph=False), dict(use_session=False)):
        plain = _run(dev, **fixed, **kw)
        guided = _run(dev, guidance=_guid(dev), **fixed, **kw)
        for s in range(T_SMALL):
            assert torch.equal(plain['pos_traj'][s][mk], guided['pos_traj'][s][mk]), f'known positions differ at step {s} ({kw})'
            assert torch.equal(plain['v_traj'][s][mk], guided['v_traj'][s][mk]), f'known types differ at step {s} ({kw})'
        assert not torch.equal(plain['pos'][~mk.to(dev)], guided['pos'][~mk.to(dev)])
    traj, lv, _ = _manual(dev, _guid(dev), fixed=fixed)
    for s in range(T_SMALL):
        assert torch.equal(traj[s], guided['pos_traj'][s]), f'manual composition with known atoms: step {s}'


def test_program_with_a_jump_renoise_slots_are_the_unguided_rule():
    dev = _dev()
    m = _model()
    native = m._native(dev)
    p = TimeProgram.from_levels(T_SMALL, [4, 2, 0, -1]).with_resampling(1, 2)
    kinds = p.kind.tolist()
    assert kinds.count(RENOISE) >= 1
    table = torch.from_numpy(p.tables(m)).to(dev)
    results = []
    for use_session, use_graph, pos_only in [(True, False, False), (True, True, False), (False, None, False), (True, False, True), (False, None, True)]:
        def go():
            s = m.begin_sampling(*_args(dev), center_pos_mode='protein', noise_source=draws.Source(4200, dev), use_graph=use_graph,
                                 use_session=use_session, guidance=_guid(dev), time_program=p, pos_only=pos_only)
            k = 0
            while not s.done:
                before_pos, before_v = s.lpos.clone(), s.lv.clone()
                s.step()
                if kinds[k] == RENOISE:          # the slot is the plain forward-process step of the state the guided steps left
                    want_pos, want_v = native.renoise_step(table[k].contiguous(), before_pos, before_v, s._noise,
                                                           None if pos_only else s._uniform)
                    assert torch.equal(s.lpos, want_pos), f'renoise slot {k}: positions'
                    assert torch.equal(s.lv, before_v if pos_only else want_v), f'renoise slot {k}: types'
                k += 1
            return s.finish()
        results.append(_on_side_stream(dev, go) if use_graph else go())
    _same(results[0], results[1], 'guided program: launch by launch vs captured hipGraph')
    _same(results[0], results[2], 'guided program: session vs stateless')
    _same(results[3], results[4], 'guided program, pos_only: session vs stateless')
    unguided = m.sample_diffusion(*_args(dev), center_pos_mode='protein', noise_source=draws.Source(4200, dev), time_program=p, use_graph=False)
    assert not torch.equal(unguided['pos'], results[0]['pos'])


def test_set_remove_set_inside_one_session():
    dev = _dev()
    g = _guid(dev)
    on = [True, True, False, True, True]

    def composite():
        s = _model().begin_sampling(*_args(dev), center_pos_mode='protein', noise_source=draws.Source(4300, dev), use_graph=True, guidance=g)
        replayed = []
        for k in range(T_SMALL):
            if k == 2:
                s.session.set_guidance(None)
            if k == 3:
                s.session.set_guidance(s._sigma, g.weight, g.max_shift)
            s.step()
            replayed.append(bool(s.session.last_step_was_graph()))
        return s.finish(), replayed
    got, replayed = _on_side_stream(dev, composite)
    assert replayed == [False, True, True, True, True]                                # re-captured after every change, then replayed
    r = _model().begin_sampling(*_args(dev), center_pos_mode='protein', noise_source=draws.Source(4300, dev), use_session=False, guidance=g)
    for k in range(T_SMALL):
        r.guidance = g if on[k] else None
        r.step()
    _same(got, r.finish(), 'set / remove / set vs the stateless steps with the same switches')
    # and against fresh sessions: all-guided and never-guided runs differ from it, the first two steps are the all-guided run's
    full = _run(dev, base=4300, guidance=g, use_graph=False)
    assert torch.equal(full['pos_traj'][1], got['pos_traj'][1]) and not torch.equal(full['pos_traj'][2], got['pos_traj'][2])
    with pytest.raises(RuntimeError, match='weight must be >= 0'):
        s = _model().begin_sampling(*_args(dev), center_pos_mode='protein', use_graph=False, guidance=g)
        s.session.set_guidance(s._sigma, -1.0, 0.0)
    with pytest.raises(ValueError, match='radius'):
        s.session.set_guidance(torch.zeros_like(s._sigma), 1.0, 0.0)


def test_noise_mean_type_session_equals_stateless():
    dev = _dev()
    a = _run(dev, base=4400, mean_type='noise', guidance=_guid(dev), use_graph=False)
    b = _run(dev, base=4400, mean_type='noise', guidance=_guid(dev), use_session=False)
    _same(a, b, "guided, model_mean_type 'noise': session vs stateless")
    assert bool(torch.isfinite(a['pos']).all())


# ------------------------------------------------------------------------------------------ 5. guidance=None
def test_guidance_none_changes_nothing():
    dev = _dev()
    for kw in (dict(use_graph=False), dict(use_session=False)):
        _same(_run(dev, base=4500, **kw), _run(dev, base=4500, guidance=None, **kw), f'guidance=None ({kw})')
    a = _on_side_stream(dev, lambda: _run(dev, base=4500, use_graph=True))
    b = _on_side_stream(dev, lambda: _run(dev, base=4500, use_graph=True, guidance=None))
    _same(a, b, 'guidance=None, captured hipGraph')


# ------------------------------------------------------------------------------------------ 6. the driver
def test_driver_and_clash_report_of_its_poses():
    from targetdiff_amd import sampling
    dev = _dev()
    pk = workloads.synthetic_pocket(301, 70, 3.0, 9.0)
    data = types.SimpleNamespace(protein_pos=torch.from_numpy(pk.pos), protein_atom_feature=torch.from_numpy(pk.feat))
    radii = torch.linspace(3.5, 5.0, 70)
    g = ClashGuidance(radius=radii, weight=1.0, max_shift=1.0)
    src = draws.Source(4600, dev)
    sizes = [4, 6, 5]
    kw = dict(batch_size=2, device=dev, ligand_num_atoms=sizes, noise_source=lambda b, st, name, like: src(st + 1 + 20 * b, name, like))
    res = sampling.sample_diffusion_ligand(_model(), data, 3, guidance=g, **kw)
    pos, v, pos_traj, v_traj, v0_traj, vt_traj, times = res
    assert len(res) == 7 and len(times) == 2
    assert [x.shape for x in pos] == [(n, 3) for n in sizes] and [x.shape for x in pos_traj] == [(T_SMALL, n, 3) for n in sizes]
    assert [x.shape for x in vt_traj] == [(T_SMALL, n, 13) for n in sizes] and [x.shape for x in v] == [(n,) for n in sizes]
    plain = sampling.sample_diffusion_ligand(_model(), data, 3, **kw)
    assert any(not np.array_equal(a, b) for a, b in zip(pos, plain[0]))
    # the report a user asks of the finished poses (the pocket as given, de-centred poses), one graph per sample
    ppos = torch.from_numpy(pk.pos).float()
    lig = [torch.from_numpy(x).float() for x in pos]                                 # (fp32 values widened by the driver: exact)
    bp = torch.arange(3).repeat_interleave(70)
    bl = torch.arange(3).repeat_interleave(torch.tensor(sizes))
    count, energy, min_dist = (t.cpu() for t in G.clash_report(ppos.repeat(3, 1).to(dev), bp.to(dev), torch.cat(lig).to(dev), bl.to(dev),
                                                              radius=radii.repeat(3)))
    for k in range(3):
        c64, e64, m64 = GR.report(ppos, radii, lig[k])
        _, e32, m32 = GR.report(ppos, radii, lig[k], dtype=torch.float32)
        if GR.min_gap(ppos, radii, lig[k]) > 1e-4:
            assert int(count[k]) == c64
        close(energy[k:k + 1], [e64], max(8 * abs(e32 - e64), FLOOR), f'driver poses: energy of sample {k}')
        close(min_dist[k:k + 1], [m64], max(8 * abs(m32 - m64), FLOOR), f'driver poses: min distance of sample {k}')
