"""Sampling time programs, host side (CPU only): the program's construction and checks, its coefficient table against the model's own
entries (unit steps, bitwise) and against an independent float64 evaluation of the stated formulas (strided and renoise slots), the
fixtures of the real reference (tools/make_golden_program.py) against the CPU restatement (tests/_program_ref.py), the sampler's host
loop and the batching driver on a stand-in native layer, the argument checks, and the StepIO layout against the library.

Tolerances are tests/_tol.py's: atom types exact, free-running trajectories TOL_TRAJ = 5e-5 A, log-probabilities TOL_H.  Each fixture
stores r, the fp32 reference's own distance from its float64 run; the generator only accepts r <= TOL_TRAJ / 5."""
import ctypes
import types

import numpy as np
import pytest
import torch

import _program_ref as PR
from _tol import TOL_FWD, TOL_H, TOL_TRAJ, close
from oracle import draws, weights
from oracle.native_stub import RecordingNative
from targetdiff_amd import schedule as SCH
from targetdiff_amd.schedule import DENOISE, RENOISE, TimeProgram


# ------------------------------------------------------------------------------------------ construction
@pytest.mark.parametrize('n,j,r', [(20, 3, 2), (8, 2, 2), (20, 10, 10), (7, 7, 3), (7, 8, 3), (5, 1, 4), (1, 1, 5), (12, 4, 1)])
def test_with_resampling_length_and_chaining(n, j, r):
    levels = list(range(999, 999 - 40 * (n + 1), -40))[:n] + [-1]
    base = TimeProgram.from_levels(1000, levels)
    assert len(base) == n and base.num_renoise == 0
    p = base.with_resampling(jump_length=j, resamplings=r)
    jumps = (n - 1) // j
    assert len(p) == n + (r - 1) * jumps * (j + 1)
    assert p.num_renoise == (r - 1) * jumps and p.num_denoise == n + (r - 1) * jumps * j
    assert int(p.t_from[0]) == 999 and int(p.t_to[-1]) == -1
    assert np.array_equal(p.t_from[1:], p.t_to[:-1])                        # the steps chain
    down = p.kind == DENOISE
    assert (p.t_to[down] < p.t_from[down]).all() and (p.t_to[~down] > p.t_from[~down]).all()
    pos = {l: i for i, l in enumerate(levels)}
    for a, b, k in zip(p.t_from.tolist(), p.t_to.tolist(), p.kind.tolist()):
        if k == RENOISE:            # back j positions, from a position that is a multiple of j and not the end
            assert pos[a] - pos[b] == j and pos[a] % j == 0 and 0 < pos[a] < n
        else:                       # one position down
            assert pos[b] - pos[a] == 1
    # every stretch of j steps that ends on such a position is sampled r times, the tail once
    visits = np.zeros(n + 1, dtype=int)
    for b, k in zip(p.t_to.tolist(), p.kind.tolist()):
        if k == DENOISE:
            visits[pos[b]] += 1
    want = np.ones(n + 1, dtype=int)
    want[0] = 0
    want[1:jumps * j + 1] = r
    assert np.array_equal(visits, want)
    with pytest.raises(ValueError):
        p.with_resampling(2, 2) if p.num_renoise else TimeProgram(1000, [0], [998], [997])


def test_constructors():
    ref = TimeProgram.reference(1000)
    assert len(ref) == 1000 and ref.levels.tolist() == list(range(998, -2, -1)) and (ref.kind == DENOISE).all()
    part = TimeProgram.reference(1000, 20)
    assert part.t_from.tolist() == list(range(999, 979, -1)) and int(part.t_to[-1]) == 979
    assert len(TimeProgram.reference(1000, 0)) == 0
    one = TimeProgram.strided(1000, 1)
    assert (one.t_from.tolist(), one.t_to.tolist()) == ([999], [-1])
    s = TimeProgram.strided(1000, 20)
    want = np.round(np.linspace(999, 0, 20)).astype(int).tolist()
    assert s.t_from.tolist() == want and s.t_to.tolist() == want[1:] + [-1] and len(s) == 20
    dense = TimeProgram.strided(10, 50)                      # more calls than levels: made unique
    assert dense == TimeProgram.reference(10)
    assert PR.program('program_stride50').t_from.tolist() == list(range(999, 0, -50))
    for case, (steps, ren) in PR.EXPECTED_STEPS.items():
        p = PR.program(case)
        assert (len(p), p.num_renoise) == (steps, ren), case
    with pytest.raises(AttributeError):
        s.T = 3
    with pytest.raises(ValueError):
        s.kind[0] = 1


@pytest.mark.parametrize('what,args', [
    ('does not start at T - 1', ([0], [998], [997])),
    ('steps do not chain', ([0, 0], [999, 900], [950, 800])),
    ('level below -1', ([0], [999], [-2])),
    ('level above T - 1', ([0, 1], [999, 500], [500, 1000])),
    ('denoise going up', ([0, 0], [999, 500], [500, 600])),
    ('denoise staying', ([0, 0], [999, 500], [500, 500])),
    ('renoise going down', ([0, 1], [999, 500], [500, 400])),
    ('unknown kind', ([0, 2], [999, 500], [500, 600])),
    ('ragged arrays', ([0, 0], [999], [500])),
])
def test_validation_raises_value_error(what, args):
    with pytest.raises(ValueError):
        TimeProgram(1000, *args)
        pytest.fail(what)


def test_other_constructor_errors():
    for bad in (lambda: TimeProgram.strided(1000, 0), lambda: TimeProgram.reference(1000, 1001), lambda: TimeProgram.from_levels(1000, []),
                lambda: TimeProgram.from_levels(1000, [999, 500, 500]), lambda: TimeProgram.reference(1000).with_resampling(0, 2),
                lambda: TimeProgram.reference(1000).with_resampling(2, 0)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError):
        TimeProgram.strided(100, 5).tables(PR.mirror('program_stride50'))          # a program of another T


# ------------------------------------------------------------------------------------------ the coefficient table
def test_unit_steps_hold_the_models_own_entries_bitwise():
    m = PR.mirror('program_stride50')
    tab = TimeProgram.reference(1000).tables(m)
    t = np.arange(999, -1, -1)
    p = np.maximum(t - 1, 0)
    own = lambda k: getattr(m, k).detach().numpy()
    for col, name, idx in [(SCH.C0, 'posterior_mean_c0_coef', t), (SCH.CT, 'posterior_mean_ct_coef', t), (SCH.LOGVAR, 'posterior_logvar', t),
                           (SCH.LOG_A, 'log_alphas_v', t), (SCH.LOG_1MA, 'log_one_minus_alphas_v', t),
                           (SCH.LOG_CA, 'log_alphas_cumprod_v', p), (SCH.LOG_1MCA, 'log_one_minus_alphas_cumprod_v', p),
                           (SCH.ABAR_TO, 'alphas_cumprod', p)]:
        assert tab.dtype == np.float32 and np.array_equal(tab[:, col].view(np.uint32), own(name)[idx].view(np.uint32)), name
    assert tab[:, SCH.LAST].tolist() == [0.0] * 999 + [1.0]
    # unit steps inside a strided program too
    mixed = TimeProgram.from_levels(1000, [999, 998, 500, 499, 0, -1]).tables(m)
    assert np.array_equal(mixed[[0, 2, 4]], tab[[0, 499, 999]])          # rows of t = 999, 500, 0


def _schedule64(cfg):
    """the float64 schedules from the configuration, written out independently of the package (sigmoid positions, cosine types)"""
    T = cfg['num_diffusion_timesteps']
    x = np.linspace(-6, 6, T)
    betas = 1.0 / (1.0 + np.exp(-x)) * (cfg['beta_end'] - cfg['beta_start']) + cfg['beta_start']
    A = np.cumprod(1.0 - betas)
    steps = T + 1
    grid = np.linspace(0, steps, steps)
    s = cfg['v_beta_s']
    cum = np.cos(((grid / steps) + s) / (1 + s) * np.pi * 0.5) ** 2
    cum = cum / cum[0]
    Lc = np.cumsum(np.log(np.sqrt(np.clip(cum[1:] / cum[:-1], a_min=0.001, a_max=1.0))))
    return (lambda l: 1.0 if l < 0 else A[l]), (lambda l: 0.0 if l < 0 else Lc[l])


def test_strided_and_renoise_slots_equal_the_float64_formulas():
    cfg = PR.model_config('program_stride50')
    assert cfg['beta_schedule'] == 'sigmoid' and cfg['v_beta_schedule'] == 'cosine'
    A, Lc = _schedule64(cfg)
    log1m = lambda a: np.log(1.0 - np.exp(a) + 1e-40)
    m = PR.mirror('program_stride50')
    for case in ('program_stride50_jump3x2_mask', 'program_uneven_jump2x2_mask'):
        p = PR.program(case)
        tab = p.tables(m)
        for row, k, f, to in zip(tab, p.kind.tolist(), p.t_from.tolist(), p.t_to.tolist()):
            want = np.zeros(SCH.ROW, dtype=np.float32)
            if k == DENOISE:
                t, s = f, to
                alpha = A(t) / A(s)
                beta = 1.0 - alpha
                var = np.float32(beta * (1.0 - A(s)) / (1.0 - A(t)))
                want[[SCH.C0, SCH.CT]] = beta * np.sqrt(A(s)) / (1.0 - A(t)), (1.0 - A(s)) * np.sqrt(alpha) / (1.0 - A(t))
                want[SCH.LOGVAR] = 0.0 if s < 0 else np.log(var)
                want[[SCH.LOG_A, SCH.LOG_1MA]] = Lc(t) - Lc(s), log1m(Lc(t) - Lc(s))
                want[[SCH.LOG_CA, SCH.LOG_1MCA]] = Lc(s), log1m(Lc(s))
                want[[SCH.ABAR_TO, SCH.LAST]] = A(s), float(s < 0)
            else:
                s, t = f, to
                want[[SCH.RHO, SCH.LOG_R, SCH.LOG_1MR]] = A(t) / A(s), Lc(t) - Lc(s), log1m(Lc(t) - Lc(s))
            assert np.array_equal(row.view(np.uint32), want.view(np.uint32)), (case, k, f, to, row, want)
    # the last strided step t -> -1: the mean is the prediction itself, and the types use Lc(-1) = 0, not the clamp to level 0
    last = PR.program('program_stride50').tables(m)[-1]
    assert last[SCH.C0] == 1.0 and last[SCH.CT] == 0.0 and last[SCH.LAST] == 1.0 and last[SCH.LOG_CA] == 0.0
    assert last[SCH.LOG_1MCA] == np.float32(np.log(1e-40))


def test_renoise_ratio_is_the_product_of_the_one_level_ratios():
    A, _ = _schedule64(PR.model_config('program_stride50'))
    m = PR.mirror('program_stride50')
    A64 = m._sched64['alphas_cumprod']
    assert np.allclose(A64, [A(l) for l in range(1000)], rtol=1e-15, atol=0)
    for s, t in [(849, 999), (0, 10), (499, 500), (-1, 3), (100, 900)]:
        prod = 1.0
        for l in range(s + 1, t + 1):
            prod *= (A64[l] / A64[l - 1]) if l > 0 else A64[0]
        rho = A64[t] / (A64[s] if s >= 0 else 1.0)
        assert abs(rho - prod) <= 1e-15 * prod, (s, t, rho, prod)
        row = TimeProgram(1000, [0, 1], [999, s], [s, t]).tables(m)[1] if s < 999 else None
        assert row[SCH.RHO] == np.float32(rho)


# ------------------------------------------------------------------------------------------ fixtures vs restatement
@pytest.mark.parametrize('case', list(PR.CASES))
def test_restatement_reproduces_reference_fixture(case):
    c = PR.CASES[case]
    g, inputs = PR.load_fixture(case)
    p = PR.program(case)
    assert float(g['r']) <= TOL_TRAJ / 5, f'{case}: the fp32 reference itself is {float(g["r"]):.2e} A from float64'
    assert int(g['draws_base']) == c['base']
    assert np.array_equal(g['kind'], p.kind) and np.array_equal(g['t_from'], p.t_from) and np.array_equal(g['t_to'], p.t_to)
    assert np.array_equal(g['table'].view(np.uint32), p.tables(PR.mirror(case)).view(np.uint32))        # the table the reference was driven with
    r = PR.run(case, inputs)
    v = torch.stack(r['v_traj'])
    assert torch.equal(v, torch.from_numpy(g['v_traj'].astype(np.int64))), f'{case}: atom types differ from the reference'
    d = close(torch.stack(r['pos_traj']), g['pos_traj'], TOL_TRAJ, (case, 'pos_traj'))
    print(f'{case}: max |dx| = {d:.3e} A over {len(p)} steps; reference fp32 vs float64 r = {float(g["r"]):.3e}')
    if not c['pos_only']:
        close(torch.stack(r['v0_traj']), g['v0_traj'], TOL_H, (case, 'v0_traj'))
        close(torch.stack(r['vt_traj']), g['vt_traj'], TOL_H, (case, 'vt_traj'))
    if c['mask'] and int(p.t_to[-1]) == -1:          # clean data was reached: the known atoms ARE the known state
        m = inputs['fixed_mask']
        close(torch.from_numpy(g['pos_traj'][-1])[m], inputs['fixed_pos'][m], TOL_FWD, (case, 'final known atoms'))
        assert np.array_equal(g['v_traj'][-1][m.numpy()], inputs['fixed_v'][m].numpy())


# ------------------------------------------------------------------------------------------ the host loop on a stand-in native layer
class _ProgNative(RecordingNative):
    """The recording stand-in plus the program forms of the two steps (the rule of tests/_program_ref.py)."""

    def posterior_step(self, t, ligand_ptr, ligand_pos, ligand_v, pred_pos, pred_v, noise, uniform, pos_next=None, v_next=None,
                       log_v0=None, log_post=None, fixed_mask=None, fixed_pos=None, fixed_v=None, prog_row=None):
        if prog_row is None:
            assert fixed_mask is None
            return super().posterior_step(t, ligand_ptr, ligand_pos, ligand_v, pred_pos, pred_v, noise, uniform, pos_next, v_next, log_v0,
                                          log_post)
        self._rec('posterior_step_program', t=t, prog_row=prog_row)
        pos, v, l0, lp = PR.denoise_step(prog_row, ligand_pos, ligand_v, pred_pos, pred_v, noise, uniform, self.num_classes, fixed_mask,
                                         fixed_pos, fixed_v)
        pos_next.copy_(pos)
        v_next.copy_(v)
        if log_v0 is not None:
            log_v0.copy_(l0)
            log_post.copy_(lp)
        return pos_next, v_next

    def renoise_step(self, prog_row, ligand_pos, ligand_v, noise, uniform=None, pos_next=None, v_next=None, log_v0=None, log_q=None):
        self._rec('renoise_step', prog_row=prog_row)
        pos, v, l0, lq = PR.renoise_step(prog_row, ligand_pos, ligand_v, noise, uniform, self.num_classes)
        pos_next.copy_(pos)
        v_next.copy_(v)
        if log_v0 is not None:
            log_v0.copy_(l0)
            log_q.copy_(lq)
        return pos_next, v_next


def _stub_model(monkeypatch, case='program_stride50'):
    from targetdiff_amd import models
    m = PR.mirror(case)
    log = []
    native = _ProgNative(PR.state_dict(case), PR.model_config(case), m.num_classes, log)
    monkeypatch.setattr(models.ScorePosNet3D, '_native', lambda self, device: native)
    return m, log


def _sample(m, case, inputs, **kw):
    b = PR.case_batch(case)
    return m.sample_diffusion(b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch, inputs['init_pos'], inputs['init_v'],
                              b.ligand_element_batch, center_pos_mode='protein', use_session=False, **kw)


@pytest.mark.parametrize('case', ['program_uneven_jump2x2_mask', 'program_pos_only'])
def test_host_loop_reproduces_reference_fixture(monkeypatch, case):
    """ReverseSampler's own loop (stateless form) with the stand-in steps: the fixture again, through the package's host code."""
    c = PR.CASES[case]
    g, inputs = PR.load_fixture(case)
    m, log = _stub_model(monkeypatch, case)
    p = PR.program(case)
    r = _sample(m, case, inputs, time_program=p, noise_source=draws.Source(c['base']), pos_only=c['pos_only'],
                **PR.fixed_kwargs(case, inputs))
    assert r['levels'] == p.t_to.tolist() and len(r['pos_traj']) == len(r['v_traj']) == len(p)
    assert torch.equal(torch.stack(r['v_traj']), torch.from_numpy(g['v_traj'].astype(np.int64)))
    close(torch.stack(r['pos_traj']), g['pos_traj'], TOL_TRAJ, (case, 'pos_traj'))
    if c['pos_only']:
        assert r['v0_traj'] == [] and r['vt_traj'] == []
    else:
        close(torch.stack(r['vt_traj']), g['vt_traj'], TOL_H, (case, 'vt_traj'))
    names = [n for n, _ in log]
    assert names.count('renoise_step') == p.num_renoise and names.count('posterior_step_program') == p.num_denoise
    assert names.count('model_forward') == p.num_denoise                     # no denoiser call on a renoise slot


def test_no_program_returns_no_levels_and_calls_the_native_layer_as_before(monkeypatch):
    _, inputs = PR.load_fixture('program_stride50')
    m, log = _stub_model(monkeypatch)
    r = _sample(m, 'program_stride50', inputs, num_steps=2, noise_source=draws.Source(1))
    assert 'levels' not in r and [n for n, _ in log].count('posterior_step') == 2


def test_argument_checks_raise_value_error(monkeypatch):
    _, inputs = PR.load_fixture('program_stride50')
    m, _ = _stub_model(monkeypatch)
    b = PR.case_batch('program_stride50')
    unsorted = b.ligand_element_batch.clone()
    unsorted[0], unsorted[-1] = 1, 0
    args = lambda bl=b.ligand_element_batch: (b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch, inputs['init_pos'],
                                               inputs['init_v'], bl)
    p = TimeProgram.strided(1000, 3)
    for what, a, kw in [
            ('together with num_steps', args(), dict(time_program=p, num_steps=3)),
            ('a program of another T', args(), dict(time_program=TimeProgram.strided(100, 3))),
            ('not a TimeProgram', args(), dict(time_program=[999, 500, -1])),
            ('unsorted ligand batch vector', args(unsorted), dict(time_program=p))]:
        with pytest.raises(ValueError):
            m.sample_diffusion(*a, center_pos_mode='protein', **kw)
            pytest.fail(what)
        with pytest.raises(ValueError):
            m.begin_sampling(*a, center_pos_mode='protein', **kw)
    with pytest.raises(TypeError):            # keyword-only
        m.sample_diffusion(*args(), None, 'protein', False, 0, None, True, None, p)


def test_driver_runs_one_program_for_all_batches(monkeypatch):
    from targetdiff_amd import models, sampling, workloads
    m, log = _stub_model(monkeypatch)
    plain = m.begin_sampling
    monkeypatch.setattr(models.ScorePosNet3D, 'begin_sampling', lambda self, *a, **k: plain(*a, **dict(k, use_session=False)))
    pk = workloads.synthetic_pocket(301, 70, 3.0, 9.0)
    g = torch.Generator().manual_seed(5)
    data = types.SimpleNamespace(protein_pos=torch.from_numpy(pk.pos), protein_atom_feature=torch.from_numpy(pk.feat),
                                 ligand_pos=torch.from_numpy(pk.pos).mean(0) + torch.randn(7, 3, generator=g),
                                 ligand_atom_feature_full=torch.randint(0, 13, (7,), generator=g))
    p = TimeProgram.from_levels(1000, [999, 600, 300, -1]).with_resampling(1, 2)
    assert len(p) == 7
    src = draws.Source(9300)
    res = sampling.sample_diffusion_ligand(m, data, 3, batch_size=2, device='cpu', ligand_num_atoms=[4, 6, 5], time_program=p,
                                           noise_source=lambda b, st, name, like: src(st + 1 + 20 * b, name, like),
                                           fixed_ligand_index=[4, 0, 5])
    pos, v, pos_traj, v_traj, v0_traj, vt_traj, times = res
    assert len(res) == 7 and len(times) == 2
    assert [x.shape for x in pos_traj] == [(7, 4, 3), (7, 6, 3), (7, 5, 3)] and [x.shape for x in vt_traj] == [(7, 4, 13), (7, 6, 13), (7, 5, 13)]
    want_pos, want_v = data.ligand_pos[[4, 0, 5]].numpy(), data.ligand_atom_feature_full[[4, 0, 5]].numpy()
    for k in range(3):          # the program ends on clean data: the known atoms end on their known state
        close(pos[k][:3], want_pos, TOL_FWD, ('fixed atoms of sample', k))
        assert np.array_equal(v[k][:3], want_v)
    names = [n for n, _ in log]
    assert names.count('renoise_step') == 2 * p.num_renoise and names.count('posterior_step_program') == 2 * p.num_denoise
    with pytest.raises(ValueError):
        sampling.sample_diffusion_ligand(m, data, 1, device='cpu', ligand_num_atoms=[4], time_program=p, num_steps=3)


# ------------------------------------------------------------------------------------------ binding layout
def test_step_io_layout_and_new_symbols():
    from targetdiff_amd import capi
    lib = capi.load_library()
    assert ctypes.sizeof(capi.StepIO) == lib.td_step_io_size()
    for name in ('td_posterior_step_program', 'td_renoise_step', 'td_session_set_program'):
        assert hasattr(lib, name) and name in capi.SIGNATURES
    assert capi.PROG_ROW == SCH.ROW == 12
    assert lib.td_session_set_program(None, None, None, 0) != 0            # a null session is an error, not a crash
