"""Sampling time programs on the MI355X (``-m gpu``): strided reverse steps and resampling jumps ("Time programs").

  * the five fixtures of the real reference's own methods (tools/make_golden_program.py) through ``sample_diffusion`` with the injected
    counter draws: types exact, positions within TOL_TRAJ, log-probabilities within TOL_H;
  * ``TimeProgram.reference(T, n)`` == ``num_steps=n`` without a program, torch.equal: with and without a mask, pos_only on and off,
    session and stateless, captured hipGraph and launch by launch, model_mean_type 'noise';
  * a program with jumps and a mask: graph replay == launch by launch == stateless, torch.equal; a denoise step after a renoise step
    replays the graph; the device step index ends at len(program);
  * the renoise step alone against the CPU restatement (tests/_program_ref.py) on given draws;
  * the batching driver with a program and ``fixed_ligand_index`` on the docked 1h36 fixture, sequential and overlapped;
  * the documented ValueErrors and the native layer's argument errors.

Tolerances: tests/_tol.py.
"""
import types

import numpy as np
import pytest
import torch

import _program_ref as PR
from _tol import TOL_FWD, TOL_H, TOL_TRAJ, TOL_X, close
from conftest import load_golden, pocket_1h36
from oracle import draws, weights
from targetdiff_amd import schedule as SCH
from targetdiff_amd.schedule import TimeProgram

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


_MODELS = {}


def _model(case='program_stride50', **over):
    key = (case, tuple(sorted(over.items())))
    if key not in _MODELS:
        from targetdiff_amd.models import ScorePosNet3D
        m = ScorePosNet3D(dict(PR.model_config(case), **over), 27, 13)
        assert not m.load_state_dict(PR.state_dict(case), strict=False).unexpected_keys
        _MODELS[key] = m.to(_dev()).eval()
    return _MODELS[key]


def _args(case, inputs, dev):
    b = PR.case_batch(case).to(dev)
    return (b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch, inputs['init_pos'].to(dev), inputs['init_v'].to(dev),
            b.ligand_element_batch)


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


# ------------------------------------------------------------------------------------------ the reference's fixtures
@pytest.mark.parametrize('case', list(PR.CASES))
def test_fixture_of_the_reference(case):
    dev = _dev()
    c = PR.CASES[case]
    m = _model(case)
    g, inputs = PR.load_fixture(case)
    p = PR.program(case)
    assert np.array_equal(g['table'].view(np.uint32), p.tables(m).view(np.uint32))
    r = m.sample_diffusion(*_args(case, inputs, dev), center_pos_mode='protein', noise_source=draws.Source(c['base'], dev),
                           pos_only=c['pos_only'], time_program=p, **PR.fixed_kwargs(case, inputs, dev))
    S = len(p)
    assert r['levels'] == p.t_to.tolist() and len(r['pos_traj']) == len(r['v_traj']) == S
    pos, v = torch.stack(r['pos_traj']), torch.stack(r['v_traj'])
    want_v = torch.from_numpy(g['v_traj'].astype(np.int64))
    flips = (v != want_v).any(dim=1)
    dx = (pos.double() - torch.from_numpy(g['pos_traj']).double()).abs().reshape(S, -1).max(dim=1).values
    print(f'{case}: max |dx| = {float(dx.max()):.3e} A (step {int(dx.argmax())}), first type flip: '
          f'{int(flips.float().argmax()) if bool(flips.any()) else None}; reference fp32 vs float64 r = {float(g["r"]):.3e}')
    assert torch.equal(v, want_v), f'{case}: atom types differ from the reference'
    close(pos, g['pos_traj'], TOL_TRAJ, (case, 'pos_traj'))
    if not c['pos_only']:
        d0 = close(torch.stack(r['v0_traj']), g['v0_traj'], TOL_H, (case, 'v0_traj'))
        dt = close(torch.stack(r['vt_traj']), g['vt_traj'], TOL_H, (case, 'vt_traj'))
        print(f'{case}: max |d v0_traj| = {d0:.3e}, max |d vt_traj| = {dt:.3e}')
    else:
        assert r['v0_traj'] == [] and r['vt_traj'] == []
        assert torch.equal(v, inputs['init_v'].expand(S, -1))            # pos_only: every type stays frozen, renoise slots too
    if c['mask'] and int(p.t_to[-1]) == -1:          # clean data was reached: the known atoms end on their known state
        mk = inputs['fixed_mask']
        assert torch.equal(r['v'].cpu()[mk], inputs['fixed_v'][mk])
        close(r['pos'].cpu()[mk], inputs['fixed_pos'][mk], TOL_FWD, (case, 'returned known positions'))


# ------------------------------------------------------------------------------------------ a unit-step program is the sampler as it was
@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('pos_only', [False, True])
def test_reference_program_is_bit_identical_to_num_steps(mask, pos_only):
    dev = _dev()
    like = 'inpaint_pos_only' if pos_only else 'inpaint_small_1000_first20'
    import _inpaint_ref as IR
    _, inputs = IR.load_fixture(like)
    b = IR.case_batch(like).to(dev)
    args = (b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch, inputs['init_pos'].to(dev), inputs['init_v'].to(dev),
            b.ligand_element_batch)
    fixed = dict(fixed_mask=inputs['fixed_mask'].to(dev), fixed_pos=inputs['fixed_pos'].to(dev), fixed_v=inputs['fixed_v'].to(dev)) if mask else {}
    n = 7
    m = _model()

    def run(program, **kw):
        steps = dict(time_program=TimeProgram.reference(1000, n)) if program else dict(num_steps=n)
        return m.sample_diffusion(*args, center_pos_mode='protein', noise_source=draws.Source(8800, dev), pos_only=pos_only, **steps,
                                  **fixed, **kw)
    for what, kw in [('session, launch by launch', dict(use_graph=False)), ('stateless', dict(use_session=False))]:
        a, bb = run(False, **kw), run(True, **kw)
        _same(a, bb, f'{what}, mask={mask}, pos_only={pos_only}')
        assert 'levels' not in a and bb['levels'] == list(range(998, 998 - n, -1))
    a, bb = _on_side_stream(dev, lambda: (run(False, use_graph=True), run(True, use_graph=True)))
    _same(a, bb, f'captured hipGraph, mask={mask}, pos_only={pos_only}')
    _same(bb, run(True, use_session=False), 'program: graph vs stateless')


def test_reference_program_runs_to_clean_data_like_the_full_chain():
    """T = 100 in full: the last unit step 0 -> -1 keeps the reference's clamp t - 1 -> 0 (models/molopt_score_model.py:403-405)"""
    dev = _dev()
    import _inpaint_ref as IR
    like = 'inpaint_small_T100'
    _, inputs = IR.load_fixture(like)
    b = IR.case_batch(like).to(dev)
    from targetdiff_amd.models import ScorePosNet3D
    m = ScorePosNet3D(IR.model_config(like), 27, 13)
    m.load_state_dict(weights.make_state_dict(2021), strict=False)
    m = m.to(dev).eval()
    args = (b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch, inputs['init_pos'].to(dev), inputs['init_v'].to(dev),
            b.ligand_element_batch)
    fixed = dict(fixed_mask=inputs['fixed_mask'].to(dev), fixed_pos=inputs['fixed_pos'].to(dev), fixed_v=inputs['fixed_v'].to(dev))
    run = lambda **kw: m.sample_diffusion(*args, center_pos_mode='protein', noise_source=draws.Source(8900, dev), **fixed, **kw)
    a = run()
    bb = run(time_program=TimeProgram.reference(100))
    _same(a, bb, 'T = 100 in full')
    assert bb['levels'][-1] == -1


def test_reference_program_with_noise_mean_type():
    dev = _dev()
    m = _model(model_mean_type='noise')
    _, inputs = PR.load_fixture('program_stride50')
    args = _args('program_stride50', inputs, dev)
    run = lambda **kw: m.sample_diffusion(*args, center_pos_mode='protein', noise_source=draws.Source(9000, dev), **kw)
    _same(run(num_steps=5, use_graph=False), run(time_program=TimeProgram.reference(1000, 5), use_graph=False), "mean type 'noise'")
    # a strided program under 'noise': the stateless and the session form agree, and the run is finite
    p = TimeProgram.from_levels(1000, [999, 940, 870, 800]).with_resampling(1, 2)
    a, bb = run(time_program=p, use_graph=False), run(time_program=p, use_session=False)
    _same(a, bb, "mean type 'noise', strided")
    assert torch.isfinite(a['pos']).all()


# ------------------------------------------------------------------------------------------ session / graph identities under a program
def test_session_graph_eager_stateless_identical_with_jumps_and_mask():
    dev = _dev()
    case = 'program_stride50_jump3x2_mask'
    c = PR.CASES[case]
    m = _model(case)
    _, inputs = PR.load_fixture(case)
    p = PR.program(case)
    kinds = p.kind.tolist()

    def run(use_graph, use_session=True):
        s = m.begin_sampling(*_args(case, inputs, dev), center_pos_mode='protein', noise_source=draws.Source(c['base'], dev),
                             use_graph=use_graph, use_session=use_session, time_program=p, **PR.fixed_kwargs(case, inputs, dev))
        replayed = []
        while not s.done:
            s.step()
            replayed.append(bool(s.session.last_step_was_graph()) if s.session is not None else False)
        index = int(s._step_index[0]) if s.session is not None else None
        return s.finish(), replayed, index
    eager, rep_e, idx_e = run(False)
    assert not any(rep_e) and idx_e == len(p)
    graph, rep_g, idx_g = _on_side_stream(dev, lambda: run(True))
    assert idx_g == len(p)
    first_renoise = kinds.index(SCH.RENOISE)
    assert first_renoise >= 2
    for k, (kind, rep) in enumerate(zip(kinds, rep_g)):
        if kind == SCH.RENOISE:
            assert not rep, f'slot {k}: a renoise step is launched eagerly, never as a graph'
        elif k >= 1:
            assert rep, f'slot {k}: a denoise step replays the captured graph (the step after a renoise step too)'
    assert rep_g[first_renoise + 1] is True and kinds[first_renoise + 1] == SCH.DENOISE
    _same(eager, graph, 'captured hipGraph vs launch by launch')
    stateless, _, _ = run(False, use_session=False)
    _same(eager, stateless, 'session vs stateless')
    # the default (use_graph=None) on the default stream: launch by launch, the same bits
    auto = m.sample_diffusion(*_args(case, inputs, dev), center_pos_mode='protein', noise_source=draws.Source(c['base'], dev),
                              time_program=p, **PR.fixed_kwargs(case, inputs, dev))
    _same(eager, auto, 'use_graph=None')


# ------------------------------------------------------------------------------------------ the renoise step alone
@pytest.mark.parametrize('jump', [(499, 500), (849, 999), (0, 30), (-1, 4)])
def test_renoise_step_matches_the_cpu_restatement(jump):
    dev = _dev()
    m = _model()
    nat = m._native(dev)
    s, t = jump
    row = torch.from_numpy(TimeProgram(1000, [0, 1], [999, s], [s, t]).tables(m)[1])
    n, K = 300, 13
    src = draws.Source(9400 + t)
    pos = 3.0 * src.noise(0, (n, 3))
    v = (src.uniform(1, (n,)) * K).long().clamp(max=K - 1)
    noise, uniform = src.noise(2, (n, 3)), src.uniform(3, (n, K))
    want_pos, want_v, want_l0, want_lq = PR.renoise_step(row, pos, v, noise, uniform, K)
    l0, lq = torch.empty(n, K, device=dev), torch.empty(n, K, device=dev)
    got_pos, got_v = nat.renoise_step(row.to(dev), pos.to(dev), v.to(dev), noise.to(dev), uniform.to(dev), log_v0=l0, log_q=lq)
    assert torch.equal(got_v.cpu(), want_v)
    close(got_pos, want_pos, TOL_X, (jump, 'positions'))
    close(lq, want_lq, TOL_H, (jump, 'log q'))
    close(l0, want_l0, TOL_H, (jump, 'log one-hot'))
    assert (got_v.cpu() != v).any() or t - s < 100        # a long jump moves some types
    # pos_only: no uniforms, the types come back untouched
    p2, v2 = nat.renoise_step(row.to(dev), pos.to(dev), v.to(dev), noise.to(dev), None)
    assert torch.equal(v2.cpu(), v) and torch.equal(p2, got_pos)
    # in place
    pd, vd = pos.to(dev), v.to(dev)
    nat.renoise_step(row.to(dev), pd, vd, noise.to(dev), uniform.to(dev), pos_next=pd, v_next=vd)
    assert torch.equal(pd, got_pos) and torch.equal(vd, got_v)


def test_native_argument_errors():
    dev = _dev()
    m = _model()
    nat = m._native(dev)
    n = 5
    pos, v = torch.randn(n, 3, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        nat.renoise_step(torch.zeros(5, device=dev), pos, v, pos)                     # not a row
    with pytest.raises(ValueError):
        nat.renoise_step(torch.zeros(12, dtype=torch.float64, device=dev), pos, v, pos)
    # a session whose program does not match the step block, and a program run past its end
    _, inputs = PR.load_fixture('program_stride50')
    p = TimeProgram.strided(1000, 2)
    s = m.begin_sampling(*_args('program_stride50', inputs, dev), center_pos_mode='protein', time_program=p, use_graph=False)
    s.session.set_program(torch.zeros(3, 12, device=dev), [0, 0, 0])
    with pytest.raises(RuntimeError, match='slots'):
        s.step()
    s.session.set_program(s._prog_table, s._prog_kinds)
    s.step(), s.step()
    with pytest.raises(RuntimeError, match='end'):
        s.session.step(s._io, use_graph=False)
    with pytest.raises(RuntimeError, match='kind'):
        s.session.set_program(s._prog_table, [0, 7])
    with pytest.raises(ValueError):
        s.session.set_program(torch.zeros(2, 11, device=dev), [0, 0])


# ------------------------------------------------------------------------------------------ the documented ValueErrors
def test_argument_checks_raise_value_error():
    dev = _dev()
    m = _model()
    _, inputs = PR.load_fixture('program_stride50')
    args = _args('program_stride50', inputs, dev)
    p = TimeProgram.strided(1000, 3)
    unsorted = args[5].clone()
    unsorted[0], unsorted[-1] = 1, 0
    for what, a, kw in [('together with num_steps', args, dict(time_program=p, num_steps=3)),
                        ('a program of another T', args, dict(time_program=TimeProgram.strided(100, 3))),
                        ('not a TimeProgram', args, dict(time_program=[999, 500, -1])),
                        ('unsorted ligand batch vector', args[:5] + (unsorted,), dict(time_program=p))]:
        with pytest.raises(ValueError):
            m.sample_diffusion(*a, center_pos_mode='protein', **kw)
            pytest.fail(what)


# ------------------------------------------------------------------------------------------ the driver
_CLASS_OF = {'C': 0, 'N': 2, 'O': 4}          # non-aromatic classes of the reference's add_aromatic featurisation


def _docked_data():
    pocket, sizes = pocket_1h36()
    lig = load_golden('ligand_1h36_docked.npz')
    full = np.asarray([_CLASS_OF.get(e, 10) for e in lig['elements']], dtype=np.int64)
    return types.SimpleNamespace(protein_pos=torch.from_numpy(pocket.pos), protein_atom_feature=torch.from_numpy(pocket.feat),
                                 ligand_pos=torch.from_numpy(lig['pos']), ligand_atom_feature_full=torch.from_numpy(full)), sizes


@pytest.mark.parametrize('overlap', [False, True])
def test_driver_with_program_keeps_the_docked_fragment(overlap):
    """1h36 with its docked ligand: 10 of its 25 atoms are kept, 4 samples in 2 batches, 20 strided steps with jumps of 3 sampled twice."""
    from targetdiff_amd import sampling
    dev = _dev()
    m = _model()
    data, sizes = _docked_data()
    idx = [3, 4, 5, 6, 7, 8, 9, 10, 11, 0]
    p = TimeProgram.strided(1000, 20).with_resampling(3, 2)
    assert len(p) == 20 + 6 * 4 and int(p.t_to[-1]) == -1
    torch.manual_seed(78)
    res = sampling.sample_diffusion_ligand(m, data, 4, batch_size=2, device=str(dev), center_pos_mode='protein',
                                           ligand_num_atoms=[int(s) for s in sizes[:3]] + [4], overlap_batches=overlap,
                                           fixed_ligand_index=idx, time_program=p)
    pos, v, pos_traj, v_traj, v0_traj, vt_traj, times = res
    assert len(res) == 7 and len(times) == 2
    want_sizes = [int(s) for s in sizes[:3]] + [10]
    assert [x.shape for x in pos] == [(n, 3) for n in want_sizes] and [x.shape for x in v] == [(n,) for n in want_sizes]
    assert [x.shape for x in pos_traj] == [(len(p), n, 3) for n in want_sizes]
    assert [x.shape for x in v_traj] == [(len(p), n) for n in want_sizes]
    assert [x.shape for x in v0_traj] == [x.shape for x in vt_traj] == [(len(p), n, 13) for n in want_sizes]
    want_pos, want_v = data.ligand_pos[idx].numpy(), data.ligand_atom_feature_full[idx].numpy()
    for k in range(4):
        close(pos[k][:10], want_pos, TOL_FWD, ('docked atoms of sample', k, 'overlap' if overlap else 'sequential'))
        assert np.array_equal(v[k][:10], want_v), k
        assert np.isfinite(pos_traj[k]).all() and (0 <= v_traj[k]).all() and (v_traj[k] < 13).all()
