"""Scaffold-constrained sampling on the MI355X (``-m gpu``): known ligand atoms are kept fixed by replacement conditioning inside the
posterior kernel (DESIGN.md "Scaffold-constrained sampling").

  * the three fixtures of the real reference's own methods (tools/make_golden_inpaint.py) through ``sample_diffusion`` with the
    injected counter draws: types exact, positions within TOL_TRAJ, log-probabilities within TOL_H; the known atoms' rows against the
    closed form within TOL_FWD; at t == 0 the centred state is the known state bit for bit;
  * no mask, an all-False mask and the call without the new arguments: torch.equal, from torch's global generator (the stream of
    draws is untouched);
  * session == stateless and captured hipGraph == launch by launch with a mask, torch.equal; a mask that changes between calls and
    inside a live session (re-capture);
  * the batching driver with ``fixed_ligand_index`` on the 1h36 pocket and its docked ligand, sequential and overlapped.

Tolerances: tests/_tol.py.
"""
import types

import numpy as np
import pytest
import torch

import _inpaint_ref as IR
from _tol import TOL_FWD, TOL_H, TOL_TRAJ, close
from conftest import load_golden, pocket_1h36
from oracle import draws, weights
from oracle import restatement as R

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


def _model(state_dict, T):
    from targetdiff_amd.models import ScorePosNet3D
    m = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG, num_diffusion_timesteps=T), 27, 13)
    assert not m.load_state_dict(state_dict, strict=False).unexpected_keys
    return m.to(_dev()).eval()


@pytest.fixture(scope='module')
def model(state_dict):
    return _model(state_dict, 1000)


@pytest.fixture(scope='module')
def model_T100(state_dict):
    return _model(state_dict, 100)


def _args(batch, inputs, dev):
    b = batch.to(dev)
    return (b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch, inputs['init_pos'].to(dev), inputs['init_v'].to(dev),
            b.ligand_element_batch)


def _fixed(inputs, dev, mask=None):
    return dict(fixed_mask=(inputs['fixed_mask'] if mask is None else mask).to(dev), fixed_pos=inputs['fixed_pos'].to(dev),
                fixed_v=inputs['fixed_v'].to(dev))


def _same(a, b, what):
    for k in ('pos_traj', 'v_traj', 'v0_traj', 'vt_traj'):
        assert len(a[k]) == len(b[k]), (what, k)
        for s, (x, y) in enumerate(zip(a[k], b[k])):
            assert torch.equal(x, y), f'{what}: {k} differs at step {s}'
    assert torch.equal(a['pos'], b['pos']) and torch.equal(a['v'], b['v']), what


# ------------------------------------------------------------------------------------------ the reference's fixtures
@pytest.mark.parametrize('case', list(IR.CASES))
def test_fixture_of_the_reference(case, model, model_T100):
    dev = _dev()
    c = IR.CASES[case]
    m = model_T100 if c['T'] == 100 else model
    g, inputs = IR.load_fixture(case)
    batch = IR.case_batch(case)
    sampler = m.begin_sampling(*_args(batch, inputs, dev), num_steps=c['num_steps'], center_pos_mode='protein',
                               noise_source=draws.Source(c['base'], dev), pos_only=c['pos_only'], **_fixed(inputs, dev))
    while not sampler.done:
        sampler.step()
    r = sampler.finish()
    S, K = c['num_steps'], 13
    mask = inputs['fixed_mask']
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
        assert torch.equal(v, inputs['init_v'].expand(S, -1))            # pos_only: every type stays frozen
    # ---- the known atoms against the closed form, every step (fp32 on the CPU, the sampler's own offset)
    cfg = IR.model_config(case)
    sched = R.diffusion_schedules(cfg)
    bl = batch.ligand_element_batch
    off = sampler.offset.cpu()
    x0c = inputs['fixed_pos'] - off[bl]
    assert torch.equal(sampler._fixed['fixed_pos'].cpu()[mask], x0c[mask])          # centred exactly as the ligand state is
    src = draws.Source(c['base'])
    for s, i in enumerate(reversed(range(c['T'] - S, c['T']))):
        t = torch.full((batch.num_graphs,), i, dtype=torch.long)
        noise = src.noise(s, (mask.numel(), 3))
        uniform = None if c['pos_only'] else src.uniform(s, (mask.numel(), K))
        xk, vk, lqk = IR.known_step(sched, t, bl, x0c, inputs['fixed_v'], noise, uniform, K)
        close(r['pos_traj'][s][mask], (xk + off[bl])[mask], TOL_FWD, (case, 'known positions, closed form'))
        if not c['pos_only']:
            assert torch.equal(r['v_traj'][s][mask], vk[mask]), (case, s)
            close(r['vt_traj'][s][mask], lqk[mask], TOL_FWD, (case, 'known log q, closed form'))
    # ---- t == 0: the centred state IS the known state
    if S == c['T']:
        assert torch.equal(sampler.lpos[mask.to(dev)], sampler._fixed['fixed_pos'][mask.to(dev)])
        assert torch.equal(sampler.lv[mask.to(dev)], inputs['fixed_v'].to(dev)[mask.to(dev)])
        assert torch.equal(r['v'].cpu()[mask], inputs['fixed_v'][mask])
        close(r['pos'][mask.to(dev)], inputs['fixed_pos'][mask], TOL_FWD, (case, 'returned known positions'))
        want_last = torch.log(torch.nn.functional.one_hot(inputs['fixed_v'], K).float().clamp(min=1e-30))
        close(r['vt_traj'][-1][mask], want_last[mask], TOL_FWD, (case, 'vt_traj of the known atoms at t == 0'))


# ------------------------------------------------------------------------------------------ no mask: nothing changes
@pytest.mark.parametrize('pos_only', [False, True])
def test_no_mask_is_bit_identical(model, pos_only):
    """From torch's global generator: the same seed gives the same bits with no mask, an all-False mask and the call as it was
    before the arguments existed -- the stream of draws is untouched.  A real mask does change the result."""
    dev = _dev()
    case = 'inpaint_pos_only' if pos_only else 'inpaint_small_1000_first20'
    _, inputs = IR.load_fixture(case)
    batch = IR.case_batch(case)
    args = _args(batch, inputs, dev)
    kw = dict(num_steps=12, center_pos_mode='protein', pos_only=pos_only)

    def run(**extra):
        torch.manual_seed(4242)
        torch.cuda.manual_seed_all(4242)
        return model.sample_diffusion(*args, **kw, **extra)
    base = run()
    _same(base, run(fixed_mask=None, fixed_pos=None, fixed_v=None), 'mask None')
    _same(base, run(**_fixed(inputs, dev, mask=torch.zeros_like(inputs['fixed_mask']))), 'all-False mask')
    _same(base, run(use_session=False), 'stateless')
    masked = run(**_fixed(inputs, dev))
    assert not torch.equal(masked['pos_traj'][0], base['pos_traj'][0])


# ------------------------------------------------------------------------------------------ session / graph identities
def test_session_stateless_graph_eager_identical_with_mask(model):
    dev = _dev()
    case = 'inpaint_small_1000_first20'
    c = IR.CASES[case]
    _, inputs = IR.load_fixture(case)
    batch = IR.case_batch(case)
    args = _args(batch, inputs, dev)

    def run(mask=None, **kw):
        return model.sample_diffusion(*args, num_steps=c['num_steps'], center_pos_mode='protein',
                                      noise_source=draws.Source(c['base'], dev), **_fixed(inputs, dev, mask), **kw)
    eager = run(use_graph=False)
    _same(eager, run(use_session=False), 'session vs stateless')
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        graph = run(use_graph=True)
        # the mask changes between two calls on the same model
        other = torch.zeros_like(inputs['fixed_mask'])
        other[[2, 3, 10]] = True
        graph2 = run(mask=other, use_graph=True)
    torch.cuda.current_stream(dev).wait_stream(side)
    _same(eager, graph, 'captured hipGraph vs launch by launch')
    eager2 = run(mask=other, use_graph=False)
    _same(eager2, graph2, 'second mask: captured hipGraph vs launch by launch')
    assert not torch.equal(eager2['pos_traj'][0], eager['pos_traj'][0])


@pytest.mark.parametrize('pos_only', [False, True])
def test_pos_only_and_mask_swap_inside_a_session(model, pos_only):
    """One live session: the argument block changes after a few replayed steps (another mask tensor), the library re-captures the
    step and keeps replaying; equal to the same sequence issued launch by launch, and to the stateless form."""
    dev = _dev()
    case = 'inpaint_pos_only'
    c = IR.CASES[case]
    _, inputs = IR.load_fixture(case)
    batch = IR.case_batch(case)
    other = torch.zeros_like(inputs['fixed_mask'])
    other[[1, 9]] = True

    def run(use_graph, use_session=True):
        s = model.begin_sampling(*_args(batch, inputs, dev), num_steps=10, center_pos_mode='protein',
                                 noise_source=draws.Source(c['base'], dev), pos_only=pos_only, use_graph=use_graph,
                                 use_session=use_session, **_fixed(inputs, dev))
        replayed = []
        other_dev = other.to(dev)
        for k in range(10):
            if k == 5:
                s._fixed = dict(s._fixed, fixed_mask=other_dev)
                if s._io is not None:
                    s._io.d_fixed_mask = other_dev.data_ptr()
            s.step()
            replayed.append(s.session.last_step_was_graph() if s.session is not None else False)
        return s.finish(), replayed
    eager, rep_e = run(False)
    assert not any(rep_e)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        graph, rep_g = run(True)
    torch.cuda.current_stream(dev).wait_stream(side)
    assert rep_g[1:5] == [True] * 4 and rep_g[5:] == [True] * 5, rep_g       # step 5 re-captures and replays
    _same(eager, graph, 'mask swapped at step 5: hipGraph vs launch by launch')
    stateless, _ = run(False, use_session=False)
    _same(eager, stateless, 'mask swapped at step 5: session vs stateless')


def test_model_without_alphas_cumprod_refuses_a_mask(model):
    """A native model created from the 7 mandatory schedules has no abar table: a mask is an error, not a read of a null table."""
    from targetdiff_amd import capi
    dev = _dev()
    nat = model._native(dev)
    sched = {k: getattr(model, k).detach().cpu().numpy() for k in capi.SCHEDULE_ORDER}
    rn = model.refine_net
    cfg = dict(hidden_dim=rn.hidden_dim, n_heads=rn.n_heads, knn=rn.k, num_layers=rn.num_layers, num_r_gaussian=rn.num_r_gaussian,
               edge_feat_dim=rn.edge_feat_dim, protein_feat_dim=27, ligand_num_classes=13, num_timesteps=1000)
    bare = capi.NativeModel(cfg, model.state_dict(), sched, device=dev)
    n = 5
    lptr = torch.tensor([0, n], dtype=torch.int32, device=dev)
    t = torch.full((1,), 500, dtype=torch.int32, device=dev)
    pos, v = torch.randn(n, 3, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    pv, u = torch.randn(n, 13, device=dev), torch.rand(n, 13, device=dev)
    bare.posterior_step(t, lptr, pos, v, pos, pv, pos, u)                                  # no mask: fine
    with pytest.raises(RuntimeError, match='alphas_cumprod'):
        bare.posterior_step(t, lptr, pos, v, pos, pv, pos, u, fixed_mask=torch.ones(n, dtype=torch.bool, device=dev), fixed_pos=pos,
                            fixed_v=v)
    del nat


# ------------------------------------------------------------------------------------------ the driver
_CLASS_OF = {'C': 0, 'N': 2, 'O': 4}          # non-aromatic classes of the reference's add_aromatic featurisation


def _docked_data():
    pocket, sizes = pocket_1h36()
    lig = load_golden('ligand_1h36_docked.npz')
    full = np.asarray([_CLASS_OF.get(e, 10) for e in lig['elements']], dtype=np.int64)
    return types.SimpleNamespace(protein_pos=torch.from_numpy(pocket.pos), protein_atom_feature=torch.from_numpy(pocket.feat),
                                 ligand_pos=torch.from_numpy(lig['pos']), ligand_atom_feature_full=torch.from_numpy(full)), sizes


@pytest.mark.parametrize('overlap', [False, True])
def test_driver_keeps_the_docked_fragment(model_T100, overlap):
    """1h36 with its docked ligand: 10 of its 25 atoms (a ring with its oxygen substituent) are kept, 4 samples, T = 100 run in full."""
    from targetdiff_amd import sampling
    dev = _dev()
    data, sizes = _docked_data()
    idx = [3, 4, 5, 6, 7, 8, 9, 10, 11, 0]
    assert all(data.ligand_atom_feature_full[i] in (0, 2, 4) for i in idx)
    torch.manual_seed(77)
    res = sampling.sample_diffusion_ligand(model_T100, data, 4, batch_size=2, device=str(dev), center_pos_mode='protein',
                                           ligand_num_atoms=[int(s) for s in sizes[:3]] + [4], overlap_batches=overlap,
                                           fixed_ligand_index=idx)
    pos, v, pos_traj, v_traj, v0_traj, vt_traj, _ = res
    assert [p.shape[0] for p in pos] == [int(s) for s in sizes[:3]] + [10] and pos_traj[0].shape[0] == 100
    want_pos, want_v = data.ligand_pos[idx].numpy(), data.ligand_atom_feature_full[idx].numpy()
    for k in range(4):
        close(pos[k][:10], want_pos, TOL_FWD, ('docked atoms of sample', k, 'overlap' if overlap else 'sequential'))
        assert np.array_equal(v[k][:10], want_v), k
        assert np.isfinite(pos[k]).all() and (0 <= v[k]).all() and (v[k] < 13).all()
    assert all(int(sz) > 10 for sz in sizes[:3])                    # the first three samples have grown atoms next to the fragment
