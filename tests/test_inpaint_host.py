"""Scaffold-constrained sampling, host side (CPU only): the fixtures of the real reference (tools/make_golden_inpaint.py) against the
CPU restatement of the rule (tests/_inpaint_ref.py), the argument checks of the sampler, the layout the batching driver builds for
``fixed_ligand_index`` (on a stand-in native layer), and the StepIO layout against the library's own sizeof(td_step_io).

Tolerances are tests/_tol.py's: atom types exact, free-running trajectories TOL_TRAJ = 5e-5 A.  Each fixture stores r, the fp32
reference's own distance from its float64 run; the generator only accepts r <= TOL_TRAJ / 5."""
import ctypes
import types

import numpy as np
import pytest
import torch

import _inpaint_ref as IR
from _tol import TOL_FWD, TOL_H, TOL_TRAJ, close
from oracle import draws, weights
from oracle.native_stub import RecordingNative, StubSession, _batch_of


# ------------------------------------------------------------------------------------------ fixtures vs restatement
@pytest.mark.parametrize('case', list(IR.CASES))
def test_restatement_reproduces_reference_fixture(case, state_dict):
    c = IR.CASES[case]
    g, inputs = IR.load_fixture(case)
    assert float(g['r']) <= TOL_TRAJ / 5, f'{case}: the fp32 reference itself is {float(g["r"]):.2e} A from float64'
    assert int(g['draws_base']) == c['base']
    r = IR.run(state_dict, IR.model_config(case), IR.case_batch(case), inputs, c['num_steps'], c['pos_only'], c['base'])
    v = torch.stack(r['v_traj'])
    assert torch.equal(v, torch.from_numpy(g['v_traj'].astype(np.int64))), f'{case}: atom types differ from the reference'
    d = close(torch.stack(r['pos_traj']), g['pos_traj'], TOL_TRAJ, (case, 'pos_traj'))
    print(f'{case}: max |dx| = {d:.3e} A over {c["num_steps"]} steps; reference fp32 vs float64 r = {float(g["r"]):.3e}')
    if not c['pos_only']:
        close(torch.stack(r['v0_traj']), g['v0_traj'], TOL_H, (case, 'v0_traj'))
        close(torch.stack(r['vt_traj']), g['vt_traj'], TOL_H, (case, 'vt_traj'))
    if c['num_steps'] == c['T']:          # t == 0 was reached: the known atoms ARE the known state
        m = inputs['fixed_mask']
        assert torch.equal(r['pos_traj_centred'][-1][m], r['x0_centred'][m])
        assert torch.equal(r['v_traj'][-1][m], inputs['fixed_v'][m])
        close(torch.from_numpy(g['pos_traj'][-1])[m], inputs['fixed_pos'][m], TOL_FWD, (case, 'final known atoms'))
        assert np.array_equal(g['v_traj'][-1][m.numpy()], inputs['fixed_v'][m].numpy())


# ------------------------------------------------------------------------------------------ argument checks
def _mirror(T=1000):
    from targetdiff_amd.models import ScorePosNet3D
    return ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG, num_diffusion_timesteps=T), 27, 13)


def _call(model, inputs, batch, **over):
    kw = dict(fixed_mask=inputs['fixed_mask'], fixed_pos=inputs['fixed_pos'], fixed_v=inputs['fixed_v'])
    kw.update(over)
    bl = kw.pop('batch_ligand', batch.ligand_element_batch)
    return model.sample_diffusion(batch.protein_pos, batch.protein_atom_feature.float(), batch.protein_element_batch, inputs['init_pos'],
                                  inputs['init_v'], bl, num_steps=2, center_pos_mode='protein', **kw)


def test_argument_checks_raise_value_error():
    case = 'inpaint_small_1000_first20'
    _, inputs = IR.load_fixture(case)
    batch = IR.case_batch(case)
    model = _mirror()
    n = inputs['init_pos'].shape[0]
    m = inputs['fixed_mask']
    bad_v = inputs['fixed_v'].clone()
    bad_v[m.nonzero()[0]] = 13
    neg_v = inputs['fixed_v'].clone()
    neg_v[m.nonzero()[-1]] = -1
    unsorted = batch.ligand_element_batch.clone()
    unsorted[0], unsorted[-1] = 1, 0
    for what, over in [
            ('mask not bool', dict(fixed_mask=m.to(torch.uint8))),
            ('mask not a tensor', dict(fixed_mask=m.tolist())),
            ('mask of the wrong length', dict(fixed_mask=m[:-1])),
            ('mask with two axes', dict(fixed_mask=m.unsqueeze(-1))),
            ('mask without fixed_pos', dict(fixed_pos=None)),
            ('mask without fixed_v', dict(fixed_v=None)),
            ('fixed_pos without a mask', dict(fixed_mask=None)),
            ('fixed_pos of the wrong shape', dict(fixed_pos=inputs['fixed_pos'][:, :2])),
            ('fixed_pos of the wrong length', dict(fixed_pos=inputs['fixed_pos'][:-1])),
            ('fixed_v of the wrong shape', dict(fixed_v=inputs['fixed_v'][:-1])),
            ('fixed_v not int64', dict(fixed_v=inputs['fixed_v'].float())),
            ('type too large on a flagged row', dict(fixed_v=bad_v)),
            ('negative type on a flagged row', dict(fixed_v=neg_v)),
            ('unsorted ligand batch vector', dict(batch_ligand=unsorted))]:
        with pytest.raises(ValueError):
            _call(model, inputs, batch, **over)
            pytest.fail(what)
    # rows outside the mask are ignored: a type out of range THERE passes the checks (and then reaches the native layer: no GPU here)
    ok_v = inputs['fixed_v'].clone()
    ok_v[(~m).nonzero()[0]] = 99
    with pytest.raises(RuntimeError, match='HIP devices only'):
        _call(model, inputs, batch, fixed_v=ok_v)
    assert n == m.numel()


# ------------------------------------------------------------------------------------------ the driver's layout
class _FixedNative(RecordingNative):
    """The recording stand-in plus the known-atom form of the posterior update (the rule of tests/_inpaint_ref.py)."""

    def posterior_step(self, t, ligand_ptr, ligand_pos, ligand_v, pred_pos, pred_v, noise, uniform, pos_next=None, v_next=None,
                       log_v0=None, log_post=None, fixed_mask=None, fixed_pos=None, fixed_v=None):
        super().posterior_step(t, ligand_ptr, ligand_pos, ligand_v, pred_pos, pred_v, noise, uniform, pos_next, v_next, log_v0, log_post)
        if fixed_mask is not None:
            self._rec('posterior_step_fixed', fixed_mask=fixed_mask, fixed_pos=fixed_pos, fixed_v=fixed_v)
            self.seen_fixed = (fixed_mask.clone(), fixed_pos.clone(), fixed_v.clone())
            xk, vk, lqk = IR.known_step(self.sched, t.long(), _batch_of(ligand_ptr), fixed_pos, fixed_v, noise, uniform, self.num_classes)
            pos_next[fixed_mask] = xk[fixed_mask]
            v_next[fixed_mask] = vk[fixed_mask]
            if log_post is not None:
                log_post[fixed_mask] = lqk[fixed_mask]
        return pos_next, v_next


class _FixedSession(StubSession):
    def make_step_io(self, *a, fixed_mask=None, fixed_pos=None, fixed_v=None, **k):
        io = super().make_step_io(*a, **k)
        io['fixed'] = {} if fixed_mask is None else dict(fixed_mask=fixed_mask, fixed_pos=fixed_pos, fixed_v=fixed_v)
        return io

    def step(self, io, use_graph=True):
        n = self.a[0]
        plain = n.posterior_step
        n.posterior_step = lambda *a, **k: plain(*a, **k, **io['fixed'])
        try:
            super().step(io, use_graph)
        finally:
            del n.posterior_step


def _driver_setup(monkeypatch, T):
    from targetdiff_amd import capi, models
    sd = weights.make_state_dict(2021)
    cfg = dict(weights.DEFAULT_MODEL_CONFIG, num_diffusion_timesteps=T)
    mirror = models.ScorePosNet3D(cfg, weights.PROTEIN_FEATURE_DIM, weights.LIGAND_FEATURE_DIM)
    assert not mirror.load_state_dict(sd, strict=False).unexpected_keys
    log = []
    native = _FixedNative(sd, cfg, mirror.num_classes, log)
    monkeypatch.setattr(models.ScorePosNet3D, '_native', lambda self, device: native)
    monkeypatch.setattr(capi, 'NativeSession', _FixedSession)
    return mirror, native, log


def _data():
    from targetdiff_amd import workloads
    p = workloads.synthetic_pocket(301, 70, 3.0, 9.0)
    g = torch.Generator().manual_seed(5)
    n = 7
    return types.SimpleNamespace(protein_pos=torch.from_numpy(p.pos), protein_atom_feature=torch.from_numpy(p.feat),
                                 ligand_pos=torch.from_numpy(p.pos).mean(0) + torch.randn(n, 3, generator=g),
                                 ligand_atom_feature_full=torch.randint(0, 13, (n,), generator=g))


@pytest.mark.parametrize('use_session', [True, False])
def test_driver_builds_the_documented_layout(monkeypatch, use_session):
    """[the fixed atoms, in the given order; new atoms], sizes raised to the number of fixed atoms; with T = 3 run in full (t == 0 is
    reached) the fixed atoms of every returned ligand are the reference ligand's, positions and types."""
    from targetdiff_amd import sampling
    mirror, native, log = _driver_setup(monkeypatch, T=3)
    if not use_session:
        from targetdiff_amd import capi
        monkeypatch.setattr(capi, 'NativeSession', None)          # would fail if a session were made
        plain = mirror.begin_sampling
        monkeypatch.setattr(mirror, 'begin_sampling', lambda *a, **k: plain(*a, **dict(k, use_session=False)))
    data = _data()
    idx = [4, 0, 5]
    src = draws.Source(9100)
    res = sampling.sample_diffusion_ligand(mirror, data, 3, batch_size=2, device='cpu', ligand_num_atoms=[2, 6, 3],
                                           noise_source=lambda b, st, name, like: src(st + 1 + 10 * b, name, like),
                                           fixed_ligand_index=idx)
    pos, v, pos_traj, v_traj, v0_traj, vt_traj, _ = res
    assert [p.shape[0] for p in pos] == [3, 6, 3]                 # 2 -> 3: at least the fixed atoms
    assert [p.shape for p in pos_traj] == [(3, 3, 3), (3, 6, 3), (3, 3, 3)]
    want_pos, want_v = data.ligand_pos[idx].numpy(), data.ligand_atom_feature_full[idx].numpy()
    for k in range(3):
        close(pos[k][:3], want_pos, TOL_FWD, ('fixed atoms of sample', k))
        assert np.array_equal(v[k][:3], want_v)
        assert np.array_equal(vt_traj[k][-1][:3].argmax(-1), want_v)
    # the last batch holds one sample of 3 atoms, all fixed; the batch before: the first 3 atoms of each of its 2 samples
    mask, fpos, fv = native.seen_fixed
    assert mask.tolist() == [True] * 3 and fv.tolist() == want_v.tolist()
    names = [n for n, _ in log]
    assert names.count('posterior_step_fixed') == names.count('posterior_step') == 6
    first = next(a for n, a in log if n == 'posterior_step_fixed')
    assert first['fixed_mask'] == ((9,), 'torch.bool', 'cpu') and first['fixed_pos'][0] == (9, 3) and first['fixed_v'][1] == 'torch.int64'


def test_driver_without_fixed_index_passes_nothing_down(monkeypatch):
    """No index, or an empty mask: the native layer is called exactly as before (the plain stub does not know the new arguments)."""
    from targetdiff_amd import capi, models, sampling
    sd = weights.make_state_dict(2021)
    cfg = dict(weights.DEFAULT_MODEL_CONFIG)
    mirror = models.ScorePosNet3D(cfg, 27, 13)
    mirror.load_state_dict(sd, strict=False)
    native = RecordingNative(sd, cfg, 13, [])
    monkeypatch.setattr(models.ScorePosNet3D, '_native', lambda self, device: native)
    monkeypatch.setattr(capi, 'NativeSession', StubSession)
    data = _data()
    src = draws.Source(9200)
    ns = lambda b, st, name, like: src(st + 1, name, like)
    a = sampling.sample_diffusion_ligand(mirror, data, 1, device='cpu', num_steps=2, ligand_num_atoms=[5], noise_source=ns)
    b = sampling.sample_diffusion_ligand(mirror, data, 1, device='cpu', num_steps=2, ligand_num_atoms=[5], noise_source=ns,
                                         fixed_ligand_index=[])
    assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[1][0], b[1][0])
    with pytest.raises(ValueError):
        sampling.sample_diffusion_ligand(mirror, data, 1, device='cpu', num_steps=2, ligand_num_atoms=[5], fixed_ligand_index=[7])
    with pytest.raises(ValueError):
        sampling.sample_diffusion_ligand(mirror, data, 1, device='cpu', num_steps=2, ligand_num_atoms=[5], fixed_ligand_index=[1, 1])
    with pytest.raises(ValueError):
        sampling.sample_diffusion_ligand(mirror, types.SimpleNamespace(protein_pos=data.protein_pos, protein_atom_feature=data.protein_atom_feature),
                                         1, device='cpu', num_steps=2, ligand_num_atoms=[5], fixed_ligand_index=[0])


# ------------------------------------------------------------------------------------------ binding layout
def test_step_io_layout_matches_library():
    from targetdiff_amd import capi
    lib = capi.load_library()
    assert ctypes.sizeof(capi.StepIO) == lib.td_step_io_size()
    names = [f[0] for f in capi.StepIO._fields_]
    assert names[-3:] == ['d_fixed_mask', 'd_fixed_pos', 'd_fixed_v']            # appended: the earlier fields keep their offsets
    assert capi.StepIO.d_ligand_graph_bias.offset + 8 == capi.StepIO.d_fixed_mask.offset
    io = capi.StepIO()                                                            # zero-initialised: the library memcmp's the block
    assert bytes(io) == b'\0' * ctypes.sizeof(capi.StepIO)
