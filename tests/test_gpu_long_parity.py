"""Parity of the HIP path on the BASELINE configurations the first fixture set did not reach (round-2 goldens, all from the
real reference: oracle/make_golden_r2.py).  Needs an MI355X: ``-m gpu``.

  * BASELINE config 1 in full: 1h36 x 4 samples, 100 steps -- free-running and teacher-forced;
  * a complete 1000-step trajectory (crosses t < 10, ends with the noiseless t = 0 step);
  * a C5-shaped forward (1000-atom pocket, > 704 nodes per graph, a 150-atom ligand) through td_model_forward and the session;
  * sampling session == stateless forward over 300 steps, bit for bit;
  * the batching driver ``sample_diffusion_ligand`` value by value, incl. its pos_only branch.

Tolerances (fp32, stated once): atom types and neighbour indices bit-exact; free-running trajectories |dx| <= 5e-5 A;
teacher-forced single steps |dx| <= 1e-5 A, |d log-prob| <= 1e-4 (tests/_tol.py).
"""
import types

import numpy as np
import pytest
import torch

from conftest import load_golden, pocket_1h36

pytestmark = pytest.mark.gpu

from _tol import TOL_TRAJ, TOL_FWD, close, maxdiff as _maxdiff
from _tol import TOL_X as TOL_STEP, TOL_H as TOL_LOGP


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def model(state_dict):
    from oracle import weights
    from targetdiff_amd.models import ScorePosNet3D
    dev = _dev()
    m = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG), 27, 13)
    assert not m.load_state_dict(state_dict, strict=False).unexpected_keys
    return m.to(dev).eval()


def _golden_or_skip(name):
    import os
    from conftest import GOLDEN
    if not os.path.exists(os.path.join(GOLDEN, name)):
        pytest.skip(f'{name} not generated yet (oracle/make_golden_r3.py)')
    return load_golden(name)


def _free_run(model, batch, init_pos, init_v, steps, base, dev, **kw):
    from oracle import draws
    b = batch.to(dev)
    return model.sample_diffusion(b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch,
                                  init_pos.to(dev), init_v.to(dev), b.ligand_element_batch, num_steps=steps,
                                  center_pos_mode='protein', noise_source=draws.Source(base, dev), **kw)


def _one_step(model, batch, pos_in, v_in, t, step, base, dev):
    """One teacher-forced reverse step at timestep ``t`` from the reference's own state (un-centred positions), with the
    draws the reference used at loop index ``step``; every call goes through the C ABI."""
    from oracle import draws
    b = batch.to(dev)
    nat = model._native(dev)
    B = b.num_graphs
    pptr, lptr = nat.graph_ptr(b.protein_element_batch, B), nat.graph_ptr(b.ligand_element_batch, B)
    ppos, lpos = b.protein_pos.clone(), pos_in.to(dev).clone().float()
    off = nat.center_pos(ppos, pptr, lpos, lptr)
    lv = v_in.to(dev).long()
    preds = nat.model_forward(ppos, b.protein_atom_feature.float(), pptr, lpos, lv, lptr, want_final_h=False)
    src = draws.Source(base, dev)
    t32 = torch.full((B,), t, dtype=torch.int32, device=dev)
    C = model.num_classes
    log_v0 = torch.empty(lpos.shape[0], C, device=dev)
    log_post = torch.empty_like(log_v0)
    pos_next, v_next = nat.posterior_step(t32, lptr, lpos, lv, preds['pred_ligand_pos'], preds['pred_ligand_v'],
                                          src.noise(step, lpos.shape), src.uniform(step, (lpos.shape[0], C)),
                                          log_v0=log_v0, log_post=log_post)
    return pos_next + off[b.ligand_element_batch], v_next, log_v0, log_post


def _check_trajectory(r, g, steps, what):
    pos = torch.stack(r['pos_traj']).numpy()
    v = torch.stack(r['v_traj']).numpy()
    same_v = (v == g['v_traj'].astype(np.int64)).all(axis=1)
    dx = np.abs(pos.astype(np.float64) - g['pos_traj'].astype(np.float64)).reshape(steps, -1).max(axis=1)
    first_flip = int(np.argmin(same_v)) if not same_v.all() else None
    print(f'{what}: max |dx| over {steps} steps = {dx.max():.3e} (step {int(dx.argmax())}), last step {dx[-1]:.3e}, '
          f'first type flip: {first_flip}')
    assert first_flip is None, f'{what}: atom types differ from the reference at step {first_flip}'
    assert dx.max() <= TOL_TRAJ, f'{what}: |dx| = {dx.max():.3e} at step {int(dx.argmax())}'
    assert np.array_equal(r['v'].cpu().numpy(), g['v'].astype(np.int64))
    close(r['pos'], g['pos'], TOL_TRAJ)
    for j, s in enumerate(g['kept_steps']):
        close(r['v0_traj'][int(s)], g['v0_traj'][j], TOL_LOGP, (what, 'v0', int(s)))
        # log-posteriors of impossible classes sit near log(1e-30): compare in probability space there
        a, b = r['vt_traj'][int(s)].double().numpy(), g['vt_traj'][j].astype(np.float64)
        live = b > -20.0
        assert np.max(np.abs(a[live] - b[live])) <= TOL_LOGP, (what, 'vt', int(s))
        assert np.max(np.abs(np.exp(a) - np.exp(b))) <= 1e-6, (what, 'vt prob', int(s))


# ------------------------------------------------------------------------------------------ BASELINE config 1 in full
def test_c1_full_100_steps_vs_reference(model):
    """1h36 x 4 samples, num_steps = 100 (t = 999 .. 900): the reference's own run with the counter draws."""
    from targetdiff_amd import workloads
    dev = _dev()
    g = load_golden('c1_full.npz')
    pocket, _ = pocket_1h36()
    batch = workloads.pack_samples(pocket, 4, g['sizes'])
    r = _free_run(model, batch, torch.from_numpy(g['init_ligand_pos']), torch.from_numpy(g['init_ligand_v'].astype(np.int64)),
                  100, int(g['draws_base']), dev)
    _check_trajectory(r, g, 100, 'C1 (session)')
    r2 = _free_run(model, batch, torch.from_numpy(g['init_ligand_pos']), torch.from_numpy(g['init_ligand_v'].astype(np.int64)),
                   100, int(g['draws_base']), dev, use_session=False)
    _check_trajectory(r2, g, 100, 'C1 (stateless)')


def test_c1_teacher_forced_steps_vs_reference(model):
    """Single steps started from the reference's recorded state, so that a (legitimate) neighbour or type flip earlier in a
    free-running trajectory could not mask a defect: 12 steps spread over t = 998 .. 900."""
    from targetdiff_amd import workloads
    dev = _dev()
    g = load_golden('c1_full.npz')
    pocket, _ = pocket_1h36()
    batch = workloads.pack_samples(pocket, 4, g['sizes'])
    worst = 0.0
    for s in (1, 2, 10, 20, 30, 40, 50, 60, 70, 80, 90, 99):
        pos, v, _, _ = _one_step(model, batch, torch.from_numpy(g['pos_traj'][s - 1]),
                                 torch.from_numpy(g['v_traj'][s - 1].astype(np.int64)), 999 - s, s, int(g['draws_base']), dev)
        assert np.array_equal(v.cpu().numpy(), g['v_traj'][s].astype(np.int64)), f'types differ at step {s}'
        worst = max(worst, close(pos, g['pos_traj'][s], TOL_STEP, f'step {s}'))
    print(f'C1 teacher-forced: max |dx| = {worst:.3e}')
    assert worst <= TOL_STEP, worst


# ------------------------------------------------------------------------------------------ a complete 1000-step run
def _small_batch():
    from oracle.make_golden import small_batch
    return small_batch()[0]


def test_1000_step_trajectory_vs_reference(model):
    """The whole reverse process on the 147-node batch: 1000 steps of the reference's own loop, t = 999 .. 0."""
    dev = _dev()
    g = load_golden('sample_small_1000.npz')
    batch = _small_batch()
    init = torch.from_numpy(g['init_ligand_pos']), torch.from_numpy(g['init_ligand_v'].astype(np.int64))
    r = _free_run(model, batch, *init, 1000, int(g['draws_base']), dev)
    _check_trajectory(r, g, 1000, '1000 steps (session)')
    r2 = _free_run(model, batch, *init, 1000, int(g['draws_base']), dev, use_session=False)
    _check_trajectory(r2, g, 1000, '1000 steps (stateless)')
    # the two HIP paths agree with each other bit for bit over the whole run
    assert torch.equal(torch.stack(r['pos_traj']), torch.stack(r2['pos_traj']))
    assert torch.equal(torch.stack(r['v_traj']), torch.stack(r2['v_traj']))


def test_late_steps_teacher_forced_vs_reference(model):
    """t < 10: c0[t] -> 1, the model output is no longer damped by the posterior; and the noiseless t = 0 step."""
    dev = _dev()
    g = load_golden('sample_small_1000.npz')
    batch = _small_batch()
    kept = {int(s): j for j, s in enumerate(g['kept_steps'])}
    worst = 0.0
    for s in (500, 900, 980, 990, 991, 992, 993, 994, 995, 996, 997, 998, 999):
        pos, v, log_v0, log_post = _one_step(model, batch, torch.from_numpy(g['pos_traj'][s - 1]),
                                             torch.from_numpy(g['v_traj'][s - 1].astype(np.int64)), 999 - s, s,
                                             int(g['draws_base']), dev)
        assert np.array_equal(v.cpu().numpy(), g['v_traj'][s].astype(np.int64)), f'types differ at step {s} (t = {999 - s})'
        worst = max(worst, close(pos, g['pos_traj'][s], TOL_STEP, f'step {s}'))
        if s in kept:
            close(log_v0, g['v0_traj'][kept[s]], TOL_LOGP)
    print(f'late steps teacher-forced: max |dx| = {worst:.3e}')
    assert worst <= TOL_STEP, worst


# ------------------------------------------------------------------------------------------ 1000 steps on the real pocket
def test_real_pocket_1000_steps_vs_reference(model):
    """The REAL reference's complete 1000-step run on 1h36 x 2 (prior sizes) with the counter draws: late-t geometry on a real
    pocket meets the session caching (oracle/make_golden_r3.py).  Free-running through the session and the stateless forward."""
    from targetdiff_amd import workloads
    dev = _dev()
    g = _golden_or_skip('sample_1h36x2_1000.npz')
    pocket, _ = pocket_1h36()
    batch = workloads.pack_samples(pocket, 2, g['sizes'])
    init = torch.from_numpy(g['init_ligand_pos']), torch.from_numpy(g['init_ligand_v'].astype(np.int64))
    r = _free_run(model, batch, *init, 1000, int(g['draws_base']), dev)
    # all 70,000 sampled atom types equal and |dx| <= 5e-5 A over the whole run (measured 2.7e-5 at the last step; the CPU
    # restatement's own free run ends 1.9e-5 from the reference).  This needs the protein centroid bit-identical to the
    # reference's CPU path (center_kernel sums in index order): with a tree-reduced centroid the centred coordinates differ in
    # the last bit, one near-tie of the k-NN search at step 424 falls the other way (a 2.5e-4 A jump for one atom) and the run
    # ends 5.5e-3 A away -- the k-NN graph is discontinuous in the coordinates, so nothing larger than rounding may enter them.
    _check_trajectory(r, g, 1000, '1h36 x 2, 1000 steps (session)')
    r2 = _free_run(model, batch, *init, 1000, int(g['draws_base']), dev, use_session=False)
    assert torch.equal(torch.stack(r['pos_traj']), torch.stack(r2['pos_traj']))
    assert torch.equal(torch.stack(r['v_traj']), torch.stack(r2['v_traj']))


def test_real_pocket_teacher_forced_steps_vs_reference(model):
    """Every 50th step and the last 12 (t = 11 .. 0) of that run, each started from the reference's own recorded state.
    (The recorded states are de-centred fp32 positions: re-centring them perturbs the coordinates by up to an ulp of the 30 A
    offset, 3.8e-6 A, which is why single steps are compared at 2e-5 and not at the free run's internal precision; of all
    999 steps exactly one -- step 424, not in the kept set -- sits on a k-NN near-tie that this perturbation flips.)"""
    from targetdiff_amd import workloads
    dev = _dev()
    g = _golden_or_skip('sample_1h36x2_1000.npz')
    pocket, _ = pocket_1h36()
    batch = workloads.pack_samples(pocket, 2, g['sizes'])
    worst = 0.0
    for j, s in enumerate(int(s) for s in g['kept_steps']):
        pos, v, log_v0, log_post = _one_step(model, batch, torch.from_numpy(g['pos_traj'][s - 1]),
                                             torch.from_numpy(g['v_traj'][s - 1].astype(np.int64)), 999 - s, s,
                                             int(g['draws_base']), dev)
        assert np.array_equal(v.cpu().numpy(), g['v_traj'][s].astype(np.int64)), f'types differ at step {s} (t = {999 - s})'
        worst = max(worst, close(pos, g['pos_traj'][s], TOL_STEP, f'step {s}'))
        close(log_v0, g['v0_traj'][j], TOL_LOGP)
    print(f'1h36 x 2 teacher-forced ({len(g["kept_steps"])} steps): max |dx| = {worst:.3e}')
    assert worst <= TOL_STEP, worst


# ------------------------------------------------------------------------------------------ C5 shape
def test_forward_c5_shape_vs_reference_golden(model):
    """1000-atom pocket x 2 with ligands of 150 and 30 atoms: graphs of 1150 / 1030 nodes (multi-pass k-NN search) and
    more than 128 ligand atoms in one graph (the session's extra merge passes), through both entry points."""
    from oracle.make_golden_r2 import C5_POCKET, C5_SIZES
    from targetdiff_amd import capi, workloads
    dev = _dev()
    g = load_golden('forward_c5.npz')
    pocket = workloads.synthetic_pocket(**C5_POCKET)
    b = workloads.pack_samples(pocket, 2, C5_SIZES).to(dev)
    nat = model._native(dev)
    ppos = torch.from_numpy(g['protein_pos_centred']).to(dev)
    lpos = torch.from_numpy(g['ligand_pos']).to(dev)
    lv = torch.from_numpy(g['ligand_v'].astype(np.int64)).to(dev)
    pptr, lptr = nat.graph_ptr(b.protein_element_batch, 2), nat.graph_ptr(b.ligand_element_batch, 2)
    pv = b.protein_atom_feature.float()
    preds = nat.model_forward(ppos, pv, pptr, lpos, lv, lptr, max_graph_nodes=1150)
    close(preds['pred_ligand_pos'], g['pred_ligand_pos'], TOL_FWD)
    close(preds['pred_ligand_v'], g['pred_ligand_v'], TOL_FWD)
    close(preds['final_ligand_h'], g['final_ligand_h'], TOL_FWD)
    close(preds['final_h'][::16], g['final_h_sample'], TOL_FWD)
    # neighbour table on the composed coordinates (protein rows first inside each graph)
    x = torch.cat([ppos[:1000], lpos[:150], ppos[1000:], lpos[150:]])
    node_ptr = torch.tensor([0, 1150, 2180], dtype=torch.int32, device=dev)
    nbr = nat.knn(x.contiguous(), node_ptr, max_graph_nodes=1150).cpu().numpy()
    assert np.array_equal(nbr, g['nbr'].astype(np.int32))
    # unknown size hint (0) and the session take other kernel instantiations; all agree
    preds0 = nat.model_forward(ppos, pv, pptr, lpos, lv, lptr, max_graph_nodes=0)
    assert torch.equal(preds0['pred_ligand_pos'], preds['pred_ligand_pos'])
    sess = capi.NativeSession(nat, ppos, pv, pptr, lptr, lpos.shape[0], 1150)
    ps = sess.forward(lpos, lv)
    assert torch.equal(ps['pred_ligand_pos'], preds['pred_ligand_pos'])
    assert torch.equal(ps['pred_ligand_v'], preds['pred_ligand_v'])
    assert torch.equal(ps['final_ligand_h'], preds['final_ligand_h'])


# ------------------------------------------------------------------------------------------ session == stateless, long
def test_session_equals_stateless_300_steps(model):
    """1h36 x 12 samples, 300 steps with injected draws: the static-protein session (merged k-NN, cached gate / layer-0
    rows, receptive-field pruning) and the stateless forward produce the same bits at every step."""
    from oracle import draws
    from targetdiff_amd import workloads
    dev = _dev()
    pocket, sizes = pocket_1h36()
    batch = workloads.pack_samples(pocket, 12, sizes[:12])
    g = torch.Generator().manual_seed(3)
    lpos, lv = workloads.init_ligand(batch, generator=g)
    out = []
    for use_session in (True, False):
        r = _free_run(model, batch, lpos, lv, 300, 4100, dev, use_session=use_session)
        out.append(r)
    for key in ('pos_traj', 'v_traj', 'v0_traj', 'vt_traj'):
        assert torch.equal(torch.stack(out[0][key]), torch.stack(out[1][key])), key
    spread = float(out[0]['pos'].std(dim=0).mean())
    print(f'session == stateless over 300 steps; final ligand cloud std {spread:.2f} A')


# ------------------------------------------------------------------------------------------ the driver, value by value
def _unpack(g, prefix, axis):
    cat, n = g[prefix + '_cat'], g[prefix + '_n']
    cuts = np.cumsum(n)[:-1]
    return np.split(cat, cuts, axis=axis)


def test_driver_values_vs_reference(model):
    """scripts/sample_diffusion.py:31-116 run by the reference itself (5 samples in batches of 2, 4 steps, prior sizes)
    against targetdiff_amd.sampling.sample_diffusion_ligand under the same draws: every element of the 7-tuple."""
    from oracle import draws
    from oracle.make_golden_r2 import DRIVER_POCKET
    from targetdiff_amd import sampling, workloads
    dev = _dev()
    g = load_golden('driver_small.npz')
    steps = int(g['steps'])
    pocket = workloads.synthetic_pocket(**DRIVER_POCKET)
    src = draws.Source(3100, dev)
    # the reference's n-th randn_like / rand_like call: per sample batch one initial draw, then one per step
    noise_source = lambda bi, st, name, like: src(bi * (steps + 1) + st + 1, name, like)
    res = sampling.sample_diffusion_ligand(model, pocket, 5, batch_size=2, device=dev, num_steps=steps,
                                           center_pos_mode='protein', ligand_num_atoms=[int(v) for v in g['pos_n']],
                                           noise_source=noise_source)
    pos, v, pos_traj, v_traj, v0_traj, vt_traj, times = res
    assert len(times) == 3 and len(pos) == 5
    for k, (a, b) in enumerate(zip(pos, _unpack(g, 'pos', 0))):
        assert a.dtype == np.float64 and a.shape == b.shape
        assert np.max(np.abs(a - b)) <= TOL_TRAJ, ('pos', k)
    for a, b in zip(v, _unpack(g, 'v', 0)):
        assert np.array_equal(a, b.astype(np.int64))
    for a, b in zip(pos_traj, _unpack(g, 'pos_traj', 1)):
        assert a.dtype == np.float64 and a.shape == b.shape and np.max(np.abs(a - b)) <= TOL_TRAJ
    for a, b in zip(v_traj, _unpack(g, 'v_traj', 1)):
        assert np.array_equal(a, b.astype(np.int64))
    for a, b in zip(v0_traj, _unpack(g, 'v0_traj', 1)):
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= TOL_LOGP
    for a, b in zip(vt_traj, _unpack(g, 'vt_traj', 1)):
        assert np.max(np.abs(np.exp(a.astype(np.float64)) - np.exp(b.astype(np.float64)))) <= 1e-6


def test_driver_pos_only_vs_reference(model):
    """pos_only=True / sample_num_atoms='ref' (:54-56, :66-67, :108-112): types frozen, v0 / vt lists stay empty."""
    from oracle import draws
    from oracle.make_golden_r2 import driver_data
    from targetdiff_amd import sampling
    dev = _dev()
    g = load_golden('driver_small.npz')
    d = driver_data(ref_ligand_atoms=9)
    data = types.SimpleNamespace(protein_pos=d.protein_pos, protein_atom_feature=d.protein_atom_feature,
                                 ligand_element=d.ligand_element, ligand_atom_feature_full=d.ligand_atom_feature_full)
    src = draws.Source(3200, dev)
    calls = {'uniform': 0}

    def noise_source(bi, st, name, like):
        if name == 'uniform':           # the reference draws no uniforms on this branch: neither may we consume any
            calls['uniform'] += 1
        return src(bi * 4 + st + 1, name, like)
    res = sampling.sample_diffusion_ligand(model, data, 3, batch_size=2, device=dev, num_steps=3, pos_only=True,
                                           center_pos_mode='protein', sample_num_atoms='ref', noise_source=noise_source)
    pos, v, pos_traj, v_traj, v0_traj, vt_traj, _ = res
    assert v0_traj == [] and vt_traj == []
    for a, b in zip(pos, _unpack(g, 'po_pos', 0)):
        assert np.max(np.abs(a - b)) <= TOL_TRAJ
    for a, b in zip(v, _unpack(g, 'po_v', 0)):
        assert np.array_equal(a, b.astype(np.int64))
    for a, b in zip(pos_traj, _unpack(g, 'po_pos_traj', 1)):
        assert np.max(np.abs(a - b)) <= TOL_TRAJ
    for a, b in zip(v_traj, _unpack(g, 'po_v_traj', 1)):
        assert np.array_equal(a, b.astype(np.int64))


# ------------------------------------------------------------------------------------------ API behaviour
def test_center_pos_mode_none_raises_like_the_reference(model):
    dev = _dev()
    batch = _small_batch().to(dev)
    lpos = torch.zeros(22, 3, device=dev)
    lv = torch.zeros(22, dtype=torch.long, device=dev)
    with pytest.raises(NotImplementedError):
        model.sample_diffusion(batch.protein_pos, batch.protein_atom_feature.float(), batch.protein_element_batch, lpos, lv,
                               batch.ligand_element_batch, num_steps=1)


def test_unsorted_batch_vectors_follow_compose_context(model, state_dict):
    """compose_context stable-sorts the nodes by graph id (models/common.py:126): unsorted batch vectors are legal, and the
    ligand outputs come back in THAT order (not the input order).  Forward: equal to the forward on the pre-sorted inputs bit
    for bit, and to the oracle restatement on the unsorted inputs within the forward tolerance (the restatement is held to the
    real reference on unsorted inputs by tests/test_oracle_vs_reference.py).  Out-of-range atom types still raise."""
    from oracle import restatement as R
    from oracle import weights
    dev = _dev()
    batch = _small_batch()
    g = torch.Generator().manual_seed(9)
    Np, Nl = batch.protein_pos.shape[0], 22
    lpos = batch.protein_pos.mean(0) + torch.randn(Nl, 3, generator=g)
    lv = torch.randint(0, 13, (Nl,), generator=g)
    bl = batch.ligand_element_batch
    pp, pl = torch.randperm(Np, generator=g), torch.randperm(Nl, generator=g)
    u = [batch.protein_pos[pp], batch.protein_atom_feature.float()[pp], batch.protein_element_batch[pp], lpos[pl], lv[pl], bl[pl]]
    assert bool((u[2][1:] < u[2][:-1]).any()) and bool((u[5][1:] < u[5][:-1]).any())
    got = model(*[t.to(dev) for t in u])
    sp, sl = torch.sort(u[2], stable=True).indices, torch.sort(u[5], stable=True).indices
    pre = model(u[0][sp].to(dev), u[1][sp].to(dev), u[2][sp].to(dev), u[3][sl].to(dev), u[4][sl].to(dev), u[5][sl].to(dev))
    for k in ('pred_ligand_pos', 'pred_ligand_v', 'final_ligand_h', 'final_h'):
        assert torch.equal(got[k], pre[k]), k
    want = R.model_forward(state_dict, None, *u)
    close(got['pred_ligand_pos'], want['pred_ligand_pos'], 2e-5)
    close(got['pred_ligand_v'], want['pred_ligand_v'], 2e-4)
    with pytest.raises(ValueError, match='ligand_v'):
        model(*[t.to(dev) for t in u[:4]], (u[4] + 13).to(dev), u[5].to(dev))


def test_sampling_with_unsorted_batch_vectors_follows_the_reference_loop(model, state_dict):
    """The reference's loop with an unsorted ligand vector keeps its state in input order while each forward answers in
    compose_context's order (models/molopt_score_model.py:644-685): reproduced as it is -- 3 steps against the oracle's loop
    (restatement forward + posterior on the same draws), protein unsorted as well."""
    from oracle import draws
    from oracle import restatement as R
    dev = _dev()
    batch = _small_batch()
    g = torch.Generator().manual_seed(10)
    Np, Nl = batch.protein_pos.shape[0], 22
    lpos = batch.protein_pos.mean(0) + torch.randn(Nl, 3, generator=g)
    lv = torch.randint(0, 13, (Nl,), generator=g)
    pp, pl = torch.randperm(Np, generator=g), torch.randperm(Nl, generator=g)
    ppos, pv, bp = batch.protein_pos[pp], batch.protein_atom_feature.float()[pp], batch.protein_element_batch[pp]
    lpos, lv, bl = lpos[pl], lv[pl], batch.ligand_element_batch[pl]
    steps = 3
    r = model.sample_diffusion(ppos.to(dev), pv.to(dev), bp.to(dev), lpos.to(dev), lv.to(dev), bl.to(dev), num_steps=steps,
                               center_pos_mode='protein', noise_source=draws.Source(8100, dev))
    # the oracle's version of the same loop (CPU)
    cfg = None
    sched = R.diffusion_schedules(dict(__import__('oracle.weights', fromlist=['x']).DEFAULT_MODEL_CONFIG))
    src = draws.Source(8100, torch.device('cpu'))
    cp, cl, off = R.center_positions(ppos, lpos, bp, bl)
    x, v = cl.clone(), lv.clone()
    T = 1000
    for s, t in enumerate(reversed(range(T - steps, T))):
        preds = R.model_forward(state_dict, cfg, cp, pv, bp, x, v, bl)            # answers in compose_context's order
        tt = torch.full((int(bp.max()) + 1,), t, dtype=torch.long)
        x, v, l0, lp = R.posterior_step(sched, tt, x, v, preds['pred_ligand_pos'], preds['pred_ligand_v'], bl,
                                        src(s, 'noise', x), src(s, 'uniform', preds['pred_ligand_v']), 13)
        close(r['pos_traj'][s], x + off[bl], 5e-5, s)
        assert torch.equal(r['v_traj'][s], v), s
def test_model_copy_after_first_use(model):
    """copy.deepcopy / pickle after a forward has created the native handle; the copy packs its own weights."""
    import copy
    dev = _dev()
    batch = _small_batch().to(dev)
    g = torch.Generator().manual_seed(1)
    lpos = torch.randn(22, 3, generator=g).to(dev)
    lv = torch.randint(0, 13, (22,), generator=g).to(dev)
    call = lambda m: m(batch.protein_pos, batch.protein_atom_feature.float(), batch.protein_element_batch, lpos, lv,
                       batch.ligand_element_batch)['pred_ligand_pos']
    ref = call(model)
    m2 = copy.deepcopy(model)
    assert m2._native_model is None and m2.refine_net._owner() is m2
    assert torch.equal(call(m2), ref)
    with torch.no_grad():
        m2.v_inference[0].weight.mul_(2.0)            # diverge the copy: the original must not see it
        m2.refine_net.base_block[0].x2h_layers[0].hq_func.net[0].weight.mul_(1.5)
    assert not torch.equal(call(m2), ref)
    assert torch.equal(call(model), ref)


def test_non_current_device_is_honoured(model):
    """--device cuda:1 with the current device left at 0: needs two visible GPUs."""
    if torch.cuda.device_count() < 2:
        pytest.skip('one visible GPU')
    import copy
    dev1 = torch.device('cuda:1')
    torch.cuda.set_device(0)
    m1 = copy.deepcopy(model).to(dev1)
    batch = _small_batch()
    g = torch.Generator().manual_seed(1)
    lpos, lv = torch.randn(22, 3, generator=g), torch.randint(0, 13, (22,), generator=g)
    outs = []
    for m, d in ((model, _dev()), (m1, dev1)):
        b = batch.to(d)
        r = m.sample_diffusion(b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch, lpos.to(d), lv.to(d),
                               b.ligand_element_batch, num_steps=2, center_pos_mode='protein',
                               noise_source=lambda s, n, like: torch.full_like(like, 0.25))
        outs.append(r['pos'].cpu())
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------ C3 at full size
def test_c3_full_size_pack_reproduces_reference_golden(model):
    """BASELINE config 3 at its full size (32 pockets x 100 samples, N = 1.04 M nodes, 3200 graphs): the reference's
    forward on one sample per pocket (graphs are independent) must come out of the full pack at the slots those samples
    occupy -- through the stateless forward and through the session."""
    from oracle.make_golden_r2 import c3_pockets
    from targetdiff_amd import capi, workloads
    dev = _dev()
    g = load_golden('forward_c3.npz')
    pockets = c3_pockets()
    slot = 37                                              # sample index inside each pocket's 100 replicas
    b = workloads.pack_samples(pockets, 100, [25] * 3200)
    gen = torch.Generator().manual_seed(99)
    lpos, lv = workloads.init_ligand(b, generator=gen, spread=2.0)          # un-centred filler for the other 3168 graphs
    idx = torch.cat([torch.arange(25) + (p * 100 + slot) * 25 for p in range(32)])
    lpos[idx] = torch.from_numpy(g['ligand_pos_uncentred'])
    lv[idx] = torch.from_numpy(g['ligand_v'].astype(np.int64))
    b = b.to(dev)
    nat = model._native(dev)
    pptr, lptr = nat.graph_ptr(b.protein_element_batch, 3200), nat.graph_ptr(b.ligand_element_batch, 3200)
    ppos, lposd = b.protein_pos.clone(), lpos.to(dev)
    nat.center_pos(ppos, pptr, lposd, lptr)
    close(lposd[idx.to(dev)], g['ligand_pos'], 1e-5)
    pv, lvd = b.protein_atom_feature.float(), lv.to(dev)
    preds = nat.model_forward(ppos, pv, pptr, lposd, lvd, lptr, max_graph_nodes=325, want_final_h=False)
    sel = idx.to(dev)
    close(preds['pred_ligand_pos'][sel], g['pred_ligand_pos'], TOL_FWD)
    close(preds['pred_ligand_v'][sel], g['pred_ligand_v'], TOL_FWD)
    close(preds['final_ligand_h'][sel], g['final_ligand_h'], TOL_FWD)
    sess = capi.NativeSession(nat, ppos, pv, pptr, lptr, lposd.shape[0], 325)
    ps = sess.forward(lposd, lvd)
    for key in ('pred_ligand_pos', 'pred_ligand_v', 'final_ligand_h'):
        assert torch.equal(ps[key], preds[key]), key


def test_overlapped_batches_equal_sequential_batches(model):
    """overlap_batches=True advances the sample batches of a pocket together, one HIP stream each; with injected draws
    every element of the 7-tuple is the same bits as in the sequential order."""
    from oracle import draws
    from targetdiff_amd import sampling, workloads
    dev = _dev()
    pocket = workloads.synthetic_pocket(77, 150)
    src = draws.Source(6100, dev)
    steps = 12
    noise_source = lambda bi, st, name, like: src(bi * (steps + 1) + st + 1, name, like)
    sizes = [10 + (k % 7) for k in range(22)]
    res = [sampling.sample_diffusion_ligand(model, pocket, 22, batch_size=5, device=dev, num_steps=steps, ligand_num_atoms=sizes,
                                            noise_source=noise_source, overlap_batches=ov) for ov in (False, True)]
    assert len(res[0][6]) == len(res[1][6]) == 5
    for a_list, b_list in zip(res[0][:6], res[1][:6]):
        assert len(a_list) == len(b_list) == 22
        for a, b in zip(a_list, b_list):
            assert a.dtype == b.dtype and np.array_equal(a, b)


def test_bench_through_the_launcher_initialises_rccl(tmp_path):
    """`bench.py` started by targetdiff_amd.launch (the way `--gpus N` starts N ranks) on this box's single GPU: a world of
    one rank still goes through dist.init_process_group('nccl'), the barrier and the max-reduction, and prints one JSON line
    (with `--full`, whose roofline leg runs on the same process group)."""
    import json
    import os
    import subprocess
    import sys
    from targetdiff_amd import launch
    _dev()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = launch.rank_env(0, 1, launch.free_port())
    p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--full',
                        '--no-cpu-baseline', '--no-full-run', '--workload', 'c1'], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith('{')][-1]
    d = json.loads(line)
    assert d['n_gpus'] == 1 and d['value'] > 0 and d['unit'] == 'ligands/s' and d['roofline'] is not None


def test_plain_bench_runs_only_the_headline_and_computes_what_full_computes(tmp_path):
    """A plain `bench.py` line carries the headline and none of the `--full` legs, and its timed steps compute bit for bit what
    those of a `--full` run compute (the roofline leg's steps stay in the sampler's length either way)."""
    import json
    import os
    import subprocess
    import sys
    _dev()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = {}
    for name, extra in (('plain', []), ('full', ['--full', '--no-cpu-baseline'])):
        p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--workload',
                            'c1', '--dump-outputs', str(tmp_path / name)] + extra, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        lines[name] = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
    plain, full = lines['plain'], lines['full']
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in plain
    assert plain['roofline'] is None and full['roofline'] is not None
    assert 'stateless_ms_per_step' not in plain and 'stateless_ms_per_step' in full
    assert not {'cpu_baseline', 'geometry_sweep', 'full_run', 'initial_state'} & set(plain)
    files = sorted(os.listdir(tmp_path / 'plain'))
    assert files and files == sorted(os.listdir(tmp_path / 'full'))
    for f in files:
        assert np.array_equal(np.load(tmp_path / 'plain' / f), np.load(tmp_path / 'full' / f)), f


def test_c4_bench_and_batch_sample_through_the_launcher_with_the_real_model(tmp_path):
    """What a multi-GPU run executes per rank, on this box's one GPU and with the real model: `bench.py --workload c4` (the
    100-pocket test-set job; every pocket's session alive at once) and `tools/batch_sample.py` (result_{i}.pt files, summary,
    size-balanced assignment flag), both started through targetdiff_amd.launch with pinned devices (HIP_VISIBLE_DEVICES = rank,
    the reference's recipe) -- so a SCALE run needs no flag that has not been exercised."""
    import json
    import os
    import subprocess
    import sys
    from targetdiff_amd import launch, results
    _dev()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = launch.rank_env(0, 1, launch.free_port(), pin_devices=True)
    assert env['HIP_VISIBLE_DEVICES'] == '0' and env['LOCAL_RANK'] == '0'
    p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1',
                        '--workload', 'c4'], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
    assert d['n_gpus'] == 1 and d['scaling'] == 'strong' and d['config']['pockets_this_rank'] == 100 and d['value'] > 0
    assert abs(d['load_balance']['max_over_mean'] - 1.0) < 1e-9
    out = tmp_path / 'res'
    env = launch.rank_env(0, 1, launch.free_port(), pin_devices=True)
    p = subprocess.run([sys.executable, os.path.join(root, 'tools', 'batch_sample.py'), '--pockets', 'synthetic:4', '--result_path',
                        str(out), '--num_samples', '6', '--num_steps', '5', '--batch_size', '4', '--ligand_atoms', '20', '--balance'],
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    s = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
    assert s['world_size'] == 1 and s['pockets_sampled'] == 4 and s['ligands'] == 24
    for i in range(4):
        r = torch.load(results.result_file(str(out), i), weights_only=False)
        assert len(r['pred_ligand_pos']) == 6 and r['pred_ligand_pos'][0].shape == (20, 3) and np.isfinite(r['pred_ligand_pos'][0]).all()
        assert r['pred_ligand_pos_traj'][0].shape == (5, 20, 3)


def test_native_options_survive_a_rebuild_of_the_handle(state_dict):
    """switches set through the module are re-applied when load_state_dict / .to() rebuild the native handle."""
    from oracle import weights
    from targetdiff_amd.models import ScorePosNet3D
    dev = _dev()
    m = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG), 27, 13)
    m.load_state_dict(state_dict, strict=False)
    m = m.to(dev).eval()
    m.set_native_option('edge_key_split', 0)
    h1 = m._native(dev)
    assert h1.get_option('edge_key_split') == 0
    m.load_state_dict(state_dict, strict=False)              # new parameter versions -> a new handle
    h2 = m._native(dev)
    assert h2 is not h1 and h2.get_option('edge_key_split') == 0 and h2.get_option('node_proj_split') == 1
