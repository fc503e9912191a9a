"""td_diffusion_loss / td_auroc (csrc/loss.hip), ScorePosNet3D.get_diffusion_loss and targetdiff_amd.validation on an MI355X (``-m gpu``).

Kernel level (planted predictions, no network): every output against the float64 restatement of tests/_loss_ref.py by the rule of
tests/_step_ref.py -- |HIP - float64| <= max(floor, 2 |fp32 restatement - float64|) -- over graphs of 1, 63, 64, 65, 130, 0 and 7 atoms,
the time-step sets 'mixed', 'all0' and 'all999', 13, 16 and 2 classes and both mean types; loss_v_graph bit for bit td_likelihood_terms'
kl_v.  AUROC: the integer counts equal the brute force.  End to end: the recordings of the real reference (tools/make_golden_loss.py), the
network's error and the loss kernel's judged apart.  tests/test_loss_host.py shows on the CPU that the restatement is the reference's
arithmetic and that the gates reject planted defects."""
import numpy as np
import pytest
import torch

import _loss_ref as L
import _step_ref as S
from _tol import TOL_FWD, close
from conftest import load_golden
from oracle import draws, weights

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SCALARS = ('loss', 'loss_pos', 'loss_v')
_HANDLES, _MODELS = {}, {}


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


def _model(name):
    """the mirror of one fixture's configuration on the device, cached for the module"""
    from targetdiff_amd.models import ScorePosNet3D
    if name not in _MODELS:
        cfg = L.LOSS_FIXTURES[name]
        sd = weights.time_emb_state_dict(2021) if cfg.get('time_emb_dim') else weights.make_state_dict(2021)
        m = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG, **cfg), 27, 13)
        m.load_state_dict(sd, strict=False)
        _MODELS[name] = m.to(_dev()).eval()
    return _MODELS[name]


def _kernel_call(case, mean_type, dev):
    i = S.inputs(case)
    nat = _native(case[1], mean_type)
    lptr = nat.graph_ptr(S.BATCH.to(dev), S.B)
    D = lambda k: i[k].to(dev).contiguous()
    out = nat.diffusion_loss(i['t'].int().to(dev), lptr, D('x0'), D('x_t'), D('noise'), D('v0'), D('v_t'), D('pred_pos'), D('pred_v'),
                             L.LOSS_V_WEIGHT)
    return nat, lptr, D, out


@pytest.mark.parametrize('case', L.CASE_IDS, ids=S.case_id)
def test_diffusion_loss_kernel_vs_float64(case):
    dev = _dev()
    i = S.inputs(case)
    empty = S.SIZES.index(0)
    for mean_type in L.MEAN_TYPES:
        nat, lptr, D, out = _kernel_call(case, mean_type, dev)
        got = {k: v.cpu() for k, v in out.items()}
        f32, f64 = L.reference(case, mean_type, F32), L.reference(case, mean_type, F64)
        for row in L.judge(got, f32, f64, case[1], f'{S.case_id(case)} {mean_type}', asserting=True):
            print(f'FIG {S.case_id(case)} {mean_type} {row[0]} d64 {row[2]:.3e} r64 {row[3]:.3e} bound {row[4]:.3e}')
        assert float(got['loss_pos_graph'][empty]) == 0 and float(got['loss_v_graph'][empty]) == 0
        # the type term is td_likelihood_terms', bit for bit
        kl_v = nat.likelihood_terms(i['t'].int().to(dev), lptr, D('x0'), D('x_t'), D('v0'), D('v_t'), D('pred_pos'), D('pred_v'))[1]
        assert torch.equal(out['loss_v_graph'], kl_v)
        # a second call: the same bits
        again = _kernel_call(case, mean_type, dev)[3]
        for k in out:
            assert torch.equal(out[k], again[k]), k
        # loss = loss_pos + w loss_v, product and sum rounded one by one
        assert torch.equal(got['loss'], got['loss_pos'] + got['loss_v'] * torch.tensor(L.LOSS_V_WEIGHT, dtype=F32))
    # 'C0' does not read the draw: NULL is accepted and changes nothing
    nat, lptr, D, b = _kernel_call(case, 'C0', dev)
    a = nat.diffusion_loss(i['t'].int().to(dev), lptr, D('x0'), D('x_t'), None, D('v0'), D('v_t'), D('pred_pos'), D('pred_v'), L.LOSS_V_WEIGHT)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_diffusion_loss_refusals():
    dev = _dev()
    case = ('base', 13)
    i = S.inputs(case)
    nat = _native(13, 'noise')
    lptr = nat.graph_ptr(S.BATCH.to(dev), S.B)
    D = lambda k: i[k].to(dev).contiguous()
    with pytest.raises(RuntimeError, match="needs d_noise"):
        nat.diffusion_loss(i['t'].int().to(dev), lptr, D('x0'), D('x_t'), None, D('v0'), D('v_t'), D('pred_pos'), D('pred_v'), 1.0)
    from targetdiff_amd import capi
    # negative sizes on a live handle, through the C ABI itself (the binding derives the sizes from the tensors)
    some = D('x0').data_ptr()
    raw = lambda Nl, B: nat.lib.td_diffusion_loss(nat.handle, some, some, Nl, B, *([some] * 7), 1.0, *([some] * 5), None)
    assert raw(-1, 7) == -1 and b'bad argument' in nat.lib.td_last_error()
    assert raw(330, -1) == -1 and b'bad argument' in nat.lib.td_last_error()
    # the binding's own checks: a short v_t would be read past its end
    good = nat.graph_ptr(S.BATCH.to(dev), S.B)
    with pytest.raises(ValueError, match='v_0 / v_t'):
        nat.diffusion_loss(i['t'].int().to(dev), good, D('x0'), D('x_t'), D('noise'), D('v0'), D('v_t')[:-1].contiguous(), D('pred_pos'), D('pred_v'), 1.0)
    short = good.clone()
    short[-1] -= 1
    with pytest.raises(ValueError, match='ligand_ptr'):
        nat.diffusion_loss(i['t'].int().to(dev), short, D('x0'), D('x_t'), D('noise'), D('v0'), D('v_t'), D('pred_pos'), D('pred_v'), 1.0)
    sched = {k: v.numpy() for k, v in S.schedules().items() if k in capi.SCHEDULE_ORDER}
    bare = capi.NativeModel(S.native_config(13), S.state_dict(13), sched, device=dev)          # no alphas_cumprod
    with pytest.raises(RuntimeError, match='alphas_cumprod'):
        bare.diffusion_loss(i['t'].int().to(dev), lptr, D('x0'), D('x_t'), D('noise'), D('v0'), D('v_t'), D('pred_pos'), D('pred_v'), 1.0)


@pytest.mark.parametrize('case', L.AUROC_CASES, ids=lambda c: f'N{c[0]}-C{c[1]}-{c[2]}')
def test_auroc_counts_equal_the_brute_force(case):
    from targetdiff_amd import capi
    dev = _dev()
    scores, labels = L.auroc_inputs(case)
    want_n, want_p = L.auroc_counts(scores, labels)
    n_pos, pairs2 = capi.auroc_counts(scores.to(dev), labels.to(dev))
    assert np.array_equal(n_pos.cpu().numpy(), want_n) and np.array_equal(pairs2.cpu().numpy(), want_p)
    n2, p2 = capi.auroc_counts(scores.to(dev), labels.to(dev))
    assert torch.equal(n2, n_pos) and torch.equal(p2, pairs2)
    if int((want_n > 0).sum()) < 2:                                       # one class holds every row
        with pytest.raises(ValueError, match='holds every row'):
            capi.auroc(scores.to(dev), labels.to(dev))
        return
    avg, per = capi.auroc(scores.to(dev), labels.to(dev))
    want_avg, want_per = L.auroc_from_counts(want_n, want_p)
    assert abs(avg - want_avg) <= 1e-15 and per.keys() == want_per.keys()
    if case[2] == 'all_equal':
        assert all(v == 0.5 for v in per.values())
    if case[2] == 'absent':
        assert case[1] - 1 not in per


# ------------------------------------------------------------------------------------------ end to end
def _fixture_call(name, g, dev, transform=None):
    """get_diffusion_loss on a fixture's batch with its recorded draws; `transform` = (R [3,3], shift [3]) moves the complex rigidly and
    turns the Gaussian draw with it"""
    m = _model(name)
    T = lambda k: torch.from_numpy(np.asarray(g[k]))
    ppos, lpos, noise = T('protein_pos').float(), T('ligand_pos').float(), T('noise')
    if transform is not None:
        R, shift = transform
        ppos, lpos, noise = ppos @ R.T + shift, lpos @ R.T + shift, noise @ R.T
    src = lambda s, kind, like: (noise if kind == 'noise' else T('uniform')).to(dev)
    return m.get_diffusion_loss(ppos.to(dev), T('protein_feat').float().to(dev), T('batch_protein').long().to(dev), lpos.to(dev),
                                T('ligand_v').long().to(dev), T('batch_ligand').long().to(dev), time_step=T('time_step').long().to(dev),
                                noise_source=src), noise


def _restate(g, r, noise, mean_type, dtype):
    """the restatement on the GPU's own state: its x0, x_t, v_t and predictions"""
    c = lambda k: r[k].cpu()
    return L.diffusion_loss(S.schedules(), c('time_step').long(), c('x0'), c('ligand_pos_perturbed'), noise, torch.from_numpy(g['ligand_v']).long(),
                            c('ligand_v_perturbed'), c('pred_ligand_pos'), c('pred_ligand_v'), torch.from_numpy(g['batch_ligand']).long(), 13,
                            L.LOSS_V_WEIGHT, dtype, mean_type)


@pytest.mark.parametrize('name', list(L.LOSS_FIXTURES))
def test_get_diffusion_loss_vs_reference_fixture(name):
    dev = _dev()
    g = load_golden(name + '.npz')
    mean_type = L.LOSS_FIXTURES[name].get('model_mean_type', 'C0')
    r, noise = _fixture_call(name, g, dev)
    assert set(r) >= {'loss_pos', 'loss_v', 'loss', 'x0', 'pred_ligand_pos', 'pred_ligand_v', 'pred_pos_noise', 'ligand_v_recon',
                      'loss_pos_graph', 'loss_v_graph', 'time_step'}
    assert all(not v.requires_grad for v in r.values())
    # the perturbed state: the types are the reference's, x_t by the rule of the perturb kernel
    assert torch.equal(r['ligand_v_perturbed'].cpu(), torch.from_numpy(g['v_t']).long())
    close(r['ligand_pos_perturbed'], g['x_t64'], max(S.FLOOR['pos'], S.FACTOR * float(g['r_x_t'])), f'{name} x_t')
    close(r['x0'], g['x064'], max(S.FLOOR['pos'], S.FACTOR * float(g['r_x0'])), f'{name} x0')
    # the network
    close(r['pred_ligand_pos'], g['pred_ligand_pos64'], TOL_FWD, f'{name} pred_ligand_pos')
    close(r['pred_ligand_v'], g['pred_ligand_v64'], TOL_FWD, f'{name} pred_ligand_v')
    # 1. the loss kernel, on the GPU's own predictions
    got = {k: r[k].cpu() for k in L.OUTPUTS}
    f32, f64 = _restate(g, r, noise, mean_type, F32), _restate(g, r, noise, mean_type, F64)
    L.judge(got, f32, f64, 13, f'{name} on own predictions', asserting=True)
    # 2. against the reference's float64 losses: what the predictions' distance moves the float64 loss by, the kernel's gate, and 2 r
    ref64 = L.fixture_loss(g, F64, mean_type=mean_type)
    for k in SCALARS:
        want = float(g[k + '64'])
        assert abs(float(ref64[k]) - want) <= 1e-12 * max(abs(want), 1e-2)
        bound = abs(float(f64[k]) - float(ref64[k])) + L.kernel_gate(f32, f64, k, 13) + S.FACTOR * float(g['r_' + k])
        d = close(r[k], want, bound, f'{name} {k} vs reference')
        print(f'FIG {name} {k} d {d:.3e} bound {bound:.3e} share {d / bound:.3f}')


def test_rigid_motion_leaves_the_losses_alone():
    """center_pos_mode 'protein': a rotated and translated complex (the Gaussian draw turned with it) gives the same losses within the
    kernel gate: the gate of the first call's restatement plus that of the second's, nothing for the network"""
    dev = _dev()
    g = load_golden('loss_c0.npz')
    R = torch.tensor([[np.cos(0.7), -np.sin(0.7), 0.0], [np.sin(0.7), np.cos(0.7), 0.0], [0.0, 0.0, 1.0]], dtype=F64)
    Rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, np.cos(1.1), -np.sin(1.1)], [0.0, np.sin(1.1), np.cos(1.1)]], dtype=F64)
    R = (R @ Rx).float()
    a, na = _fixture_call('loss_c0', g, dev)
    b, nb = _fixture_call('loss_c0', g, dev, transform=(R, torch.tensor([3.0, -2.0, 5.0])))
    assert not torch.allclose(a['x0'], b['x0'], atol=0.1)                 # the complex did turn
    assert torch.equal(a['ligand_v_perturbed'], b['ligand_v_perturbed'])
    fa32, fa64 = _restate(g, a, na, 'C0', F32), _restate(g, a, na, 'C0', F64)
    fb32, fb64 = _restate(g, b, nb, 'C0', F32), _restate(g, b, nb, 'C0', F64)
    for k in SCALARS:
        bound = L.kernel_gate(fa32, fa64, k, 13) + L.kernel_gate(fb32, fb64, k, 13)
        d = close(a[k], b[k], bound, f'rigid motion {k}')
        print(f'FIG rigid {k} d {d:.3e} bound {bound:.3e}')


def test_no_gradient_even_when_parameters_require_grad():
    dev = _dev()
    g = load_golden('loss_c0.npz')
    m = _model('loss_c0')
    assert any(p.requires_grad for p in m.parameters())
    with torch.enable_grad():
        r, _ = _fixture_call('loss_c0', g, dev)
    assert all(not v.requires_grad and v.grad_fn is None for v in r.values())
    with pytest.raises(RuntimeError):
        r['loss'].backward()


# ------------------------------------------------------------------------------------------ validation
def _validate_inputs(g, dev):
    T = lambda k: torch.from_numpy(np.asarray(g[k]))
    batches = []
    for i in range(2):
        p = f'b{i}_'
        batches.append({'protein_pos': T(p + 'protein_pos').float().to(dev), 'protein_atom_feature': T(p + 'protein_feat').float().to(dev),
                        'protein_element_batch': T(p + 'batch_protein').long().to(dev), 'ligand_pos': T(p + 'ligand_pos').float().to(dev),
                        'ligand_atom_feature_full': T(p + 'ligand_v').long().to(dev), 'ligand_element_batch': T(p + 'batch_ligand').long().to(dev)})
    sizes = [int(b['ligand_pos'].shape[0]) for b in batches]
    assert sizes[0] != sizes[1]
    base = int(g['draws_base'])

    def source(l, name, like):        # batch i, level l: the streams tools/make_golden_loss.py drew from (the batches differ in size)
        i = sizes.index(int(like.shape[0]))
        d = draws.normal(base + 10 * i, l, tuple(like.shape)) if name == 'noise' else draws.uniform(base + 10 * i + 1, l, tuple(like.shape))
        return d.to(dev)
    return batches, source


def test_validate_small_vs_reference_fixture():
    """validate(fused=True) and validate(fused=False) against the recorded loop of the reference script.  The bound of a loss: what the GPU's
    predictions move the float64 loss by (the float64 restatement on the GPU's own state of every batch and level, summed as validate sums,
    against the recorded float64 value), the kernel gate averaged the same way, and 2 r.  The AUROC in two parts as well, for both forms.
    Counting: `atom_auroc` equals the brute-force AUROC of the very rows that form produced (validation._level_losses), to 1e-12.  Network:
    against the reference's fp32 run -- within 1e-9 when the GPU's rows order every (positive, negative) pair as the recorded fp32 rows do
    (equal pairs2 of every class); otherwise within what the pairs whose recorded fp32 scores differ by less than TOL_FWD, the forward
    gate, can move it by: a flipped pair moves class c's AUROC by at most 1 / (n_pos n_neg)."""
    from targetdiff_amd import validation
    dev = _dev()
    g = load_golden('validate_small.npz')
    m = _model('loss_c0')
    batches, source = _validate_inputs(g, dev)
    levels = g['levels'].tolist()
    # the restatement on the GPU's own state, level by level, summed as validate() sums
    sums = {k: 0.0 for k in SCALARS}
    gates = {k: 0.0 for k in SCALARS}
    n = 0
    recon, v_t = [], []
    for i, b in enumerate(batches):
        B = int(b['protein_element_batch'].max()) + 1
        for l, t in enumerate(levels):
            noise = source(l, 'noise', b['ligand_pos'])
            r = m.get_diffusion_loss(b['protein_pos'], b['protein_atom_feature'], b['protein_element_batch'], b['ligand_pos'],
                                     b['ligand_atom_feature_full'], b['ligand_element_batch'], time_step=torch.tensor([t] * B, device=dev),
                                     noise_source=lambda s, name, like, l=l, b=b: source(l, name, like if like is not None else b['ligand_pos'].new_empty(b['ligand_pos'].shape[0], 13)))
            gg = {'ligand_v': b['ligand_atom_feature_full'].cpu().numpy(), 'batch_ligand': b['ligand_element_batch'].cpu().numpy()}
            f32, f64 = _restate(gg, r, noise.cpu(), 'C0', F32), _restate(gg, r, noise.cpu(), 'C0', F64)
            for k in SCALARS:
                sums[k] += float(f64[k]) * B
                gates[k] += L.kernel_gate(f32, f64, k, 13) * B
            n += B
            recon.append(r['ligand_v_recon'].cpu())
            v_t.append(r['ligand_v_perturbed'].cpu())
    assert np.array_equal(torch.cat(v_t).numpy(), g['v_t'].astype(np.int64))
    recon = torch.cat(recon).numpy()
    y = g['labels'].astype(np.int64)
    # pairs that may flip: closer than the forward gate in the recorded fp32 scores
    s32 = g['ligand_v_recon']
    assert s32.dtype == np.float32
    N = len(y)
    flip = 0.0
    for c in sorted(set(y.tolist())):
        pos, neg = s32[y == c, c].astype(np.float64), s32[y != c, c].astype(np.float64)
        near = int((np.abs(pos[:, None] - neg[None, :]) < TOL_FWD).sum())
        flip += near / (N * len(neg))                                     # (n_pos / N) * near / (n_pos n_neg)
    want_pairs = L.auroc_counts(s32, y)[1]
    want_auroc = float(g['atom_auroc'])
    assert abs(L.auroc_from_counts(*L.auroc_counts(s32, y))[0] - want_auroc) <= 1e-12
    print(f'FIG validate auroc: pairs closer than TOL_FWD in the fp32 record move it by at most {flip:.3e}')
    for fused in (True, False):
        rep = validation.validate(m, batches, num_levels=10, fused=fused, noise_source=source)
        assert rep['per_level']['levels'] == levels and len(rep['per_level']['loss']) == 10
        for k in SCALARS:
            want = float(g[k + '64'])
            bound = abs(sums[k] / n - want) + gates[k] / n + S.FACTOR * float(g['r_' + k])
            d = close(rep[k], want, bound, f'validate fused={fused} {k}')
            print(f'FIG validate fused={fused} {k} d {d:.3e} bound {bound:.3e} share {d / bound:.3f}')
            lv = np.asarray(rep['per_level'][k])
            assert abs(float(lv.mean()) - rep[k]) <= 1e-9 * max(abs(rep[k]), 1.0)
        # the rows this form scored (the same calls, the same draws: the same bits), and their AUROC by brute force
        rows = torch.cat([validation._level_losses(m, b, validation.levels_of(1000, 10), fused, source)[2] for b in batches]).cpu().numpy()
        assert rows.shape == s32.shape
        if not fused:
            assert np.array_equal(rows, recon)
        counts = L.auroc_counts(rows, y)
        brute, brute_per = L.auroc_from_counts(*counts)
        assert abs(rep['atom_auroc'] - brute) <= 1e-12
        assert max(abs(rep['per_class_auroc'][c] - brute_per[c]) for c in brute_per) <= 1e-12
        assert sorted(rep['per_class_auroc']) == g['classes'].tolist()
        same_order = np.array_equal(counts[1], want_pairs)
        d = abs(rep['atom_auroc'] - want_auroc)
        print(f'FIG validate fused={fused} atom_auroc {rep["atom_auroc"]:.9f} fp32 record {want_auroc:.9f} d {d:.3e} same order {same_order}; '
              f'float64 record {float(g["atom_auroc64"]):.9f}')
        assert d <= (1e-9 if same_order else flip), (d, same_order, flip)
    line = validation.format_line(7, rep)
    assert line.startswith('[Validate] Iter 00007 | Loss ')
