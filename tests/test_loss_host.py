"""CPU-only checks of the diffusion loss and the validation loop: the restatement of tests/_loss_ref.py reproduces the recordings of the real
reference (tests/golden/loss_*.npz, validate_small.npz; tools/make_golden_loss.py) within each fixture's own fp32-to-float64 distance, the
gates reject every planted defect, the brute-force AUROC is sklearn's, and the host side of the new surface (header, exports, binding,
sample_time, format_line, refusals that need no GPU)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _loss_ref as L
import _step_ref as S
from conftest import ROOT, load_golden
from oracle import draws, weights
from targetdiff_amd import capi, validation
from targetdiff_amd.models import ScorePosNet3D

F32, F64 = torch.float32, torch.float64
SCALARS = ('loss', 'loss_pos', 'loss_v')


def _mean_type(name):
    return L.LOSS_FIXTURES[name].get('model_mean_type', 'C0')


@pytest.mark.parametrize('name', list(L.LOSS_FIXTURES))
def test_restatement_reproduces_the_reference_fixtures(name):
    """float64 restatement on the float64 run's state = the float64 run (1e-12 relative); fp32 restatement on the fp32 run's state within
    2 r + the floor of the float64 run, r the fixture's own fp32-to-float64 distance of that output"""
    g = load_golden(name + '.npz')
    assert sorted(g['time_step'].tolist()) == [0, 537, 999]               # both ends of the schedule and the decoder branch
    assert np.array_equal(g['noise'], draws.normal(int(g['draws_base']), 0, g['noise'].shape).numpy())
    assert np.array_equal(g['uniform'], draws.uniform(int(g['draws_base']) + 1, 0, g['uniform'].shape).numpy())
    r64 = L.fixture_loss(g, F64, mean_type=_mean_type(name))
    r32 = L.fixture_loss(g, F32, mean_type=_mean_type(name))
    for k in SCALARS + ('pred_pos_noise', 'ligand_v_recon'):
        want = torch.from_numpy(np.asarray(g[k + '64']))
        scale = max(float(want.abs().max()), 1e-2)
        assert float((r64[k] - want).abs().max()) <= 1e-12 * scale, (name, k)
        bound = S.FACTOR * float(g['r_' + k]) + S.FLOOR['kl'] * scale
        d = float((r32[k].double() - want).abs().max())
        print(f'{name} {k}: |fp32 restatement - float64 reference| {d:.3e}, bound {bound:.3e}')
        assert d <= bound, (name, k, d, bound)
    assert float(r64['loss']) == pytest.approx(float(r64['loss_pos']) + L.LOSS_V_WEIGHT * float(r64['loss_v']), rel=1e-14)


@pytest.mark.parametrize('defect', L.DEFECTS)
def test_every_planted_loss_defect_fails_the_gate(defect):
    """a wrong kernel, played by the fp32 restatement with one wrong line, is rejected on a kernel-level case of both mean types, and on a
    fixture of the reference.  The ignored decoder mask is shown on the fixture's state with planted perturbed types: at t == 0 the draw
    leaves v_t = v0, the true posterior is then the one-hot of v0 up to 1e-30 and the KL against it IS the decoder NLL, whatever the
    logits -- the defect cannot be seen on such a state by any gate; with v_t != v0 on the t == 0 graph (as the kernel-level cases
    have it) the true posterior is no one-hot and the two terms part"""
    seen = 0
    for mean_type in L.MEAN_TYPES:
        case = ('base', 13)
        f32, f64 = L.reference(case, mean_type, F32), L.reference(case, mean_type, F64)
        assert all(row[1] for row in L.judge(f32, f32, f64, 13)), 'the rule must pass the fp32 restatement itself'
        bad = L.reference(case, mean_type, F32, defect)
        seen += any(not row[1] for row in L.judge(bad, f32, f64, 13))
    assert seen == len(L.MEAN_TYPES), defect
    g = load_golden('loss_c0.npz')
    kw, want = {}, {k: float(g[k + '64']) for k in SCALARS}
    if defect == 'decoder_mask_ignored':
        v0, tb = torch.from_numpy(g['ligand_v']).long(), torch.from_numpy(g['time_step']).long()[torch.from_numpy(g['batch_ligand']).long()]
        assert torch.equal(torch.from_numpy(g['v_t']).long()[tb == 0], v0[tb == 0])
        kw = dict(v_t=torch.where(tb == 0, (v0 + 1) % 13, torch.from_numpy(g['v_t']).long()))
        want = {k: float(v) for k, v in L.fixture_loss(g, F64, **kw).items() if k in SCALARS}
        ok = L.fixture_loss(g, F32, **kw)                  # the gate passes the right arithmetic on this state
        assert all(abs(float(ok[k]) - want[k]) <= S.FACTOR * float(g['r_' + k]) + S.FLOOR['kl'] * max(abs(want[k]), 1e-2) for k in SCALARS)
    bad = L.fixture_loss(g, F32, defect=defect, **kw)
    moved = False
    for k in SCALARS:
        moved |= abs(float(bad[k]) - want[k]) > S.FACTOR * float(g['r_' + k]) + S.FLOOR['kl'] * max(abs(want[k]), 1e-2)
    assert moved, defect


def test_kernel_cases_cover_what_they_claim():
    assert S.SIZES == [1, 63, 64, 65, 130, 0, 7] and S.CLASSES == (13, 16, 2)
    tsets = {S.CASES[name][0] for name, _ in L.CASE_IDS}
    assert tsets == {'mixed', 'all0', 'all999'}
    f64 = L.reference(('base', 13), 'C0', F64)
    empty = S.SIZES.index(0)
    assert float(f64['loss_pos_graph'][empty]) == 0 and float(f64['loss_v_graph'][empty]) == 0         # an empty graph: 0 / 1
    kp, kv = S.likelihood_terms(S.schedules(), S.inputs(('base', 13))['t'], *(S.inputs(('base', 13))[k] for k in ('x0', 'x_t', 'v0', 'v_t', 'pred_pos', 'pred_v')),
                                S.BATCH, 13, F64)
    assert torch.equal(kv, f64['loss_v_graph'])                           # the type term is _step_ref's likelihood term
    a, b = L.reference(('base', 13), 'C0', F64), L.reference(('base', 13), 'noise', F64)
    assert not torch.allclose(a['loss_pos_graph'], b['loss_pos_graph']) and torch.equal(a['loss_v_graph'], b['loss_v_graph'])


@pytest.mark.parametrize('case', L.AUROC_CASES, ids=lambda c: f'N{c[0]}-C{c[1]}-{c[2]}')
def test_brute_force_auroc_is_sklearns(case):
    scores, labels = L.auroc_inputs(case)
    n_pos, pairs2 = L.auroc_counts(scores, labels)
    assert int(n_pos.sum()) == case[0]
    if case[2] == 'absent':
        assert n_pos[case[1] - 1] == 0
    if case[2] == 'one_atom':
        assert n_pos[1] == 1
    if int((n_pos > 0).sum()) < 2:                                        # one class holds every row
        with pytest.raises(ValueError):
            L.auroc_from_counts(n_pos, pairs2)
        with pytest.raises(ValueError, match='holds every row'):
            capi.auroc_from_counts(n_pos.tolist(), pairs2.tolist())
        return
    avg, per = L.auroc_from_counts(n_pos, pairs2)
    avg_b, per_b = capi.auroc_from_counts(n_pos.tolist(), pairs2.tolist())                 # the binding's float64 formulas
    assert avg_b == pytest.approx(avg, abs=1e-15) and per_b.keys() == per.keys()
    if case[2] == 'all_equal':
        assert all(v == 0.5 for v in per_b.values()) and avg_b == pytest.approx(0.5, abs=1e-15)
    sk = L.sklearn_auroc(scores, labels)
    assert abs(sk[0] - avg) <= 1e-12 and sk[1].keys() == per.keys()
    assert max(abs(sk[1][c] - per[c]) for c in per) <= 1e-12
    if case[2] != 'all_equal' and case[0] > 2:
        for defect in L.AUROC_DEFECTS:
            counts = L.auroc_counts(scores, labels, defect)
            assert abs(L.auroc_from_counts(*counts, defect)[0] - sk[0]) > 1e-9, defect


def test_validate_fixture_is_consistent():
    """the recorded validation: ten reference levels, every class on both sides, the brute-force AUROC of the recorded rows = sklearn's"""
    g = load_golden('validate_small.npz')
    assert g['levels'].tolist() == validation.levels_of(1000, 10).tolist() == [0, 111, 222, 333, 444, 555, 666, 777, 888, 999]
    y = g['labels'].astype(np.int64)
    assert len(y) == 10 * (22 + 13) and all(0 < int((y == c).sum()) < len(y) for c in set(y.tolist()))
    n_pos, pairs2 = L.auroc_counts(g['ligand_v_recon'], y)
    avg, per = L.auroc_from_counts(n_pos, pairs2)
    assert abs(avg - float(g['atom_auroc'])) <= 1e-12
    assert np.abs(np.asarray([per[int(c)] for c in g['classes']]) - g['per_class_auroc']).max() <= 1e-12
    assert float(g['loss64']) == pytest.approx(float(g['per_level64'][:, 0].mean()), rel=1e-12)


def test_format_line_is_the_reference_format():
    g = load_golden('validate_small.npz')
    rep = {k: float(g[k]) for k in ('loss', 'loss_pos', 'loss_v', 'atom_auroc')}
    line = validation.format_line(1000, rep)
    assert line == '[Validate] Iter %05d | Loss %.6f | Loss pos %.6f | Loss v %.6f e-3 | Avg atom auroc %.6f' % (
        1000, rep['loss'], rep['loss_pos'], rep['loss_v'] * 1000, rep['atom_auroc'])
    assert line.startswith('[Validate] Iter 01000 | Loss 1.0546') and 'e-3 | Avg atom auroc 0.6062' in line


def test_sample_time_structure():
    m = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG), 27, 13)
    T = m.num_timesteps
    for n in (1, 2, 5, 8):
        gen = torch.Generator().manual_seed(n)
        t, pt = m.sample_time(n, 'cpu', 'symmetric', generator=gen)
        assert t.shape == (n,) and t.dtype == torch.int64 and bool(((t >= 0) & (t < T)).all())
        assert torch.equal(pt, torch.full((n,), 1.0 / T))
        k = n // 2 + 1
        first = torch.randint(0, T, size=(k,), generator=torch.Generator().manual_seed(n))
        assert torch.equal(t, torch.cat([first, T - first - 1])[:n])      # k draws, mirrored, cut
    t2, _ = m.sample_time(6, 'cpu', 'importance', generator=torch.Generator().manual_seed(3))      # Lt_count is 0: the fallback
    t3, _ = m.sample_time(6, 'cpu', 'symmetric', generator=torch.Generator().manual_seed(3))
    assert torch.equal(t2, t3)
    m.Lt_count.fill_(11)
    with pytest.raises(NotImplementedError):
        m.sample_time(6, 'cpu', 'importance')
    with pytest.raises(ValueError):
        m.sample_time(6, 'cpu', 'uniform')
    assert {'Lt_history', 'Lt_count'} <= set(m.state_dict())             # persistent, as in the reference's state_dict


def test_header_exports_and_binding_surface():
    header = open(os.path.join(ROOT, 'include', 'targetdiff_hip.h')).read()
    assert re.search(r'#define TD_ABI_VERSION 5\b', header)
    for name in ('td_diffusion_loss', 'td_auroc'):
        assert re.search(r'\bint %s\(' % name, header) and name in capi.SIGNATURES
    lib = capi.load_library()
    assert lib.td_abi_version() == 5 and hasattr(lib, 'td_diffusion_loss') and hasattr(lib, 'td_auroc')
    assert 'td_*' in open(os.path.join(ROOT, 'targetdiff_amd', 'csrc', 'exports.map')).read()
    # one type term for both kernels: neither file keeps a copy of its own
    csrc = os.path.join(ROOT, 'targetdiff_amd', 'csrc')
    for f in ('likelihood.hip', 'loss.hip'):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "td_type_term.h"' in text and 'TD_TYPE_TERM(' in text and 'categorical_kl' not in text
    sig = inspect.signature(ScorePosNet3D.get_diffusion_loss)
    assert list(sig.parameters)[:8] == ['self', 'protein_pos', 'protein_v', 'batch_protein', 'ligand_pos', 'ligand_v', 'batch_ligand', 'time_step']
    assert sig.parameters['noise_source'].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters['generator'].kind is inspect.Parameter.KEYWORD_ONLY
    assert 'no gradient' in ScorePosNet3D.get_diffusion_loss.__doc__.lower()
    assert list(inspect.signature(validation.validate).parameters) == ['model', 'batches', 'num_levels', 'fused', 'noise_source']
    assert hasattr(capi.NativeModel, 'diffusion_loss') and callable(capi.auroc)


def test_library_refusals_without_a_gpu():
    lib = capi.load_library()
    some = 8                                                             # a non-null pointer that is never dereferenced
    call = lambda N=4, C=13, scores=some, labels=some, n_pos=some, pairs2=some: lib.td_auroc(scores, labels, N, C, n_pos, pairs2, None)
    assert call(N=-1) == -1 and b'td_auroc' in lib.td_last_error()
    assert call(N=(1 << 20) + 1) == -1 and b'rows' in lib.td_last_error()
    assert call(C=17) == -1 and b'17 classes' in lib.td_last_error()
    assert call(C=0) == -1
    assert call(n_pos=None) == -1 and b'null pointer' in lib.td_last_error()
    assert call(scores=None) == -1 and call(labels=None) == -1
    none = [None] * 7
    rc = lib.td_diffusion_loss(None, None, None, 0, 0, *none, 1.0, None, None, None, None, None, None)
    assert rc == -1 and b'td_diffusion_loss' in lib.td_last_error()      # no model handle


def test_more_classes_than_the_kernels_hold_are_refused():
    """C > TD_MAXC: td_diffusion_loss takes C from its model handle and refuses it there; no such handle can exist, because td_model_create
    refuses the configuration first (both checked: the library's text for each is in the source); td_auroc, which takes C itself, refuses
    17 (test_library_refusals_without_a_gpu)"""
    import ctypes
    lib = capi.load_library()
    cfg = capi.TdConfig(hidden_dim=128, n_heads=16, knn=32, num_layers=9, num_r_gaussian=20, edge_feat_dim=4, protein_feat_dim=27,
                        ligand_num_classes=17, num_timesteps=1000)
    h = ctypes.c_void_p()
    dummy = (ctypes.c_float * 4)()
    assert lib.td_model_create(ctypes.byref(cfg), dummy, 4, None, 0, ctypes.byref(h)) == -1 and not h.value
    text = open(os.path.join(ROOT, 'targetdiff_amd', 'csrc', 'loss.hip')).read()
    assert 'C > TD_MAXC' in text and 'N_l < 0 || B < 0' in text


def test_validate_checkpoint_tool_opens_a_train_script_checkpoint(tmp_path):
    """a file shaped like the reference's train script's (scripts/train_diffusion.py:222-226): a dict with an attribute-dict `config`
    beside 'model', 'optimizer', 'scheduler', 'iteration' -- and a data file whose fields are numpy arrays"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import validate_checkpoint as V
    from oracle import shims
    m = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG), 27, 13)
    m.load_state_dict(weights.make_state_dict(5), strict=False)
    path = str(tmp_path / '1000.pt')
    torch.save({'config': shims.EasyDict({'model': shims.EasyDict(dict(weights.DEFAULT_MODEL_CONFIG))}), 'model': m.state_dict(),
                'optimizer': {}, 'scheduler': {}, 'iteration': 1000}, path)
    sd, strict = V.load_weights(path)
    assert strict and set(sd) == set(m.state_dict())
    model, C = V.model_from(dict(weights.DEFAULT_MODEL_CONFIG), sd, strict)         # strict=True: the schedule constants included
    assert C == 13 and all(torch.equal(v, model.state_dict()[k]) for k, v in m.state_dict().items())
    torch.save(sd, str(tmp_path / 'bare.pt'))
    assert set(V.load_weights(str(tmp_path / 'bare.pt'))[0]) == set(sd)
    items = [{'protein_pos': np.zeros((4, 3), np.float32), 'protein_atom_feature': np.zeros((4, 27), np.float32),
              'ligand_pos': np.zeros((2, 3), np.float32), 'ligand_atom_feature_full': np.array([1, 2])}] * 2
    torch.save(items, str(tmp_path / 'data.pt'))
    b = validation.collate(torch.load(str(tmp_path / 'data.pt'), map_location='cpu', weights_only=False))
    assert b['ligand_element_batch'].tolist() == [0, 0, 1, 1] and b['protein_atom_feature'].shape == (8, 27)


def test_binding_refusals_before_any_device_work():
    with pytest.raises(ValueError, match='scores'):
        capi.auroc(torch.zeros(4), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match='NaN'):
        capi.auroc(torch.tensor([[0.0, float('nan')], [0.0, 1.0]]), torch.tensor([0, 1]))
    with pytest.raises(ValueError, match='labels must be in'):
        capi.auroc(torch.zeros(2, 2), torch.tensor([0, 2]))
    with pytest.raises(ValueError, match='at most'):
        capi.auroc(torch.zeros(capi.AUROC_MAX_ROWS + 1, 1), torch.zeros(capi.AUROC_MAX_ROWS + 1, dtype=torch.int64))
    m = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG), 27, 13)
    z = torch.zeros
    with pytest.raises(RuntimeError, match='HIP devices only'):
        m.get_diffusion_loss(z(4, 3), z(4, 27), z(4, dtype=torch.int64), z(2, 3), z(2, dtype=torch.int64), z(2, dtype=torch.int64))
    with pytest.raises(ValueError, match='no batches'):
        validation.validate(m, [])
