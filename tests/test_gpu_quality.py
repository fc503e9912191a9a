"""td_quality_report on the GPU (csrc/quality.hip) against the reference's own results.

  1. every fixture of tools/make_golden_quality.py (made with the real reference: check_stability, get_pair_length_profile, the
     element Counter) through the kernel: nr_bonds, stable atoms, stable flags, element counts and histogram entries with array_equal,
     hist / hist.sum() bit for bit against the reference's distribution.  quality_thresholds holds 425 two-atom molecules within two
     fp32 ulps of a threshold: fp32 arithmetic, a fused multiply-add or a non-IEEE square root changes an order there.
  2. a molecule's result depends on that molecule alone: S frames in one call == S calls of one frame, molecules reversed, an
     unrelated pack in front -- all array_equal; a non-default stream; a null nr_bonds pointer; include='stable'.
  3. end to end: sample_quality of the driver's trajectories == tests/_quality_ref.py (pinned to the same fixtures on the host), with
     num_steps and with a strided time program.
"""
import types

import numpy as np
import pytest
import torch

import _quality_ref as QR
from conftest import load_golden
from oracle import draws, weights
from targetdiff_amd import capi, quality, workloads
from targetdiff_amd.schedule import TimeProgram

pytestmark = pytest.mark.gpu

CLASS_Z = quality.class_atomic_numbers('add_aromatic')
PROFILES = quality.default_profiles()
KEYS = ('nr_bonds', 'stable_atoms', 'mol_stable', 'hist', 'counts')


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


def report(pos, v, ptr, include=None, profiles=PROFILES, **kw):
    """capi.quality_report of numpy inputs, as numpy"""
    dev = _dev()
    inc = None if include is None else torch.as_tensor(np.ascontiguousarray(include), dtype=torch.bool, device=dev)
    r = capi.quality_report(torch.as_tensor(np.ascontiguousarray(pos), device=dev), torch.as_tensor(np.ascontiguousarray(v), dtype=torch.int64, device=dev),
                            torch.as_tensor(np.asarray(ptr), dtype=torch.int32, device=dev), CLASS_Z, profiles, inc, **kw)
    return {k: (None if t is None else t.cpu().numpy()) for k, t in r.items()}


def same(a, b, what):
    for k in KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f'{what}: {k}')


_CACHE = {}


def sizes_report():
    """the sizes fixture through the kernel, once: the baseline of the independence tests"""
    if 'sizes' not in _CACHE:
        g = load_golden('quality_sizes.npz')
        _CACHE['sizes'] = (g, report(g['pos'], g['v'], g['ptr'], g['include']))
    return _CACHE['sizes']


@pytest.mark.parametrize('name', ['quality_docked.npz', 'quality_thresholds.npz'])
def test_fixture_of_the_reference(name):
    g = load_golden(name)
    r = report(g['pos'], g['v'], g['ptr'])
    assert r['nr_bonds'].dtype == np.int32 and r['mol_stable'].dtype == np.uint8 and r['hist'].dtype == np.int64 and r['hist'].shape[1:] == (2, 128)
    QR.check_against_fixture(r, g)


def test_fixture_sizes_and_include_mask():
    g, r = sizes_report()
    QR.check_against_fixture(r, g)                       # 0, 1, 2, 63, 64, 65, 130, 300 and 600 atoms: more than two tiles of 256
    assert r['hist'][2, 0].sum() == 0 and r['hist'][2, 1].sum() == 1


def test_fixture_trajectory_1000_frames():
    g = load_golden('quality_traj.npz')
    t = load_golden('sample_small_1000.npz')
    r = report(t['pos_traj'], t['v_traj'], g['ptr'], return_nr_bonds=False)
    assert r['nr_bonds'] is None
    np.testing.assert_array_equal(r['stable_atoms'], g['stable_atoms'])
    np.testing.assert_array_equal(r['mol_stable'], g['mol_stable'])
    np.testing.assert_array_equal(r['hist'][:, 1, :101], g['hist_All_12A'])
    np.testing.assert_array_equal(r['hist'][:, 1].sum(1), g['n_All_12A'])
    np.testing.assert_array_equal(r['hist'][:, 0].sum(1), g['n_CC_2A'])
    np.testing.assert_array_equal(r['counts'], g['counts'])


def test_frames_one_by_one_reversed_and_behind_another_pack():
    g, base = sizes_report()
    pos, v, ptr, inc = g['pos'], g['v'], g['ptr'], g['include']
    S, B = inc.shape
    # S calls of one frame
    for s in range(S):
        one = report(pos[s:s + 1], v[s:s + 1], ptr, inc[s:s + 1])
        same(one, {k: base[k][s:s + 1] for k in KEYS}, f'frame {s} alone')
    # the molecules in reversed order
    order = np.concatenate([np.arange(ptr[b], ptr[b + 1]) for b in reversed(range(B))]).astype(np.int64)
    rptr = np.concatenate([[0], np.cumsum(np.diff(ptr)[::-1])])
    rev = report(pos[:, order], v[:, order], rptr, inc[:, ::-1])
    np.testing.assert_array_equal(rev['nr_bonds'], base['nr_bonds'][:, order])
    np.testing.assert_array_equal(rev['stable_atoms'], base['stable_atoms'][:, ::-1])
    np.testing.assert_array_equal(rev['mol_stable'], base['mol_stable'][:, ::-1])
    np.testing.assert_array_equal(rev['hist'], base['hist'])
    np.testing.assert_array_equal(rev['counts'], base['counts'])
    # an unrelated pack in front, kept out of the histograms by the mask
    d = load_golden('quality_docked.npz')
    n0 = d['pos'].shape[1]
    fpos = np.concatenate([np.repeat(d['pos'], S, 0) + np.float32(3.0), pos], axis=1)
    fv = np.concatenate([np.repeat(d['v'], S, 0), v], axis=1)
    fptr = np.concatenate([d['ptr'][:-1], ptr + n0])
    finc = np.concatenate([np.zeros((S, 5), bool), inc], axis=1)
    front = report(fpos, fv, fptr, finc)
    np.testing.assert_array_equal(front['nr_bonds'][:, n0:], base['nr_bonds'])
    np.testing.assert_array_equal(front['stable_atoms'][:, 5:], base['stable_atoms'])
    np.testing.assert_array_equal(front['mol_stable'][:, 5:], base['mol_stable'])
    np.testing.assert_array_equal(front['hist'], base['hist'])
    np.testing.assert_array_equal(front['counts'], base['counts'])


def test_side_stream_null_nr_bonds_and_profiles():
    dev = _dev()
    g, base = sizes_report()
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        side = report(g['pos'], g['v'], g['ptr'], g['include'])
        bare = report(g['pos'], g['v'], g['ptr'], g['include'], return_nr_bonds=False)
    torch.cuda.current_stream(dev).wait_stream(st)
    same(side, base, 'side stream')
    assert bare['nr_bonds'] is None
    for k in KEYS[1:]:
        np.testing.assert_array_equal(bare[k], base[k], err_msg=k)
    # no profile at all, and four of them (one with a single edge, one with 127, element pairs in either order)
    none = report(g['pos'], g['v'], g['ptr'], g['include'], profiles=())
    assert none['hist'].shape == (3, 0, 128)
    np.testing.assert_array_equal(none['stable_atoms'], base['stable_atoms'])
    np.testing.assert_array_equal(none['counts'], base['counts'])
    four = ((8, 7, 3.0, np.linspace(0.5, 3.0, 127)), (7, 8, 3.0, np.linspace(0.5, 3.0, 127)), (0, 6, 4.0, [1.5]), PROFILES[1])
    r4 = report(g['pos'], g['v'], g['ptr'], g['include'], profiles=four)
    want = QR.quality_report(g['pos'], g['v'], g['ptr'], CLASS_Z, four, g['include'])
    np.testing.assert_array_equal(r4['hist'], want['hist'])
    np.testing.assert_array_equal(r4['hist'][:, 0], r4['hist'][:, 1])
    np.testing.assert_array_equal(r4['hist'][:, 3], base['hist'][:, 1])
    assert r4['hist'][:, 0].sum() > 0 and r4['hist'][0, 2, :2].all() and not r4['hist'][:, 2, 2:].any()


def test_public_functions_and_include_stable():
    dev = _dev()
    d = load_golden('quality_docked.npz')
    batch = torch.arange(5).repeat_interleave(25)
    ok, ns, nb = quality.stability(torch.from_numpy(d['pos'][0]).to(dev), torch.from_numpy(d['v'][0]).to(dev), batch_ligand=batch, return_nr_bonds=True)
    assert ok.dtype == torch.bool and ok.is_cuda and ok.tolist() == [True, False, False, False, False]
    np.testing.assert_array_equal(ns.cpu().numpy(), d['stable_atoms'][0])
    np.testing.assert_array_equal(nb.cpu().numpy(), d['nr_bonds'][0])
    # float64 holding fp32 values, as the driver returns them; a stack of frames
    ok2, ns2 = quality.stability(d['pos'].astype(np.float64), d['v'], ligand_ptr=d['ptr'])
    assert tuple(ok2.shape) == (1, 5) and ns2.cpu().numpy().tolist() == d['stable_atoms'].tolist()
    hist, counts = quality.pair_profiles(d['pos'], d['v'], ligand_ptr=d['ptr'])
    np.testing.assert_array_equal(hist.cpu().numpy()[:, 1].sum(1), d['n_All_12A'])
    np.testing.assert_array_equal(counts.cpu().numpy(), d['counts'])
    # include='stable': only the docked original enters the profiles; the stability numbers stay those of all five
    split = lambda a: [a[:, 25 * k:25 * (k + 1)].astype(np.float64) for k in range(5)]
    res = (None, None, split(d['pos']), [d['v'][:, 25 * k:25 * (k + 1)] for k in range(5)], [], [], [])
    ref = load_golden('quality_reference_distributions.npz')
    ref = {k: ref[k] for k in ('CC_2A', 'All_12A', 'atom_type')}
    rep = quality.sample_quality(res, include='stable', reference=ref)
    only = report(d['pos'][:, :25], d['v'][:, :25], [0, 25])
    np.testing.assert_array_equal(rep.hist, only['hist'])
    np.testing.assert_array_equal(rep.counts, only['counts'])
    assert rep.stable_mols.tolist() == [1] and rep.stable_atoms.tolist() == [int(d['stable_atoms'].sum())]
    full = quality.sample_quality(res, reference=ref)
    assert full.mol_stable[0] == 1 / 5.0 and full.atm_stable[0] == int(d['stable_atoms'].sum()) / 125.0
    js = full.js()
    for name in ('CC_2A', 'All_12A'):
        assert abs(js['JSD_' + name] ** 2 - float(d['js_' + name][0]) ** 2) <= 1e-12
    assert abs(js['atom_type_js'] ** 2 - float(d['js_atom_type'][0]) ** 2) <= 1e-12
    with pytest.raises(ValueError, match='35'):
        quality.stability(d['pos'], d['v'], ligand_ptr=d['ptr'], atom_enc_mode=[6] * 12 + [35])


def _model():
    if 'model' not in _CACHE:
        from targetdiff_amd.models import ScorePosNet3D
        m = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG), 27, 13)
        assert not m.load_state_dict(weights.make_state_dict(2021), strict=False).unexpected_keys
        _CACHE['model'] = m.to(_dev()).eval()
    return _CACHE['model']


@pytest.mark.parametrize('mode', ['num_steps', 'strided'])
def test_sample_quality_of_a_sampled_trajectory(mode):
    """4 samples x 20 steps on a small pocket with seeded random weights: the whole-trajectory report equals the restatement"""
    from targetdiff_amd import sampling
    dev = _dev()
    pk = workloads.synthetic_pocket(301, 70, 3.0, 9.0)
    data = types.SimpleNamespace(protein_pos=torch.from_numpy(pk.pos), protein_atom_feature=torch.from_numpy(pk.feat))
    src = draws.Source(9900, dev)
    sizes = [6, 9, 4, 11]
    steps = dict(num_steps=20) if mode == 'num_steps' else dict(time_program=TimeProgram.strided(1000, 5))
    frames = 20 if mode == 'num_steps' else len(steps['time_program'])
    res = sampling.sample_diffusion_ligand(_model(), data, 4, batch_size=4, device=dev, ligand_num_atoms=sizes,
                                           noise_source=lambda b, st, name, like: src(st + 1, name, like), **steps)
    assert [p.shape for p in res[2]] == [(frames, n, 3) for n in sizes]
    rep = quality.sample_quality(res, 'all', reference={})
    pos = np.concatenate([p.astype(np.float32) for p in res[2]], axis=1)
    v = np.concatenate(res[3], axis=1)
    want = QR.quality_report(pos, v, np.cumsum([0] + sizes), CLASS_Z, PROFILES)
    assert rep.num_frames == frames and rep.n_samples == 4 and rep.n_atoms == 30
    np.testing.assert_array_equal(rep.hist, want['hist'])
    np.testing.assert_array_equal(rep.counts, want['counts'])
    np.testing.assert_array_equal(rep.stable_atoms, want['stable_atoms'].sum(1))
    np.testing.assert_array_equal(rep.stable_mols, want['mol_stable'].sum(1))
    last = quality.sample_quality(res, reference={})
    np.testing.assert_array_equal(last.hist[0], want['hist'][-1])
    assert last.stable_atoms[0] == want['stable_atoms'][-1].sum() and last.summary()['JSD_All_12A'] is None
