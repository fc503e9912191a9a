"""Clash guidance, host side (CPU; DESIGN.md section 3, "Clash guidance"): the rule as tests/_guidance_ref.py states it -- autograd of the
float64 energy equals the closed form, one overlapping pair ends at the contact distance, the cap, coincident pairs -- and the
argument checks of ``ClashGuidance``, of the ``guidance`` keyword of the sampler and of the batching driver.
"""
import types

import numpy as np
import pytest
import torch

import _guidance_ref as GR
import _program_ref as PR
from _tol import close
from oracle.native_stub import RecordingNative
from targetdiff_amd.guidance import ClashGuidance, check_guidance


def _cloud(seed, P=40, L=9):
    g = torch.Generator().manual_seed(seed)
    protein = 4.0 * torch.randn(P, 3, generator=g, dtype=torch.float64)
    sigma = 2.5 + 1.5 * torch.rand(P, generator=g, dtype=torch.float64)
    x = 3.0 * torch.randn(L, 3, generator=g, dtype=torch.float64)
    return protein, sigma, x


# ------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize('seed', [1, 2, 3])
def test_autograd_of_the_energy_is_the_closed_form(seed):
    protein, sigma, x = _cloud(seed)
    assert GR.report(protein, sigma, x)[0] > 10                      # the cloud does clash
    want = GR.shift_autograd(protein, sigma, x, w=0.7)
    got = GR.shift_closed(protein, sigma, x, w=0.7)
    # float64 on both sides, a few hundred terms of order 1: 1e-12 is four orders above the rounding of either
    close(got, want, 1e-12, 'closed form vs autograd')
    assert float(want.abs().max()) > 0.1


def test_energy_decreases_along_the_shift():
    protein, sigma, x = _cloud(4)
    e0 = float(GR.energy(protein, sigma, x))
    d = GR.shift_closed(protein, sigma, x, w=1.0)
    e1 = float(GR.energy(protein, sigma, x + 1e-3 * d))
    assert e1 < e0                                                    # -grad E is a descent direction


@pytest.mark.parametrize('d0,sigma', [(0.5, 3.0), (2.9, 3.0), (1.0, 2.5)])
def test_single_pair_ends_at_the_contact_distance(d0, sigma):
    """one ligand atom at distance d < sigma from one protein atom, w = 1, no cap: it ends at distance sigma"""
    p = torch.tensor([[1.0, -2.0, 0.5]], dtype=torch.float64)
    u = torch.tensor([0.6, 0.0, -0.8], dtype=torch.float64)
    x = p + d0 * u
    s = torch.tensor([sigma], dtype=torch.float64)
    x1 = x + GR.shift_closed(p, s, x, w=1.0, max_shift=0.0)
    assert abs(float((x1 - p).norm()) - sigma) <= 1e-14 * sigma * 4
    close(x1, p + sigma * u, 1e-14, 'along the pair axis')
    # outside the radius nothing moves
    far = p + (sigma + 1e-3) * u
    assert torch.equal(GR.shift_closed(p, s, far), torch.zeros(1, 3, dtype=torch.float64))


def test_cap_scales_to_max_shift_and_leaves_short_shifts_alone():
    protein, sigma, x = _cloud(5)
    raw = GR.shift_closed(protein, sigma, x, w=1.0)
    n = raw.norm(dim=-1)
    cap = float(n.median())
    assert bool((n > cap).any()) and bool((n < cap).any())
    got = GR.shift_closed(protein, sigma, x, w=1.0, max_shift=cap)
    long = n > cap
    assert torch.equal(got[~long], raw[~long])
    close(got[long].norm(dim=-1), torch.full((int(long.sum()),), cap, dtype=torch.float64), 1e-13, 'capped length')
    close(got[long] / cap, raw[long] / n[long, None], 1e-13, 'capped direction')
    assert torch.equal(GR.shift_closed(protein, sigma, x, w=1.0, max_shift=0.0), raw)            # 0: no cap


def test_coincident_pair_adds_nothing():
    protein, sigma, x = _cloud(6)
    x = x.clone()
    x[3] = protein[7]                                                  # d = 0
    x[4] = protein[9] + torch.tensor([3e-7, 0.0, 0.0], dtype=torch.float64)          # d < 1e-6
    got = GR.shift_closed(protein, sigma, x)
    assert bool(torch.isfinite(got).all())
    keep = torch.ones(protein.shape[0], dtype=torch.bool)
    keep[7] = False
    close(got[3], GR.shift_closed(protein[keep], sigma[keep], x[3:4])[0], 1e-13, 'atom on a protein atom: that pair is skipped')
    keep = torch.ones(protein.shape[0], dtype=torch.bool)
    keep[9] = False
    close(got[4], GR.shift_closed(protein[keep], sigma[keep], x[4:5])[0], 1e-13, 'atom 3e-7 from a protein atom')
    cnt, e, mn = GR.report(protein, sigma, x)
    assert mn == 0.0 and cnt >= 2 and e >= 0.5 * float(sigma[7]) ** 2            # the report counts the pair and its energy


def test_report_of_empty_graphs():
    protein, sigma, x = _cloud(7)
    assert GR.report(protein[:0], sigma[:0], x) == (0, 0.0, float('inf'))
    assert GR.report(protein, sigma, x[:0]) == (0, 0.0, float('inf'))
    assert GR.shift_closed(protein[:0], sigma[:0], x).abs().max() == 0


def test_kernel_test_pack_keeps_its_promises():
    """the pack of tests/test_gpu_guidance.py: no d_ij within 1e-4 A of sigma_j in float64 (so the pair counts are exact), the ragged
    sizes, and the three special atoms"""
    from targetdiff_amd import capi
    tile = capi.CLASH_TILE
    pk = GR.make_pack(tile)
    pp, lp, sp = pk['pptr'], pk['lptr'], pk['special']
    assert np.diff(pp).tolist() == [1, tile - 1, tile, tile + 77] and np.diff(lp).tolist() == [0, 1, 5, 37]
    assert all(t.dtype == torch.float32 for t in (pk['protein'], pk['sigma'], pk['x']))
    assert float(pk['sigma'].min()) >= 2.5 and float(pk['sigma'].max()) <= 4.0
    assert min(GR.per_graph(GR.min_gap, pk['protein'], pk['sigma'], pp, pk['x'], lp)) > 1e-4
    assert torch.equal(pk['x'][sp['coincident']], pk['protein'][sp['coincident_protein']]) and sp['coincident_protein'] - pp[3] >= tile
    raw = torch.cat(GR.per_graph(GR.shift_closed, pk['protein'], pk['sigma'], pp, pk['x'], lp, 1.0, 0.0))
    assert torch.equal(raw[sp['outside']], torch.zeros(3, dtype=torch.float64))
    n = raw.norm(dim=-1)
    assert float(n[sp['capped']]) > 2 * pk['max_shift'] and int((n < pk['max_shift']).sum()) >= 1
    r64 = GR.per_graph(GR.report, pk['protein'], pk['sigma'], pp, pk['x'], lp)
    r32 = GR.per_graph(GR.report, pk['protein'], pk['sigma'], pp, pk['x'], lp, dtype=torch.float32)
    assert [c for c, _, _ in r64] == [c for c, _, _ in r32] and sum(c for c, _, _ in r64) > 3 * pk['x'].shape[0]


# ------------------------------------------------------------------------------------------ ClashGuidance
def test_clash_guidance_defaults_and_radii():
    g = ClashGuidance()
    assert (g.radius, g.weight, g.max_shift) == (3.0, 1.0, 1.0) and not g.per_atom
    r = g.radii(5)
    assert r.dtype == torch.float32 and r.tolist() == [3.0] * 5
    t = torch.tensor([2.5, 3.0, 4.0], dtype=torch.float64)
    gt = ClashGuidance(radius=t, weight=0.5, max_shift=0.0)
    assert gt.per_atom and gt.radii(3).dtype == torch.float32 and gt.radii(3).tolist() == [2.5, 3.0, 4.0]
    with pytest.raises(ValueError):
        gt.radii(4)
    rep = gt.replicated(3, 2)
    assert rep.radius.tolist() == [2.5, 3.0, 4.0, 2.5, 3.0, 4.0] and (rep.weight, rep.max_shift) == (0.5, 0.0)
    assert g.replicated(3, 2) is g
    with pytest.raises(ValueError):
        gt.replicated(4, 2)
    p = ClashGuidance.parse('3.5')
    assert (p.radius, p.weight, p.max_shift) == (3.5, 1.0, 1.0)
    p = ClashGuidance.parse('3.5:0.25:2')
    assert (p.radius, p.weight, p.max_shift) == (3.5, 0.25, 2.0)


@pytest.mark.parametrize('what,kw', [
    ('zero radius', dict(radius=0.0)),
    ('negative radius', dict(radius=-1.0)),
    ('nan radius', dict(radius=float('nan'))),
    ('radius of another type', dict(radius='3')),
    ('bool radius', dict(radius=True)),
    ('2-D radii', dict(radius=torch.ones(3, 1))),
    ('integer radii', dict(radius=torch.ones(3, dtype=torch.int64))),
    ('a non-positive radius among the radii', dict(radius=torch.tensor([3.0, 0.0, 2.0]))),
    ('an infinite radius among the radii', dict(radius=torch.tensor([3.0, float('inf')]))),
    ('negative weight', dict(weight=-0.1)),
    ('nan weight', dict(weight=float('nan'))),
    ('negative max_shift', dict(max_shift=-1.0)),
    ('max_shift of another type', dict(max_shift=None)),
])
def test_clash_guidance_validation(what, kw):
    with pytest.raises(ValueError):
        ClashGuidance(**kw)
        pytest.fail(what)


@pytest.mark.parametrize('text', ['', 'a', '3:b', '1:2:3:4', '-1', '3:-1', '3:1:-2'])
def test_parse_refuses(text):
    with pytest.raises(ValueError):
        ClashGuidance.parse(text)


def test_check_guidance():
    g = ClashGuidance(radius=torch.full((5,), 3.0))
    assert check_guidance(None, 5, True) is None
    assert check_guidance(g, 5, False) is g
    with pytest.raises(ValueError, match='5 radii'):
        check_guidance(g, 6, False)
    with pytest.raises(ValueError, match='unsorted batch_ligand'):
        check_guidance(ClashGuidance(), 6, True)
    with pytest.raises(ValueError, match='ClashGuidance'):
        check_guidance(3.0, 6, False)


# ------------------------------------------------------------------------------------------ the sampler's keyword
def _stub_model(monkeypatch, case='program_stride50'):
    from targetdiff_amd import models
    m = PR.mirror(case)
    log = []
    native = RecordingNative(PR.state_dict(case), PR.model_config(case), m.num_classes, log)
    monkeypatch.setattr(models.ScorePosNet3D, '_native', lambda self, device: native)
    return m, log


def test_sampler_keyword_checks_raise_value_error(monkeypatch):
    _, inputs = PR.load_fixture('program_stride50')
    m, log = _stub_model(monkeypatch)
    b = PR.case_batch('program_stride50')
    Np = b.protein_pos.shape[0]
    unsorted = b.ligand_element_batch.clone()
    unsorted[0], unsorted[-1] = 1, 0
    args = lambda bl=b.ligand_element_batch: (b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch, inputs['init_pos'],
                                               inputs['init_v'], bl)
    for what, a, kw in [
            ('not a ClashGuidance', args(), dict(guidance=3.0)),
            ('a dict', args(), dict(guidance=dict(radius=3.0))),
            ('radii of another length', args(), dict(guidance=ClashGuidance(radius=torch.full((Np + 1,), 3.0)))),
            ('unsorted ligand batch vector', args(unsorted), dict(guidance=ClashGuidance()))]:
        with pytest.raises(ValueError):
            m.sample_diffusion(*a, center_pos_mode='protein', num_steps=2, use_session=False, **kw)
            pytest.fail(what)
        with pytest.raises(ValueError):
            m.begin_sampling(*a, center_pos_mode='protein', num_steps=2, use_session=False, **kw)
    assert not log                                           # refused before anything ran
    with pytest.raises(TypeError):                           # keyword-only
        m.sample_diffusion(*args(), None, 'protein', False, 0, None, True, None, None, None, None, None, ClashGuidance())


def test_guidance_none_calls_the_native_layer_as_before(monkeypatch):
    from oracle import draws
    _, inputs = PR.load_fixture('program_stride50')
    m, log = _stub_model(monkeypatch)
    b = PR.case_batch('program_stride50')
    args = (b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch, inputs['init_pos'], inputs['init_v'],
            b.ligand_element_batch)
    a = m.sample_diffusion(*args, center_pos_mode='protein', num_steps=2, use_session=False, noise_source=draws.Source(1))
    calls = [(n, sorted(k)) for n, k in log]
    del log[:]
    bb = m.sample_diffusion(*args, center_pos_mode='protein', num_steps=2, use_session=False, noise_source=draws.Source(1), guidance=None)
    assert [(n, sorted(k)) for n, k in log] == calls
    assert torch.equal(a['pos'], bb['pos']) and torch.equal(a['v'], bb['v'])


# ------------------------------------------------------------------------------------------ the driver
def test_driver_replicates_the_radii_per_sample(monkeypatch):
    from targetdiff_amd import models, sampling, workloads
    m, _ = _stub_model(monkeypatch)
    seen = []

    class _Stop(Exception):
        pass

    def fake(self, **kw):
        seen.append(kw)
        raise _Stop
    monkeypatch.setattr(models.ScorePosNet3D, 'sample_diffusion', fake)
    pk = workloads.synthetic_pocket(301, 70, 3.0, 9.0)
    data = types.SimpleNamespace(protein_pos=torch.from_numpy(pk.pos), protein_atom_feature=torch.from_numpy(pk.feat))
    radii = torch.linspace(2.5, 4.0, 70)
    for g, want in [(ClashGuidance(radius=radii, weight=0.5, max_shift=0.75), radii.repeat(3)), (ClashGuidance(radius=3.25), 3.25)]:
        del seen[:]
        with pytest.raises(_Stop):
            sampling.sample_diffusion_ligand(m, data, 3, batch_size=3, device='cpu', ligand_num_atoms=[4, 6, 5], num_steps=2, guidance=g)
        got = seen[0]['guidance']
        assert isinstance(got, ClashGuidance) and (got.weight, got.max_shift) == (g.weight, g.max_shift)
        if torch.is_tensor(want):
            assert torch.equal(got.radius, want) and seen[0]['protein_pos'].shape[0] == want.numel()
        else:
            assert got.radius == want
    del seen[:]
    with pytest.raises(_Stop):                                # no guidance: the keyword is not passed on at all
        sampling.sample_diffusion_ligand(m, data, 3, batch_size=3, device='cpu', ligand_num_atoms=[4, 6, 5], num_steps=2)
    assert 'guidance' not in seen[0]
    for bad in (ClashGuidance(radius=torch.full((69,), 3.0)), 3.0):
        with pytest.raises(ValueError):
            sampling.sample_diffusion_ligand(m, data, 3, batch_size=3, device='cpu', ligand_num_atoms=[4, 6, 5], num_steps=2, guidance=bad)


def test_batch_sample_flag(monkeypatch, tmp_path):
    """tools/batch_sample.py --clash-guidance reaches the driver as a ClashGuidance; a malformed value is a usage error"""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location('batch_sample_tool', os.path.join(ROOT, 'tools', 'batch_sample.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    from targetdiff_amd import sampling
    seen = {}

    def fake_run(model, pockets, num_samples, **kw):
        seen.update(kw)
        return {}
    monkeypatch.setattr(sampling, 'run_sharded', fake_run)
    m, _ = _stub_model(monkeypatch)
    base = ['--pockets', 'synthetic:1', '--result_path', str(tmp_path), '--device', 'cpu', '--num_samples', '1', '--num_steps', '1']
    tool.main(base + ['--clash-guidance', '3.25:0.5:0.75'], model_factory=lambda args, dev: m)
    g = seen['guidance']
    assert isinstance(g, ClashGuidance) and (g.radius, g.weight, g.max_shift) == (3.25, 0.5, 0.75)
    seen.clear()
    tool.main(base, model_factory=lambda args, dev: m)
    assert 'guidance' not in seen
    with pytest.raises(SystemExit):
        tool.main(base + ['--clash-guidance', '3:x'], model_factory=lambda args, dev: m)


def test_new_symbols_are_bound():
    from targetdiff_amd import capi
    lib = capi.load_library()
    for name in ('td_clash_shift', 'td_clash_report', 'td_posterior_step_guided', 'td_session_set_guidance'):
        assert hasattr(lib, name) and name in capi.SIGNATURES
    assert len(capi.SIGNATURES['td_posterior_step_guided'][1]) == len(capi.SIGNATURES['td_posterior_step_program'][1]) + 1
