"""tests/_step_ref.py on the CPU: the restatement reproduces the recordings of the real reference, the cases are the regimes they claim to be,
and the rule of tests/test_gpu_step_float64.py rejects wrong kernels -- every planted defect of _step_ref.DEFECTS, put into the fp32
restatement in place of the HIP result, is rejected by a named case."""
import numpy as np
import pytest
import torch

import _program_ref as PR
import _step_ref as S
from conftest import load_golden
from oracle import restatement as R

F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------------------------------ pinned to the recordings
def test_schedules_are_the_oracles():
    sch, want = S.schedules(), R.diffusion_schedules()
    for k, v in want.items():
        if k in sch:
            assert torch.equal(sch[k], v), k
    assert set(sch) >= {'alphas_cumprod', 'sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod', 'posterior_logvar'}


def test_posterior_reproduces_the_recording():
    """tests/golden/posterior_kat.npz (the real reference's posterior step) at the bounds of test_oracle_golden's test_posterior_known_answers"""
    g = load_golden('posterior_kat.npz')
    T = lambda k: torch.from_numpy(g[k])
    out = S.posterior(S.schedules(), T('t'), T('x_t'), T('v_t'), T('x0'), T('v0_logits'), T('batch_ligand'), T('noise'), T('uniform'), 13, F32)
    assert S.distance(out['pos'], T('pos_next')) < 1e-6
    assert S.distance(out['log_v0'], T('log_v0')) < 1e-6
    assert S.distance(out['log_post'], T('log_post')) < 1e-5
    assert torch.equal(out['v'], T('v_next'))
    o64 = S.posterior(S.schedules(), T('t'), T('x_t'), T('v_t'), T('x0'), T('v0_logits'), T('batch_ligand'), T('noise'), T('uniform'), 13, F64)
    assert o64['pos'].dtype == o64['log_post'].dtype == F64 and torch.equal(o64['v'], T('v_next'))
    assert S.distance(o64['pos'], T('pos_next')) < 1e-6 and S.distance(o64['log_post'], T('log_post')) < 1e-5


def test_likelihood_agrees_with_the_oracle_on_the_recorded_inputs():
    """tests/golden/likelihood_small.npz: on its ligands, draws and time steps the fp32 restatement is oracle.restatement's perturb, likelihood_terms
    and likelihood_prior (which test_oracle_golden holds to the real reference's recorded results) to the last bits"""
    g = load_golden('likelihood_small.npz')
    T = lambda k: torch.from_numpy(g[k])
    sch, bl, t = S.schedules(), T('batch_ligand'), T('time_step')
    gen = torch.Generator().manual_seed(5)
    for ts in (t, torch.tensor([999, 0, 3])):
        want_x, want_v = R.perturb(sch, ts, T('ligand_pos'), T('ligand_v'), bl, T('noise'), T('uniform'), 13)
        got = S.perturb(sch, ts, T('ligand_pos'), T('ligand_v'), bl, T('noise'), T('uniform'), 13, F32)
        assert S.distance(got['pos'], want_x) <= 1e-6 and torch.equal(got['v'], want_v)
        pred_pos = want_x + 0.3 * torch.randn(want_x.shape, generator=gen)
        pred_v = 2.0 * torch.randn(len(bl), 13, generator=gen)
        want = R.likelihood_terms(sch, ts, T('ligand_pos'), want_x, T('ligand_v'), want_v, pred_pos, pred_v, bl, 13)
        got = S.likelihood_terms(sch, ts, T('ligand_pos'), want_x, T('ligand_v'), want_v, pred_pos, pred_v, bl, 13, F32)
        for a, b in zip(got, want):
            assert S.distance(a, b, rel=True) <= 1e-6
    want = R.likelihood_prior(sch, T('ligand_pos'), bl, bl, 13)
    got = S.likelihood_prior(sch, T('ligand_pos'), bl, bl, 13, 3, F32)
    for a, b in zip(got, want):
        assert S.distance(a, b, rel=True) <= 1e-6


def test_program_steps_agree_with_the_program_restatement():
    """tests/_program_ref.py's denoise_step / renoise_step (pinned to tests/golden/program_*.npz) on this file's rows and inputs"""
    case = ('base', 13)
    i = S.inputs(case)
    for name in S.DENOISE_ROWS:
        row, _ = S.program_rows()[name]
        for known in (False, True):
            kw = dict(mask=i['mask'], x0c=i['x0'], v0=i['v0']) if known else {}
            want = PR.denoise_step(row, i['x_t'], i['v_t'], i['pred_pos'], i['pred_v'], i['noise'], i['uniform'], 13, **kw)
            got = S.reference(f'posterior_prog_{"fixed_" if known else ""}{name}', case, F32)
            for a, k in zip(want, ('pos', 'v', 'log_v0', 'log_post')):
                assert S.distance(got[k], a) <= 1e-6, (name, known, k)
    for name in S.RENOISE_ROWS:
        row, _ = S.program_rows()[name]
        want = PR.renoise_step(row, i['x_t'], i['v_t'], i['noise'], i['uniform'], 13)
        got = S.reference(f'renoise_{name}', case, F32)
        for a, k in zip(want, ('pos', 'v', 'log_v0', 'log_post')):
            assert S.distance(got[k], a) <= 1e-6, (name, k)


def test_noise_reconstruction_and_head_against_the_oracle():
    i = S.inputs(('base', 13))
    tb = i['t'][S.BATCH]
    sch = S.schedules()
    x0 = S.x0_of_noise(sch, tb, i['pred_pos'], i['x_t'], F32)
    eps = i['pred_pos'] - i['x_t']
    want = sch['sqrt_recip_alphas_cumprod'][tb].unsqueeze(-1) * i['x_t'] - sch['sqrt_recipm1_alphas_cumprod'][tb].unsqueeze(-1) * eps
    assert torch.equal(x0, want)
    got = S.reference('posterior_noise', ('base', 13), F32)
    c0c = S.posterior(sch, i['t'], i['x_t'], i['v_t'], x0, i['pred_v'], S.BATCH, i['noise'], i['uniform'], 13, F32)
    assert torch.equal(got['pos'], c0c['pos']) and torch.equal(got['v'], c0c['v'])
    # the head and the embedding as oracle.restatement.model_forward computes them
    sd = S.state_dict(13)
    h, _ = S.head_rows(13)
    y = torch.nn.functional.softplus(torch.nn.functional.linear(h, sd['v_inference.0.weight'], sd['v_inference.0.bias'])) - np.log(2.0)
    want = torch.nn.functional.linear(y, sd['v_inference.2.weight'], sd['v_inference.2.bias'])
    assert S.distance(S.v_inference(sd, h, F32), want) <= 1e-6
    e = S.embed_ligand(sd, torch.arange(40) % 13, F64)
    assert e.shape == (40, 128) and e.dtype == F64 and bool((e[:, 127] == 1).all())
    assert torch.equal(e[:13, :127].float(), (sd['ligand_atom_emb.weight'].double().T + sd['ligand_atom_emb.bias'].double()).float())


# ------------------------------------------------------------------------------------------ the regimes are what they claim
def test_shapes():
    assert S.N == 330 and 0 in S.SIZES[1:-1] and {63, 64, 65} <= set(S.SIZES) and max(S.SIZES) > 128 and S.N > 256
    assert S.BATCH.bincount(minlength=S.B).tolist() == S.SIZES
    assert set(sum(S.T_SETS.values(), [])) == {0, 1, 2, 537, 998, 999}
    assert set(S.T_SETS['all0']) == {0} and set(S.T_SETS['all999']) == {999}
    mixed = S.T_SETS['mixed']
    assert mixed[S.SIZES.index(63)] == 0 and mixed[S.SIZES.index(130)] > 0          # a decoder graph and a KL graph of more than 64 lanes' worth
    assert set(S.CLASSES) == {13, 16, 2}
    m = S.known_atoms()
    assert 0.25 < float(m.float().mean()) < 0.42
    assert bool(m[S.BATCH == S.FULL_GRAPH].all()) and not bool(m[S.BATCH == S.FREE_GRAPH].any()) and not bool(m[S.TIE])
    rows = S.program_rows()
    from targetdiff_amd import schedule as SCH
    assert rows['last'][0][SCH.LAST] == 1 and rows['unit'][0][SCH.LAST] == 0 and rows['stride130'][0][SCH.LAST] == 0
    assert 0.99 < float(rows['renoise1'][0][SCH.RHO]) < 1 and 0.3 < float(rows['renoise_0_999'][0][SCH.RHO]) < 0.4


@pytest.mark.parametrize('C', S.CLASSES)
def test_regimes(C):
    i = {name: S.inputs((name, C)) for name in S.CASES}
    # saturation: log_softmax reaches -300 at x 100, and fp32 exp underflows inside a row (exp(-104) == 0)
    lv0 = S.reference('posterior_plain', ('sat100', C), F64)['log_v0']
    assert float(lv0.min()) < (-300 if C > 2 else -200)
    assert float(S.reference('posterior_plain', ('sat30', C), F64)['log_v0'].min()) < -104
    assert float(S.reference('posterior_plain', ('base', C), F64)['log_v0'].min()) > -20
    # the perfect prediction: both KLs cancel on every graph with t > 0, the decoder graphs do not
    for name in ('perfect', 'all0_perfect'):
        kp, kv = (S.reference('likelihood_terms', (name, C), F64)[k] for k in ('kl_pos', 'kl_v'))
        kl = (i[name]['t'] > 0) & (torch.tensor(S.SIZES) > 0)
        assert bool((kp[kl].abs() < 1e-12).all()) and bool((kv[kl].abs() < 1e-4).all()), (kp, kv)
        assert bool((kp[~kl & (torch.tensor(S.SIZES) > 0)].abs() > 1).all())
        assert torch.equal(i[name]['pred_pos'], i[name]['x0'])
    assert float(i['sat100']['x0'].abs().max()) > 100 and float(i['base']['x0'].abs().max()) < 12
    # the planted draws
    u = i['base']['uniform']
    assert float(u.min()) == 0.0 and float(u.max()) == 1 - 2.0 ** -24 and bool((u == 2.0 ** -24).any()) and bool((u < 1).all())
    if C > 2:
        assert float(u[S.TIE, 1]) == float(u[S.TIE, 2]) and float(i['base']['pred_v'][S.TIE, 1]) == float(i['base']['pred_v'][S.TIE, 2])
    # an empty graph gives 0
    e = S.SIZES.index(0)
    for op in ('likelihood_terms', 'likelihood_prior'):
        r = S.reference(op, ('base', C), F64)
        assert float(r['kl_pos'][e]) == 0 and float(r['kl_v'][e]) == 0
    # the head's rows: pre-activations from -100 to 100, both sides of the softplus threshold, beyond fp32's exp overflow, a zero row
    h, grp = S.head_rows(C)
    pre = S.head_preact(S.state_dict(C), h, F64)
    assert float(pre.min()) < -99 and float(pre.max()) > 99 and not bool(h[5].any())
    assert bool(((pre > 15) & (pre < 20)).any()) and bool(((pre > 20) & (pre < 25)).any()) and bool(((pre < -20) & (pre > -100)).any())
    near = pre[grp == S.HEAD_TARGETS.index(20.5)]
    assert 20 < float(near.max()) < 21
    for n in S.HEAD_ROWS[1:]:
        assert n > 5               # the zero row is among them


@pytest.mark.parametrize('case', S.CASE_IDS, ids=S.case_id)
def test_clean_restatement_passes_and_margins_are_clear(case):
    """The fp32 restatement itself keeps the rule on every operation (it is 1 r64 away), and at most 1 % of the case's atoms sit under the
    type margin of any draw: an input change cannot hide a kernel behind the margin."""
    for op in S.OPS:
        for out, ok, d, r64, bound, why in S.judge(op, case, S.reference(op, case, F32)):
            assert ok, (op, out, d, r64, bound, why)
            if out == 'v':
                assert d <= S.UNDER_CAP, (op, d)
                tie = S.inputs(case)['tie']
                f64 = S.reference(op, case, F64)
                if tie is not None and f64['score'] is not None and not bool(f64['forced'][tie]):
                    top = f64['score'][tie].topk(2)
                    assert float(top.values[0] - top.values[1]) == 0 and sorted(top.indices.tolist()) == [1, 2] and int(f64['v'][tie]) == 1


# ------------------------------------------------------------------------------------------ the rule rejects wrong kernels
# defect -> (operation, case, output) that must reject it
CAUGHT_BY = {
    'tm1_unclamped': ('posterior_plain', ('all0', 13), 'log_post'),
    'tm1_is_t': ('likelihood_terms', ('base', 16), 'kl_v'),
    'lnk_dropped': ('renoise_renoise1', ('base', 2), 'log_post'),
    'noise_at_last': ('posterior_prog_last', ('sat100', 13), 'pos'),
    'first64': ('likelihood_terms', ('all0', 13), 'kl_pos'),
    'mean_div64': ('likelihood_prior', ('base', 13), 'kl_pos'),
    'count_unclamped': ('likelihood_terms', ('perfect', 2), 'kl_v'),
    'decoder_swapped': ('likelihood_terms', ('all0_perfect', 16), 'kl_pos'),
    'logvar_full': ('posterior_plain', ('all999', 2), 'pos'),
    'last_max': ('perturb', ('base', 13), 'v'),
}


_NON_PROGRAM = ('posterior_plain', 'posterior_fixed', 'posterior_guided', 'posterior_noise')
_PROGRAM = tuple(f'posterior_{f}' for f in S.FORMS if f.startswith('prog_'))
_DRAWS = _NON_PROGRAM + _PROGRAM + ('renoise_renoise1', 'renoise_renoise_0_999', 'perturb')
# defect -> operation -> how many of the 21 cases reject it there (every other operation: none).  18: the cases with a graph at t = 0; 15: those
# with a graph at t > 0; 14: those with C > 2 (room for the planted tie); 12: perturb sees a dropped ln K only through a type that flips.
SWEEP = {
    'tm1_unclamped': {**{o: 18 for o in _NON_PROGRAM}, 'likelihood_terms': 18},
    'tm1_is_t': {**{o: 15 for o in _NON_PROGRAM}, 'likelihood_terms': 12},
    'lnk_dropped': {**{o: 21 for o in _DRAWS}, 'perturb': 12, 'likelihood_terms': 21, 'likelihood_prior': 21},
    'noise_at_last': {**{o: 18 for o in _NON_PROGRAM}, 'posterior_prog_last': 21, 'posterior_prog_fixed_last': 21},
    'first64': {'likelihood_terms': 18, 'likelihood_prior': 21},
    'mean_div64': {'likelihood_terms': 21, 'likelihood_prior': 21},
    'count_unclamped': {'likelihood_terms': 21, 'likelihood_prior': 21},
    'decoder_swapped': {'likelihood_terms': 21},
    'logvar_full': {**{o: 15 for o in _NON_PROGRAM}, **{o: 21 for o in _PROGRAM if not o.endswith('_last')}},
    'last_max': {o: 14 for o in _DRAWS},
}


@pytest.mark.parametrize('defect', [d for d in S.DEFECTS if d != 'softplus_no_threshold'])
def test_rule_rejects(defect):
    """The named case rejects the defect, and over every operation and case the defect is rejected exactly where SWEEP says (the table of
    EXPERIMENTS.md): nowhere it cannot show, everywhere it can."""
    op, case, out = CAUGHT_BY[defect]
    rows = {r[0]: r for r in S.judge(op, case, S.reference(op, case, F32, defect))}
    assert not rows[out][1], (defect, rows[out])
    caught = {o: [S.case_id(c) for c in S.CASE_IDS if not all(r[1] for r in S.judge(o, c, S.reference(o, c, F32, defect)))] for o in S.OPS}
    assert {o: len(c) for o, c in caught.items() if c} == SWEEP[defect], caught
    if defect == 'last_max':         # the planted tie shows it in every draw of every case that has room for one
        assert all(c == [S.case_id(x) for x in S.CASE_IDS if x[1] > 2] for c in caught.values() if c)
    if defect in ('tm1_unclamped', 'noise_at_last'):      # all999 has no graph at t = 0
        assert all('all999' not in x for x in caught['posterior_plain'])
    if defect in ('tm1_is_t', 'logvar_full'):             # at t = 0 t - 1 clamps to t, and no noise is added
        assert all(not x.startswith('all0') for x in caught['posterior_plain'])


def test_rule_rejects_count_unclamped_as_nan():
    got = S.reference('likelihood_terms', ('base', 13), F32, 'count_unclamped')
    assert bool(torch.isnan(got['kl_pos'][S.SIZES.index(0)]))
    ok, d64, r64, bound = S.verdict(got['kl_pos'], *(S.reference('likelihood_terms', ('base', 13), d)['kl_pos'] for d in (F32, F64)), S.FLOOR['kl'], rel=True)
    assert not ok and d64 != d64


@pytest.mark.parametrize('C', S.CLASSES)
def test_rule_rejects_softplus_without_threshold(C):
    """log1p(exp(x)) is x to fp32 precision for 20 < x < 88 and overflows beyond: the rows with pre-activations of 100 show it, the others cannot"""
    sd = S.state_dict(C)
    h, grp = S.head_rows(C)
    f32, f64 = S.v_inference(sd, h, F32), S.v_inference(sd, h, F64)
    bad = S.v_inference(sd, h, F32, 'softplus_no_threshold')
    for n in S.HEAD_ROWS:
        assert not S.verdict(bad[:n], f32[:n], f64[:n], S.head_floor, groups=grp[:n])[0], n
        assert S.verdict(f32[:n], f32[:n], f64[:n], S.head_floor, groups=grp[:n])[0], n
    quiet = grp != 0
    assert S.verdict(bad[quiet], f32[quiet], f64[quiet], S.head_floor, groups=grp[quiet])[0]


def test_rule_rejects_three_r64():
    """A result 3 r64 from float64 is rejected wherever r64 is above a third of the floor, and the floor is what lets it pass elsewhere."""
    rejected, under_floor = [], []
    for case in S.CASE_IDS:
        for op in ('posterior_plain', 'likelihood_terms', 'perturb'):
            f32, f64 = S.reference(op, case, F32), S.reference(op, case, F64)
            for out, (floor, rel) in S.OUTPUTS.items():
                if out not in f64:
                    continue
                floor = S.floor_of(floor, case[1])
                r64, bound = S.bounds(f32[out], f64[out], floor, rel)
                den = f64[out].abs().clamp(min=S.KL_DEN) if rel else torch.ones_like(f64[out])
                k = int((f32[out].double() - f64[out]).abs().div(den).argmax())          # move the element that sets r64, away from float64
                got = f64[out].clone()
                sign = 1.0 if float((f32[out].double() - f64[out]).flatten()[k]) >= 0 else -1.0
                got.view(-1)[k] += sign * 3.0 * r64 * float(den.flatten()[k])
                bound = float(bound.flatten()[k])                                         # the moved element's own
                ok = S.verdict(got, f32[out], f64[out], floor, rel)[0]
                assert ok == (3.0 * r64 <= bound * (1 + 1e-9)), (case, op, out, r64, bound)
                (under_floor if ok else rejected).append((S.case_id(case), op, out))
    assert ('sat100-C13', 'posterior_plain', 'pos') in rejected and ('sat100-C13', 'posterior_plain', 'log_v0') in rejected
    assert ('all999-C13', 'likelihood_terms', 'kl_pos') in rejected and ('base-C13', 'likelihood_terms', 'kl_v') in rejected
    assert ('all999-C13', 'perturb', 'pos') in rejected
    assert len(rejected) > len(under_floor) / 4
