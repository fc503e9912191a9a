"""The diffusion-step and likelihood kernels (csrc/misc.hip, csrc/likelihood.hip) restated in plain torch, generic in dtype, and the one list
of cases that tests/test_step_ref_host.py (CPU) and tests/test_gpu_step_float64.py (MI355X) share (TEST INFRASTRUCTURE).

Every function runs at fp32 and at float64 on THE SAME fp32 inputs: the schedule tables and the program rows are the fp32 tensors the native
handle receives, upcast; the one-hot, log(1e-30) and ln K are formed in the working dtype.  The formulas are those of oracle/restatement.py and
tests/_program_ref.py (which the host test pins this file to on the recorded fixtures); nothing of their code is imported here.

The rule, for one output of one case:

    r64 = max |fp32 restatement - float64 restatement|,  d64 = max |HIP - float64 restatement|,  pass when d64 <= max(floor, 2 r64)

with the floors of FLOOR and floor_of below; the per-graph likelihood outputs are measured as |x - f64| / max(|f64|, 1e-2).  Sampled types come from the
float64 argmax: an atom whose float64 top-two score margin exceeds MARGIN must agree, an atom under it must pick one of the two top classes, at
most UNDER_CAP of a case's atoms may be under it, and the planted exact tie must give the lower index.

`defect=` plants one wrong line (DEFECTS) into a restatement: the host test shows with them that the rule rejects wrong kernels.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from _tol import TOL_FWD, close
from oracle import weights
from targetdiff_amd import schedule as SCH
from targetdiff_amd.schedule import TimeProgram

T = 1000
SIZES = [1, 63, 64, 65, 130, 0, 7]         # an empty graph in the middle, one on each side of the 64-lane stride, two 128-atom workgroups crossed
B = len(SIZES)
N = sum(SIZES)
PTR = np.concatenate([[0], np.cumsum(SIZES)]).tolist()
BATCH = torch.repeat_interleave(torch.arange(B), torch.tensor(SIZES))
CLASSES = (13, 16, 2)                       # 16 = TD_MAXC: no padding lanes
HEAD_ROWS = (1, 7, 8, 9, 330)               # rows of v_inference / embed_ligand: the head kernel takes 8 rows per workgroup

MARGIN = 1e-4                               # float64 top-two margin of gumbel + log p above which the sampled type must agree
UNDER_CAP = 0.01                            # share of a case's atoms that may sit under it
FLOOR = {'pos': 2e-6, 'log_v0': 1e-5, 'log_post': 2e-5, 'fwd': TOL_FWD, 'kl': 2e-6}       # 'kl': on the relative scale
FACTOR = 2.0
KL_DEN = 1e-2
HEAD_K = 128                                # terms of one dot product of the head


def floor_of(name, C):
    """The floor of one output: a number, or for 'kl_v' a function of the float64 result that gives one floor per graph.  A type KL is a sum
    of p (log p_true - log p_model) over log-probabilities of size ln K, each known to half an fp32 ulp at best, so no fp32 evaluation holds
    it closer than one ulp of that size, 2^-23 max(1, ln K) nats -- 1.2e-7 (K = 2) to 3.3e-7 (K = 16).  On the relative scale that is
    max(2e-6, ulp / max(|f64|, 1e-2)): 2e-6 wherever kl_v is above 0.06 .. 0.17, more only on graphs whose kl_v is smaller (EXPERIMENTS.md,
    "Step and likelihood kernels against float64")."""
    if name == 'kl_v':
        ulp = 2.0 ** -23 * max(1.0, math.log(C))
        return lambda f64: (ulp / f64.double().abs().clamp(min=KL_DEN)).clamp(min=FLOOR['kl'])
    return FLOOR[name]


def head_floor(f64):
    """The floor of the head's logits for rows of one scale: TOL_FWD, or where the logits are large the rounding of HEAD_K fp32 accumulations
    into a running sum of the outputs' size, added as a random walk -- sqrt(128) 2^-24 max |logit| (torch's blocked sums, which set r64, do not
    take that walk; the kernel's k-ascending fmaf chain does)."""
    return max(TOL_FWD, math.sqrt(HEAD_K) * 2.0 ** -24 * float(f64.abs().max())) if f64.numel() else TOL_FWD

T_SETS = {'mixed': [2, 0, 999, 1, 537, 998, 0], 'all0': [0] * B, 'all999': [999] * B}
# name -> time steps, logits, predicted positions
CASES = {
    'base': ('mixed', 'x2', 'near'),
    'sat30': ('mixed', 'x30', 'near'),
    'sat100': ('mixed', 'x100', 'far'),
    'perfect': ('mixed', 'perfect', 'exact'),
    'all0': ('all0', 'x2', 'near'),
    'all0_perfect': ('all0', 'perfect', 'exact'),
    'all999': ('all999', 'x30', 'far'),
}
CASE_IDS = [(name, C) for name in CASES for C in CLASSES]


def case_id(case):
    return f'{case[0]}-C{case[1]}'


# planted uniform draws: (atom, class or -1 for the last, value); the tie atom's row is set apart (TIE)
U_LO, U_HI = 2.0 ** -24, 1.0 - 2.0 ** -24
PLANTED = [(0, 0, 0.0), (64, 1, U_LO), (129, 0, U_HI), (N - 1, -1, U_HI), (N - 1, 0, 0.0)]
TIE = PTR[3] + 5          # an atom of the graph without known atoms: classes 1 and 2 tie exactly at the top (C > 2), class 1 must win
FULL_GRAPH, FREE_GRAPH = 2, 3               # every atom known / no atom known

DEFECTS = ('tm1_unclamped', 'tm1_is_t', 'lnk_dropped', 'noise_at_last', 'first64', 'mean_div64', 'count_unclamped', 'decoder_swapped',
           'logvar_full', 'last_max', 'softplus_no_threshold')


# ------------------------------------------------------------------------------------------ the restatement
def _lae(a, b):
    m = torch.max(a, b)
    return m + torch.log(torch.exp(a - m) + torch.exp(b - m))


def _log_onehot(v, K, dtype):
    return torch.log(F.one_hot(v, K).to(dtype).clamp(min=1e-30))


def _ln(K, dtype):
    return torch.log(torch.tensor(float(K), dtype=dtype))


def _gumbel(u, dtype):
    return -torch.log(-torch.log(u.to(dtype) + 1e-30) + 1e-30)


def _argmax(score, defect):
    if defect == 'last_max':
        return score.shape[-1] - 1 - score.flip(-1).argmax(dim=-1)
    return score.argmax(dim=-1)           # the first maximum


def _tm1(tb, defect):
    if defect == 'tm1_unclamped':
        return tb - 1                      # -1 reads the table's last entry
    if defect == 'tm1_is_t':
        return tb
    return (tb - 1).clamp(min=0)


def x0_of_noise(sched, tb, out, x_t, dtype):
    """model_mean_type 'noise': the network's output is x_t + eps, x0 = rc[t] x_t - rm1[t] (out - x_t).  tb: [N] per-atom time step."""
    rc = sched['sqrt_recip_alphas_cumprod'].to(dtype)[tb].unsqueeze(-1)
    rm1 = sched['sqrt_recipm1_alphas_cumprod'].to(dtype)[tb].unsqueeze(-1)
    return rc * x_t.to(dtype) - rm1 * (out.to(dtype) - x_t.to(dtype))


def _posterior_core(co, last, tb, pos, v, pred_pos, pred_v, noise, uniform, K, dtype, sched, mean_type, mask, x0c, v0, x0_shift, defect):
    """co: the step's coefficients, each [N, 1] or a 0-d tensor in `dtype`; last: [N] bool, the step ends on clean data."""
    pos, noise, pred_v = pos.to(dtype), noise.to(dtype), pred_v.to(dtype)
    x0 = x0_of_noise(sched, tb, pred_pos, pos, dtype) if mean_type == 'noise' else pred_pos.to(dtype)
    if x0_shift is not None:
        x0 = x0 + x0_shift.to(dtype)
    lastc = last.unsqueeze(-1)
    sd = torch.exp((1.0 if defect == 'logvar_full' else 0.5) * co['logvar'])
    nz = torch.ones_like(lastc) if defect == 'noise_at_last' else ~lastc
    pos_next = co['c0'] * x0 + co['ct'] * pos + nz.to(dtype) * sd * noise
    lnK = _ln(K, dtype)
    log_v0 = F.log_softmax(pred_v, dim=-1)
    q_prev = _lae(log_v0 + co['log_ca'], co['log_1mca'] - (0.0 if defect == 'lnk_dropped' else lnK))
    q_one = _lae(_log_onehot(v, K, dtype) + co['log_a'], co['log_1ma'] - lnK)
    un = q_prev + q_one
    log_post = un - torch.logsumexp(un, dim=-1, keepdim=True)
    forced = torch.zeros_like(last)
    if mask is not None:                   # known atoms: a forward-diffused copy of their state at the level the step ends on
        a, l0 = co['abar_to'], _log_onehot(v0, K, dtype)
        xk = a.sqrt() * x0c.to(dtype) + (1.0 - a).sqrt() * noise
        lqk = _lae(l0 + co['log_ca'], co['log_1mca'] - lnK)
        if defect != 'noise_at_last':
            xk, lqk = torch.where(lastc, x0c.to(dtype), xk), torch.where(lastc, l0, lqk)
            forced = mask & last
        pos_next = torch.where(mask.unsqueeze(-1), xk, pos_next)
        log_post = torch.where(mask.unsqueeze(-1), lqk, log_post)
    score = _gumbel(uniform, dtype) + log_post
    v_next = torch.where(forced, v0, _argmax(score, defect)) if mask is not None else _argmax(score, defect)
    return dict(pos=pos_next, v=v_next, log_v0=log_v0, log_post=log_post, score=score, forced=forced)


def posterior(sched, t, pos, v, pred_pos, pred_v, batch, noise, uniform, K, dtype, mean_type='C0', mask=None, x0c=None, v0=None,
              x0_shift=None, defect=None):
    """One reverse step t -> t - 1 from the per-t tables (td_posterior_step and its _fixed / _guided forms).  t: int64 [B]."""
    tb = t[batch]
    tm1 = _tm1(tb, defect)
    g = lambda k, i: sched[k].to(dtype)[i].unsqueeze(-1)
    co = dict(c0=g('posterior_mean_c0_coef', tb), ct=g('posterior_mean_ct_coef', tb), logvar=g('posterior_logvar', tb),
              log_a=g('log_alphas_v', tb), log_1ma=g('log_one_minus_alphas_v', tb), log_ca=g('log_alphas_cumprod_v', tm1),
              log_1mca=g('log_one_minus_alphas_cumprod_v', tm1))
    if mask is not None:
        co['abar_to'] = g('alphas_cumprod', tm1)
    return _posterior_core(co, tb == 0, tb, pos, v, pred_pos, pred_v, noise, uniform, K, dtype, sched, mean_type, mask, x0c, v0,
                           x0_shift, defect)


def posterior_program(row, t, pos, v, pred_pos, pred_v, batch, noise, uniform, K, dtype, sched=None, mean_type='C0', mask=None, x0c=None,
                      v0=None, x0_shift=None, defect=None):
    """One denoise slot of a time program: the coefficients are the slot's fp32 row (td_posterior_step_program); t only names the level the
    network ran at ('noise')."""
    r = row.to(dtype)
    co = dict(c0=r[SCH.C0], ct=r[SCH.CT], logvar=r[SCH.LOGVAR], log_a=r[SCH.LOG_A], log_1ma=r[SCH.LOG_1MA], log_ca=r[SCH.LOG_CA],
              log_1mca=r[SCH.LOG_1MCA], abar_to=r[SCH.ABAR_TO])
    last = torch.full((pos.shape[0],), bool(row[SCH.LAST] != 0))
    return _posterior_core(co, last, t[batch], pos, v, pred_pos, pred_v, noise, uniform, K, dtype, sched, mean_type, mask, x0c, v0,
                           x0_shift, defect)


def renoise(row, pos, v, noise, uniform, K, dtype, defect=None):
    """One renoise slot s -> t (td_renoise_step); uniform None: the types stay."""
    r = row.to(dtype)
    rho = r[SCH.RHO]
    pos_next = rho.sqrt() * pos.to(dtype) + (1.0 - rho).sqrt() * noise.to(dtype)
    l0 = _log_onehot(v, K, dtype)
    lq = _lae(l0 + r[SCH.LOG_R], r[SCH.LOG_1MR] - (0.0 if defect == 'lnk_dropped' else _ln(K, dtype)))
    if uniform is None:
        return dict(pos=pos_next, v=v.clone(), log_v0=l0, log_post=lq, score=None, forced=torch.ones(len(v), dtype=torch.bool))
    score = _gumbel(uniform, dtype) + lq
    return dict(pos=pos_next, v=_argmax(score, defect), log_v0=l0, log_post=lq, score=score, forced=torch.zeros(len(v), dtype=torch.bool))


def _q_v_pred(sched, log_v0, tb, K, dtype, defect=None):
    return _lae(log_v0 + sched['log_alphas_cumprod_v'].to(dtype)[tb].unsqueeze(-1),
                sched['log_one_minus_alphas_cumprod_v'].to(dtype)[tb].unsqueeze(-1) - (0.0 if defect == 'lnk_dropped' else _ln(K, dtype)))


def perturb(sched, t, pos, v, batch, noise, uniform, K, dtype, defect=None):
    """The forward-process sample x_t, v_t at per-graph t (td_perturb)."""
    tb = t[batch]
    a = sched['alphas_cumprod'].to(dtype)[tb].unsqueeze(-1)
    pos_t = a.sqrt() * pos.to(dtype) + (1.0 - a).sqrt() * noise.to(dtype)
    score = _gumbel(uniform, dtype) + _q_v_pred(sched, _log_onehot(v, K, dtype), tb, K, dtype, defect)
    return dict(pos=pos_t, v=_argmax(score, defect), score=score, forced=torch.zeros(len(v), dtype=torch.bool))


def _q_v_posterior(sched, log_v0, log_vt, tb, K, dtype, defect):
    un = _q_v_pred(sched, log_v0, _tm1(tb, defect), K, dtype, defect) + _lae(
        log_vt + sched['log_alphas_v'].to(dtype)[tb].unsqueeze(-1), sched['log_one_minus_alphas_v'].to(dtype)[tb].unsqueeze(-1) - _ln(K, dtype))
    return un - torch.logsumexp(un, dim=-1, keepdim=True)


def _graph_mean(x, batch, nb, defect=None):
    cnt = torch.bincount(batch, minlength=nb)
    if defect == 'first64':                # only the first wave-load of a graph's atoms
        first = torch.tensor(np.concatenate([[0], np.cumsum(cnt.numpy())]))[batch]
        x = x * (torch.arange(len(batch)) - first < 64).to(x.dtype)
    s = torch.zeros(nb, dtype=x.dtype).index_add_(0, batch, x)
    if defect == 'mean_div64':
        return s / 64.0
    return s / (cnt if defect == 'count_unclamped' else cnt.clamp(min=1)).to(x.dtype)


def likelihood_terms(sched, t, x0, xt, v0, vt, pred_pos, pred_v, batch, K, dtype, defect=None):
    """kl_pos, kl_v per graph (td_likelihood_terms): KL of the true and the model posterior in bits / nats for t > 0, decoder NLL at t == 0."""
    nb = int(t.numel())
    tb = t[batch]
    x0, xt, pred_pos, pred_v = x0.to(dtype), xt.to(dtype), pred_pos.to(dtype), pred_v.to(dtype)
    g = lambda k: sched[k].to(dtype)[tb].unsqueeze(-1)
    c0, ct, logvar = g('posterior_mean_c0_coef'), g('posterior_mean_ct_coef'), g('posterior_logvar')
    model_mean, true_mean = c0 * pred_pos + ct * xt, c0 * x0 + ct * xt
    kl_pos = (0.5 * (-1.0 + logvar - logvar + torch.exp(logvar - logvar) + (true_mean - model_mean) ** 2 * torch.exp(-logvar))).sum(-1) / math.log(2.0)
    log_scales = 0.5 * logvar
    nll_pos = -(-((x0 - model_mean) ** 2) / (2 * torch.exp(log_scales * 2)) - log_scales - math.log(math.sqrt(2 * math.pi))).sum(-1)
    dec = tb == 0
    if defect == 'decoder_swapped':
        dec = ~dec
    log_v0, log_vt = _log_onehot(v0, K, dtype), _log_onehot(vt, K, dtype)
    log_model = _q_v_posterior(sched, F.log_softmax(pred_v, dim=-1), log_vt, tb, K, dtype, defect)
    log_true = _q_v_posterior(sched, log_v0, log_vt, tb, K, dtype, defect)
    kl_v = (log_true.exp() * (log_true - log_model)).sum(dim=1)
    nll_v = -(log_v0.exp() * log_model).sum(dim=1)
    return _graph_mean(torch.where(dec, nll_pos, kl_pos), batch, nb, defect), _graph_mean(torch.where(dec, nll_v, kl_v), batch, nb, defect)


def likelihood_prior(sched, x0, v_index, batch, K, nb, dtype, defect=None):
    """kl_pos_prior, kl_v_prior per graph (td_likelihood_prior): the level T - 1 against N(0, 1) and the uniform categorical."""
    a = sched['alphas_cumprod'].to(dtype)[-1]
    mean2 = a.sqrt() * x0.to(dtype)
    logvar2 = torch.log((1.0 - a).sqrt())
    kl = (0.5 * (-1.0 + logvar2 - 0.0 + torch.exp(0.0 - logvar2) + (0.0 - mean2) ** 2 * torch.exp(-logvar2))).sum(-1)
    log_q = _q_v_pred(sched, _log_onehot(v_index, K, dtype), torch.full_like(batch, len(sched['alphas_cumprod']) - 1), K, dtype, defect)
    kl_v = (log_q.exp() * (log_q + _ln(K, dtype))).sum(dim=1)
    return _graph_mean(kl, batch, nb, defect), _graph_mean(kl_v, batch, nb, defect)


def head_preact(sd, h, dtype):
    return F.linear(h.to(dtype), sd['v_inference.0.weight'].to(dtype), sd['v_inference.0.bias'].to(dtype))


def v_inference(sd, h, dtype, defect=None):
    """Linear -> ShiftedSoftplus (softplus with threshold 20, minus ln 2) -> Linear on free-standing rows (td_v_inference)."""
    y = head_preact(sd, h, dtype)
    sp = torch.log1p(torch.exp(y)) if defect == 'softplus_no_threshold' else F.softplus(y)
    return F.linear(sp - math.log(2.0), sd['v_inference.2.weight'].to(dtype), sd['v_inference.2.bias'].to(dtype))


def embed_ligand(sd, v, dtype):
    """[Linear(one_hot(v)) ; 1] (td_embed_ligand): 127 embedding columns and the node indicator."""
    W, b = sd['ligand_atom_emb.weight'].to(dtype), sd['ligand_atom_emb.bias'].to(dtype)
    e = F.linear(F.one_hot(v, W.shape[1]).to(dtype), W, b)
    return torch.cat([e, torch.ones(len(v), 1, dtype=dtype)], dim=-1)


# ------------------------------------------------------------------------------------------ models, schedules, program rows
@functools.lru_cache(maxsize=None)
def state_dict(C):
    return weights.make_state_dict(2021, ligand_dim=C)


@functools.lru_cache(maxsize=None)
def mirror(mean_type='C0'):
    """The package's parameter holder on the CPU: the owner of the fp32 schedule tables the native handle receives."""
    from targetdiff_amd.models import ScorePosNet3D
    return ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG, num_diffusion_timesteps=T, model_mean_type=mean_type), 27, 13).eval()


@functools.lru_cache(maxsize=None)
def schedules():
    from targetdiff_amd import capi
    m = mirror()
    return {k: getattr(m, k).detach().float().clone() for k in capi.SCHEDULE_ORDER + capi.SCHEDULE_OPTIONAL}


def native_config(C, mean_type='C0'):
    """A one-layer handle's configuration, as _native_with_layers of tests/test_gpu_parity.py builds it"""
    return dict(hidden_dim=128, n_heads=16, knn=32, num_layers=1, num_r_gaussian=20, edge_feat_dim=4, protein_feat_dim=27,
                ligand_num_classes=C, num_timesteps=T, model_mean_type=mean_type)


# one program that holds every kind of slot: (kind, from, to)
_PROGRAM = [(SCH.DENOISE, 999, 998), (SCH.DENOISE, 998, 868), (SCH.DENOISE, 868, 0), (SCH.RENOISE, 0, 999), (SCH.DENOISE, 999, 998),
            (SCH.RENOISE, 998, 999), (SCH.DENOISE, 999, 0), (SCH.DENOISE, 0, -1)]
DENOISE_ROWS = {'unit': 0, 'stride130': 1, 'last': 7}          # 1 level, 130 levels, the last slot
RENOISE_ROWS = {'renoise1': 5, 'renoise_0_999': 3}             # 1 level (rho next to 1), level 0 to 999


@functools.lru_cache(maxsize=None)
def program_rows():
    """name -> (fp32 row [ROW] of TimeProgram.tables, the level the slot starts from)"""
    kind, a, b = zip(*_PROGRAM)
    prog = TimeProgram(T, kind, a, b)
    tab = torch.from_numpy(prog.tables(mirror()))
    return {name: (tab[i].clone(), int(prog.t_from[i])) for name, i in {**DENOISE_ROWS, **RENOISE_ROWS}.items()}


# ------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def known_atoms():
    """a mask over a third of the atoms: every atom of FULL_GRAPH, none of FREE_GRAPH"""
    g = torch.Generator().manual_seed(515)
    m = torch.rand(N, generator=g) < 0.23
    m[BATCH == FULL_GRAPH] = True
    m[BATCH == FREE_GRAPH] = False
    return m


@functools.lru_cache(maxsize=None)
def inputs(case):
    """Every input of one case, fp32 / int64 on the CPU, from seeds."""
    name, C = case
    tset, logit, posk = CASES[name]
    g = torch.Generator().manual_seed(9000 + 100 * list(CASES).index(name) + C)
    rn = lambda *s: torch.randn(*s, generator=g)
    scale = 30.0 if posk == 'far' else 1.0
    x0 = 2.0 * scale * rn(N, 3)
    x_t = x0 + 0.5 * scale * rn(N, 3)
    pred_pos = x0.clone() if posk == 'exact' else x_t + 0.3 * scale * rn(N, 3)
    v0, v_t = torch.randint(0, C, (N,), generator=g), torch.randint(0, C, (N,), generator=g)
    if logit == 'perfect':
        pred_v = 60.0 * F.one_hot(v0, C).float()
    else:
        pred_v = float(logit[1:]) * rn(N, C)
    uniform = torch.rand(N, C, generator=g)
    for at, c, val in PLANTED:
        uniform[at, c] = val
    tie = C > 2
    if tie:        # classes 1 and 2 share the top score exactly, in fp32 and in float64: equal logits, equal draws, neither the atom's type
        v0[TIE] = v_t[TIE] = 0
        if logit == 'perfect':
            pred_v[TIE] = 0.0
        pred_v[TIE, 1] = pred_v[TIE, 2] = float(pred_v[TIE].max()) + 5.0
        uniform[TIE] = 0.5
        uniform[TIE, 0] = U_LO
        uniform[TIE, 1] = uniform[TIE, 2] = U_HI
    return dict(C=C, t=torch.tensor(T_SETS[tset]), x0=x0, x_t=x_t, pred_pos=pred_pos, v0=v0, v_t=v_t, pred_v=pred_v, noise=rn(N, 3),
                uniform=uniform, x0_shift=0.2 * scale * rn(N, 3), mask=known_atoms(), tie=TIE if tie else None)


FORMS = ('plain', 'fixed', 'guided', 'noise') + tuple(f'prog_{r}' for r in DENOISE_ROWS) + tuple(f'prog_fixed_{r}' for r in DENOISE_ROWS)


def posterior_call(case, form):
    """The arguments of one posterior form as capi.NativeModel.posterior_step names them (CPU tensors), the mean type, and a function
    (dtype, defect) -> restatement.  `t` of a program form is the level the slot starts from, on every graph."""
    i = inputs(case)
    kw = dict(t=i['t'], ligand_pos=i['x_t'], ligand_v=i['v_t'], pred_pos=i['pred_pos'], pred_v=i['pred_v'], noise=i['noise'],
              uniform=i['uniform'])
    fixed = dict(fixed_mask=i['mask'], fixed_pos=i['x0'], fixed_v=i['v0'])
    rkw = {}
    mean_type = 'noise' if form == 'noise' else 'C0'
    if form in ('fixed',) or form.startswith('prog_fixed_'):
        kw.update(fixed)
        rkw.update(mask=i['mask'], x0c=i['x0'], v0=i['v0'])
    if form == 'guided':
        kw['x0_shift'] = i['x0_shift']
        rkw['x0_shift'] = i['x0_shift']
    if form.startswith('prog_'):
        row, t_from = program_rows()[form.split('_')[-1]]
        kw['prog_row'] = row
        kw['t'] = torch.full((B,), t_from)

        def ref(dtype, defect=None):
            return posterior_program(row, kw['t'], i['x_t'], i['v_t'], i['pred_pos'], i['pred_v'], BATCH, i['noise'], i['uniform'], i['C'],
                                     dtype, sched=schedules(), defect=defect, **rkw)
    else:
        def ref(dtype, defect=None):
            return posterior(schedules(), i['t'], i['x_t'], i['v_t'], i['pred_pos'], i['pred_v'], BATCH, i['noise'], i['uniform'], i['C'],
                             dtype, mean_type=mean_type, defect=defect, **rkw)
    return kw, mean_type, ref


RENOISE_OPS = tuple(f'renoise_{r}' for r in RENOISE_ROWS) + tuple(f'renoise_{r}_pos_only' for r in RENOISE_ROWS)
OPS = tuple(f'posterior_{f}' for f in FORMS) + RENOISE_OPS + ('perturb', 'likelihood_terms', 'likelihood_prior')
# output -> (its floor, measured on the relative scale of the likelihood outputs?)
OUTPUTS = {'pos': ('pos', False), 'log_v0': ('log_v0', False), 'log_post': ('log_post', False), 'kl_pos': ('kl', True), 'kl_v': ('kl_v', True)}


def expected_outputs(op):
    """what one operation must return: judge fails on a missing one"""
    if op.startswith('likelihood_'):
        return ('kl_pos', 'kl_v')
    if op == 'perturb' or op.endswith('_pos_only'):         # pos_only: the kernel writes no log-probabilities
        return ('pos', 'v')
    return ('pos', 'log_v0', 'log_post', 'v')


def _reference(op, case, dtype, defect=None):
    i = inputs(case)
    C = i['C']
    if op.startswith('posterior_'):
        return posterior_call(case, op[len('posterior_'):])[2](dtype, defect)
    if op.startswith('renoise_'):
        po = op.endswith('_pos_only')
        row = program_rows()[op[len('renoise_'):-len('_pos_only')] if po else op[len('renoise_'):]][0]
        return renoise(row, i['x_t'], i['v_t'], i['noise'], None if po else i['uniform'], C, dtype, defect)
    if op == 'perturb':
        return perturb(schedules(), i['t'], i['x0'], i['v0'], BATCH, i['noise'], i['uniform'], C, dtype, defect)
    if op == 'likelihood_terms':
        kp, kv = likelihood_terms(schedules(), i['t'], i['x0'], i['x_t'], i['v0'], i['v_t'], i['pred_pos'], i['pred_v'], BATCH, C, dtype, defect)
        return dict(kl_pos=kp, kl_v=kv)
    if op == 'likelihood_prior':
        kp, kv = likelihood_prior(schedules(), i['x0'], i['v0'], BATCH, C, B, dtype, defect)
        return dict(kl_pos=kp, kl_v=kv)
    raise KeyError(op)


_cached_reference = functools.lru_cache(maxsize=None)(_reference)


def reference(op, case, dtype, defect=None):
    """The restatement of one operation of one case: a dict of its outputs (shared, do not modify)"""
    return _cached_reference(op, case, dtype) if defect is None else _reference(op, case, dtype, defect)


def judge(op, case, got, asserting=False):
    """Every output of the operation (expected_outputs; `got`: a dict as `reference` returns it, 'v' the sampled types) by the rule and the type
    comparison.  Returns rows (output, passes, d64 or the under-margin share, r64, bound, note); `asserting`: fail at once, through _tol.close."""
    f32, f64 = reference(op, case, torch.float32), reference(op, case, torch.float64)
    what = f'{case_id(case)} {op}'
    missing = [o for o in expected_outputs(op) if o not in got or o not in f64]
    assert not missing, (what, 'outputs missing', missing)
    rows = []
    for out in expected_outputs(op):
        if out == 'v':
            ok, share, why = types_verdict(got['v'], f64, inputs(case)['tie'])
            assert ok or not asserting, (what, 'v', why)
            rows.append(('v', ok, share, 0.0, UNDER_CAP, why))
            continue
        floor, rel = OUTPUTS[out]
        floor = floor_of(floor, case[1])
        if asserting:
            d64, r64, bound = check(got[out], f32[out], f64[out], floor, f'{what} {out}', rel)
            rows.append((out, True, d64, r64, bound, ''))
        else:
            rows.append((out,) + verdict(got[out], f32[out], f64[out], floor, rel) + ('',))
    return rows


HEAD_TARGETS = (100.0, 60.0, 25.0, 20.5, 15.0, 0.0, 3.0)        # the largest |pre-activation| of the row; 0: the all-zero row


@functools.lru_cache(maxsize=None)
def head_rows(C):
    """h [330, 128] (the test takes the first n rows) and the rows' target index: row r is scaled so that its largest |pre-activation| of the
    head's first Linear is HEAD_TARGETS[r % 7] -- [-100, -20], [15, 25] and both sides of the softplus threshold 20 are covered, row 5 is zero."""
    g = torch.Generator().manual_seed(31)
    h = torch.randn(HEAD_ROWS[-1], 128, generator=g)
    grp = torch.arange(len(h)) % len(HEAD_TARGETS)
    tgt = torch.tensor(HEAD_TARGETS)[grp]
    sd = state_dict(C)
    for _ in range(2):                      # the bias makes the pre-activations affine in the scale: a second pass settles it
        m = head_preact(sd, h, torch.float64).abs().max(dim=1).values
        h = h * torch.where(tgt > 0, tgt / m, torch.zeros_like(tgt)).float().unsqueeze(-1)
    return h.contiguous(), grp


# ------------------------------------------------------------------------------------------ the rule
def distance(a, f64, rel=False):
    """max |a - f64|, or that over max(|f64|, KL_DEN); nan where either is not finite and they are not the same"""
    a, f64 = a.detach().cpu().double(), f64.detach().cpu().double()
    if a.numel() == 0:
        return 0.0
    d = (a - f64).abs()
    if rel:
        d = d / f64.abs().clamp(min=KL_DEN)
    return float('nan') if bool(torch.isnan(d).any()) else float(d.max())


def bounds(f32, f64, floor, rel=False):
    """r64 and the bound max(floor, 2 r64) of every element (the floor: a number, or a function of f64 that gives a number or one per element)"""
    assert bool(torch.isfinite(f64).all()), 'the float64 restatement is not finite'
    r64 = distance(f32, f64, rel)
    fl = floor(f64) if callable(floor) else floor
    fl = torch.as_tensor(fl, dtype=torch.float64).expand(f64.shape)
    return r64, fl.clamp(min=FACTOR * r64)


def _weighed(got, f32, f64, floor, rel):
    """(a, b, r64, bound): the rule holds when max |a - b| <= bound.  Where the bound differs per element, every difference is scaled to the
    largest bound, so that one comparison holds each element to its own."""
    got, f64 = got.detach().cpu().double(), f64.detach().cpu().double()
    r64, bound = bounds(f32, f64, floor, rel)
    if f64.numel() == 0:
        return got, f64, r64, float(floor) if not callable(floor) else 0.0
    w = float(bound.max()) / bound / (f64.abs().clamp(min=KL_DEN) if rel else 1.0)
    return got * w, f64 * w, r64, float(bound.max())


def verdict(got, f32, f64, floor, rel=False, groups=None):
    """(passes, d64, r64, bound) of the rule; with `groups` ([rows] int) per group of rows, the worst group's figures (`floor` may then be a
    function of the group's float64 rows)."""
    out = []
    for gi in ([None] if groups is None else sorted(set(groups.tolist()))):
        rows = slice(None) if gi is None else groups == gi
        a, b, r64, bound = _weighed(got[rows], f32[rows], f64[rows], floor, rel)
        d64 = distance(a, b)
        out.append((d64 <= bound, d64, r64, bound))                # nan fails
    return max(out, key=lambda o: (not o[0], o[1] / o[3] if o[1] == o[1] else math.inf))


def check(got, f32, f64, floor, what, rel=False, groups=None):
    """The rule as an assertion through _tol.close, so that the margin lands in the margins table.  Returns (d64, r64, bound) of the worst group."""
    got = got.detach().cpu()
    assert got.shape == f64.shape == f32.shape, (what, got.shape, f32.shape, f64.shape)
    assert bool(torch.isfinite(got).all()), (what, 'not finite where the float64 restatement is')
    worst = (0.0, 0.0, 1.0)
    for gi in ([None] if groups is None else sorted(set(groups.tolist()))):
        rows = slice(None) if gi is None else groups == gi
        a, b, r64, bound = _weighed(got[rows], f32[rows], f64[rows], floor, rel)
        d64 = close(a, b, bound, what if gi is None else (what, 'rows', gi))
        if d64 / bound >= worst[0] / worst[2]:
            worst = (d64, r64, bound)
    return worst


def types_verdict(got_v, ref64, tie=None):
    """Sampled types against the float64 restatement `ref64` (v, score, forced).  Returns (passes, share of atoms under MARGIN, why)."""
    got_v, want = got_v.detach().cpu(), ref64['v']
    n = len(want)
    if n == 0:
        return True, 0.0, ''
    if ref64['score'] is None:
        return bool(torch.equal(got_v, want)), 0.0, 'types moved without a draw'
    top = ref64['score'].topk(2, dim=-1)
    under = (top.values[:, 0] - top.values[:, 1] <= MARGIN) & ~ref64['forced']
    share = float(under.sum()) / n
    clear = ~under
    if not bool(torch.equal(got_v[clear], want[clear])):
        bad = torch.nonzero(got_v[clear] != want[clear]).flatten()
        return False, share, f'{len(bad)} atoms over the margin differ, the first at {int(torch.nonzero(clear).flatten()[bad[0]])}'
    if not bool(((got_v[under] == top.indices[under, 0]) | (got_v[under] == top.indices[under, 1])).all()):
        return False, share, 'an atom under the margin took a class outside the top two'
    if tie is not None and not bool(ref64['forced'][tie]):
        if not bool(under[tie]) or int(want[tie]) != 1:
            return False, share, 'the planted tie is not a tie at the top of the float64 scores'
        if int(got_v[tie]) != 1:
            return False, share, f'the planted tie went to class {int(got_v[tie])}, not to the first maximum'
    if share > UNDER_CAP:
        return False, share, f'{share:.1%} of the atoms under the margin'
    return True, share, ''


def check_types(got_v, ref64, what, tie=None):
    ok, share, why = types_verdict(got_v, ref64, tie)
    assert ok, (what, why)
    return share
