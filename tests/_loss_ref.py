"""The diffusion loss (csrc/loss.hip: td_diffusion_loss) restated in plain torch, generic in dtype, a brute-force integer AUROC (td_auroc), and
the cases tests/test_loss_host.py (CPU) and tests/test_gpu_loss.py (MI355X) share (TEST INFRASTRUCTURE).

The loss is the arithmetic of models/molopt_score_model.py:521-563 after the network call.  It runs at fp32 and at float64 on THE SAME fp32
inputs and is judged by the rule of tests/_step_ref.py, whose helpers, cases (graph sizes, time-step sets, class counts, planted predictions)
and floors it reuses:

    r64 = max |fp32 restatement - float64 restatement|,  d64 = max |HIP - float64 restatement|,  pass when d64 <= max(floor, 2 r64)

per-graph and scalar losses on the relative scale |x - f64| / max(|f64|, 1e-2) with the floors 'kl' / 'kl_v', ligand_v_recon with the floor
'log_v0' (probabilities are at most 1, so the floor of a log-probability covers them), pred_pos_noise with 'pos'.

`defect=` plants one wrong line (DEFECTS, AUROC_DEFECTS): the host test shows with them that the gates reject wrong kernels.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import _step_ref as S

LOSS_V_WEIGHT = 100.0                       # configs/training.yml
MEAN_TYPES = ('C0', 'noise')
DEFECTS = ('target_swapped', 'weight_dropped', 'atom_mean', 'decoder_mask_ignored')
AUROC_DEFECTS = ('ties_as_wins', 'nneg_is_n')
# output -> (floor name of _step_ref.floor_of, measured on the relative scale?)
OUTPUTS = {'loss_pos_graph': ('kl', True), 'loss_v_graph': ('kl_v', True), 'loss_pos': ('kl', True), 'loss_v': ('kl_v', True),
           'loss': ('kl', True), 'pred_pos_noise': ('pos', False), 'ligand_v_recon': ('log_v0', False)}
CASE_IDS = [(name, C) for name in ('base', 'sat30', 'all0', 'all999') for C in S.CLASSES]      # t sets 'mixed', 'all0', 'all999'


def diffusion_loss(sched, t, x0, x_t, noise, v0, v_t, pred_pos, pred_v, batch, K, w, dtype, mean_type='C0', defect=None):
    """Every output of td_diffusion_loss (a dict).  t: int64 [B]."""
    nb = int(t.numel())
    tb = t[batch]
    x0, x_t, noise, pred_pos, pred_v = (a.to(dtype) for a in (x0, x_t, noise, pred_pos, pred_v))
    eps = pred_pos - x_t                                                                  # pred_pos_noise (:522)
    use_noise = (mean_type == 'noise') != (defect == 'target_swapped')
    target, pred = (noise, eps) if use_noise else (x0, pred_pos)                          # :536-541
    sq = ((pred - target) ** 2).sum(-1)
    loss_pos_g = S._graph_mean(sq, batch, nb)
    log_v0, log_vt = S._log_onehot(v0, K, dtype), S._log_onehot(v_t, K, dtype)
    log_model = S._q_v_posterior(sched, F.log_softmax(pred_v, dim=-1), log_vt, tb, K, dtype, None)
    log_true = S._q_v_posterior(sched, log_v0, log_vt, tb, K, dtype, None)
    kl_v = (log_true.exp() * (log_true - log_model)).sum(dim=1)
    nll_v = -(log_v0.exp() * log_model).sum(dim=1)
    dec = torch.zeros_like(tb, dtype=torch.bool) if defect == 'decoder_mask_ignored' else tb == 0
    per_atom_v = torch.where(dec, nll_v, kl_v)
    loss_v_g = S._graph_mean(per_atom_v, batch, nb)
    if defect == 'atom_mean':
        loss_pos, loss_v = sq.mean(), per_atom_v.mean()
    else:
        loss_pos, loss_v = loss_pos_g.mean(), loss_v_g.mean()                             # :543, :551
    wt = torch.tensor(1.0 if defect == 'weight_dropped' else float(w), dtype=dtype)
    return dict(loss_pos_graph=loss_pos_g, loss_v_graph=loss_v_g, loss_pos=loss_pos, loss_v=loss_v, loss=loss_pos + loss_v * wt,
                pred_pos_noise=eps, ligand_v_recon=F.softmax(pred_v, dim=-1))


def _reference(case, mean_type, dtype, defect=None):
    i = S.inputs(case)
    return diffusion_loss(S.schedules(), i['t'], i['x0'], i['x_t'], i['noise'], i['v0'], i['v_t'], i['pred_pos'], i['pred_v'], S.BATCH, i['C'],
                          LOSS_V_WEIGHT, dtype, mean_type, defect)


_cached = functools.lru_cache(maxsize=None)(_reference)


def reference(case, mean_type, dtype, defect=None):
    """the restatement of one kernel-level case (shared, do not modify)"""
    return _cached(case, mean_type, dtype) if defect is None else _reference(case, mean_type, dtype, defect)


def _rows(x):
    x = torch.as_tensor(x).detach().cpu()
    return x.reshape(1) if x.dim() == 0 else x


def judge(got, f32, f64, C, what=None, asserting=False):
    """Every output of OUTPUTS by the rule.  Returns rows (output, passes, d64, r64, bound); `asserting`: through _tol.close."""
    rows = []
    for out, (floor, rel) in OUTPUTS.items():
        fl = S.floor_of(floor, C)
        g, a, b = (_rows(x[out]) for x in (got, f32, f64))              # the scalars as one-element rows
        if asserting:
            d64, r64, bound = S.check(g, a, b, fl, f'{what} {out}', rel)
            rows.append((out, True, d64, r64, bound))
        else:
            rows.append((out,) + S.verdict(g, a, b, fl, rel))
    return rows


def kernel_gate(f32, f64, out, C):
    """the absolute bound the rule puts on one scalar output: max(floor, 2 r64) times the scale max(|f64|, 1e-2)"""
    floor, rel = OUTPUTS[out]
    a, b = _rows(f32[out]), _rows(f64[out])
    r64, bound = S.bounds(a, b, S.floor_of(floor, C), rel)
    scale = b.double().abs().clamp(min=S.KL_DEN) if rel else 1.0
    return float((bound * scale).max())


# ------------------------------------------------------------------------------------------ AUROC
AUROC_N = (2, 63, 64, 65, 257, 1000)
AUROC_KINDS = ('random', 'absent', 'all_equal', 'one_atom')
AUROC_CASES = [(N, C, 'random') for N in AUROC_N for C in S.CLASSES] + [(257, C, k) for C in S.CLASSES for k in AUROC_KINDS[1:]]


@functools.lru_cache(maxsize=None)
def auroc_inputs(case):
    """scores [N, C] fp32 quantised to 5 values (many ties) and labels [N] int64 with at least two classes present.  'absent': class C - 1 has
    no row; 'all_equal': one score everywhere (every AUROC exactly 0.5); 'one_atom': class 1 holds exactly one row."""
    N, C, kind = case
    g = torch.Generator().manual_seed(4000 + 17 * N + C + 1000 * AUROC_KINDS.index(kind))
    scores = torch.randint(0, 5, (N, C), generator=g).float() / 4.0
    labels = torch.randint(0, C, (N,), generator=g)
    labels[0], labels[1] = 0, 1
    if kind == 'absent':
        labels[labels == C - 1] = 0
        labels[1] = 1 if C > 2 else 0
        if C == 2:                       # two classes, one absent: the other holds every row
            labels[:] = 0
    if kind == 'all_equal':
        scores[:] = 0.25
    if kind == 'one_atom':
        labels[labels == 1] = 0
        labels[N // 2] = 1
    return scores.contiguous(), labels.contiguous()


def auroc_counts(scores, labels, defect=None):
    """n_pos [C], pairs2 [C] int64 by brute force: every (positive, negative) pair of every class compared"""
    s, l = np.asarray(scores, dtype=np.float32), np.asarray(labels)
    C = s.shape[1]
    n_pos, pairs2 = np.zeros(C, np.int64), np.zeros(C, np.int64)
    for c in range(C):
        pos, neg = s[l == c, c], s[l != c, c]
        gt = int((pos[:, None] > neg[None, :]).sum())
        eq = int((pos[:, None] == neg[None, :]).sum())
        n_pos[c] = len(pos)
        pairs2[c] = 2 * gt + (2 * eq if defect == 'ties_as_wins' else eq)
    return n_pos, pairs2


def auroc_from_counts(n_pos, pairs2, defect=None):
    """(weighted average, {class: auroc}) in float64, get_auroc's formulas (scripts/train_diffusion.py:22-36)"""
    N = int(np.sum(n_pos))
    per, avg = {}, 0.0
    for c, (n, p2) in enumerate(zip(n_pos.tolist(), pairs2.tolist())):
        if n == 0:
            continue
        n_neg = N if defect == 'nneg_is_n' else N - n
        if n_neg == 0:
            raise ValueError('one class holds every row')
        per[c] = p2 / (2.0 * n * n_neg)
        avg += per[c] * n
    return avg / N, per


def sklearn_auroc(scores, labels):
    """get_auroc with sklearn.metrics.roc_auc_score: (weighted average, {class: auroc})"""
    from sklearn.metrics import roc_auc_score
    y, p = np.asarray(labels), np.asarray(scores, dtype=np.float64)
    per = {int(c): float(roc_auc_score(y == c, p[:, c])) for c in sorted(set(y.tolist()))}
    return sum(per[c] * int(np.sum(y == c)) for c in per) / len(y), per


# ------------------------------------------------------------------------------------------ fixtures of the reference
LOSS_FIXTURES = {'loss_c0': {}, 'loss_noise': dict(model_mean_type='noise'), 'loss_center_none': dict(center_pos_mode='none'),
                 'loss_time_simple': dict(time_emb_dim=8, time_emb_mode='simple')}


def fixture_loss(g, dtype, preds=None, defect=None, mean_type='C0', v_t=None):
    """The restatement on a fixture's recorded state: x0, x_t, v_t, the draws, and either the recorded predictions of that precision or
    `preds` = (pred_pos, pred_v); `v_t` replaces the recorded perturbed types."""
    from targetdiff_amd import capi
    s = '64' if dtype == torch.float64 else ''
    T = lambda k: torch.from_numpy(np.asarray(g[k]))
    sched = {k: v for k, v in S.schedules().items()}
    assert set(sched) >= set(capi.SCHEDULE_ORDER)
    pp, pv = preds if preds is not None else (T('pred_ligand_pos' + s), T('pred_ligand_v' + s))
    x_t = T('x_t64') if s else T('x_t')
    return diffusion_loss(sched, T('time_step').long(), T('x0' + s), x_t, T('noise'), T('ligand_v').long(), T('v_t').long() if v_t is None else v_t, pp, pv,
                          T('batch_ligand').long(), 13, LOSS_V_WEIGHT, dtype, mean_type, defect)
