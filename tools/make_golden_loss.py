"""Fixtures of the diffusion loss and the validation loop from the REAL reference (build container only: needs the reference tree):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_loss.py [case ...]

Every number is an output of the unmodified reference model (oracle.reference_loader): its get_diffusion_loss
(models/molopt_score_model.py:485-563) on the small batch of the forward fixtures (oracle.make_golden.small_batch) with mixed time steps
that include 0 and T - 1.  The draws are the counter-based ones of oracle/draws.py: torch.Tensor.normal_ / torch.rand_like are patched for the
duration of a call, as oracle/make_golden.py does to record them, so that the call's Gaussian draw is draws.normal(base, step) and its
uniform draw draws.uniform(base + 1, step); a test injects the very same arrays through ``noise_source``.

Cases (tests/golden/<case>.npz): loss_c0, loss_noise (model_mean_type 'noise'), loss_center_none (center_pos_mode 'none'),
loss_time_simple (time_emb_mode 'simple'), and validate_small: two batches x 10 levels with the loop arithmetic of validate()
(scripts/train_diffusion.py:153-208: sums of float(loss) * batch_size, get_auroc's weighted one-vs-rest sklearn.metrics.roc_auc_score).

Each case runs in fp32 and in float64 (the module cast to double) and stores both result sets, the perturbed x_t / v_t, and r_<output>, the
fp32 run's largest distance from the float64 run.  Stream bases are tried in turn until both runs pick the same v_t at every atom (no atom
is excluded), and for validate_small until every class of the labels has rows on both sides of its one-vs-rest split; both are asserted.
"""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import draws, reference_loader, shims, weights  # noqa: E402
from oracle.make_golden import small_batch  # noqa: E402
from oracle.make_golden_r6 import float64_run  # noqa: E402
from targetdiff_amd import workloads  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
T = 1000
SEED = 2021
CASES = {
    'loss_c0': dict(cfg={}, base=7100),
    'loss_noise': dict(cfg=dict(model_mean_type='noise'), base=7200),
    'loss_center_none': dict(cfg=dict(center_pos_mode='none'), base=7300),
    'loss_time_simple': dict(cfg=dict(time_emb_dim=8, time_emb_mode='simple'), base=7400),
}
TIME_STEP = [0, T - 1, 537]                    # the small batch has three graphs
VALIDATE_BASE = 7500
NUM_LEVELS = 10
SCALARS = ('loss', 'loss_pos', 'loss_v')
TENSORS = ('x0', 'pred_ligand_pos', 'pred_ligand_v', 'pred_pos_noise', 'ligand_v_recon')


def state_dict(cfg):
    return weights.time_emb_state_dict(SEED) if cfg.get('time_emb_dim') else weights.make_state_dict(SEED)


def build(ref, cfg, dtype):
    model = ref.ScorePosNet3D(shims.EasyDict(dict(weights.DEFAULT_MODEL_CONFIG, **cfg)), weights.PROTEIN_FEATURE_DIM,
                              weights.LIGAND_FEATURE_DIM)
    res = model.load_state_dict(state_dict(cfg), strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    model = model.eval()
    return model.double() if dtype == torch.float64 else model


@contextlib.contextmanager
def counter_draws(base, step, rec):
    """torch.Tensor.normal_ / torch.rand_like give the counter draws of (base, step); `rec` receives what was handed out"""
    o_normal, o_rand = torch.Tensor.normal_, torch.rand_like

    def normal_(self, *a, **kw):
        d = draws.normal(base, step, tuple(self.shape))
        rec['noise'] = d
        return self.copy_(d.to(self.dtype))

    def rand_like(x, *a, **kw):
        d = draws.uniform(base + 1, step, tuple(x.shape))
        rec['uniform'] = d
        return d.to(x.dtype)
    torch.Tensor.normal_, torch.rand_like = normal_, rand_like
    try:
        yield
    finally:
        torch.Tensor.normal_, torch.rand_like = o_normal, o_rand


def loss_run(model, batch, time_step, base, step, dtype):
    """One get_diffusion_loss call of the reference `model` (built by `build`, outside float64_run: its schedule tables are the fp32 ones,
    cast with the module); returns its dict plus x_t, v_t and the draws"""
    b, lpos, lv = batch
    f = lambda x: x.to(dtype)
    rec = {}
    seen = {}
    fwd = model.forward

    def forward(*a, **kw):                      # the perturbed state is what the network is called with (:510-519)
        seen['x_t'], seen['v_t'] = kw['init_ligand_pos'].clone(), kw['init_ligand_v'].clone()
        return fwd(*a, **kw)
    model.forward = forward
    try:
        return _loss_call(model, b, lpos, lv, f, time_step, base, step, rec, seen)
    finally:
        del model.forward


def _loss_call(model, b, lpos, lv, f, time_step, base, step, rec, seen):
    with counter_draws(base, step, rec), torch.no_grad():
        out = model.get_diffusion_loss(protein_pos=f(b.protein_pos), protein_v=f(b.protein_atom_feature), batch_protein=b.protein_element_batch,
                                       ligand_pos=f(lpos), ligand_v=lv, batch_ligand=b.ligand_element_batch, time_step=time_step)
    out = dict(out)
    out.update(x_t=seen['x_t'], v_t=seen['v_t'], noise=rec['noise'], uniform=rec['uniform'])
    return out


def both(ref, cfg, batch, time_step, base, step):
    m32, m64 = build(ref, cfg, torch.float32), build(ref, cfg, torch.float64)
    r32 = loss_run(m32, batch, time_step, base, step, torch.float32)
    with float64_run():
        r64 = loss_run(m64, batch, time_step, base, step, torch.float64)
    assert r64['loss'].dtype == torch.float64 and r64['pred_ligand_pos'].dtype == torch.float64
    return r32, r64


def batch_arrays(batch, prefix=''):
    b, lpos, lv = batch
    return {prefix + 'protein_pos': b.protein_pos.numpy(), prefix + 'protein_feat': b.protein_atom_feature.numpy().astype(np.int8),
            prefix + 'batch_protein': b.protein_element_batch.numpy(), prefix + 'batch_ligand': b.ligand_element_batch.numpy(),
            prefix + 'ligand_pos': lpos.numpy(), prefix + 'ligand_v': lv.numpy()}


def second_batch():
    """two more graphs of other sizes than the small batch's"""
    pockets = [workloads.synthetic_pocket(201, 50, 3.0, 8.5), workloads.synthetic_pocket(202, 30, 2.5, 7.0)]
    b = workloads.pack_samples(pockets, 1, [8, 5])
    pos, v = workloads.init_ligand(b, generator=torch.Generator().manual_seed(17))
    return b, pos, v


def gen_loss(ref, name):
    c = CASES[name]
    batch = small_batch()
    time_step = torch.tensor(TIME_STEP, dtype=torch.long)
    for base in range(c['base'], c['base'] + 20, 2):
        r32, r64 = both(ref, c['cfg'], batch, time_step, base, 0)
        same = torch.equal(r32['v_t'], r64['v_t'])
        print(f'{name}: base {base}: fp32 and float64 pick the same v_t: {same}', flush=True)
        if same:
            break
    assert torch.equal(r32['v_t'], r64['v_t']), f'{name}: no base gives equal v_t at every atom'
    arrays = dict(batch_arrays(batch), time_step=time_step.numpy(), draws_base=np.int64(base), noise=r32['noise'].numpy(),
                  uniform=r32['uniform'].numpy(), x_t=r32['x_t'].numpy(), v_t=r32['v_t'].numpy(), x_t64=r64['x_t'].numpy())
    for k in SCALARS + TENSORS:
        arrays[k] = r32[k].numpy()
        arrays[k + '64'] = r64[k].numpy()
        arrays['r_' + k] = np.float64((r32[k].double() - r64[k]).abs().max())
    arrays['r_x_t'] = np.float64((r32['x_t'].double() - r64['x_t']).abs().max())
    path = os.path.join(GOLDEN, name + '.npz')
    np.savez_compressed(path, **arrays)
    print(f'   {name}: loss {float(r64["loss"]):.6f} pos {float(r64["loss_pos"]):.6f} v {float(r64["loss_v"]):.6f}; r_loss '
          f'{arrays["r_loss"]:.2e}; wrote {path} ({os.path.getsize(path) / 1e3:.1f} kB)', flush=True)


def auroc(y_true, y_pred):
    """get_auroc's arithmetic (scripts/train_diffusion.py:22-36) with sklearn's roc_auc_score; also the per-class values"""
    from sklearn.metrics import roc_auc_score
    avg, per = 0.0, {}
    for c in sorted(set(y_true.tolist())):
        per[c] = roc_auc_score(y_true == c, y_pred[:, c])
        avg += per[c] * np.sum(y_true == c)
    return avg / len(y_true), per


def validate_run(ref, batches, base, dtype):
    """validate() of the reference script over `batches`: batch i, level l takes the draws of (base + 10 i, step l)"""
    levels = np.linspace(0, T - 1, NUM_LEVELS).astype(int)
    sums = np.zeros(3)
    per_level = np.zeros((NUM_LEVELS, 3))
    sum_n = n_level = 0
    pred, true, v_t, x_t = [], [], [], []
    model = build(ref, {}, dtype)
    for i, batch in enumerate(batches):
        bs = batch[0].num_graphs
        for l, t in enumerate(levels):
            ts = torch.tensor([int(t)] * bs)
            if dtype == torch.float64:
                with float64_run():
                    r = loss_run(model, batch, ts, base + 10 * i, l, dtype)
            else:
                r = loss_run(model, batch, ts, base + 10 * i, l, dtype)
            row = [float(r[k]) for k in SCALARS]
            for k in range(3):
                sums[k] += row[k] * bs
                per_level[l, k] += row[k] * bs
            sum_n += bs
            pred.append(r['ligand_v_recon'].numpy())
            true.append(batch[2].numpy())
            v_t.append(r['v_t'].numpy())
            x_t.append(r['x_t'].numpy())
        n_level += bs
    y_true, y_pred = np.concatenate(true), np.concatenate(pred, axis=0)
    atom_auroc, per_class = auroc(y_true, y_pred)
    classes = sorted(per_class)
    return dict(loss=sums[0] / sum_n, loss_pos=sums[1] / sum_n, loss_v=sums[2] / sum_n, atom_auroc=atom_auroc,
                classes=np.asarray(classes), per_class_auroc=np.asarray([per_class[c] for c in classes]), per_level=per_level / n_level,
                levels=levels, y_true=y_true, y_pred=y_pred, v_t=np.concatenate(v_t), x_t=np.concatenate(x_t, axis=0))


def gen_validate(ref):
    batches = [small_batch(), second_batch()]
    for base in range(VALIDATE_BASE, VALIDATE_BASE + 400, 40):
        v32 = validate_run(ref, batches, base, torch.float32)
        v64 = validate_run(ref, batches, base, torch.float64)
        same = np.array_equal(v32['v_t'], v64['v_t'])
        y = v64['y_true']
        split = all(0 < int(np.sum(y == c)) < len(y) for c in set(y.tolist()))
        print(f'validate_small: base {base}: same v_t: {same}; every class on both sides: {split}', flush=True)
        if same and split:
            break
    assert np.array_equal(v32['v_t'], v64['v_t']), 'validate_small: no base gives equal v_t at every atom'
    assert split, 'validate_small: a class holds every row'
    arrays = dict(draws_base=np.int64(base), levels=v64['levels'], labels=v64['y_true'].astype(np.int8), v_t=v64['v_t'].astype(np.int8),
                  classes=v64['classes'].astype(np.int8), ligand_v_recon=v32['y_pred'], ligand_v_recon64=v64['y_pred'],
                  r_ligand_v_recon=np.float64(np.abs(v32['y_pred'].astype(np.float64) - v64['y_pred']).max()))
    for i, batch in enumerate(batches):
        arrays.update(batch_arrays(batch, f'b{i}_'))
    for k in SCALARS + ('atom_auroc', 'per_class_auroc', 'per_level'):
        arrays[k] = np.asarray(v32[k], dtype=np.float64)
        arrays[k + '64'] = np.asarray(v64[k], dtype=np.float64)
        arrays['r_' + k] = np.float64(np.abs(arrays[k] - arrays[k + '64']).max())
    path = os.path.join(GOLDEN, 'validate_small.npz')
    np.savez_compressed(path, **arrays)
    print(f'   validate_small: loss {v64["loss"]:.6f} pos {v64["loss_pos"]:.6f} v {v64["loss_v"]:.6f} auroc {v64["atom_auroc"]:.6f} '
          f'(fp32 run {v32["atom_auroc"]:.6f}); wrote {path} ({os.path.getsize(path) / 1e3:.1f} kB)', flush=True)


def main():
    names = [a for a in sys.argv[1:] if not a.startswith('--')] or list(CASES) + ['validate_small']
    ref = reference_loader.load()
    torch.set_num_threads(8)
    for name in names:
        if name == 'validate_small':
            gen_validate(ref)
        else:
            gen_loss(ref, name)


if __name__ == '__main__':
    main()
