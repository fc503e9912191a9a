"""Fixtures of scaffold-constrained sampling from the REAL reference (build container only: needs the reference tree):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_inpaint.py [case ...]

The reference has no inpainting loop, but it has every piece of one.  The loop below is this project's; every piece of arithmetic
in it is a call of the unmodified reference model (oracle.reference_loader): center_pos, forward, q_pos_posterior, posterior_logvar
through extract, q_v_posterior, log_sample_categorical, index_to_log_onehot, q_v_pred / q_v_sample and alphas_cumprod.  The order
is the reference's sample_diffusion (models/molopt_score_model.py:633-703) with the rule of tests/_inpaint_ref.py applied to the
known atoms after every step.  Draws are the counter-based ones of oracle/draws.py: torch.randn_like / rand_like are patched so
that every call inside step s returns draws.normal(base, s) / draws.uniform(base + 1, s) -- the posterior's categorical draw and
q_v_sample's therefore see the SAME uniform row of an atom, which is the rule: an atom uses its own draw of the step for one or the
other.

Cases: tests/_inpaint_ref.CASES (inpaint_small_T100: T = 100 run in full, one graph without a known atom;
inpaint_small_1000_first20: the default schedule, 20 of 1000 steps; inpaint_pos_only: 5 steps with frozen types).  Each case runs in
fp32 and in float64 (the module cast to double, oracle.make_golden_r6.float64_run); the generator asserts that both pick the same
type at every step and atom and tries the next seed otherwise, and stores r = the fp32 run's largest position distance from the
float64 run.  It also prints alphas_cumprod[T-1] of the position schedule and the deviation of q(v_{T-1} | v0) from uniform.
"""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from oracle import draws, reference_loader, shims, weights  # noqa: E402
from oracle.make_golden_r6 import float64_run  # noqa: E402
import _inpaint_ref as IR  # noqa: E402
from _tol import TOL_TRAJ  # noqa: E402


@contextlib.contextmanager
def step_draws(base, state, dtype):
    """torch.randn_like / rand_like return the draws of step state['s'], whatever the number of calls inside the step"""
    o_randn, o_rand = torch.randn_like, torch.rand_like
    torch.randn_like = lambda x, *a, **k: draws.normal(base, state['s'], tuple(x.shape)).to(dtype)
    torch.rand_like = lambda x, *a, **k: draws.uniform(base + 1, state['s'], tuple(x.shape)).to(dtype)
    try:
        yield
    finally:
        torch.randn_like, torch.rand_like = o_randn, o_rand


def build(ref, cfg, dtype):
    model = ref.ScorePosNet3D(shims.EasyDict(dict(cfg)), weights.PROTEIN_FEATURE_DIM, weights.LIGAND_FEATURE_DIM)
    res = model.load_state_dict(weights.make_state_dict(2021), strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    model = model.eval()
    return model.double() if dtype == torch.float64 else model


def reference_run(ref, case, inputs, dtype):
    c = IR.CASES[case]
    model = build(ref, IR.model_config(case), dtype)
    b = IR.case_batch(case)
    bp, bl, B = b.protein_element_batch, b.ligand_element_batch, b.num_graphs
    T, K = model.num_timesteps, model.num_classes
    f = lambda x: x.to(dtype)
    mask, v0 = inputs['fixed_mask'], inputs['fixed_v']
    m3 = mask.unsqueeze(-1)
    ppos, lpos, offset = ref.center_pos(f(b.protein_pos), f(inputs['init_pos']), bp, bl, mode='protein')
    _, x0c, _ = ref.center_pos(f(b.protein_pos), f(inputs['fixed_pos']), bp, bl, mode='protein')
    pv = f(b.protein_atom_feature)
    a = ref.extract(model.alphas_cumprod, torch.full((B,), T - 1, dtype=torch.long), bl)
    lpos = torch.where(m3, a.sqrt() * x0c + (1.0 - a).sqrt() * lpos, lpos)            # the form of :585
    lv = inputs['init_v']
    log_v0_known = ref.index_to_log_onehot(v0, K)
    out = {k: [] for k in ('pos_traj', 'v_traj', 'v0_traj', 'vt_traj')}
    state = {'s': 0}
    with step_draws(c['base'], state, dtype), torch.no_grad():
        for s, i in enumerate(reversed(range(T - c['num_steps'], T))):
            state['s'] = s
            t = torch.full((B,), i, dtype=torch.long)
            preds = model(protein_pos=ppos, protein_v=pv, batch_protein=bp, init_ligand_pos=lpos, init_ligand_v=lv, batch_ligand=bl,
                          time_step=t)
            mean = model.q_pos_posterior(x0=preds['pred_ligand_pos'], xt=lpos, t=t, batch=bl)
            logvar = ref.extract(model.posterior_logvar, t, bl)
            nz = (1 - (t == 0).float())[bl].unsqueeze(-1)
            eps = torch.randn_like(lpos)
            pos_next = mean + nz * (0.5 * logvar).exp() * eps                            # :677
            tm1 = (t - 1).clamp(min=0)
            if i > 0:
                a = ref.extract(model.alphas_cumprod, tm1, bl)
                known = a.sqrt() * x0c + (1.0 - a).sqrt() * eps                          # :585 at level t - 1
            else:
                known = x0c
            lpos = torch.where(m3, known, pos_next)
            if not c['pos_only']:
                log_recon = F.log_softmax(preds['pred_ligand_v'], dim=-1)
                log_v = ref.index_to_log_onehot(lv, K)
                log_prob = model.q_v_posterior(log_recon, log_v, t, bl)
                v_next = ref.log_sample_categorical(log_prob)
                if i > 0:
                    v_known, _ = model.q_v_sample(log_v0_known, tm1, bl)
                    lq = model.q_v_pred(log_v0_known, tm1, bl)
                else:
                    v_known, lq = v0, log_v0_known
                lv = torch.where(mask, v_known, v_next)
                out['v0_traj'].append(log_recon.clone())
                out['vt_traj'].append(torch.where(m3, lq, log_prob))
            out['pos_traj'].append((lpos + offset[bl]).clone())
            out['v_traj'].append(lv.clone())
    return {k: torch.stack(v) if v else torch.zeros(0) for k, v in out.items()}, model


def main():
    names = [a for a in sys.argv[1:] if not a.startswith('--')] or list(IR.CASES)
    ref = reference_loader.load()
    torch.set_num_threads(8)
    for case in names:
        c = IR.CASES[case]
        for seed in range(31, 41):
            inputs = IR.case_inputs(case, seed)
            r32, model = reference_run(ref, case, inputs, torch.float32)
            with float64_run():
                r64, _ = reference_run(ref, case, inputs, torch.float64)
            same = torch.equal(r32['v_traj'], r64['v_traj'])
            r = float((r32['pos_traj'].double() - r64['pos_traj']).abs().max())
            print(f'{case}: seed {seed}: fp32 and float64 reference pick the same types: {same}; r = {r:.3e} A '
                  f'({r / TOL_TRAJ:.3f} of TOL_TRAJ)')
            if same and r <= TOL_TRAJ / 5:
                break
        else:
            raise SystemExit(f'{case}: no seed gives equal types and r <= TOL_TRAJ / 5: shorten the case')
        T = model.num_timesteps
        abar = float(model.alphas_cumprod[T - 1])
        ca = float(np.exp(np.float64(model.log_alphas_cumprod_v[T - 1])))
        K = model.num_classes
        print(f'   T = {T}: alphas_cumprod[T-1] = {abar:.6f} (known atoms start at {abar ** 0.5:.4f} x0 + {(1 - abar) ** 0.5:.4f} init); '
              f'exp(log_alphas_cumprod_v[T-1]) = {ca:.3e}, max |q(v_T-1 | v0) - 1/K| = {ca * (1 - 1 / K):.3e}')
        arrays = dict(seed=np.int64(seed), draws_base=np.int64(c['base']), r=np.float64(r), alphas_cumprod_last=np.float64(abar),
                      init_pos=inputs['init_pos'].numpy(), init_v=inputs['init_v'].numpy().astype(np.int8),
                      fixed_mask=inputs['fixed_mask'].numpy(), fixed_pos=inputs['fixed_pos'].numpy(),
                      fixed_v=inputs['fixed_v'].numpy().astype(np.int8),
                      pos_traj=r32['pos_traj'].numpy(), v_traj=r32['v_traj'].numpy().astype(np.int8))
        if not c['pos_only']:
            arrays.update(v0_traj=r32['v0_traj'].numpy(), vt_traj=r32['vt_traj'].numpy())
        path = os.path.join(IR.GOLDEN, case + '.npz')
        np.savez_compressed(path, **arrays)
        print(f'   wrote {path} ({os.path.getsize(path) / 1e3:.1f} kB)')


if __name__ == '__main__':
    main()
