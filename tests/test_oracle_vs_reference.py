"""Oracle restatement vs the REAL reference model files on fresh inputs (beyond the committed golden vectors).

The reference's answers are fixtures (tests/golden/reference_fresh.npz, reference_state_dict.npz, reference_api.json), made from a
reference checkout by ``oracle/make_golden_fresh.py``; these tests need nothing outside the repository.  CPU only."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from oracle import make_golden_fresh as F
from oracle import restatement as R
from oracle import weights


def _maxdiff(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max())


@pytest.fixture(scope='module')
def ref_out():
    return load_golden('reference_fresh.npz')


@pytest.fixture(scope='module')
def sd():
    return weights.make_state_dict(77)


def _batch(seed):
    return F.fresh_batch(seed)


@pytest.mark.parametrize('seed', [1, 2])
def test_forward_fresh_inputs(ref_out, sd, seed):
    b, lpos, lv = _batch(seed)
    ppos, lposc, _ = R.center_positions(b.protein_pos, lpos, b.protein_element_batch, b.ligand_element_batch)
    got = R.model_forward(sd, None, ppos, b.protein_atom_feature.float(), b.protein_element_batch, lposc, lv,
                          b.ligand_element_batch)
    assert _maxdiff(got['pred_ligand_pos'], ref_out[f'forward{seed}_pred_ligand_pos']) < 2e-5
    assert _maxdiff(got['pred_ligand_v'], ref_out[f'forward{seed}_pred_ligand_v']) < 2e-5
    assert _maxdiff(got['final_h'], ref_out[f'forward{seed}_final_h']) < 2e-5


def test_likelihood_fresh_inputs(ref_out, sd):
    b, lpos, lv = _batch(3)
    ts = torch.tensor(F.LIKELIHOOD_T, dtype=torch.long)
    got = R.likelihood_estimation(sd, None, b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch, lpos, lv,
                                  b.ligand_element_batch, ts, noise=torch.from_numpy(ref_out['likelihood_noise']),
                                  uniform=torch.from_numpy(ref_out['likelihood_uniform']))
    want = ref_out['likelihood_terms']
    assert len(got) == len(want)
    for g, w in zip(got, want):
        np.testing.assert_allclose(g.numpy(), w, rtol=1e-4, atol=1e-6)


def test_egnn_fresh_inputs(ref_out):
    esd = weights.make_egnn_state_dict(9, num_layers=4)
    b, lpos, _ = _batch(4)
    h, x, batch, mask = F.egnn_inputs(b, lpos)
    got = R.egnn_forward(esd, h, x, mask, batch, num_layers=4)
    assert _maxdiff(got['x'], ref_out['egnn_x']) < 2e-5 and _maxdiff(got['h'], ref_out['egnn_h']) < 5e-5


def test_mirror_loads_the_full_reference_state_dict_strict():
    """All 384 entries of the real reference model's state_dict (learnable tensors, the 15 frozen schedule Parameters,
    Lt_history / Lt_count, the unused init_h_emb_layer) load into the mirror with strict=True, as
    scripts/sample_diffusion.py:163 loads a checkpoint -- and the schedule constants the mirror builds itself are the
    reference's, bit for bit.  The fixture holds the reference's keys, shapes, frozen Parameters and buffers; the learnable
    tensors get seeded values of the reference's shapes."""
    from targetdiff_amd.models import ScorePosNet3D
    lay = load_golden('reference_state_dict.npz')
    keys, shapes = [str(k) for k in lay['keys']], [tuple(json.loads(str(s))) for s in lay['shapes']]
    assert len(keys) == 384
    g = torch.Generator().manual_seed(123)
    ref_sd = {k: (torch.from_numpy(lay['value:' + k]) if 'value:' + k in lay else torch.randn(s, generator=g))
              for k, s in zip(keys, shapes)}
    mirror = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG), weights.PROTEIN_FEATURE_DIM, weights.LIGAND_FEATURE_DIM)
    own = {k: v.clone() for k, v in mirror.state_dict().items()}
    assert list(own) == keys                                            # same keys, same order
    assert [tuple(v.shape) for v in own.values()] == shapes
    frozen = [str(k) for k in lay['frozen']]
    assert len(frozen) == 15
    for k in frozen:
        assert torch.equal(own[k], ref_sd[k]), k
    res = mirror.load_state_dict(ref_sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in mirror.state_dict().items():
        assert torch.equal(v, ref_sd[k]), k


def test_call_signatures_are_drop_in():
    """INTEGRATION.md route A is an import swap: every parameter of the reference's call signatures on this path exists in
    the mirror under the same name, in the same position and with the same default (the mirror may add keyword-only
    extras at the end).  The reference's signatures are the fixture tests/golden/reference_api.json."""
    import inspect
    from targetdiff_amd import models as M
    from targetdiff_amd import sampling as S
    with open(os.path.join(GOLDEN, 'reference_api.json')) as f:
        ref = json.load(f)
    pairs = [('ScorePosNet3D.__init__', M.ScorePosNet3D.__init__), ('ScorePosNet3D.forward', M.ScorePosNet3D.forward),
             ('ScorePosNet3D.sample_diffusion', M.ScorePosNet3D.sample_diffusion),
             ('ScorePosNet3D.fetch_embedding', M.ScorePosNet3D.fetch_embedding),
             ('ScorePosNet3D.likelihood_estimation', M.ScorePosNet3D.likelihood_estimation),
             ('get_refine_net', M.get_refine_net), ('sample_diffusion_ligand', S.sample_diffusion_ligand),
             ('unbatch_v_traj', S.unbatch_v_traj)]
    for name, f_own in pairs:
        want = ref[name]
        got = list(inspect.signature(inspect.unwrap(f_own)).parameters.values())
        assert len(got) >= len(want), name
        for (a_name, a_default), b in zip(want, got):
            assert a_name == b.name and a_default == repr(b.default), (name, a_name, a_default, b)
        for extra in got[len(want):]:
            assert extra.default is not inspect.Parameter.empty, (f_own.__qualname__, extra)      # optional additions only
    # the refine net seam (models/uni_transformer.py:301) and the attributes the drivers read
    want = [n for n, _ in ref['UniTransformerO2TwoUpdateGeneral.forward']]
    got = [p.name for p in inspect.signature(M.UniTransformerO2TwoUpdateGeneral.forward).parameters.values()]
    assert got[:len(want)] == want
    want = ref['UniTransformerO2TwoUpdateGeneral.__init__']
    got = list(inspect.signature(M.UniTransformerO2TwoUpdateGeneral.__init__).parameters.values())
    for (a_name, a_default), b in zip(want, got):
        assert a_name == b.name and a_default == repr(b.default), (a_name, a_default, b)
    m = M.ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG), 27, 13)
    assert m.num_classes == 13 and m.num_timesteps == 1000 and m.center_pos_mode == 'protein'


def test_unsorted_batch_vectors_forward_and_sampling_loop(ref_out, sd):
    """Unsorted batch vectors are legal input of the reference (compose_context stable-sorts, models/common.py:126): the forward
    answers in compose_context's order (the ligand rows are NOT put back in input order), and the sampling loop combines those
    answers element by element with its state in input order.  The restatement follows both, which is what the GPU tests then
    hold the HIP path to (tests/test_gpu_long_parity.py::test_unsorted_batch_vectors_*)."""
    b, lpos, lv = _batch(4)
    pp, pl = F.unsorted_permutations(b, lpos)
    ppos, pv, bp = b.protein_pos[pp], b.protein_atom_feature.float()[pp], b.protein_element_batch[pp]
    xl, vl, bl = lpos[pl], lv[pl], b.ligand_element_batch[pl]
    # the reference answered the unsorted and the pre-sorted call alike
    assert np.array_equal(ref_out['unsorted_pred_ligand_pos'], ref_out['unsorted_presorted_pred_ligand_pos'])
    assert np.array_equal(ref_out['unsorted_final_h'], ref_out['unsorted_presorted_final_h'])
    cp, cl, off = R.center_positions(ppos, xl, bp, bl)
    got = R.model_forward(sd, None, cp, pv, bp, cl, vl, bl)
    assert _maxdiff(got['pred_ligand_pos'], ref_out['unsorted_pred_ligand_pos']) < 2e-5
    assert _maxdiff(got['pred_ligand_v'], ref_out['unsorted_pred_ligand_v']) < 2e-5
    # three steps of the reference's own loop on the unsorted vectors vs the restatement's loop on the same draws
    from oracle import draws
    steps, base = F.UNSORTED_STEPS, F.UNSORTED_DRAW_BASE
    sched = R.diffusion_schedules(dict(weights.DEFAULT_MODEL_CONFIG))
    x, v = cl.clone(), vl.clone()
    for s, t in enumerate(reversed(range(1000 - steps, 1000))):
        preds = R.model_forward(sd, None, cp, pv, bp, x, v, bl)                 # answers in compose_context's order ...
        tt = torch.full((int(bp.max()) + 1,), t, dtype=torch.long)
        x, v, _, _ = R.posterior_step(sched, tt, x, v, preds['pred_ligand_pos'], preds['pred_ligand_v'], bl,    # ... met by the state in input order
                                      draws.normal(base, s, tuple(x.shape)), draws.uniform(base + 1, s, (x.shape[0], 13)), 13)
        assert _maxdiff(ref_out['unsorted_pos_traj'][s], x + off[bl]) < 5e-5, s
        assert np.array_equal(ref_out['unsorted_v_traj'][s], v.numpy()), s
