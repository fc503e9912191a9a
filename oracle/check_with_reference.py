"""Checks that execute the REFERENCE's own code on the mirror (TEST INFRASTRUCTURE; needs a reference checkout, so it is not part of
the suite under tests/):

    TARGETDIFF_REFERENCE=<reference checkout> python -m pytest oracle/check_with_reference.py

The import swap of INTEGRATION.md, executed: the REFERENCE's own batching driver (scripts/sample_diffusion.py:31-116,
imported unmodified) drives ``targetdiff_amd.models.ScorePosNet3D`` -- the class a maintainer swaps in at
scripts/sample_diffusion.py:17 -- through its whole call sequence: Batch.from_data_list, model.num_classes, the keyword call of
``model.sample_diffusion``, the un-batching of the returned CPU trajectories.

There is no GPU where the reference checkout lives and no reference checkout beside the GPU, so the native layer is replaced here by a
RECORDING STUB with capi's method surface whose arithmetic comes from the oracle restatement (test infrastructure).  What this
pins is the seam: argument names / order / dtypes / devices the reference passes, the members it reads, the dictionary keys,
list lengths, dtypes and de-centring it expects back.  Because the restatement is pinned to the reference, the driver's
7-tuple must equal the fixture the reference's driver produced with the reference's own model (tests/golden/driver_small.npz).
CPU only; skipped where the reference tree is absent.

The second check runs ``python -m targetdiff_amd.run scripts/sample_diffusion.py ...``: the reference's sampling script, as a file and
unmodified, executed as __main__ with `models.molopt_score_model.ScorePosNet3D` bound to the mirror class, on the same recording stub;
what is checked is the seam -- the script constructs, loads, moves and drives the mirror exactly as it does its own class, and writes
result_{id}.pt."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from oracle import reference_loader, weights
from oracle.make_golden import GOLDEN_DIR
from oracle.native_stub import RecordingNative, StubSession, route_draws

pytestmark = pytest.mark.skipif(not reference_loader.available(), reason='reference tree not present')


def load_golden(name):
    with np.load(os.path.join(GOLDEN_DIR, name)) as z:
        return {k: z[k] for k in z.files}



def test_reference_driver_runs_on_the_mirror_and_reproduces_its_own_outputs(monkeypatch):
    from oracle.make_golden import SEED
    from oracle.make_golden_r2 import counter_draws, driver_data
    from targetdiff_amd import capi, models
    drv = reference_loader.load_driver()
    sd = weights.make_state_dict(SEED)
    cfg = dict(weights.DEFAULT_MODEL_CONFIG)
    mirror = models.ScorePosNet3D(cfg, weights.PROTEIN_FEATURE_DIM, weights.LIGAND_FEATURE_DIM)
    assert not mirror.load_state_dict(sd, strict=False).unexpected_keys
    log = []
    native = RecordingNative(sd, cfg, mirror.num_classes, log)
    monkeypatch.setattr(models.ScorePosNet3D, '_native', lambda self, device: native)
    monkeypatch.setattr(capi, 'NativeSession', StubSession)

    route_draws(monkeypatch)
    g = load_golden('driver_small.npz')
    steps = int(g['steps'])
    np.random.seed(SEED)
    with counter_draws(3100, lambda kind, n: n):
        res = drv.sample_diffusion_ligand(mirror, driver_data(), 5, batch_size=2, device='cpu', num_steps=steps, pos_only=False,
                                          center_pos_mode='protein', sample_num_atoms='prior')
    pos, v, pos_traj, v_traj, v0_traj, vt_traj, time_list = res
    # the call sequence the reference drove: three sample batches (2 + 2 + 1), each one session + `steps` x (forward, posterior)
    names = [n for n, _ in log]
    assert names.count('session_create') == 3 and names.count('model_forward') == 3 * steps == names.count('posterior_step')
    first_fwd = next(a for n, a in log if n == 'model_forward')
    assert first_fwd['protein_v'][1] == 'torch.float32' and first_fwd['ligand_v'][1] == 'torch.int64'
    assert len(time_list) == 3 and len(pos) == 5
    # ... and its outputs equal what the same driver produced with the reference's own model
    sizes = g['pos_n']
    assert [p.shape[0] for p in pos] == sizes.tolist() and pos[0].dtype == np.float64
    assert np.abs(np.concatenate(pos) - g['pos_cat']).max() < 5e-5
    assert np.array_equal(np.concatenate(v), g['v_cat'].astype(np.int64))
    assert pos_traj[0].shape == (steps, sizes[0], 3)
    assert np.abs(np.concatenate(pos_traj, axis=1) - g['pos_traj_cat']).max() < 5e-5
    assert np.array_equal(np.concatenate(v_traj, axis=1), g['v_traj_cat'].astype(np.int64))
    assert np.abs(np.concatenate(v0_traj, axis=1) - g['v0_traj_cat']).max() < 2e-4
    # pos_only / sample_num_atoms='ref' branch (:66-67, :108-112)
    log.clear()
    with counter_draws(3200, lambda kind, n: n):
        res2 = drv.sample_diffusion_ligand(mirror, driver_data(ref_ligand_atoms=9), 3, batch_size=2, device='cpu', num_steps=3,
                                           pos_only=True, center_pos_mode='protein', sample_num_atoms='ref')
    assert res2[4] == [] and res2[5] == []
    assert np.abs(np.concatenate(res2[0]) - g['po_pos_cat']).max() < 5e-5
    assert np.array_equal(np.concatenate(res2[1]), g['po_v_cat'].astype(np.int64))


def test_reference_sampling_script_runs_unmodified_on_the_mirror(tmp_path, monkeypatch):
    from oracle import shims, weights
    from oracle.shims import EasyDict
    from oracle.make_golden import SEED
    from oracle.make_golden_r2 import counter_draws, driver_data
    from targetdiff_amd import capi, models, run
    shims.install()                                            # torch_geometric / torch_scatter stand-ins (not installed here)
    # what only the script's __main__ uses and this container lacks (rdkit, lmdb): transforms and the dataset
    tr = types.ModuleType('utils.transforms')

    class _Feat:
        def __init__(self, *a, dim=None):
            self._dim = dim

        @property
        def feature_dim(self):
            return self._dim

        def __call__(self, data):
            return data
    tr.FeaturizeProteinAtom = lambda: _Feat(dim=weights.PROTEIN_FEATURE_DIM)
    tr.FeaturizeLigandAtom = lambda mode: _Feat(dim=weights.LIGAND_FEATURE_DIM)
    tr.FeaturizeLigandBond = lambda: _Feat()
    import importlib
    if reference_loader.REFERENCE_ROOT not in sys.path:
        monkeypatch.syspath_prepend(reference_loader.REFERENCE_ROOT)
    importlib.import_module('utils')
    monkeypatch.setitem(sys.modules, 'utils.transforms', tr)
    ds = types.ModuleType('datasets')
    ds.get_dataset = lambda config, transform: (None, {'train': [], 'test': [driver_data(), driver_data()]})
    pl = types.ModuleType('datasets.pl_data')
    pl.FOLLOW_BATCH = ('protein_element', 'ligand_element', 'ligand_bond_type',)           # datasets/pl_data.py:7
    ds.pl_data = pl
    monkeypatch.setitem(sys.modules, 'datasets', ds)
    monkeypatch.setitem(sys.modules, 'datasets.pl_data', pl)

    cfg = dict(weights.DEFAULT_MODEL_CONFIG)
    # a checkpoint as the reference's training loop writes it: the full state_dict of the reference's own class (384 keys)
    refmod = reference_loader.load()
    ref_cls = getattr(refmod, '_reference_ScorePosNet3D', None) or refmod.ScorePosNet3D
    ref_model = ref_cls(EasyDict(cfg), weights.PROTEIN_FEATURE_DIM, weights.LIGAND_FEATURE_DIM)
    ref_model.load_state_dict(weights.make_state_dict(SEED), strict=False)
    sd = {k: v.clone() for k, v in ref_model.state_dict().items()}
    assert len(sd) == 384
    ckpt = {'config': EasyDict(model=cfg, data=EasyDict(transform=EasyDict(ligand_atom_mode='add_aromatic'))), 'model': sd}
    ckpt_path = tmp_path / 'model.pt'
    torch.save({'model': sd}, ckpt_path)                       # (the script's torch.load is routed to `ckpt` below: EasyDict pickles)
    monkeypatch.setattr(torch, 'load', lambda *a, **k: ckpt)
    yml = tmp_path / 'sampling.yml'
    yml.write_text(f'model:\n  checkpoint: {ckpt_path}\nsample:\n  seed: 2021\n  num_samples: 3\n  num_steps: 2\n  pos_only: False\n'
                   '  center_pos_mode: protein\n  sample_num_atoms: prior\n')
    log = []
    native = RecordingNative(sd, cfg, weights.LIGAND_FEATURE_DIM, log)
    monkeypatch.setattr(models.ScorePosNet3D, '_native', lambda self, device: native)
    monkeypatch.setattr(capi, 'NativeSession', StubSession)
    made = []
    orig_init = models.ScorePosNet3D.__init__

    def spy_init(self, *a, **k):
        made.append(self)
        orig_init(self, *a, **k)
    monkeypatch.setattr(models.ScorePosNet3D, '__init__', spy_init)
    out = tmp_path / 'out'
    script = os.path.join(reference_loader.REFERENCE_ROOT, 'scripts', 'sample_diffusion.py')
    before = open(script, 'rb').read()
    monkeypatch.setattr(sys, 'argv', list(sys.argv))
    sys.modules.pop('scripts.sample_diffusion', None)
    with counter_draws(3300, lambda kind, n: n):
        run.main(['--reference-root', reference_loader.REFERENCE_ROOT, 'scripts/sample_diffusion.py', str(yml), '-i', '1', '--device', 'cpu',
                  '--batch_size', '2', '--result_path', str(out)])
    assert open(script, 'rb').read() == before
    assert sys.modules['models.molopt_score_model'].ScorePosNet3D is models.ScorePosNet3D
    run.uninstall()                    # other tests of this process use the reference's own class
    # the script built ONE model, and it is the mirror; it loaded the checkpoint strictly and drove it through both batches
    assert len(made) == 1 and type(made[0]) is models.ScorePosNet3D
    names = [n for n, _ in log]
    assert names.count('session_create') == 2 and names.count('model_forward') == 2 * 2 == names.count('posterior_step')
    monkeypatch.undo()
    res = torch.load(out / 'result_1.pt', weights_only=False)
    assert set(res) == {'data', 'pred_ligand_pos', 'pred_ligand_v', 'pred_ligand_pos_traj', 'pred_ligand_v_traj', 'time'}
    assert len(res['pred_ligand_pos']) == 3 and res['pred_ligand_pos'][0].dtype == np.float64
    assert res['pred_ligand_pos_traj'][0].shape[0] == 2 and len(res['time']) == 2
    assert (out / 'sample.yml').exists()
