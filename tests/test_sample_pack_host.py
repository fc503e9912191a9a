"""CPU-only checks of quality.SamplePack, the one pack and the one bond graph the reports of a result file share, with the bindings
patched by the restatements the GPU tests compare the kernels with.

  1. tools/evaluate_samples.py packs every result file once and makes the binding calls listed here, no more.
  2. a report taken as a method of a shared pack equals the report of the matching sample_* function on the raw result, field by
     field, and the tool's dictionary equals the one its own assembly makes from the five sample_* functions.
  3. the host's look at a pack runs with its first binding call, whichever report that is, and not again.
tests/test_gpu_sample_pack.py runs the second on the library.
"""
import types

import numpy as np
import pytest
import torch

import _bonds_ref as BR
import _fingerprint_ref as FR
import _geometry_ref as GR
import _quality_ref as QR
import _rings_ref as RR
from targetdiff_amd import capi, quality
from test_bonds_host import load_tool, save_results
from test_rings_host import ringed_result

FLAGS = ['--connectivity', '--rings', '--diversity', '--geometry', '--eval_step', 'all']
MODES = ('all', 'complete', 'stable')
# what one result file costs with all four flags: the plain bond graph once and once more for the bond-length histograms, the ring
# report for the ratios and for bond_ring, and with 'stable' the stability flags before the masked pair profiles
CALLS = {'all': ['bond_graph', 'ring_report', 'fingerprint', 'fingerprint_similarity', 'bond_graph', 'ring_report', 'geometry_report',
                 'quality_report'],
         'complete': ['bond_graph', 'bond_graph', 'ring_report', 'fingerprint', 'fingerprint_similarity', 'ring_report', 'geometry_report',
                      'quality_report'],
         'stable': ['bond_graph', 'ring_report', 'fingerprint', 'fingerprint_similarity', 'bond_graph', 'ring_report', 'geometry_report',
                    'quality_report', 'quality_report']}


@pytest.fixture
def numpy_binding(monkeypatch):
    """every binding of the evaluation patched by its restatement; the calls as (name, the ``check`` it was given or None), a new pack
    as ('pack', None)"""
    calls = []

    def patched(name, fn):
        def binding(*a, **kw):
            calls.append((name, kw.get('check')))
            return fn(*a, **kw)
        return binding

    def ring_report(pos, v, ligand_ptr, class_z, class_aromatic=None, include=None, bond_ptr=None, return_atom_ring=True, check=True):
        capi._bond_inputs(pos, v, ligand_ptr, class_z, class_aromatic, include, (), check)      # the binding's validator, as the others run it
        return RR.torch_ring_report(pos, v, ligand_ptr, class_z, class_aromatic, include, bond_ptr, return_atom_ring, check)

    for name, fn in (('quality_report', QR.torch_binding), ('bond_graph', BR.torch_bond_graph), ('bond_list', BR.torch_bond_list),
                     ('ring_report', ring_report), ('fingerprint', FR.torch_fingerprint),
                     ('fingerprint_similarity', FR.torch_similarity), ('geometry_report', GR.torch_geometry_report)):
        monkeypatch.setattr(capi, name, patched(name, fn))
    init = quality.SamplePack.__init__

    def counted(self, *a, **kw):
        calls.append(('pack', None))
        init(self, *a, **kw)

    monkeypatch.setattr(quality.SamplePack, '__init__', counted)
    return calls


class RawPack:
    """SamplePack's reports, each through the matching sample_* function on the raw result: its own packing, its own bond graph"""

    def __init__(self, result, eval_step=-1, atom_enc_mode='add_aromatic', device='cuda'):
        self.result, self.eval_step, self.kw = result, eval_step, dict(atom_enc_mode=atom_enc_mode, device=device)

    def quality(self, include='all', reference=None, profiles=None):
        return quality.sample_quality(self.result, self.eval_step, include, reference=reference, profiles=profiles, **self.kw)

    def connectivity(self, include='all', reference=None, bond_profiles=None):
        return quality.sample_connectivity(self.result, self.eval_step, include, reference=reference, bond_profiles=bond_profiles, **self.kw)

    def rings(self, include='all'):
        return quality.sample_rings(self.result, self.eval_step, include, **self.kw)

    def diversity(self, include='all', radius=2, key_rounds=8, reference_ligand=None):
        return quality.sample_diversity(self.result, self.eval_step, include, radius, key_rounds, reference_ligand, **self.kw)

    def geometry(self, include='all', reference=None, profiles=None, clash_scale=0.7, radii=None):
        return quality.sample_geometry(self.result, self.eval_step, include, reference, profiles, clash_scale, radii, **self.kw)


def assert_same_report(got, want):
    """every array field np.array_equal, every summary equal (a nan equals a nan: a pocket without a pair has no diversity)"""
    assert type(got) is type(want) and vars(got).keys() == vars(want).keys()
    arrays = 0
    for k, x in vars(want).items():
        if isinstance(x, np.ndarray):
            assert np.array_equal(getattr(got, k), x, equal_nan=x.dtype.kind == 'f'), k
            arrays += 1
    assert arrays >= 3
    for s in range(want.num_frames):
        np.testing.assert_equal(got.summary(s), want.summary(s))


def assert_pack_equals_raw(result, device, modes=('all', 'complete'), seed=0):
    """the five reports of one shared pack, for every include mode and a random mask, against the sample_* functions on ``result``"""
    shared, raw = quality.SamplePack(result, 'all', device=device), RawPack(result, 'all', device=device)
    rng = np.random.default_rng(seed)
    mask = rng.random((shared.S, len(shared.sizes))) < 0.5
    assert 0 < mask.sum() < mask.size
    ligand = (np.asarray(result[2][-1][-1], np.float32), np.asarray(result[3][-1][-1], np.int64))
    for include in modes + (mask,):
        assert_same_report(shared.connectivity(include, {}), raw.connectivity(include, {}))
        assert_same_report(shared.rings(include), raw.rings(include))
        assert_same_report(shared.diversity(include, reference_ligand=ligand), raw.diversity(include, reference_ligand=ligand))
        assert_same_report(shared.geometry(include), raw.geometry(include))
    for include in modes + ('stable', mask):
        assert_same_report(shared.quality(include, {}), raw.quality(include, {}))
    return shared


def assert_tool_equals_raw(tmp_path, monkeypatch, device, modes=MODES):
    """evaluate_samples' dictionary against the one its assembly makes from the five sample_* functions and ``merged``"""
    tool = load_tool('evaluate_samples')
    for include in modes:
        argv = ['--sample_path', str(tmp_path), '--device', device, '--include', include] + FLAGS
        with monkeypatch.context() as m:
            m.setattr(tool, 'quality', types.SimpleNamespace(**dict(vars(quality), SamplePack=RawPack)))      # the tool's own name only
            want = tool.main(argv)
        np.testing.assert_equal(tool.main(argv), want)
        assert want['include'] == include and {'connectivity', 'rings', 'diversity', 'geometry', 'curve'} <= set(want)


def results_with_both_sizes():
    """two result files whose molecules straddle the 128-atom boundary between the kernels' two instantiations"""
    return {10: ringed_result(5, [6, 130, 9], 3), 2: ringed_result(6, [4, 11, 129, 5], 3)}


def test_the_tool_packs_a_file_once_and_shares_its_bond_graph(numpy_binding, tmp_path):
    tool = load_tool('evaluate_samples')
    save_results(tmp_path, results_with_both_sizes())
    for include in MODES:
        del numpy_binding[:]
        tool.main(['--sample_path', str(tmp_path), '--device', 'cpu', '--include', include] + FLAGS)
        names = [name for name, _ in numpy_binding]
        assert names == (['pack'] + CALLS[include]) * 2, include                # one packing per file, then exactly these calls
        per_file = CALLS[include]
        assert per_file.count('bond_graph') <= 2 and per_file.count('ring_report') <= 2
        assert per_file.count('quality_report') == (2 if include == 'stable' else 1)
        # the host looks at a pack once: with the first call on it
        later = [None if name == 'fingerprint_similarity' else False for name in per_file[1:]]      # it takes no pack
        assert [check for _, check in numpy_binding] == ([None, True] + later) * 2, include


def test_reports_of_a_shared_pack_equal_the_sample_functions(numpy_binding, tmp_path, monkeypatch):
    # small molecules: the restatements know no size classes (tests/test_gpu_sample_pack.py straddles the boundary on the library)
    results = {10: ringed_result(5, [6, 9, 14], 3), 2: ringed_result(6, [4, 11, 5, 1], 3)}
    for result in results.values():
        shared = assert_pack_equals_raw(result, 'cpu')
        assert shared._graph is not None and shared._stable is not None and shared._bond_ring is not None      # computed, and kept
    save_results(tmp_path, results)
    assert_tool_equals_raw(tmp_path, monkeypatch, 'cpu')


REPORTS = {'quality': lambda p: p.quality('all', {}), 'connectivity': lambda p: p.connectivity('all', {}), 'rings': lambda p: p.rings(),
           'diversity': lambda p: p.diversity(), 'geometry': lambda p: p.geometry()}


@pytest.mark.parametrize('first', sorted(REPORTS))
def test_the_host_checks_run_with_the_first_report_and_not_again(numpy_binding, first):
    result = ringed_result(7, [6, 9, 14], 2)
    pack = quality.SamplePack(result, 'all', device='cpu')
    order = [first] + [k for k in sorted(REPORTS) if k != first]
    for k in order:
        REPORTS[k](pack)
    checks = [check for _, check in numpy_binding if check is not None]
    # quality_report's look does not bound the molecule sizes: after it, the first call of the bond graph's family looks once more
    assert checks[0] is True and checks[1:].count(True) == (1 if first == 'quality' else 0)
    if first == 'quality':
        assert checks[1] is True
    # offsets that are no prefix offsets are refused by whichever report runs first
    pack = quality.SamplePack(result, 'all', device='cpu')
    pack.ligand_ptr = torch.tensor([0, 15, 6, 29], dtype=torch.int32)
    with pytest.raises(ValueError, match='prefix offsets'):
        REPORTS[first](pack)
