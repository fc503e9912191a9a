"""quality.SamplePack on the library: a report taken as a method of one shared pack equals the report of the matching sample_*
function on the raw result, bit for bit, and tools/evaluate_samples.py prints the numbers the five sample_* functions give
(tests/test_sample_pack_host.py holds the same checks on the restatements).  The kernels themselves are held against the restatements
by tests/test_gpu_{quality,bonds,rings,fingerprint,geometry}.py."""
import numpy as np
import pytest

from targetdiff_amd import quality
from test_bonds_host import save_results
from test_sample_pack_host import assert_pack_equals_raw, assert_tool_equals_raw

pytestmark = pytest.mark.gpu

SIZES, FRAMES = (0, 1, 2, 128, 129), 3      # the empty molecule, and both sides of the boundary between the 128- and the 512-lane kernels


def lattice_result(seed):
    """a 7-tuple as sample_diffusion_ligand returns it: carbons and nitrogens of both kinds on a cubic lattice of 1.45 A, a single bond
    along every edge, jittered by 0.12 A so that some bonds break and some frames fall into fragments"""
    rng = np.random.default_rng(seed)
    grid = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing='ij'), -1).reshape(-1, 3) * 1.45
    pos_traj = [(grid[None, :n] + rng.normal(0, 0.12, (FRAMES, n, 3))).astype(np.float32).astype(np.float64) for n in SIZES]
    v_traj = [rng.integers(1, 5, (FRAMES, n)) for n in SIZES]
    return ([p[-1] for p in pos_traj], [v[-1] for v in v_traj], pos_traj, v_traj, [], [], [0.0])


def test_a_shared_pack_and_the_tool_give_the_numbers_of_the_sample_functions(tmp_path, monkeypatch):
    result = lattice_result(0)
    shared = assert_pack_equals_raw(result, 'cuda')
    complete, stable = shared.mask('complete').cpu().numpy(), shared.mask('stable', ('stable',)).cpu().numpy()
    assert shared.S == FRAMES and tuple(shared.sizes) == SIZES
    assert 0 < complete.sum() < complete.size and not complete[:, 0].any() and complete[:, 1].all()    # no atom: no fragment
    assert 0 < stable.sum() < stable.size
    assert int(shared.graph['bond_ptr'][-1]) > 500 and int((shared.bond_ring > 0).sum()) > 100            # a lattice that bonds, in rings
    save_results(tmp_path, {0: result, 1: lattice_result(1)})
    assert_tool_equals_raw(tmp_path, monkeypatch, 'cuda')
