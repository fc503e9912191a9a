"""quality.PocketSide on the GPU: one decode and one upload of a pocket under the three pocket reports (csrc/pocket.hip,
csrc/interactions.hip, csrc/sasa.hip; DESIGN.md section 3, "Host side").  One small pack: two frames of three molecules of 0, 1 and 130
atoms -- an empty one, a single atom, and one past the 128-atom instantiation of the surface kernel --, a pocket of 65 atoms (two words
of bits, the last one partial), an include mask that drops a molecule, and a reference ligand.

  1. the three reports of a shared pack and a shared PocketSide equal the same three taken each from the raw result, every field;
  2. the raw outputs of the three bindings on the PocketSide's tensors equal the numpy restatements, every output, no tolerance.
tests/test_pocket_side_host.py runs the first on the restatements.
"""
import types

import numpy as np
import pytest
import torch

import _interactions_ref as IR
import _pocket_ref as PR
import _sasa_ref as SR
from targetdiff_amd import capi, quality, workloads

pytestmark = pytest.mark.gpu

CLASS_Z = quality.class_atomic_numbers('add_aromatic')
SIZES, S, N_P = (0, 1, 130), 2, 65
INCLUDE = np.asarray([[True, True, False], [True, True, True]])                # the large molecule is out of the first frame


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


def case():
    """(result dictionary with its pocket, reference ligand): clouds of every class around the origin inside a pocket of N_P atoms, one
    in ten a hydrogen"""
    rng = np.random.default_rng(65)
    ball = lambda n, r: (rng.normal(size=(n, 3)) * (r / 3.0)).astype(np.float32)
    z = rng.choice(workloads.PROTEIN_ELEMENTS, N_P, p=(0.1, 0.5, 0.15, 0.2, 0.03, 0.02))
    feat = workloads.featurize_protein(z, rng.integers(0, 20, N_P), rng.random(N_P) < 0.5)
    data = types.SimpleNamespace(protein_pos=torch.from_numpy(ball(N_P, 9.0)), protein_atom_feature=torch.from_numpy(feat))
    pos_traj = [np.stack([ball(n, 7.0) for _ in range(S)]).astype(np.float64) for n in SIZES]
    v_traj = [rng.integers(0, 13, (S, n)) for n in SIZES]
    ligand = (ball(8, 5.0), rng.integers(0, 13, 8).astype(np.int64))
    return {'data': data, 'pred_ligand_pos_traj': pos_traj, 'pred_ligand_v_traj': v_traj}, ligand


def assert_equal_reports(got, want):
    assert type(got) is type(want) and vars(got).keys() == vars(want).keys()
    arrays = 0
    for k, x in vars(want).items():
        if isinstance(x, np.ndarray):
            assert torch.equal(torch.from_numpy(getattr(got, k)), torch.from_numpy(x)), k
            arrays += 1
        else:
            assert getattr(got, k) == x, k
    assert arrays >= 8
    for s in range(want.num_frames):
        np.testing.assert_equal(got.summary(s), want.summary(s))


def test_reports_of_a_shared_pocket_side_equal_those_from_the_raw_pocket_and_the_raw_outputs_equal_the_restatements():
    dev = _dev()
    result, ligand = case()
    data = result['data']
    pack, side = quality.SamplePack(result, 'all', device=dev), quality.PocketSide(data, dev)
    assert pack.S == S and tuple(pack.sizes) == SIZES and side.pos.shape == (N_P, 3) and side.pos.device == dev
    for include in (INCLUDE, 'all'):
        reports = (pack.pocket(side, include, ligand), pack.interactions(side, include, ligand), pack.sasa(side, include, ligand))
        assert_equal_reports(reports[0], quality.sample_pocket(result, 'all', include, ligand, device=dev))
        assert_equal_reports(reports[1], quality.sample_interactions(result, 'all', include, ligand, device=dev))
        assert_equal_reports(reports[2], quality.sample_sasa(result, 'all', include, ligand, device=dev))
    poc, ia, sa = reports
    assert poc.sum_contacts[-1] > 0 and ia.sum_hbonds[-1] > 0 and ia.sum_hydrophobic[-1] > 0 and sa.sum_buried[-1, 0] > 0
    assert poc.n_ref[-1] == 1 and sa.n_ref[-1] == 1 and poc.pocket_freq.shape == (S, N_P)

    # the raw outputs, on the tensors the PocketSide hands out, against the restatements on numpy's own decode
    ppos, feat = data.protein_pos.numpy(), data.protein_atom_feature.numpy()
    elem, kind, names = quality.pocket_kinds(feat)
    role, sasa_elem = IR.pocket_roles(feat), quality.pocket_kinds(feat, 'element')[1]
    assert (elem == 0).any() and (kind[elem == 0] == -1).all()                   # the hydrogens are in the pocket, and take no part
    pos, v, ptr = pack.pos.cpu().numpy(), pack.v.cpu().numpy(), pack.ligand_ptr.cpu().numpy()
    mask = torch.from_numpy(INCLUDE).to(dev)
    (skind, snames), lig = side.kinds(), pack._reference(ligand)
    assert snames == names and len(names) == 40

    def same(got, want, what):
        for k, x in want.items():
            if x is None:
                assert got[k] is None, f'{what}: {k}'
            else:
                assert got[k].dtype == torch.from_numpy(x).dtype and torch.equal(got[k].cpu(), torch.from_numpy(x)), f'{what}: {k}'

    table = quality.pocket_clash_thresholds()
    ref_bits = capi.pocket_report(*lig, side.pos, side.elem, skind, 40, 4.0, None, None, None, False, True)['bits'][0, 0].contiguous()
    assert ref_bits.shape == (2,) and int(ref_bits[1]) >> 1 == 0                # two words, and of the last one a single bit
    got = capi.pocket_report(*pack._args, side.pos, side.elem, skind, 40, 4.0, table, mask, ref_bits)
    want = PR.pocket_report(pos, v, ptr, CLASS_Z, ppos, elem, kind, 40, 4.0, table, INCLUDE, ref_bits.cpu().numpy())
    same(got, want, 'pocket_report')
    assert want['n_contacts'][:, 0].tolist() == [0, 0] and (want['n_contacts'][:, 2] > 0).all() and want['n_ref_common'].sum() > 0

    ref3 = capi.interaction_report(*lig, side.pos, side.elem, skind, side.roles(), 40, return_atoms=False)['bits'][0, 0].contiguous()
    got = capi.interaction_report(*pack._args, side.pos, side.elem, skind, side.roles(), 40, include=mask, ref_bits=ref3)
    want = IR.interaction_report(pos, v, ptr, CLASS_Z, ppos, elem, kind, role, 40, include=INCLUDE, ref_bits=ref3.cpu().numpy())
    same(got, want, 'interaction_report')
    assert (want['n_hbonds'][:, 2] > 0).all() and (want['n_hydrophobic'][:, 2] > 0).all() and not want['n_hbonds'][:, 0].any()

    lr, pr = quality.sasa_reaches()
    dirs = quality.sasa_directions()
    got = capi.sasa_report(*pack._args, side.pos, side.kinds('element')[0], lr, pr, torch.from_numpy(dirs).to(dev), mask)
    want = SR.sasa_report(pos, v, ptr, CLASS_Z, ppos, sasa_elem, lr, pr, dirs, INCLUDE)
    same(got, want, 'sasa_report')
    assert not want['free'][:, 0].any() and (want['bound'].sum(-1) < want['free'].sum(-1))[:, 2].all() and want['bits'].shape == (S, 3, 2)
