"""CPU-only checks of quality.PocketSide, the one decode and the one upload of a pocket that the three pocket reports of a result file
share ("Host side"), with the bindings patched by the restatements the GPU tests compare the kernels with.

  1. tools/evaluate_samples.py --pocket --interactions --sasa --diversity --eval_step all on two result files with a reference ligand,
     over all and over the complete molecules: its stdout, the bytes of quality.json and the binding calls equal a recording taken
     before the three reports shared anything (tests/golden/pocket_side_tool.json).
  2. the three reports of a shared pack and a shared PocketSide equal the sample_* functions on the raw result, field by field.
  3. per result file the pocket is decoded once and uploaded once, and the reference ligand is packed once.
  4. ``merged`` of the five report classes on the shared base adds, carries or drops every field as their hand-written merges did.
tests/test_gpu_pocket_side.py runs the second on the library.
"""
import json
import os

import numpy as np
import pytest
import torch

import _interactions_ref as IR
import _pocket_ref as PR
import _sasa_ref as SR
from targetdiff_amd import capi, quality
from test_bonds_host import load_tool
from test_interactions_host import typed_pocket, typed_result
from test_pocket_host import save_with_pockets
from test_sample_pack_host import assert_same_report, numpy_binding  # noqa: F401  (the fixture that patches the other bindings)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pocket_side_tool.json')
FLAGS = ['--pocket', '--interactions', '--sasa', '--diversity', '--eval_step', 'all']
MODES = ('all', 'complete')


@pytest.fixture
def pocket_bindings(numpy_binding, monkeypatch):  # noqa: F811
    """numpy_binding, and the three pocket bindings patched by their restatements too"""
    def patched(name, fn):
        def binding(*a, **kw):
            numpy_binding.append((name, kw.get('check')))
            return fn(*a, **kw)
        return binding

    for name, fn in (('pocket_report', PR.torch_pocket_report), ('interaction_report', IR.torch_interaction_report),
                     ('sasa_report', SR.torch_sasa_report)):
        monkeypatch.setattr(capi, name, patched(name, fn))
    return numpy_binding


def two_files():
    results = {10: typed_result(5, [6, 9, 14], 3), 2: typed_result(6, [4, 11, 5, 1], 3)}
    pockets = {10: typed_pocket(1), 2: typed_pocket(2, 45)}
    ligand = (np.asarray(results[10][2][0][-1], np.float32), np.asarray(results[10][3][0][-1], np.int64))
    return results, pockets, ligand


def run_tool(tmp_path, monkeypatch, capsys, calls, include):
    """the tool from inside ``tmp_path``, so that no line it prints depends on where that is: (stdout, quality.json, binding calls)"""
    monkeypatch.chdir(tmp_path)
    del calls[:]
    capsys.readouterr()
    load_tool('evaluate_samples').main(['--sample_path', 'samples', '--device', 'cpu', '--include', include, '--reference_npz', 'ref.npz'] + FLAGS)
    with open(tmp_path / 'samples' / 'eval_results' / 'quality.json', 'rb') as f:
        return capsys.readouterr().out, f.read().decode('ascii'), [[name, check] for name, check in calls]


def saved(tmp_path):
    results, pockets, ligand = two_files()
    (tmp_path / 'samples').mkdir()
    save_with_pockets(tmp_path / 'samples', results, pockets)
    np.savez(tmp_path / 'ref.npz', ligand_pos=ligand[0], ligand_v=ligand[1])


def test_the_tool_prints_and_writes_what_it_did_before_the_reports_shared_a_pocket(pocket_bindings, tmp_path, monkeypatch, capsys):
    saved(tmp_path)
    with open(GOLDEN) as f:
        golden = json.load(f)
    for include in MODES:
        stdout, written, calls = run_tool(tmp_path, monkeypatch, capsys, pocket_bindings, include)
        assert stdout == golden[include]['stdout'], include
        assert written == golden[include]['quality_json'], include
        assert calls == golden[include]['calls'], include                       # the three binding call lists, and every other, unchanged
        out = json.loads(written)
        assert {'pocket', 'interactions', 'sasa', 'diversity', 'curve'} <= set(out) and out['pocket']['mean_contacts'] > 0
        assert out['interactions']['mean_hbonds'] > 0 and out['sasa']['sasa_buried'] > 0 and 'ref_tanimoto' in out['sasa']


def test_reports_of_a_shared_pocket_equal_the_sample_functions(pocket_bindings):
    results, pockets, ligand = two_files()
    rng = np.random.default_rng(0)
    for i, res in results.items():
        as_dict = {'data': pockets[i], 'pred_ligand_pos_traj': res[2], 'pred_ligand_v_traj': res[3]}
        pack = quality.SamplePack(res, 'all', device='cpu')
        side = quality.PocketSide(pockets[i], 'cpu')
        mask = rng.random((pack.S, len(pack.sizes))) < 0.5
        assert 0 < mask.sum() < mask.size
        for include in MODES + (mask,):
            for ref in (ligand, None):
                assert_same_report(pack.pocket(side, include, ref), quality.sample_pocket(as_dict, 'all', include, ref, device='cpu'))
                assert_same_report(pack.interactions(side, include, ref), quality.sample_interactions(as_dict, 'all', include, ref, device='cpu'))
                assert_same_report(pack.sasa(side, include, ref), quality.sample_sasa(as_dict, 'all', include, ref, device='cpu'))
        assert_same_report(pack.pocket(side, 'all', ligand, kinds='element'), quality.sample_pocket(as_dict, 'all', 'all', ligand, kinds='element', device='cpu'))
        # the readers of the one decode are the public functions
        feat = pockets[i].protein_atom_feature
        for by in ('residue', 'element'):
            for hydrogens in (False, True):
                elem, kind, names = quality.pocket_kinds(feat, by, hydrogens)
                assert np.array_equal(side.kinds(by, hydrogens)[0].numpy(), kind) and side.kinds(by, hydrogens)[1] == names
                assert np.array_equal(side.elem.numpy(), elem) and kind.dtype == elem.dtype == np.int32
        assert np.array_equal(side.roles().numpy(), quality.pocket_roles(feat)) and np.array_equal(side.roles().numpy(), IR.pocket_roles(feat.numpy()))


def test_a_result_file_decodes_and_uploads_its_pocket_once_and_packs_the_reference_once(pocket_bindings, tmp_path, monkeypatch, capsys):
    """counts of calls, not times: before the reports shared a pocket they were 4, 3 and 4 per file"""
    saved(tmp_path)
    seen = dict(pocket_of=0, uploads=0, reference=0)
    pocket_of, fp32, pack = quality.pocket_of, quality._fp32_positions, quality._pack

    def counted_pocket_of(data):
        seen['pocket_of'] += 1
        return pocket_of(data)

    def counted_fp32(pos, device):
        seen['uploads'] += int(pos.ndim == 2 and pos.shape[0] in (45, 60))      # the two pockets; the reference ligand has 6 atoms
        return fp32(pos, device)

    def counted_pack(pos, *a):
        seen['reference'] += int(pos.ndim == 2)                                 # a result's pack is [S, N_l, 3]
        return pack(pos, *a)

    monkeypatch.setattr(quality, 'pocket_of', counted_pocket_of)
    monkeypatch.setattr(quality, '_fp32_positions', counted_fp32)
    monkeypatch.setattr(quality, '_pack', counted_pack)
    for include in MODES:
        seen.update(pocket_of=0, uploads=0, reference=0)
        run_tool(tmp_path, monkeypatch, capsys, pocket_bindings, include)
        assert seen == dict(pocket_of=2, uploads=2, reference=2), include       # two files: one decode, one upload, one packing each


# what the hand-written ``merged`` of every class did with every constructor argument before the classes shared a base: added over the
# reports, carried from the first, kept only for a single report (a per-pocket map), or added only with a reference ligand
MERGES = {
    quality.RingReport: dict(added=('ring_hist', 'n_included', 'n_large', 'sum_atom_share', 'n_nonempty', 'n_samples')),
    quality.DiversityReport: dict(added=('sum_diversity', 'n_diversity', 'sum_nearest', 'sum_uniqueness', 'n_unique', 'n_included', 'n_distinct',
                                         'n_samples'), reference=('sum_ref', 'n_ref')),
    quality.PocketReport: dict(added=('n_included', 'n_clash_free', 'sum_clashes', 'sum_contacts', 'n_no_contact', 'sum_buried', 'n_nonempty',
                                      'sum_min_dist', 'n_min_dist', 'kind_hist', 'n_samples'), carried=('names', 'backbone'),
                               single=('pocket_freq',), reference=('sum_ref', 'n_ref')),
    quality.InteractionReport: dict(added=('n_included', 'sum_hbonds', 'sum_donated', 'sum_accepted', 'sum_hydrophobic', 'n_no_hbond',
                                           'sum_hb_atoms', 'sum_polar_atoms', 'kind_hist', 'n_samples'), carried=('names',),
                                    single=('pocket_freq',), reference=('sum_ref', 'n_ref')),
    quality.SasaReport: dict(added=('n_included', 'sum_free', 'sum_bound', 'sum_buried', 'sum_share', 'n_nothing', 'sum_pocket', 'n_samples'),
                             carried=('points', 'probe'), single=('pocket_buried_sum',), reference=('sum_own', 'n_own', 'sum_ref', 'n_ref')),
}
CARRIED = dict(names=('x.sc', 'x.bb'), backbone=[False, True], points=96, probe=1.4)


@pytest.mark.parametrize('cls', list(MERGES), ids=lambda c: c.__name__)
def test_merged_treats_every_field_as_the_hand_written_merges_did(cls):
    how = dict(dict(added=(), carried=(), single=(), reference=()), **MERGES[cls])
    assert sorted(sum(how.values(), ())) == sorted(name for name, _ in cls.FIELDS)      # every constructor argument is in the table

    def report(k, reference=True):
        """planted values that differ from report to report; a sum is an int for n_samples and a [2] array otherwise"""
        kw = {name: (3 + k if name == 'n_samples' else np.asarray([1 + k, 10 * (k + 2)])) for name in how['added']}
        kw.update({name: CARRIED[name] for name in how['carried']}, **{name: np.asarray([[k, 7, 2 * k]] * 2) for name in how['single']})
        if reference:
            kw.update({name: np.asarray([k + 1, 4]) for name in how['reference']})
        return cls(**kw)

    def same(x, y):
        return np.array_equal(x, y) if isinstance(x, np.ndarray) or isinstance(y, np.ndarray) else x == y

    a, b, c = report(0), report(1), report(2)
    for reports, flat in (([a, b], [a, b]), ([a, b, c], [a, b, c]), ([cls.merged([a, b]), c], [a, b, c])):      # a merged report merges again
        m = cls.merged(reports)
        for name in how['added'] + how['reference']:
            assert same(getattr(m, name), sum(getattr(r, name) for r in flat)), name
        for name in how['carried']:
            assert same(getattr(m, name), getattr(a, name)) and type(getattr(m, name)) is type(getattr(a, name)), name
        for name in how['single']:
            assert getattr(m, name) is None, name
    one = cls.merged([b])
    for name, _ in cls.FIELDS:
        assert same(getattr(one, name), getattr(b, name)), name                 # a single report keeps everything, its map too
    plain = cls.merged([report(0, False), report(1, False)])
    assert all(getattr(plain, name) is None for name in how['reference'])
    if how['reference']:
        with pytest.raises(ValueError, match='do not merge'):
            cls.merged([a, report(1, False)])
    if cls is quality.SasaReport:
        assert cls.merged([a, b]).points == a.points == 96 and cls.merged([a, b]).probe == 1.4
