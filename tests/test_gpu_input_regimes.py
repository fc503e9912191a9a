"""The attention and EGNN layers over the input regimes of tests/_regime_ref.py against the float64 restatement: feature scales from 1e-6 to 1e3
(per pack and per row), exact zero rows, a spiking channel; every ligand edge beyond the last Gaussian centre, coincident atoms as real edges,
coordinates 500 A out, a lattice with exact distance ties; attention sharpened until fp32 exp underflows inside a row.  tests/test_regimes_host.py
shows on the CPU that the regimes are what they claim and that the rule bites.  Needs an MI355X: ``-m gpu``.

The rule (tests/_regime_ref.py: check): |HIP - float64| <= max(TOL_FWD, 2 x |fp32 restatement - float64|), per decade of the input rows where
they differ by orders of magnitude.  Every arithmetic variant of the attention passes is held to it on the same float64 result."""
import pytest
import torch

import _regime_ref as G
from _tol import TOL_H, maxdiff

pytestmark = pytest.mark.gpu

OPTIONS = ('edge_key_split', 'edge_first_layer_f16', 'edge_second_layer_f16')
# Cases whose h, with the second layer on f16 piece pairs (two operands carried to 22 bits instead of 24: up to 8 r64 is what the design allows),
# measured further than 2 r64 from float64 while both fp32 variants of the same case kept the rule: (measured d64 / r64, EXPERIMENTS.md).  They
# are bound at 1.5 x the measured ratio, never above 8; the fp32 variants and x stay at 2.
F16_RATIOS = {('mixed', 'cloud', 300): 2.91}
_MODELS = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


def _native_layer(s, graph, dev):
    """a one-layer NativeModel of the sharpened weights on the graph mode, as _native_with_layers of test_gpu_parity.py builds it"""
    from oracle import restatement as R
    from targetdiff_amd import capi
    if (s, graph) not in _MODELS:
        cfg = dict(dict(hidden_dim=128, n_heads=16, knn=32, num_layers=1, num_r_gaussian=20, edge_feat_dim=4, protein_feat_dim=27,
                        ligand_num_classes=13, num_timesteps=1000), **G.GRAPHS[graph])
        sched = {k: v.numpy() for k, v in R.diffusion_schedules().items()}
        with torch.cuda.device(dev):
            nat = capi.NativeModel(cfg, G.sharpened(G.base_state_dict(), s), sched, device=dev)
        assert nat.get_option('fold_fp32_mlps') == 0          # no MLP was moved to the fp32 fallback: the variants below are what they say
        _MODELS[(s, graph)] = nat
    return _MODELS[(s, graph)]


def layer_results(case, graph, dev):
    """Every HIP result of one (case, graph) next to its references: yields (variant, what, got, fp32 restatement, float64 restatement, h_in for
    the per-decade rule or None).  Also asserts what is exact: option read-back, protein rows, fix_x, reruns, the neighbour table, pad gates."""
    r = G.refine_reference(case, graph)
    nat = _native_layer(case[2], graph, dev)
    h, x, mask = r['h'].to(dev).contiguous(), r['x'].to(dev).contiguous(), G.PACK.mask.to(dev)
    ptr = nat.graph_ptr(G.PACK.batch.to(dev), len(G.PACK.sizes))
    assert ptr.cpu().tolist() == G.PACK.ptr
    h_in = r['h'] if case[0] in G.GROUPED else None
    prot = ~G.PACK.mask
    for variant in G.VARIANTS:
        for name, value in zip(OPTIONS, variant):
            nat.set_option(name, value)
            assert nat.get_option(name) == value
        default = variant == (1, 1, 1)
        want_graph = default and graph == 'knn32'
        out_h, out_x, nbr, ew = nat.refine_forward(h, x, mask, ptr, want_graph=want_graph)
        assert torch.equal(out_x.cpu()[prot], r['x'][prot]), (case, graph, variant, 'a protein row moved')
        yield variant, 'h', out_h, r['f32']['h'], r['f64']['h'], h_in
        yield variant, 'x', out_x, r['f32']['x'], r['f64']['x'], None
        if want_graph:
            assert torch.equal(nbr.cpu().long(), r['f64_nbr'])
            valid = r['f64_nbr'] >= 0
            assert bool((ew.cpu()[~valid] == 0).all())
            yield variant, 'e_w', ew.cpu()[valid], r['f32_ew'][valid], r['f64_ew'][valid], None
        if default:
            again_h, again_x, _, _ = nat.refine_forward(h, x, mask, ptr)
            assert torch.equal(again_h, out_h) and torch.equal(again_x, out_x), (case, graph, 'rerun differs')
            fix_h, fix_x, _, _ = nat.refine_forward(h, x, mask, ptr, fix_x=True)
            assert torch.equal(fix_x.cpu(), r['x']), (case, graph, 'fix_x moved an atom')
            yield variant, 'h fix_x', fix_h, r['f32_fix']['h'], r['f64_fix']['h'], h_in
    for name, value in zip(OPTIONS, G.VARIANTS[0]):
        nat.set_option(name, value)


@pytest.mark.parametrize('graph', list(G.GRAPHS))
@pytest.mark.parametrize('case', G.CASES, ids=G.case_id)
def test_refine_layer_vs_float64(case, graph):
    """One attention layer through td_refine_forward, every arithmetic variant, against float64 by the rule (factor 2).

    One exception, F16_RATIOS: mixed-cloud-s300 (one feature scale per row over nine decades, logits up to 300).  Among its rows of small input
    scale, h of the variants with the second layer on f16 piece pairs is up to 2.91 r64 from float64 (decade 1e-4, first layer on bf16 triples,
    k = 32: 7.7e-6 against r64 = 2.6e-6; the default variant 2.18 r64 at k = 48) while both fp32 variants stay inside 2 r64 (1.92 at most).  A
    logit of 300 carried to 22 bits is off by up to 7e-5, four times the fp32 rounding, and the nearly one-hot softmax passes that on to the
    weights; the design allows 8 r64.  These variants of this case are held to 1.5 x 2.91 = 4.37 r64."""
    dev = _dev()
    for variant, what, got, f32, f64, h_in in layer_results(case, graph, dev):
        floor = 1e-5 if what == 'e_w' else G.TOL_FWD
        factor = 2.0
        if case in F16_RATIOS and variant[2] == 1 and what.startswith('h'):
            factor = min(8.0, 1.5 * F16_RATIOS[case])
        ratio = G.check(got, f32, f64, (G.case_id(case), graph, variant, what), h_in=h_in, floor=floor, factor=factor)
        print(f'{G.case_id(case)} {graph} {variant} {what}: d64 / max(r64, floor / 2) = {ratio:.3f}')


@pytest.mark.parametrize('geometry', G.GEOMETRIES[1:])
def test_model_and_session_on_geometry_regimes(geometry):
    """The nine-layer model on the same pack, positions as given (no centring), against float64; the caching session, whose receptive-field
    pruning and row lists meet duplicates and 500 A offsets here, equals the stateless forward bit for bit."""
    from oracle import weights
    from targetdiff_amd import capi
    from targetdiff_amd.models import ScorePosNet3D
    dev = _dev()
    if 'full' not in _MODELS:
        m = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG), 27, 13)
        assert not m.load_state_dict(G.base_state_dict(), strict=False).unexpected_keys
        _MODELS['full'] = m.to(dev).eval()
    model = _MODELS['full']
    ref = G.model_reference(geometry)
    ppos, pv, pb, lpos, lv, lb = [t.to(dev) for t in G.model_inputs(geometry)]
    got = model(ppos, pv, pb, lpos, lv, lb)
    for key in ('pred_ligand_pos', 'pred_ligand_v', 'final_h'):
        ratio = G.check(got[key], ref['f32'][key], ref['f64'][key], (geometry, key))
        print(f'{geometry} {key}: d64 / max(r64, floor / 2) = {ratio:.3f}')
    nat = model._native(dev)
    B = len(G.PACK.sizes)
    pptr, lptr = nat.graph_ptr(pb, B), nat.graph_ptr(lb, B)
    sess = capi.NativeSession(nat, ppos, pv, pptr, lptr, lpos.shape[0])
    for _ in range(2):                                          # twice: the second call starts from the cached rows
        ps = sess.forward(lpos, lv)
        for key in ('pred_ligand_pos', 'pred_ligand_v', 'final_ligand_h'):
            assert torch.equal(ps[key], got[key]), (geometry, key, maxdiff(ps[key], got[key]))


@pytest.mark.parametrize('geometry', G.GEOMETRIES)
@pytest.mark.parametrize('feature', G.EGNN_FEATURES)
def test_egnn_layer_vs_float64(feature, geometry):
    """One EGNN layer (egnn.hip) on the 72-node graph and the (1, 1) graph.  x to max(5e-5, 2 r64), h to max(TOL_H max(1, max |h_out|), 2 r64):
    the tolerances of test_egnn_vs_reference_golden, scaled with the features as there."""
    from targetdiff_amd.egnn import EGNN
    dev = _dev()
    r = G.egnn_reference(feature, geometry)
    P = G.EGNN_PACK
    net = EGNN(num_layers=1, hidden_dim=128, edge_feat_dim=4, num_r_gaussian=1, k=32, cutoff_mode='knn')
    net.load_state_dict(r['sd'], strict=True)
    net = net.to(dev)
    args = (r['h'].to(dev), r['x'].to(dev), P.mask.to(dev), P.batch.to(dev))
    out = net(*args)
    scale = max(1.0, float(r['f64']['h'].abs().max()))
    rx = G.check(out['x'], r['f32']['x'], r['f64']['x'], (feature, geometry, 'x'), floor=5e-5)
    rh = G.check(out['h'], r['f32']['h'], r['f64']['h'], (feature, geometry, 'h'), floor=TOL_H * scale)
    print(f'egnn {feature} {geometry}: max |h_out| {scale:.3g}, d64 / max(r64, floor / 2): x {rx:.3f}, h {rh:.3f}')
    assert torch.equal(out['x'].cpu()[~P.mask], r['x'][~P.mask])
    again = net(*args)
    assert torch.equal(again['h'], out['h']) and torch.equal(again['x'], out['x'])
