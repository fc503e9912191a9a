"""Graph constructions other than the k = 32 kNN graph (models/uni_transformer.py:276-286):
k-NN with any k <= 64, `hybrid` (models/common.py:165-212) and a radius graph with a fan-out cap, through the chunked
neighbour table and the ragged (CSR-segment) edge kernels.  Needs an MI355X: ``-m gpu``.

References: goldens of the REAL reference for k in {16, 48, 64} and hybrid (it runs those); the radius mode is dead code in
the reference, so it is held to the project's rule in oracle/shims.py through the oracle restatement.
Tolerances (tests/_tol.py): neighbour sets bit-exact; one forward vs a reference golden 5e-6; teacher-forced |dx| <= 1e-5 A, |dh|, |dlogit| <= 1e-4.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden, pocket_1h36

pytestmark = pytest.mark.gpu

from _tol import TOL_X, TOL_H, TOL_FWD, TOL_TRAJ, close, maxdiff as _maxdiff


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


def _model(state_dict, **cfg):
    from oracle import weights
    from targetdiff_amd.models import ScorePosNet3D
    m = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG, **cfg), 27, 13)
    assert not m.load_state_dict(state_dict, strict=False).unexpected_keys
    return m.to(_dev()).eval()


def _rows(table):
    return [sorted(int(j) for j in r if j >= 0) for r in table.tolist()]


def _csr_rows(g):
    rp, col = g['row_ptr'], g['col']
    return [sorted(col[rp[i]:rp[i + 1]].tolist()) for i in range(len(rp) - 1)]


def _batch_for(name):
    from oracle.make_golden import small_batch
    from oracle.make_golden_r2 import hybrid_small_batch
    from targetdiff_amd import workloads
    if name == 'forward_1h36x2_hybrid':
        pocket, sizes = pocket_1h36()
        return workloads.pack_samples(pocket, 2, sizes[:2])
    return (hybrid_small_batch if 'hybrid' in name else small_batch)()[0]


def _centred_inputs(model, b, ligand_pos, dev):
    """protein centred by the library (the fixtures hold centred ligand positions), graph offsets, composed coordinates"""
    nat = model._native(dev)
    b = b.to(dev)
    B = b.num_graphs
    pptr, lptr = nat.graph_ptr(b.protein_element_batch, B), nat.graph_ptr(b.ligand_element_batch, B)
    ppos, scratch = b.protein_pos.clone(), torch.zeros(ligand_pos.shape[0], 3, device=dev)
    nat.center_pos(ppos, pptr, scratch, lptr)
    lpos = ligand_pos.to(dev)
    # compose_context order: per graph protein rows, then ligand rows
    pp, lp = pptr.cpu().tolist(), lptr.cpu().tolist()
    xs, mask, node_ptr = [], [], [0]
    for g in range(B):
        xs += [ppos[pp[g]:pp[g + 1]], lpos[lp[g]:lp[g + 1]]]
        mask += [torch.zeros(pp[g + 1] - pp[g], dtype=torch.bool), torch.ones(lp[g + 1] - lp[g], dtype=torch.bool)]
        node_ptr.append(node_ptr[-1] + pp[g + 1] - pp[g] + lp[g + 1] - lp[g])
    return (nat, b, pptr, lptr, ppos, lpos, torch.cat(xs).contiguous(), torch.cat(mask).to(dev),
            torch.tensor(node_ptr, dtype=torch.int32, device=dev))


# ------------------------------------------------------------------------------------------ k-NN with any k
@pytest.mark.parametrize('k', [1, 16, 31, 33, 48, 64])
@pytest.mark.parametrize('sizes', [[147], [40, 70, 20, 5, 1, 2], [1100, 90]])
def test_knn_any_k_bit_exact(state_dict, k, sizes):
    from oracle import shims
    dev = _dev()
    nat = _model(state_dict)._native(dev)
    g = torch.Generator().manual_seed(k * 100 + len(sizes))
    x = torch.cat([torch.randn(n, 3, generator=g) * (n ** (1 / 3)) for n in sizes])
    x[3] = x[2]                                              # exact duplicates: ties -> lower index
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    want = shims.knn_neighbours(x, k, batch)
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
    got = nat.knn(x.to(dev), ptr, k=k, max_graph_nodes=max(sizes)).cpu()
    assert torch.equal(got.long(), want)


# ------------------------------------------------------------------------------------------ reference goldens
@pytest.mark.parametrize('name,cfg', [('forward_small_k16', dict(knn=16)), ('forward_small_k48', dict(knn=48)),
                                      ('forward_small_k64', dict(knn=64)), ('forward_small_hybrid', dict(cutoff_mode='hybrid')),
                                      ('forward_1h36x2_hybrid', dict(cutoff_mode='hybrid'))])
def test_forward_other_graphs_vs_reference_golden(state_dict, name, cfg):
    from targetdiff_amd import capi
    dev = _dev()
    g = load_golden(name + '.npz')
    model = _model(state_dict, **cfg)
    nat, b, pptr, lptr, ppos, lpos, x, mask, node_ptr = _centred_inputs(model, _batch_for(name), torch.from_numpy(g['ligand_pos']), dev)
    # the graph: the reference's own edge list, as neighbour sets per dst node
    table = nat.graph_build(x, mask, node_ptr, width=128).cpu()
    assert _rows(table) == _csr_rows(g)
    lv = torch.from_numpy(g['ligand_v'].astype(np.int64)).to(dev)
    pv = b.protein_atom_feature.float()
    preds = nat.model_forward(ppos, pv, pptr, lpos, lv, lptr)
    close(preds['pred_ligand_pos'], g['pred_ligand_pos'], TOL_FWD)
    close(preds['pred_ligand_v'], g['pred_ligand_v'], TOL_FWD)
    close(preds['final_ligand_h'], g['final_ligand_h'], TOL_FWD)
    if 'final_h' in g:
        close(preds['final_h'], g['final_h'], TOL_FWD)
    else:
        close(preds['final_h'][::16], g['final_h_sample'], TOL_FWD)
    # the session of a general graph keeps the layout only: same kernels, same bits
    sess = capi.NativeSession(nat, ppos, pv, pptr, lptr, lpos.shape[0], 0)
    for _ in range(2):                                       # twice: the per-step reset of the protein rows
        ps = sess.forward(lpos, lv)
        for key in ('pred_ligand_pos', 'pred_ligand_v', 'final_ligand_h'):
            assert torch.equal(ps[key], preds[key]), key
    # the refine_net seam (mask + batch instead of separate protein / ligand arrays)
    out = model.refine_net(torch.randn(x.shape[0], 128, generator=torch.Generator().manual_seed(1)).to(dev), x, mask,
                           torch.repeat_interleave(torch.arange(b.num_graphs, device=dev), (node_ptr[1:] - node_ptr[:-1]).long()))
    assert torch.isfinite(out['h']).all() and out['x'].shape == x.shape


def test_refine_seam_hybrid_vs_oracle(state_dict):
    """td_refine_forward on a general graph (layout derived from mask + node_ptr on the host) against the restatement."""
    from oracle import restatement as R
    from oracle import weights
    from oracle.make_golden_r2 import hybrid_small_batch
    dev = _dev()
    model = _model(state_dict, cutoff_mode='hybrid')
    b, lpos, lv = hybrid_small_batch()
    _, lpos_c, _ = R.center_positions(b.protein_pos, lpos, b.protein_element_batch, b.ligand_element_batch)
    nat, bd, pptr, lptr, ppos, lposd, x, mask, node_ptr = _centred_inputs(model, b, lpos_c, dev)
    h = torch.randn(x.shape[0], 128, generator=torch.Generator().manual_seed(2))
    batch = torch.repeat_interleave(torch.arange(b.num_graphs), (node_ptr[1:] - node_ptr[:-1]).cpu().long())
    want = R.refine_forward(state_dict, dict(weights.DEFAULT_MODEL_CONFIG, cutoff_mode='hybrid'), h, x.cpu(), mask.cpu(), batch)
    got = model.refine_net(h.to(dev), x, mask, batch.to(dev))
    close(got['h'], want['h'], TOL_H)
    close(got['x'], want['x'], TOL_X)
    want_f = R.refine_forward(state_dict, dict(weights.DEFAULT_MODEL_CONFIG, cutoff_mode='hybrid'), h, x.cpu(), mask.cpu(), batch, fix_x=True)
    got_f = model.refine_net(h.to(dev), x, mask, batch.to(dev), fix_x=True)
    close(got_f['h'], want_f['h'], TOL_H)
    assert torch.equal(got_f['x'], x)


# ------------------------------------------------------------------------------------------ the C5 sweep at C5 size
@pytest.mark.parametrize('name,cfg', [('forward_c5_k48', dict(knn=48)), ('forward_c5_k64', dict(knn=64)),
                                      ('forward_c5_hybrid', dict(cutoff_mode='hybrid')),
                                      ('forward_c5_radius', dict(cutoff_mode='radius', r=6.0, max_num_neighbors=48))])
def test_forward_c5_size_general_graphs_vs_golden(state_dict, name, cfg):
    """The chunked kernels on 1000-atom graphs (oracle/make_golden_r3.py): multi-pass knn_general_kernel (graphs of 1150 / 1030
    nodes), two chunks per row at k = 48 / 64, six chunks on the 150-atom ligand's hybrid rows.  k = 48 / 64 / hybrid are the
    REAL reference's outputs and edge sets; the radius graph (dead code in the reference) is the project rule through the
    restatement (`source` in the fixture says which).  Stateless forward, then the session -- which caches the protein-only
    lists and the clean rows' gate / layer-0 output on general graphs too -- over several steps, bit for bit."""
    from oracle.make_golden_r2 import C5_POCKET, C5_SIZES
    from targetdiff_amd import capi, workloads
    dev = _dev()
    g = load_golden(name + '.npz')
    assert ('reference' == str(g['source'])) == (name != 'forward_c5_radius')
    model = _model(state_dict, **cfg)
    nat = model._native(dev)
    b = workloads.pack_samples(workloads.synthetic_pocket(**C5_POCKET), 2, C5_SIZES).to(dev)
    ppos = torch.from_numpy(g['protein_pos_centred']).to(dev)
    lpos = torch.from_numpy(g['ligand_pos']).to(dev)
    lv = torch.from_numpy(g['ligand_v'].astype(np.int64)).to(dev)
    pptr, lptr = nat.graph_ptr(b.protein_element_batch, 2), nat.graph_ptr(b.ligand_element_batch, 2)
    pv = b.protein_atom_feature.float()
    # the graph on the composed coordinates (protein rows first inside each graph)
    n0 = 1000 + C5_SIZES[0]
    x = torch.cat([ppos[:1000], lpos[:C5_SIZES[0]], ppos[1000:], lpos[C5_SIZES[0]:]]).contiguous()
    mask = torch.zeros(x.shape[0], dtype=torch.bool, device=dev)
    mask[1000:n0] = True
    mask[n0 + 1000:] = True
    node_ptr = torch.tensor([0, n0, x.shape[0]], dtype=torch.int32, device=dev)
    if name == 'forward_c5_radius':
        table = nat.graph_build(x, mask, node_ptr, width=48).cpu().long()
        assert torch.equal(table, torch.from_numpy(g['table'].astype(np.int64)))     # index order is part of the rule
    else:
        table = nat.graph_build(x, mask, node_ptr, width=192).cpu()
        assert _rows(table) == _csr_rows({'row_ptr': g['row_ptr'], 'col': g['col'].astype(np.int64)})
    preds = nat.model_forward(ppos, pv, pptr, lpos, lv, lptr, max_graph_nodes=n0)
    print(f'{name}: |dx| {_maxdiff(preds["pred_ligand_pos"], g["pred_ligand_pos"]):.2e}  |dh| '
          f'{_maxdiff(preds["final_h"][::16], g["final_h_sample"]):.2e}')
    close(preds['pred_ligand_pos'], g['pred_ligand_pos'], TOL_FWD)
    close(preds['pred_ligand_v'], g['pred_ligand_v'], TOL_FWD)
    close(preds['final_ligand_h'], g['final_ligand_h'], TOL_FWD)
    close(preds['final_h'][::16], g['final_h_sample'], TOL_FWD)
    sess = capi.NativeSession(nat, ppos, pv, pptr, lptr, lpos.shape[0], n0)
    for _ in range(2):
        ps = sess.forward(lpos, lv)
        for key in ('pred_ligand_pos', 'pred_ligand_v', 'final_ligand_h'):
            assert torch.equal(ps[key], preds[key]), key
    # move the ligands (another set of clean rows), come back: the session must track the stateless forward bit for bit
    lpos2 = lpos + 0.7 * torch.randn(lpos.shape, generator=torch.Generator().manual_seed(5)).to(dev)
    want2 = nat.model_forward(ppos, pv, pptr, lpos2, lv, lptr, max_graph_nodes=n0)
    got2 = sess.forward(lpos2, lv)
    for key in ('pred_ligand_pos', 'pred_ligand_v', 'final_ligand_h'):
        assert torch.equal(got2[key], want2[key]), key
    got3 = sess.forward(lpos, lv)
    assert torch.equal(got3['pred_ligand_pos'], preds['pred_ligand_pos'])


def test_sampling_hybrid_20_steps_vs_reference(state_dict):
    """20 reverse steps (t = 999 .. 980) of the REAL reference's loop on 1h36 x 2 with cutoff_mode = 'hybrid' and the counter
    draws: sampling on a general graph against the reference itself, through the session and the stateless forward."""
    from oracle import draws
    from targetdiff_amd import workloads
    dev = _dev()
    g = load_golden('sample_1h36x2_hybrid_20.npz')
    model = _model(state_dict, cutoff_mode='hybrid')
    pocket, _ = pocket_1h36()
    b = workloads.pack_samples(pocket, 2, g['sizes']).to(dev)
    outs = []
    for use_session in (True, False):
        r = model.sample_diffusion(b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch,
                                   torch.from_numpy(g['init_ligand_pos']).to(dev),
                                   torch.from_numpy(g['init_ligand_v'].astype(np.int64)).to(dev), b.ligand_element_batch,
                                   num_steps=20, center_pos_mode='protein', noise_source=draws.Source(int(g['draws_base']), dev),
                                   use_session=use_session)
        v = torch.stack(r['v_traj']).numpy()
        assert np.array_equal(v, g['v_traj'].astype(np.int64))
        dx = _maxdiff(torch.stack(r['pos_traj']), g['pos_traj'])
        print(f'hybrid 20 steps ({"session" if use_session else "stateless"}): max |dx| = {dx:.2e}')
        assert dx <= 5e-5
        for j, s in enumerate(g['kept_steps']):
            close(r['v0_traj'][int(s)], g['v0_traj'][j], TOL_H)
        outs.append(r)
    assert torch.equal(outs[0]['pos'], outs[1]['pos'])


# ------------------------------------------------------------------------------------------ radius graph with fan-out cap
@pytest.mark.parametrize('r,cap', [(4.0, 16), (5.0, 32), (6.5, 48), (30.0, 64), (0.5, 32)])
def test_radius_graph_and_forward_vs_oracle(state_dict, r, cap):
    from oracle import restatement as R
    from oracle import shims, weights
    from oracle.make_golden import small_batch
    dev = _dev()
    model = _model(state_dict, cutoff_mode='radius', r=r, max_num_neighbors=cap)
    b, lpos, lv = small_batch()
    ppos_c, lpos_c, _ = R.center_positions(b.protein_pos, lpos, b.protein_element_batch, b.ligand_element_batch)
    nat, bd, pptr, lptr, ppos, lposd, x, mask, node_ptr = _centred_inputs(model, b, lpos_c, dev)
    batch = torch.repeat_interleave(torch.arange(b.num_graphs), (node_ptr[1:] - node_ptr[:-1]).cpu().long())
    want_tab = shims.radius_neighbours(x.cpu(), r, batch, cap)
    got_tab = nat.graph_build(x, mask, node_ptr, width=cap).cpu().long()
    assert torch.equal(got_tab, want_tab)                    # index order is part of the rule: compare as is
    full = dict(weights.DEFAULT_MODEL_CONFIG, cutoff_mode='radius', r=r, max_num_neighbors=cap)
    want = R.model_forward(state_dict, full, ppos.cpu(), b.protein_atom_feature.float(), b.protein_element_batch, lpos_c, lv,
                           b.ligand_element_batch)
    got = nat.model_forward(ppos, bd.protein_atom_feature.float(), pptr, lposd, lv.to(dev), lptr)
    close(got['pred_ligand_pos'], want['pred_ligand_pos'], TOL_X)
    close(got['pred_ligand_v'], want['pred_ligand_v'], TOL_H)
    close(got['final_h'], want['final_h'], TOL_H)


# ------------------------------------------------------------------------------------------ sampling on a general graph
@pytest.mark.parametrize('cfg', [dict(cutoff_mode='hybrid'), dict(knn=48), dict(knn=16), dict(knn=5),
                                 dict(cutoff_mode='radius', r=5.0, max_num_neighbors=24),
                                 dict(cutoff_mode='radius', r=6.0, max_num_neighbors=40)])
def test_sampling_steps_on_general_graph_vs_oracle(state_dict, cfg):
    """5 reverse steps with injected draws through the sampler against the restatement's loop.  hybrid / k = 48: the plain
    session of the chunked path; k = 16 / 5: the caching session of the 32-slot path with the slots >= k masked (merged
    k-NN lists, cached gate / layer-0 rows, receptive-field pruning), which must equal the stateless forward bit for bit."""
    from oracle import draws
    from oracle import restatement as R
    from oracle import weights
    from oracle.make_golden_r2 import hybrid_small_batch
    dev = _dev()
    model = _model(state_dict, **cfg)
    b, lpos, lv = hybrid_small_batch()
    src = draws.Source(5100)
    nl = lpos.shape[0]
    noises = torch.stack([src.noise(s, (nl, 3)) for s in range(5)])
    unis = torch.stack([src.uniform(s, (nl, 13)) for s in range(5)])
    want = R.sample_diffusion(state_dict, dict(weights.DEFAULT_MODEL_CONFIG, **cfg), b.protein_pos, b.protein_atom_feature.float(),
                              b.protein_element_batch, lpos, lv, b.ligand_element_batch, num_steps=5, noises=noises,
                              uniforms=unis, record=True)
    bd = b.to(dev)
    outs = []
    for use_session in (True, False):
        r = model.sample_diffusion(bd.protein_pos, bd.protein_atom_feature.float(), bd.protein_element_batch, lpos.to(dev),
                                   lv.to(dev), bd.ligand_element_batch, num_steps=5, center_pos_mode='protein',
                                   noise_source=draws.Source(5100, dev), use_session=use_session)
        assert torch.equal(torch.stack(r['v_traj']), torch.stack(want['v_traj']))
        close(torch.stack(r['pos_traj']), torch.stack(want['pos_traj']), 5e-5)
        outs.append(r)
    assert torch.equal(outs[0]['pos'], outs[1]['pos'])


def test_model_options_live_in_the_handle(state_dict):
    """node_proj_split / h2x_fused / edge_key_split are per-model switches (no environment variables): both settings of each
    reproduce the reference golden, fp32 MFMA and exact bf16 x 3 splitting to the same tolerance."""
    from conftest import small_inputs
    dev = _dev()
    g = load_golden('forward_small.npz')
    inp = {k: v.to(dev) for k, v in small_inputs(g).items()}
    res = {}
    for split in (1, 0):
        for fused in (1, 0):
            model = _model(state_dict)
            nat = model._native(dev)
            assert nat.get_option('node_proj_split') == 1 and nat.get_option('h2x_fused') == 1       # shipped defaults
            nat.set_option('node_proj_split', split)
            nat.set_option('h2x_fused', fused)
            p = model(inp['protein_pos'], inp['protein_v'], inp['batch_protein'], inp['ligand_pos'], inp['ligand_v'], inp['batch_ligand'])
            res[(split, fused)] = p
            close(p['pred_ligand_pos'], g['pred_ligand_pos'], TOL_X)
            close(p['final_h'], g['final_h'], TOL_H)
            print(f'split={split} fused={fused}: |dx| = {_maxdiff(p["pred_ligand_pos"], g["pred_ligand_pos"]):.2e}  '
                  f'|dh| = {_maxdiff(p["final_h"], g["final_h"]):.2e}')
    assert torch.equal(res[(1, 1)]['final_h'], res[(1, 0)]['final_h'])          # fusing the h2x halves changes no arithmetic
    with pytest.raises(RuntimeError, match='unknown option'):
        nat.set_option('no_such_switch', 1)
    # the runs above had the x2h passes' radial/type first layer on bf16 piece triples (edge_key_split, default 1): fp32 MFMA
    for fused in (1, 0):
        model = _model(state_dict)
        nat = model._native(dev)
        assert nat.get_option('edge_key_split') == 1
        nat.set_option('edge_key_split', 0)
        nat.set_option('h2x_fused', fused)
        assert nat.get_option('edge_key_split') == 0
        p = model(inp['protein_pos'], inp['protein_v'], inp['batch_protein'], inp['ligand_pos'], inp['ligand_v'], inp['batch_ligand'])
        print(f'edge_key_split=0 fused={fused}: |dx| = {_maxdiff(p["pred_ligand_pos"], g["pred_ligand_pos"]):.2e}  '
              f'|dh| = {_maxdiff(p["final_h"], g["final_h"]):.2e}  vs bf16 x 3 first layer '
              f'{float((p["final_h"] - res[(1, fused)]["final_h"]).abs().max()):.2e}')
        close(p['pred_ligand_pos'], g['pred_ligand_pos'], TOL_X)
        close(p['final_h'], g['final_h'], TOL_H)


def test_row_distribution_settings_are_bit_identical(state_dict):
    """edge_row_dealing = 0 (contiguous shares) / 1 (dealt, fixed sequence per wave) / 2 (dealt, rows handed to the workgroup's waves
    through an LDS counter; default): which wave runs a row changes nothing in its arithmetic.  32 pockets x 8 samples (83 k nodes:
    every wave draws several rows), k-NN and hybrid graphs (32-slot and chunk-walking kernels), the stateless forward and two
    session steps, bit for bit."""
    from oracle.make_golden_r2 import c3_pockets
    from targetdiff_amd import workloads
    dev = _dev()
    b = workloads.pack_samples(c3_pockets(), 8, [25] * 256)
    lpos, lv = workloads.init_ligand(b, generator=torch.Generator().manual_seed(5), spread=2.0)
    b = b.to(dev)
    for cfg in ({}, {'cutoff_mode': 'hybrid'}):
        outs = []
        for deal in (2, 1, 0):
            model = _model(state_dict, **cfg)
            nat = model._native(dev)
            assert nat.get_option('edge_row_dealing') == 2            # shipped default
            nat.set_option('edge_row_dealing', deal)
            o = model(b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch, lpos.to(dev), lv.to(dev), b.ligand_element_batch)
            smp = model.begin_sampling(b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch, lpos.to(dev), lv.to(dev),
                                       b.ligand_element_batch, num_steps=2, center_pos_mode='protein',
                                       noise_source=lambda s, name, like: torch.full_like(like, 0.25))
            smp.step(); smp.step()
            outs.append((o['final_h'].clone(), o['pred_ligand_pos'].clone(), smp.lpos.clone(), smp.lv.clone()))
        for o in outs[1:]:
            assert all(torch.equal(x, y) for x, y in zip(o, outs[0])), cfg


def test_workgroup_trace_hook(state_dict):
    """td_debug_wg_trace (include/targetdiff_hip.h): a traced forward leaves ordered stamps for every workgroup that ran in the x2h
    key / value and fused h2x launches, changes no result, and switches off again."""
    import ctypes
    from conftest import small_inputs
    from targetdiff_amd import capi
    dev = _dev()
    g = load_golden('forward_small.npz')
    inp = {k: v.to(dev) for k, v in small_inputs(g).items()}
    model = _model(state_dict)
    call = lambda: model(inp['protein_pos'], inp['protein_v'], inp['batch_protein'], inp['ligand_pos'], inp['ligand_v'], inp['batch_ligand'])
    want = call()['final_h'].clone()
    slots = 9
    buf = torch.zeros(slots, 3, 256, 8, dtype=torch.int64, device=dev)
    buf[..., 2] = torch.iinfo(torch.int64).max
    lib = capi.load_library()
    assert lib.td_debug_wg_trace(ctypes.c_void_p(buf.data_ptr()), slots) == 0
    try:
        got = call()['final_h'].clone()
        torch.cuda.synchronize()
    finally:
        lib.td_debug_wg_trace(None, 0)
    assert torch.equal(got, want)
    t = buf.cpu()
    for p in range(3):
        ran = t[:, p, :, 1] > 0
        assert ran.any(dim=1).all()                              # every layer's launch of the pass left stamps
        entry, start, end, first, total = (t[:, p, :, k][ran] for k in (4, 0, 1, 2, 3))
        assert (entry <= start).all() and (start <= end).all() and (entry <= first).all() and (first <= end).all() and (total > 0).all()
    before = buf.clone()
    call()
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                              # off again: nothing written


def test_sampling_with_fp32_edge_first_layer(state_dict):
    """edge_key_split = 0 (radial/type first layer on fp32 MFMA) stays a tested path: 5 reverse steps through the session and
    the stateless forward against the default (bf16 piece triples): same types, positions within the sampling tolerance, and
    session == stateless bit for bit under either setting."""
    from oracle import draws
    from oracle.make_golden_r2 import hybrid_small_batch
    dev = _dev()
    b, lpos, lv = hybrid_small_batch()
    bd = b.to(dev)
    res = {}
    for split in (1, 0):
        for use_session in (True, False):
            model = _model(state_dict)
            model._native(dev).set_option('edge_key_split', split)
            res[(split, use_session)] = model.sample_diffusion(
                bd.protein_pos, bd.protein_atom_feature.float(), bd.protein_element_batch, lpos.to(dev), lv.to(dev),
                bd.ligand_element_batch, num_steps=5, center_pos_mode='protein', noise_source=draws.Source(77, dev),
                use_session=use_session)
        assert torch.equal(res[(split, True)]['pos'], res[(split, False)]['pos'])
    assert torch.equal(torch.stack(res[(1, True)]['v_traj']), torch.stack(res[(0, True)]['v_traj']))
    close(torch.stack(res[(1, True)]['pos_traj']), torch.stack(res[(0, True)]['pos_traj']), 5e-5)


@pytest.mark.parametrize('opt', ['edge_second_layer_f16', 'edge_first_layer_f16'])
@pytest.mark.parametrize('cfg', [dict(), dict(cutoff_mode='hybrid'), dict(knn=48)], ids=['knn32', 'hybrid', 'knn48'])
def test_sampling_with_fp32_second_layer(state_dict, cfg, opt):
    """edge_second_layer_f16 = 0 (logits and alpha^T z on the fp32 matrix instruction instead of f16 piece pairs) and edge_first_layer_f16 = 0
    (the radial / type first layer of the x2h passes on the exact bf16 piece triples instead of f16 piece pairs) stay tested paths: 5 reverse
    steps through the session and the stateless forward against the default -- same types, positions within the sampling tolerance, session ==
    stateless bit for bit under either setting.  On the default graph, on a `hybrid` graph (protein rows through the default graph's kernels,
    ligand rows through the chunk walk) and at k = 48 (chunk walk: the value pass follows the option; the key pass takes f16 logits only while
    edge_first_layer_f16 and edge_second_layer_f16 are both on, fp32 logits otherwise -- launch_key16_walk, edge16.hip).  (That
    the option is live -- the two settings do not produce identical features -- is asserted in
    tests/test_gpu_weight_regimes.py::test_forward_weight_regimes_vs_reference.)"""
    from oracle import draws
    from oracle.make_golden_r2 import hybrid_small_batch
    dev = _dev()
    b, lpos, lv = hybrid_small_batch()
    bd = b.to(dev)
    res = {}
    for l2 in (1, 0):
        for use_session in (True, False):
            model = _model(state_dict, **cfg)
            assert model._native(dev).get_option(opt) == 1            # shipped default
            model._native(dev).set_option(opt, l2)
            res[(l2, use_session)] = model.sample_diffusion(
                bd.protein_pos, bd.protein_atom_feature.float(), bd.protein_element_batch, lpos.to(dev), lv.to(dev),
                bd.ligand_element_batch, num_steps=5, center_pos_mode='protein', noise_source=draws.Source(77, dev),
                use_session=use_session)
        assert torch.equal(res[(l2, True)]['pos'], res[(l2, False)]['pos'])
    assert torch.equal(torch.stack(res[(1, True)]['v_traj']), torch.stack(res[(0, True)]['v_traj']))
    close(torch.stack(res[(1, True)]['pos_traj']), torch.stack(res[(0, True)]['pos_traj']), 5e-5)


@pytest.mark.parametrize('seed,gain', [(7, 1.8), (11, 0.5)])
def test_forward_other_weight_scales_vs_reference(seed, gain):
    """Parity must not depend on the one seeded weight set the fixtures use: other seeds and weight scales (stronger /
    weaker non-linearity, larger coordinate updates) against the REAL reference's outputs (forward_small_seed*.npz,
    oracle/make_golden_r3.py) and, beside it, the oracle restatement."""
    from oracle import restatement as R
    from oracle import weights
    from oracle.make_golden import small_batch
    dev = _dev()
    g = load_golden(f'forward_small_seed{seed}.npz')
    assert float(g['gain']) == gain
    sd = weights.make_state_dict(seed, gain=gain)
    model = _model(sd)
    b, lpos, lv = small_batch()
    ppos, lpos_c = torch.from_numpy(g['protein_pos_centred']), torch.from_numpy(g['ligand_pos'])
    got = model(ppos.to(dev), b.protein_atom_feature.float().to(dev), b.protein_element_batch.to(dev), lpos_c.to(dev), lv.to(dev),
                b.ligand_element_batch.to(dev))
    scale = max(1.0, float(np.abs(g['final_h']).max()))
    print(f'seed {seed} gain {gain}: vs reference |dx| {_maxdiff(got["pred_ligand_pos"], g["pred_ligand_pos"]):.2e}  '
          f'|dh| {_maxdiff(got["final_h"], g["final_h"]):.2e} (max |h| {scale:.1f})')
    close(got['pred_ligand_pos'], g['pred_ligand_pos'], TOL_X * scale)
    close(got['final_h'], g['final_h'], TOL_H * scale)
    close(got['pred_ligand_v'], g['pred_ligand_v'], TOL_H * scale)
    want = R.model_forward(sd, None, ppos, b.protein_atom_feature.float(), b.protein_element_batch, lpos_c, lv, b.ligand_element_batch)
    close(got['final_h'], want['final_h'], TOL_H * scale)


@pytest.mark.parametrize('sizes', [[(1, 1)], [(3, 2)], [(1, 1), (40, 1), (2, 9)], [(33, 1), (1, 30)], [(200, 24)] * 3])
def test_forward_and_sampling_on_tiny_and_lopsided_batches(state_dict, sizes):
    """Launch shapes at the small end: graphs of one protein and one ligand atom, rows with a single in-edge, batches where the
    ligand rows outnumber the protein rows, a handful of rows per launch (fewer rows than waves; the value pass must still
    give each destination class a workgroup).  Forward against the oracle; 3 sampling steps session == stateless bit for bit."""
    from oracle import draws
    from oracle import restatement as R
    dev = _dev()
    gen = torch.Generator().manual_seed(1234 + len(sizes) * 17 + sizes[0][0])
    ppos, lpos, pb, lb = [], [], [], []
    for gi, (n_p, n_l) in enumerate(sizes):
        ppos.append(torch.randn(n_p, 3, generator=gen) * 4.0)
        lpos.append(torch.randn(n_l, 3, generator=gen) * 1.5)
        pb += [gi] * n_p
        lb += [gi] * n_l
    ppos, lpos = torch.cat(ppos), torch.cat(lpos)
    pb, lb = torch.tensor(pb), torch.tensor(lb)
    pv = torch.zeros(len(pb), 27)
    pv[torch.arange(len(pb)), torch.randint(0, 6, (len(pb),), generator=gen)] = 1.0
    pv[torch.arange(len(pb)), 6 + torch.randint(0, 20, (len(pb),), generator=gen)] = 1.0
    lv = torch.randint(0, 13, (len(lb),), generator=gen)
    model = _model(state_dict)
    ppos_c, lpos_c, _ = R.center_positions(ppos, lpos, pb, lb)
    want = R.model_forward(state_dict, None, ppos_c, pv, pb, lpos_c, lv, lb)
    got = model(ppos_c.to(dev), pv.to(dev), pb.to(dev), lpos_c.to(dev), lv.to(dev), lb.to(dev))
    close(got['pred_ligand_pos'], want['pred_ligand_pos'], TOL_X)
    close(got['pred_ligand_v'], want['pred_ligand_v'], TOL_H)
    close(got['final_h'], want['final_h'], TOL_H)
    outs = []
    for use_session in (True, False):
        outs.append(model.sample_diffusion(ppos.to(dev), pv.to(dev), pb.to(dev), lpos.to(dev), lv.to(dev), lb.to(dev), num_steps=3,
                                           center_pos_mode='protein', noise_source=draws.Source(31, dev), use_session=use_session))
    assert torch.equal(outs[0]['pos'], outs[1]['pos']) and torch.equal(outs[0]['v'], outs[1]['v'])
    assert bool(torch.isfinite(outs[0]['pos']).all())
