"""Parity of the HIP path (through the C ABI) against the oracle restatement and against the golden
vectors of the real reference.  Needs an MI355X: run with ``-m gpu``.

Tolerances (fp32, stated once in tests/_tol.py): neighbour indices and sampled atom types bit-exact; one forward pass against a
reference golden 5e-6 (positions in A, features and logits alike); teacher-forced steps |dx| <= 1e-5 A on
coordinates, |dh|, |dlogit| <= 1e-4 on features / type logits (the re-association noise floor of one
reference forward is ~4e-7 A / 8e-7).
"""
import numpy as np
import pytest
import torch

from conftest import load_golden, small_inputs, pocket_1h36

pytestmark = pytest.mark.gpu

from _tol import TOL_X, TOL_H, TOL_FWD, close, maxdiff as _maxdiff      # 1e-5 A / 1e-4 teacher-forced, 5e-6 for one forward vs a golden


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def model(state_dict):
    from oracle import weights
    from targetdiff_amd.models import ScorePosNet3D
    dev = _dev()
    m = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG), 27, 13)
    res = m.load_state_dict(state_dict, strict=False)
    assert not res.unexpected_keys
    return m.to(dev).eval()


def _native_with_layers(state_dict, num_layers, dev):
    from oracle import weights
    from targetdiff_amd import capi
    cfg = dict(hidden_dim=128, n_heads=16, knn=32, num_layers=num_layers, num_r_gaussian=20, edge_feat_dim=4,
               protein_feat_dim=27, ligand_num_classes=13, num_timesteps=1000)
    from oracle import restatement as R
    sched = {k: v.numpy() for k, v in R.diffusion_schedules().items()}
    with torch.cuda.device(dev):
        return capi.NativeModel(cfg, state_dict, sched, device=dev)


# ------------------------------------------------------------------------------------------ device helpers
def test_cross_lane_reductions():
    """DPP / permlane32 reduction helpers used by the softmax and LayerNorm code paths (integer-valued inputs:
    every partial sum is exact in fp32, so the comparison is bit exact)."""
    from ctypes import c_void_p
    from targetdiff_amd import capi
    dev = _dev()
    lib = capi.load_library()
    g = torch.Generator().manual_seed(4)
    x = torch.randint(-1000, 1000, (64,), generator=g).float()
    out = torch.empty(6, 64, device=dev)
    xd = x.to(dev)
    rc = lib.td_debug_reductions(c_void_p(xd.data_ptr()), c_void_p(out.data_ptr()), c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    out = out.cpu()
    assert torch.equal(out[0], x.view(8, 8).sum(1, keepdim=True).expand(8, 8).reshape(64))
    assert torch.equal(out[1], x.view(2, 32).sum(1, keepdim=True).expand(2, 32).reshape(64))
    assert torch.equal(out[2], x.sum().expand(64))
    assert torch.equal(out[3], (x[:32] + x[32:]).repeat(2))
    assert torch.equal(out[4], torch.maximum(x[:32], x[32:]).repeat(2))
    assert torch.equal(out[5], torch.cat([x[32:], x[:32]]))


# ------------------------------------------------------------------------------------------ graph ops
def test_graph_ptr(model):
    dev = _dev()
    nat = model._native(dev)
    batch = torch.tensor([0, 0, 0, 2, 2, 3, 5, 5, 5, 5], device=dev)
    ptr = nat.graph_ptr(batch, 7).cpu().tolist()
    assert ptr == [0, 3, 3, 5, 6, 6, 10, 10]


@pytest.mark.parametrize('sizes', [[147], [40, 33, 32, 5, 1, 2], [700], [1100, 90], [64, 65, 63, 128, 129]])
def test_knn_bit_exact(model, sizes):
    from oracle import shims
    dev = _dev()
    nat = model._native(dev)
    g = torch.Generator().manual_seed(sum(sizes))
    x = torch.randn(sum(sizes), 3, generator=g) * 6.0
    x[3] = x[1]                                # exact duplicate: ties resolved towards the lower index
    if sum(sizes) > 50:
        x[17] = x[40]
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    want = shims.knn_neighbours(x, 32, batch)
    ptr = nat.graph_ptr(batch.to(dev), len(sizes))
    for hint in (0, max(sizes)):
        got = nat.knn(x.to(dev), ptr, 32, hint).cpu().long()
        np.testing.assert_array_equal(got.numpy(), want.numpy())


def test_knn_1h36_real_geometry(model):
    from oracle import shims
    from targetdiff_amd import workloads
    dev = _dev()
    nat = model._native(dev)
    g = load_golden('forward_1h36x2.npz')
    pocket, _ = pocket_1h36()
    b = workloads.pack_samples(pocket, 2, g['sizes'])
    # composed order: per graph [protein..., ligand...]
    from oracle import restatement as R
    ppos, _, _ = R.center_positions(b.protein_pos, torch.zeros(len(b.ligand_element_batch), 3),
                                    b.protein_element_batch, b.ligand_element_batch)
    _, pos, batch_all, _ = R.compose_context(torch.zeros(len(ppos), 1), torch.zeros(len(g['ligand_pos']), 1), ppos,
                                             torch.from_numpy(g['ligand_pos']), b.protein_element_batch,
                                             b.ligand_element_batch)
    ptr = nat.graph_ptr(batch_all.to(dev), 2)
    got = nat.knn(pos.to(dev).contiguous(), ptr, 32, 0).cpu().numpy()
    np.testing.assert_array_equal(got, g['nbr'])          # == what the real reference ran on


# ------------------------------------------------------------------------------------------ node GEMMs
def test_node_stage_projections(model, state_dict):
    dev = _dev()
    nat = model._native(dev)
    g = torch.Generator().manual_seed(3)
    for N in (1, 37, 128, 300):
        h = torch.randn(N, 128, generator=g)
        for layer, stage in ((0, 0), (4, 1), (8, 0)):
            P, q = nat.debug_node_stage(layer, stage, h.to(dev))
            names = ('hk_func', 'hv_func', 'hq_func') if stage == 0 else ('xk_func', 'xv_func', 'xq_func')
            pre = f'refine_net.base_block.{layer}.' + ('x2h_layers.0.' if stage == 0 else 'h2x_layers.0.')
            hd = h.double()
            want = []
            for nm in names[:2]:
                w0 = state_dict[pre + nm + '.net.0.weight'].double()
                b0 = state_dict[pre + nm + '.net.0.bias'].double()
                # the projections come out in the folded form the edge MLPs' LayerNorm is packed for (FoldedMlp, csrc/pack.cpp):
                # centred over the hidden units, times the sign of the LayerNorm weight
                sg = torch.where(state_dict[pre + nm + '.net.1.weight'].double() < 0, -1.0, 1.0)
                fold = lambda p: sg * (p - p.mean(dim=1, keepdim=True))
                want.append(fold(hd @ w0[:, 84:212].T + b0))
                want.append(fold(hd @ w0[:, 212:340].T))
            want = torch.cat(want, dim=1)
            # the whole first layer of an edge MLP is packed in units of 2^e, the power of two that puts the largest folded per-edge
            # weight (type + radial columns) into [2^13, 2^14): the f16 piece-pair tables of the attention kernels need it there, and their
            # products accumulate onto these projections (FoldedMlp::first_scale_exp, csrc/pack.cpp); the activations are scale-free
            P = P.clone()
            for seg, nm in enumerate(names[:2]):
                w0 = state_dict[pre + nm + '.net.0.weight'].double()
                sg = torch.where(state_dict[pre + nm + '.net.1.weight'].double() < 0, -1.0, 1.0)
                edge = (sg[:, None] * (w0[:, :84] - w0[:, :84].mean(dim=0, keepdim=True))).float().abs().max().item()
                e = 13 - int(np.floor(np.log2(edge)))
                P[:, 256 * seg:256 * (seg + 1)] = torch.ldexp(P[:, 256 * seg:256 * (seg + 1)], torch.tensor(-e, device=P.device))
            close(P, want, 5e-5, (N, layer, stage))
            from oracle import restatement as R
            qw = R._mlp(state_dict, pre + names[2], hd, torch.float64)
            close(q, qw, 5e-5, (N, layer, stage))


# ------------------------------------------------------------------------------------------ backbone stages
def _compose_small(state_dict, g):
    from oracle import restatement as R
    import torch.nn.functional as F
    inp = small_inputs(g)
    col = {}
    out = R.model_forward(state_dict, None, inp['protein_pos'], inp['protein_v'], inp['batch_protein'],
                          inp['ligand_pos'], inp['ligand_v'], inp['batch_ligand'], collect=col)
    return inp, out, col


def test_refine_first_layer_stagewise(state_dict, golden_small):
    """num_layers = 1 model through td_refine_forward: neighbour table bit exact, gate, h and x after layer 0."""
    from oracle import restatement as R
    import torch.nn.functional as F
    dev = _dev()
    g = golden_small
    inp = small_inputs(g)
    nat1 = _native_with_layers(state_dict, 1, dev)
    # the composed inputs of the backbone, from the restatement's own embedding + compose
    C = 13
    lv = F.one_hot(inp['ligand_v'], C).float()
    h_p = F.linear(inp['protein_v'], state_dict['protein_atom_emb.weight'], state_dict['protein_atom_emb.bias'])
    h_l = F.linear(lv, state_dict['ligand_atom_emb.weight'], state_dict['ligand_atom_emb.bias'])
    h_p = torch.cat([h_p, torch.zeros(len(h_p), 1)], -1)
    h_l = torch.cat([h_l, torch.ones(len(h_l), 1)], -1)
    h, x, batch_all, mask = R.compose_context(h_p, h_l, inp['protein_pos'], inp['ligand_pos'], inp['batch_protein'],
                                              inp['batch_ligand'])
    B = int(batch_all.max()) + 1
    ptr = nat1.graph_ptr(batch_all.to(dev), B)
    out_h, out_x, nbr, ew = nat1.refine_forward(h.to(dev).contiguous(), x.to(dev).contiguous(), mask.to(dev), ptr,
                                                want_graph=True)
    np.testing.assert_array_equal(nbr.cpu().numpy(), g['nbr'])
    valid = g['nbr'] >= 0
    close(ew.cpu().numpy()[valid], g['e_w'][valid], 1e-5)
    assert np.all(ew.cpu().numpy()[~valid] == 0)
    close(out_h, g['h_layers'][0], TOL_FWD, 'layer 0 h')
    close(out_x, g['x_layers'][0], TOL_FWD, 'layer 0 x')
    # fix_x: coordinates untouched, same h
    out_h2, out_x2, _, _ = nat1.refine_forward(h.to(dev).contiguous(), x.to(dev).contiguous(), mask.to(dev), ptr,
                                               fix_x=True)
    assert torch.equal(out_x2.cpu(), x)
    close(out_h2, g['h_layers'][0], TOL_FWD)


def test_refine_net_module_full_depth(model, state_dict, golden_small):
    """refine_net(h, x, mask_ligand, batch) seam, all 9 layers, vs the real reference's per-layer outputs."""
    from oracle import restatement as R
    import torch.nn.functional as F
    dev = _dev()
    g = golden_small
    inp = small_inputs(g)
    lv = F.one_hot(inp['ligand_v'], 13).float()
    h_p = F.linear(inp['protein_v'], state_dict['protein_atom_emb.weight'], state_dict['protein_atom_emb.bias'])
    h_l = F.linear(lv, state_dict['ligand_atom_emb.weight'], state_dict['ligand_atom_emb.bias'])
    h_p = torch.cat([h_p, torch.zeros(len(h_p), 1)], -1)
    h_l = torch.cat([h_l, torch.ones(len(h_l), 1)], -1)
    h, x, batch_all, mask = R.compose_context(h_p, h_l, inp['protein_pos'], inp['ligand_pos'], inp['batch_protein'],
                                              inp['batch_ligand'])
    out = model.refine_net(h.to(dev), x.to(dev), mask.to(dev), batch_all.to(dev), return_all=True)
    assert len(out['all_x']) == 2 and torch.equal(out['all_x'][1], out['x']) and torch.equal(out['all_h'][0].cpu(), h)
    close(out['h'], g['h_layers'][8], TOL_FWD, 'layer 8 h')
    close(out['x'], g['x_layers'][8], TOL_FWD, 'layer 8 x')


# ------------------------------------------------------------------------------------------ full forward
def _forward(model, inp, dev, **kw):
    return model(inp['protein_pos'].to(dev), inp['protein_v'].to(dev), inp['batch_protein'].to(dev),
                 inp['ligand_pos'].to(dev), inp['ligand_v'].to(dev), inp['batch_ligand'].to(dev), **kw)


def test_forward_small_vs_reference_golden(model, golden_small):
    dev = _dev()
    g = golden_small
    out = _forward(model, small_inputs(g), dev)
    for k in ('pred_ligand_pos', 'pred_ligand_v', 'final_h', 'final_ligand_h'):
        close(out[k], g[k], TOL_FWD, k)


def test_forward_small_fix_x(model, golden_small):
    dev = _dev()
    g = load_golden('forward_small_fixx.npz')
    inp = small_inputs(golden_small)
    out = _forward(model, inp, dev, fix_x=True)
    assert torch.equal(out['pred_ligand_pos'].cpu(), inp['ligand_pos'])
    close(out['pred_ligand_v'], g['pred_ligand_v'], TOL_FWD)
    close(out['final_ligand_h'], g['final_ligand_h'], TOL_FWD)
    emb = model.fetch_embedding(inp['protein_pos'].to(dev), inp['protein_v'].to(dev), inp['batch_protein'].to(dev),
                                inp['ligand_pos'].to(dev), inp['ligand_v'].to(dev), inp['batch_ligand'].to(dev))
    assert torch.equal(emb['final_ligand_h'], out['final_ligand_h'])


def test_forward_1h36_vs_reference_golden(model):
    from oracle import restatement as R
    from targetdiff_amd import workloads
    dev = _dev()
    g = load_golden('forward_1h36x2.npz')
    pocket, _ = pocket_1h36()
    b = workloads.pack_samples(pocket, 2, g['sizes'])
    ppos, _, _ = R.center_positions(b.protein_pos, torch.zeros(len(b.ligand_element_batch), 3),
                                    b.protein_element_batch, b.ligand_element_batch)
    out = model(ppos.to(dev), b.protein_atom_feature.float().to(dev), b.protein_element_batch.to(dev),
                torch.from_numpy(g['ligand_pos']).to(dev), torch.from_numpy(g['ligand_v']).to(dev),
                b.ligand_element_batch.to(dev))
    for k in ('pred_ligand_pos', 'pred_ligand_v', 'final_ligand_h'):
        close(out[k], g[k], TOL_FWD, k)
    close(out['final_h'][::16], g['final_h_sample'], TOL_FWD, 'final_h')


def test_forward_deterministic_and_batch_independent(model):
    """Size-independent properties at a larger batch: bit-identical reruns (no atomics in any arithmetic), and every replica
    of the same (pocket, ligand) graph gets bit-identical outputs wherever it sits in the ragged pack."""
    from targetdiff_amd import workloads
    dev = _dev()
    pocket = workloads.synthetic_pocket(1000, 300)
    reps = 24
    b = workloads.pack_samples(pocket, reps, [25] * reps).to(dev)
    g = torch.Generator(device='cpu').manual_seed(1)
    one = workloads.pack_samples(pocket, 1, [25])
    pos1, v1 = workloads.init_ligand(one, generator=g)
    lpos = pos1.repeat(reps, 1).to(dev)
    lv = v1.repeat(reps).to(dev)
    args = (b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch, lpos, lv, b.ligand_element_batch)
    o1 = model(*args)
    o2 = model(*args)
    for k in ('pred_ligand_pos', 'pred_ligand_v', 'final_h'):
        assert torch.equal(o1[k], o2[k]), k
    pp = o1['pred_ligand_pos'].view(reps, 25, 3)
    pv = o1['pred_ligand_v'].view(reps, 25, 13)
    assert torch.equal(pp, pp[:1].expand_as(pp))
    assert torch.equal(pv, pv[:1].expand_as(pv))


def test_forward_rotation_equivariance(model):
    """SE(3) property at a size the oracle would take minutes for: rotating + translating every input
    coordinate rotates the predicted positions and leaves invariant features (almost) unchanged."""
    from targetdiff_amd import workloads
    dev = _dev()
    pockets = [workloads.synthetic_pocket(1000 + p, 300) for p in range(4)]
    b = workloads.pack_samples(pockets, 8, [25] * 32).to(dev)
    g = torch.Generator().manual_seed(2)
    lpos, lv = workloads.init_ligand(workloads.pack_samples(pockets, 8, [25] * 32), generator=g)
    lpos, lv = lpos.to(dev), lv.to(dev)
    nat = model._native(dev)
    pptr = nat.graph_ptr(b.protein_element_batch, 32)
    lptr = nat.graph_ptr(b.ligand_element_batch, 32)
    ppos = b.protein_pos.clone()
    nat.center_pos(ppos, pptr, lpos, lptr)
    A = torch.linalg.qr(torch.randn(3, 3, generator=g)).Q
    if torch.det(A) < 0:
        A[:, 0] = -A[:, 0]
    A = A.to(dev)
    pv = b.protein_atom_feature.float()
    o1 = model(ppos, pv, b.protein_element_batch, lpos, lv, b.ligand_element_batch)
    o2 = model(ppos @ A.T, pv, b.protein_element_batch, lpos @ A.T, lv, b.ligand_element_batch)
    # per graph: a near-tie at the 32nd/33rd neighbour may legitimately flip under rotation (discrete kNN),
    # so require the property on all but at most 2 of the 32 graphs.
    dpos = ((o1['pred_ligand_pos'] @ A.T) - o2['pred_ligand_pos']).abs().view(32, 25, 3).amax(dim=(1, 2))
    dv = (o1['pred_ligand_v'] - o2['pred_ligand_v']).abs().view(32, 25, 13).amax(dim=(1, 2))
    print('rotation: max dpos per graph', dpos.max().item(), 'median', dpos.median().item())
    assert int((dpos < 2e-4).sum()) >= 30 and int((dv < 2e-3).sum()) >= 30


# ------------------------------------------------------------------------------------------ sampling session
@pytest.mark.parametrize('case', ['small', '1h36', 'multi'])
def test_session_forward_equals_stateless_forward(model, case):
    """td_session (static-protein caching: merged kNN, cached gate rows / layer-0 rows) must reproduce
    td_model_forward bit for bit, step after step, and must really skip work (dirty rows << N)."""
    from targetdiff_amd import capi, workloads
    dev = _dev()
    nat = model._native(dev)
    if case == 'small':
        from oracle.make_golden import small_batch
        b, lpos, lv = small_batch()
    elif case == '1h36':
        pocket, sizes = pocket_1h36()
        b = workloads.pack_samples(pocket, 6, sizes[:6])
        lpos, lv = workloads.init_ligand(b, generator=torch.Generator().manual_seed(5))
    else:
        pockets = [workloads.synthetic_pocket(300 + p, 150 + 40 * p) for p in range(3)]
        b = workloads.pack_samples(pockets, 4, [20, 30, 25, 18] * 3)
        lpos, lv = workloads.init_ligand(b, generator=torch.Generator().manual_seed(6))
    b = b.to(dev)
    lpos, lv = lpos.to(dev), lv.to(dev)
    B = b.num_graphs
    pptr = nat.graph_ptr(b.protein_element_batch, B)
    lptr = nat.graph_ptr(b.ligand_element_batch, B)
    ppos = b.protein_pos.clone()
    nat.center_pos(ppos, pptr, lpos, lptr)
    pv = b.protein_atom_feature.float()
    sess = capi.NativeSession(nat, ppos, pv, pptr, lptr, lpos.shape[0])
    g = torch.Generator(device='cpu').manual_seed(9)
    N = ppos.shape[0] + lpos.shape[0]
    for step in range(3):
        want = nat.model_forward(ppos, pv, pptr, lpos, lv, lptr, want_final_h=False)
        got = sess.forward(lpos, lv)
        for k in ('pred_ligand_pos', 'pred_ligand_v', 'final_ligand_h'):
            assert torch.equal(got[k], want[k]), (case, step, k, _maxdiff(got[k], want[k]))
        n_all, dirty, levels = sess.row_counts()
        assert n_all == N and lpos.shape[0] <= dirty <= N
        # the step's row lists come from one launch (a workgroup per graph) or, for graphs too large for that kernel's LDS flags,
        # from the separate list kernels: same sets, same outputs
        nat.set_option('session_step_lists', 0)
        again = sess.forward(lpos, lv)
        assert sess.row_counts() == (n_all, dirty, levels) and sess.forward_reach_rows() is not None
        n_fwd0 = sess.forward_reach_rows()
        nat.set_option('session_step_lists', 1)
        for k in ('pred_ligand_pos', 'pred_ligand_v', 'final_ligand_h'):
            assert torch.equal(again[k], want[k]), (case, step, k, 'separate list kernels')
        once_more = sess.forward(lpos, lv)
        assert sess.forward_reach_rows() == n_fwd0 and sess.row_counts() == (n_all, dirty, levels)
        assert torch.equal(once_more['pred_ligand_pos'], want['pred_ligand_pos'])
        # receptive-field levels of the ligand outputs: nested, each at least the ligand atoms, at most every node
        assert len(levels) >= 1 and all(lpos.shape[0] <= a <= b <= N for a, b in zip(levels, levels[1:] + [N]))
        if case == '1h36':
            assert dirty < 0.5 * N, (dirty, N)
        # move the ligand like a sampling step would (and shuffle the types) before the next comparison
        lpos = (0.98 * want['pred_ligand_pos'] * 0.02 + 0.98 * lpos + 0.3 * torch.randn(lpos.shape, generator=g).to(dev)).contiguous()
        lv = torch.randint(0, 13, lv.shape, generator=g).to(dev)


# ------------------------------------------------------------------------------------------ posterior / sampling
def test_posterior_known_answers(model):
    dev = _dev()
    nat = model._native(dev)
    g = load_golden('posterior_kat.npz')
    bl = torch.from_numpy(g['batch_ligand']).to(dev)
    lptr = nat.graph_ptr(bl, 3)
    T = lambda k, dt=None: torch.from_numpy(g[k]).to(dev)
    n = bl.numel()
    log_v0 = torch.empty(n, 13, device=dev)
    log_post = torch.empty(n, 13, device=dev)
    pos_next, v_next = nat.posterior_step(torch.from_numpy(g['t']).int().to(dev), lptr, T('x_t'), T('v_t'), T('x0'),
                                          T('v0_logits'), T('noise'), T('uniform'), log_v0=log_v0, log_post=log_post)
    close(pos_next, g['pos_next'], 2e-6)
    close(log_v0, g['log_v0'], 1e-5)
    close(log_post, g['log_post'], 2e-5)
    np.testing.assert_array_equal(v_next.cpu().numpy(), g['v_next'])


def test_center_pos(model):
    from targetdiff_amd import workloads
    from oracle import restatement as R
    dev = _dev()
    nat = model._native(dev)
    pockets = [workloads.synthetic_pocket(7, 50), workloads.synthetic_pocket(8, 300)]
    b = workloads.pack_samples(pockets, 2, [5, 6, 7, 8])
    lpos = torch.randn(26, 3)
    wp, wl, woff = R.center_positions(b.protein_pos, lpos, b.protein_element_batch, b.ligand_element_batch)
    pptr = nat.graph_ptr(b.protein_element_batch.to(dev), 4)
    lptr = nat.graph_ptr(b.ligand_element_batch.to(dev), 4)
    pp, ll = b.protein_pos.clone().to(dev), lpos.clone().to(dev)
    off = nat.center_pos(pp, pptr, ll, lptr)
    # bit-identical to the reference's CPU path (scatter_mean = index_add_ in index order, then a division): the centred
    # coordinates feed the k-NN search, where a last-bit difference can flip a near-tie (tests/test_gpu_long_parity.py)
    assert torch.equal(off.cpu(), woff) and torch.equal(pp.cpu(), wp) and torch.equal(ll.cpu(), wl)
    pocket, _ = pocket_1h36()
    b2 = workloads.pack_samples(pocket, 3, [20, 25, 30])
    _, _, woff2 = R.center_positions(b2.protein_pos, torch.zeros(75, 3), b2.protein_element_batch, b2.ligand_element_batch)
    pp2 = b2.protein_pos.clone().to(dev)
    off2 = nat.center_pos(pp2, nat.graph_ptr(b2.protein_element_batch.to(dev), 3), torch.zeros(75, 3, device=dev),
                          nat.graph_ptr(b2.ligand_element_batch.to(dev), 3))
    assert torch.equal(off2.cpu(), woff2)


def test_sample_diffusion_trajectory_vs_reference(model):
    """6 reverse steps with the reference's own recorded randn/rand draws injected: every step's positions
    within tolerance, every sampled atom type bit-exact."""
    from oracle.make_golden import small_batch
    dev = _dev()
    g = load_golden('sample_small.npz')
    b, lpos, lv = small_batch()
    noises = torch.from_numpy(g['noises']).to(dev)
    unis = torch.from_numpy(g['uniforms']).to(dev)

    def src(step, name, like):
        return (noises if name == 'noise' else unis)[step].contiguous()
    r = model.sample_diffusion(b.protein_pos.to(dev), b.protein_atom_feature.float().to(dev),
                               b.protein_element_batch.to(dev), lpos.to(dev), lv.to(dev),
                               b.ligand_element_batch.to(dev), num_steps=6, center_pos_mode='protein',
                               noise_source=src)
    assert len(r['pos_traj']) == 6 and not r['pos_traj'][0].is_cuda
    np.testing.assert_array_equal(torch.stack(r['v_traj']).numpy(), g['v_traj'])
    d = dict(pos=_maxdiff(torch.stack(r['pos_traj']), g['pos_traj']), v0=_maxdiff(torch.stack(r['v0_traj']), g['v0_traj']),
             vt=_maxdiff(torch.stack(r['vt_traj']), g['vt_traj']), final=_maxdiff(r['pos'], g['pos']))
    print(d)
    assert d['pos'] < 5e-5 and d['final'] < 5e-5 and d['v0'] < 5e-4 and d['vt'] < 5e-4
    np.testing.assert_array_equal(r['v'].cpu().numpy(), g['v'])


def test_sample_diffusion_ligand_driver(model):
    from targetdiff_amd import sampling, workloads
    dev = _dev()
    pocket = workloads.synthetic_pocket(55, 120)
    res = sampling.sample_diffusion_ligand(model, pocket, num_samples=5, batch_size=3, device=dev, num_steps=3,
                                           ligand_num_atoms=[9, 10, 11, 12, 13])
    pos, v, pos_traj, v_traj, v0_traj, vt_traj, times = res
    assert [p.shape for p in pos] == [(n, 3) for n in (9, 10, 11, 12, 13)] and pos[0].dtype == np.float64
    assert [t.shape for t in pos_traj] == [(3, n, 3) for n in (9, 10, 11, 12, 13)]
    assert [t.shape for t in v0_traj] == [(3, n, 13) for n in (9, 10, 11, 12, 13)]
    assert len(times) == 2 and all(np.isfinite(p).all() for p in pos)
    assert all(((x >= 0) & (x < 13)).all() for x in v)


def test_fails_loudly_without_device_tensors(model):
    cpu = torch.zeros(4, 3)
    with pytest.raises(RuntimeError):
        model(cpu, torch.zeros(4, 27), torch.zeros(4, dtype=torch.long), cpu, torch.zeros(4, dtype=torch.long),
              torch.zeros(4, dtype=torch.long))


# ------------------------------------------------------------------------------------------ alternative kernel paths
def test_return_all_vs_reference_golden(model, golden_small):
    """forward(return_all=True) (models/molopt_score_model.py:360-367): block input and block output predictions."""
    dev = _dev()
    g = load_golden('forward_small_return_all.npz')
    out = _forward(model, small_inputs(golden_small), dev, return_all=True)
    assert len(out['layer_pred_ligand_pos']) == len(out['layer_pred_ligand_v']) == 2
    for l in range(2):
        close(out['layer_pred_ligand_pos'][l], g['layer_pred_ligand_pos'][l], TOL_X)
        close(out['layer_pred_ligand_v'][l], g['layer_pred_ligand_v'][l], TOL_H)


def test_likelihood_estimation_vs_reference_golden(model):
    """ScorePosNet3D.likelihood_estimation (scripts/likelihood_est_diffusion.py:30,48) with the reference's recorded
    draws: KL terms at t = (0, 1, 537) -- rtol 1e-4 (the t = 0 decoder NLL is O(1e3)), atol 1e-6 -- and the prior terms.
    Also checked against the oracle restatement on the same inputs."""
    from oracle import restatement as R
    from oracle import weights
    dev = _dev()
    g = load_golden('likelihood_small.npz')
    T = lambda k, dt=None: torch.from_numpy(g[k].astype(dt) if dt else g[k])
    args = (T('protein_pos').to(dev), T('protein_feat', np.float32).to(dev), T('batch_protein').to(dev),
            T('ligand_pos').to(dev), T('ligand_v').to(dev), T('batch_ligand').to(dev))
    noise, uni = T('noise').to(dev), T('uniform').to(dev)
    src = lambda step, name, like: noise if name == 'noise' else uni
    kl_pos, kl_v = model.likelihood_estimation(*args, T('time_step').to(dev), noise_source=src)
    np.testing.assert_allclose(kl_pos.cpu().numpy(), g['kl_pos'], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(kl_v.cpu().numpy(), g['kl_v'], rtol=1e-4, atol=1e-6)
    klp, klv = model.likelihood_estimation(*args, torch.full((3,), 1000, dtype=torch.long, device=dev))
    np.testing.assert_allclose(klp.cpu().numpy(), g['kl_pos_prior'], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(klv.cpu().numpy(), g['kl_v_prior'], rtol=1e-4, atol=1e-7)
    # oracle on a different set of time steps
    ts = torch.tensor([999, 0, 3], dtype=torch.long)
    sd = weights.make_state_dict(2021)
    want_pos, want_v = R.likelihood_estimation(sd, None, *[a.cpu() for a in args], time_step=ts, noise=noise.cpu(),
                                               uniform=uni.cpu())
    got_pos, got_v = model.likelihood_estimation(*args, ts.to(dev), noise_source=src)
    np.testing.assert_allclose(got_pos.cpu().numpy(), want_pos.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(got_v.cpu().numpy(), want_v.numpy(), rtol=1e-4, atol=1e-6)


def test_sample_diffusion_pos_only(model):
    """pos_only=True (models/molopt_score_model.py:681): atom types frozen, no type trajectories, positions of the first
    step identical to the regular sampler's (same Gaussian draw)."""
    from oracle.make_golden import small_batch
    dev = _dev()
    g = load_golden('sample_small.npz')
    b, lpos, lv = small_batch()
    noises = torch.from_numpy(g['noises']).to(dev)
    unis = torch.from_numpy(g['uniforms']).to(dev)
    src = lambda step, name, like: (noises if name == 'noise' else unis)[step].contiguous()
    args = (b.protein_pos.to(dev), b.protein_atom_feature.float().to(dev), b.protein_element_batch.to(dev), lpos.to(dev),
            lv.to(dev), b.ligand_element_batch.to(dev))
    r = model.sample_diffusion(*args, num_steps=4, center_pos_mode='protein', noise_source=src, pos_only=True)
    assert len(r['pos_traj']) == 4 and len(r['v_traj']) == 4 and r['v0_traj'] == [] and r['vt_traj'] == []
    assert torch.equal(r['v'].cpu(), lv) and all(torch.equal(v, lv) for v in r['v_traj'])
    # step 0 of the T-4 .. T-1 schedule differs from the golden's T-6 schedule, so compare with a regular 4-step run
    r2 = model.sample_diffusion(*args, num_steps=4, center_pos_mode='protein', noise_source=src)
    assert torch.equal(r['pos_traj'][0], r2['pos_traj'][0])
    assert all(torch.isfinite(p).all() for p in r['pos_traj'])


# ------------------------------------------------------------------------------------------ BASELINE config 2, full size
def test_full_size_c2_pack_reproduces_reference_golden(model):
    """The benchmark's full-size batch (1h36 x 100 samples, N = 60,708 nodes): the two graphs whose ligands are the
    reference golden's ligands must reproduce the reference outputs wherever they sit in the ragged pack (graphs are
    independent), through the stateless forward AND through the sampling session (row skipping, receptive-field pruning),
    and the two paths must agree bit for bit on every ligand atom of the batch."""
    from oracle import restatement as R
    from targetdiff_amd import capi, workloads
    dev = _dev()
    g = load_golden('forward_1h36x2.npz')
    pocket, sizes = pocket_1h36()
    sizes = [int(v) for v in sizes[:100]]
    assert sizes[:2] == [int(v) for v in g['sizes']]
    n2 = sizes[0] + sizes[1]
    # put the golden ligands (already centred) into graphs 37 and 81 instead of 0 and 1: swap the sizes accordingly
    order = list(range(100))
    order[0], order[37] = order[37], order[0]
    order[1], order[81] = order[81], order[1]
    sizes_p = [sizes[k] for k in order]
    b = workloads.pack_samples(pocket, 100, sizes_p)
    cum = np.cumsum([0] + sizes_p)
    lpos_p = torch.randn(int(cum[-1]), 3, generator=torch.Generator().manual_seed(12)) * 2.0
    lv_p = torch.randint(0, 13, (int(cum[-1]),), generator=torch.Generator().manual_seed(13))
    gp, gv = torch.from_numpy(g['ligand_pos']), torch.from_numpy(g['ligand_v'])
    lpos_p[cum[37]:cum[38]], lv_p[cum[37]:cum[38]] = gp[:sizes[0]], gv[:sizes[0]]
    lpos_p[cum[81]:cum[82]], lv_p[cum[81]:cum[82]] = gp[sizes[0]:n2], gv[sizes[0]:n2]
    ppos_c, _, _ = R.center_positions(b.protein_pos, torch.zeros(int(cum[-1]), 3), b.protein_element_batch,
                                      b.ligand_element_batch)
    b = b.to(dev)
    ppos_c, lpos_p, lv_p = ppos_c.to(dev), lpos_p.to(dev).contiguous(), lv_p.to(dev)
    assert ppos_c.shape[0] + lpos_p.shape[0] > 60000
    pv = b.protein_atom_feature.float()
    out = model(ppos_c, pv, b.protein_element_batch, lpos_p, lv_p, b.ligand_element_batch)
    nat = model._native(dev)
    pptr = nat.graph_ptr(b.protein_element_batch, 100)
    lptr = nat.graph_ptr(b.ligand_element_batch, 100)
    sess = capi.NativeSession(nat, ppos_c, pv, pptr, lptr, lpos_p.shape[0])
    got = sess.forward(lpos_p, lv_p)
    sel = torch.cat([torch.arange(cum[37], cum[38]), torch.arange(cum[81], cum[82])]).to(dev)
    for name, res in (('stateless', out), ('session', got)):
        for k in ('pred_ligand_pos', 'pred_ligand_v', 'final_ligand_h'):
            close(res[k][sel], g[k], TOL_FWD, f'{name} {k}')
    for k in ('pred_ligand_pos', 'pred_ligand_v', 'final_ligand_h'):
        assert torch.equal(out[k], got[k]), k
    n_all, dirty, levels = sess.row_counts()
    assert n_all == ppos_c.shape[0] + lpos_p.shape[0] and dirty < n_all and levels[0] < n_all


# ------------------------------------------------------------------------------------------ standalone EGNN refine net
def test_egnn_vs_reference_golden():
    """models/egnn.py EGNN built as get_refine_net('egnn', config) does, 9 layers with a fresh kNN graph each: every
    layer's coordinates and the recorded feature layers against the real reference's outputs."""
    from oracle import weights
    from targetdiff_amd.models import get_refine_net
    dev = _dev()
    g = load_golden('egnn_small.npz')
    L = int(g['num_layers'])
    cfg = dict(weights.DEFAULT_MODEL_CONFIG)
    net = get_refine_net('egnn', cfg)
    assert net.num_layers == L
    res = net.load_state_dict(weights.make_egnn_state_dict(2021, num_layers=L), strict=True)
    net = net.to(dev)
    h, x = torch.from_numpy(g['h']).to(dev), torch.from_numpy(g['x']).to(dev)
    mask, batch = torch.from_numpy(g['mask_ligand']).to(dev), torch.from_numpy(g['batch']).to(dev)
    out = net(h, x, mask, batch, return_all=True)
    assert len(out['all_x']) == L + 1 and len(out['all_h']) == L + 1
    # (the EGNN's features grow by three orders of magnitude over its nine residual layers: the last layer's tolerance is scaled with them)
    for l in range(L + 1):
        close(out['all_x'][l], g['all_x'][l], 5e-5, f'x after layer {l}')
    close(out['all_h'][1], g['h_layer1'], TOL_H, 'h layer 1')
    close(out['all_h'][5], g['h_layer5'], TOL_H, 'h layer 5')
    close(out['h'], g['h_final'], 5e-4, 'h final')
    # protein rows never move
    assert torch.equal(out['x'][~mask], x[~mask])
    out2 = net(h, x, mask, batch)
    assert torch.equal(out2['h'], out['h']) and torch.equal(out2['x'], out['x'])


def test_egnn_large_batch_replicas():
    """EGNN at a size that takes the large-launch code paths (N > 16 k): every replica of the same graph gets bit-identical
    outputs wherever it sits in the pack, equal to a 2-replica run of the same graph, and reruns are bit-identical."""
    from oracle import weights
    from targetdiff_amd import workloads
    from targetdiff_amd.egnn import EGNN
    dev = _dev()
    net = EGNN(num_layers=3, hidden_dim=128, edge_feat_dim=4, num_r_gaussian=1, k=32, cutoff_mode='knn')
    net.load_state_dict(weights.make_egnn_state_dict(7, num_layers=3), strict=True)
    net = net.to(dev)
    pocket = workloads.synthetic_pocket(2000, 300)
    g = torch.Generator().manual_seed(3)
    h1 = torch.randn(325, 128, generator=g)
    one = workloads.pack_samples(pocket, 1, [25])
    lpos1, _ = workloads.init_ligand(one, generator=g, spread=2.0)
    x1 = torch.cat([one.protein_pos, lpos1])
    mask1 = torch.cat([torch.zeros(300, dtype=torch.bool), torch.ones(25, dtype=torch.bool)])

    def run(reps):
        h = h1.repeat(reps, 1).to(dev)
        x = x1.repeat(reps, 1).to(dev)
        mask = mask1.repeat(reps).to(dev)
        batch = torch.arange(reps).repeat_interleave(325).to(dev)
        return net(h, x, mask, batch)
    big, big2, small = run(60), run(60), run(2)
    assert big['h'].shape[0] == 60 * 325 > 16384
    assert torch.equal(big['h'], big2['h']) and torch.equal(big['x'], big2['x'])
    hb, xb = big['h'].view(60, 325, 128), big['x'].view(60, 325, 3)
    assert torch.equal(hb, hb[:1].expand_as(hb)) and torch.equal(xb, xb[:1].expand_as(xb))
    assert torch.equal(hb[0], small['h'][:325]) and torch.equal(xb[0], small['x'][:325])
    assert float((big['x'].view(60, 325, 3)[0, 300:] - x1[300:].to(dev)).abs().max()) > 1e-3      # the ligand moved


def test_same_seed_sampling_is_bit_reproducible(model):
    """No atomics-ordered arithmetic anywhere on the path (including the initial centroid): two driver calls with the same
    torch seed return identical coordinates, types and trajectories."""
    from targetdiff_amd import sampling
    dev = _dev()
    pocket, sizes = pocket_1h36()
    sizes = [int(v) for v in sizes[:12]]

    def run():
        torch.manual_seed(123)
        return sampling.sample_diffusion_ligand(model, pocket, num_samples=12, batch_size=12, device=dev, num_steps=25,
                                                ligand_num_atoms=sizes)
    a, b = run(), run()
    for k in range(6):
        assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), k
