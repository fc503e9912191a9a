"""CPU-only checks of the host side: C-ABI library loads and exports every declared symbol, the Python mirror is
state_dict-compatible with the reference layout, the product fails loudly without a HIP device, input packing and the
pocket partition follow the reference driver."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, small_inputs
from oracle import weights
from targetdiff_amd import capi, workloads


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, 'include', 'targetdiff_hip.h')).read()
    declared = set(re.findall(r'\b(td_[a-z_0-9]+)\s*\(', header))
    declared -= {'td_model'}                      # the opaque struct tag
    assert {'td_model_create', 'td_knn', 'td_refine_forward', 'td_model_forward', 'td_posterior_step'} <= declared
    lib = capi.load_library()
    for name in sorted(declared):
        assert hasattr(lib, name), f'{name} declared in targetdiff_hip.h but not exported'
    assert declared == set(capi.SIGNATURES), declared ^ set(capi.SIGNATURES)
    assert lib.td_abi_version() == capi.ABI_VERSION == 5


def test_weight_blob_layout_matches_library():
    lib = capi.load_library()
    cfg = capi.TdConfig(hidden_dim=128, n_heads=16, knn=32, num_layers=9, num_r_gaussian=20, edge_feat_dim=4,
                        protein_feat_dim=27, ligand_num_classes=13, num_timesteps=1000)
    blob = capi.flatten_state_dict(weights.make_state_dict(2021), 9)
    assert blob.size == lib.td_model_num_weights(ctypes.byref(cfg)) == 2670780
    # init_h_emb_layer (154,112 dead parameters) is the only learnable block left out
    total = sum(int(np.prod(s)) for _, s, kind, _ in weights.parameter_spec())
    dead = sum(int(np.prod(s)) for k, s, kind, _ in weights.parameter_spec() if 'init_h_emb_layer' in k)
    per_layer_offsets = 0          # offsets are part of both counts
    assert total - dead == blob.size + per_layer_offsets


def test_workspace_block_sizes_are_pinned():
    """td_workspace_bytes / td_egnn_workspace_bytes: the sizes the block layout had before every layout moved onto the shared
    carver (tdapi::Carver) -- the order of buffers, the 256-byte alignment and the zero-size rule must not have moved with it."""
    lib = capi.load_library()
    want = {(0, 0, 0): 9472, (1, 1, 1): 9472, (1000, 4, 100): 7973120, (60708, 100, 2400): 483974912}
    for (N, B, Nl), size in want.items():
        assert lib.td_workspace_bytes(None, N, B, Nl) == size, (N, B, Nl)
    for N, size in {0: 3584, 1: 3584, 1000: 2724352}.items():
        assert lib.td_egnn_workspace_bytes(N) == size, N


def test_unsupported_config_is_rejected_not_emulated():
    lib = capi.load_library()
    cfg = capi.TdConfig(hidden_dim=256, n_heads=16, knn=32, num_layers=9, num_r_gaussian=20, edge_feat_dim=4,
                        protein_feat_dim=27, ligand_num_classes=13, num_timesteps=1000)
    h = ctypes.c_void_p()
    dummy = (ctypes.c_float * 4)()
    rc = lib.td_model_create(ctypes.byref(cfg), dummy, 4, None, 0, ctypes.byref(h))
    assert rc == -1 and b'unsupported configuration' in lib.td_last_error()
    # graph construction is a run-time choice (knn with k <= 64, hybrid, radius); anything else is refused by both layers
    cfg2 = capi.TdConfig(hidden_dim=128, n_heads=16, knn=65, num_layers=9, num_r_gaussian=20, edge_feat_dim=4,
                         protein_feat_dim=27, ligand_num_classes=13, num_timesteps=1000)
    assert lib.td_model_create(ctypes.byref(cfg2), dummy, 4, None, 0, ctypes.byref(h)) == -1
    cfg3 = capi.TdConfig(hidden_dim=128, n_heads=16, knn=32, num_layers=9, num_r_gaussian=20, edge_feat_dim=4,
                         protein_feat_dim=27, ligand_num_classes=13, num_timesteps=1000, cutoff_mode=2, radius=0.0,
                         max_num_neighbors=32)
    assert lib.td_model_create(ctypes.byref(cfg3), dummy, 4, None, 0, ctypes.byref(h)) == -1      # radius mode needs r > 0
    from targetdiff_amd.models import ScorePosNet3D
    for bad in (dict(cutoff_mode='cutoff'), dict(knn=100), dict(ew_net_type='m', knn=48), dict(ew_net_type='r', knn=48), dict(ew_net_type='r', cutoff_mode='hybrid'),
                dict(num_blocks=9), dict(num_x2h=5), dict(num_x2h=2, sync_twoup=True), dict(act_fn='silu'), dict(hidden_dim=256)):
        with pytest.raises(NotImplementedError):
            ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG, **bad), 27, 13)
    # the gate / output options of the attention layers (round 4): the reference's key sets (oracle.weights mirrors the reference modules)
    for opt in (dict(ew_net_type='r', x2h_out_fc=True), dict(ew_net_type='none'), dict(x2h_out_fc=True), dict(ew_net_type='m'),
                dict(num_x2h=2, num_h2x=3, ew_net_type='r')):
        cfgo = dict(weights.DEFAULT_MODEL_CONFIG, **opt)
        m = ScorePosNet3D(cfgo, 27, 13)
        learn = {k for k, p in m.named_parameters() if p.requires_grad}
        assert learn == {k for k in weights.make_state_dict(2021, cfgo) if not k.endswith('distance_expansion.offset')}, opt
        blob = capi.flatten_state_dict(weights.make_state_dict(2021, cfgo), 9, cfgo['ew_net_type'], cfgo['x2h_out_fc'], cfgo['num_x2h'], cfgo['num_h2x'])
        c = capi.TdConfig(hidden_dim=128, n_heads=16, knn=32, num_layers=9, num_r_gaussian=20, edge_feat_dim=4, protein_feat_dim=27,
                          ligand_num_classes=13, num_timesteps=1000, ew_net_type=capi.ew_net_code(cfgo['ew_net_type']),
                          x2h_out_fc=int(cfgo['x2h_out_fc']), num_x2h=cfgo['num_x2h'], num_h2x=cfgo['num_h2x'])
        assert lib.td_model_num_weights(ctypes.byref(c)) == blob.size, opt
    for ok in (dict(cutoff_mode='hybrid'), dict(knn=48), dict(cutoff_mode='radius', r=6.0, max_num_neighbors=16)):
        m = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG, **ok), 27, 13)
        assert len(m.state_dict()) == 384             # the weights do not depend on the graph construction


def test_model_mirror_state_dict_and_loud_failure(state_dict):
    from targetdiff_amd.models import ScorePosNet3D
    m = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG), 27, 13)
    sd = m.state_dict()
    assert len(sd) == 384
    assert set(state_dict) <= set(sd)
    res = m.load_state_dict(state_dict, strict=False)
    assert not res.unexpected_keys and all(k.count('.') == 0 for k in res.missing_keys)   # only schedule consts/buffers
    assert sum(p.numel() for p in m.parameters() if p.requires_grad) == 2824692
    g = load_golden('schedules.npz')
    for k, v in g.items():
        np.testing.assert_array_equal(getattr(m, k).detach().numpy(), v, err_msg=k)
    inp = small_inputs(load_golden('forward_small.npz'))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU path'):
            m(inp['protein_pos'], inp['protein_v'], inp['batch_protein'], inp['ligand_pos'], inp['ligand_v'],
              inp['batch_ligand'])
        with pytest.raises(RuntimeError):
            m.sample_diffusion(inp['protein_pos'], inp['protein_v'], inp['batch_protein'], inp['ligand_pos'],
                               inp['ligand_v'], inp['batch_ligand'], num_steps=1, center_pos_mode='protein')


def test_pack_samples_matches_reference_batching():
    p1, p2 = workloads.synthetic_pocket(1, 20), workloads.synthetic_pocket(2, 31)
    b = workloads.pack_samples([p1, p2], 2, [3, 4, 5, 6])
    assert b.num_graphs == 4 and b.protein_pos.shape == (2 * 20 + 2 * 31, 3)
    assert b.protein_element_batch.tolist() == [0] * 20 + [1] * 20 + [2] * 31 + [3] * 31
    assert b.ligand_element_batch.tolist() == [0] * 3 + [1] * 4 + [2] * 5 + [3] * 6
    assert b.protein_atom_feature.shape[1] == 27 and b.protein_atom_feature.sum(1).min() >= 2   # element + residue
    g = torch.Generator().manual_seed(0)
    pos, v = workloads.init_ligand(b, generator=g)
    assert pos.shape == (18, 3) and v.dtype == torch.int64 and int(v.max()) < 13
    centre = torch.from_numpy(p1.pos).mean(0)
    assert float((pos[:3] - centre).norm(dim=1).max()) < 6.0     # centroid + N(0, I)


def test_pdb_parser_and_featuriser(tmp_path):
    block = ('HEADER    POCKET\n'
             'ATOM    219  N   LEU A  36      36.155  52.241  55.687  1.00 30.88         A N\n'
             'ATOM    220  CA  LEU A  36      35.391  51.712  54.566  1.00 30.88         A C\n'
             'ATOM    221  SG  CYS A  37      35.560  50.200  54.537  1.00 30.88         A S\n')
    p = workloads.pocket_from_pdb(block)
    assert p.num_atoms == 3 and p.feat.shape == (3, 27)
    np.testing.assert_allclose(p.pos[0], [36.155, 52.241, 55.687], rtol=1e-6)
    assert p.feat[0, 2] == 1 and p.feat[1, 1] == 1 and p.feat[2, 4] == 1        # N, C, S one-hots
    assert p.feat[0, 6 + workloads.AA_NAMES.index('LEU')] == 1 and p.feat[2, 6 + workloads.AA_NAMES.index('CYS')] == 1
    assert p.feat[:, 26].tolist() == [1, 1, 0]                                  # backbone flag


def test_partition_is_the_reference_round_robin():
    # scripts/batch_sample_diffusion.sh:15-20: task i -> worker i % NODE_ALL, starting at START_IDX
    parts = [workloads.partition_pockets(100, 8, r) for r in range(8)]
    assert sorted(sum(parts, [])) == list(range(100)) and parts[3][:3] == [3, 11, 19]
    assert workloads.partition_pockets(10, 4, 1, start_idx=4) == [5, 9]


def test_egnn_mirror_state_dict_and_loud_failure():
    """targetdiff_amd.egnn.EGNN has the reference's state_dict layout (models/egnn.py as get_refine_net('egnn') builds it),
    its blob order matches the library's expectation, unsupported settings raise, and it refuses to run on CPU tensors."""
    from targetdiff_amd.egnn import EGNN
    from targetdiff_amd.models import get_refine_net
    net = get_refine_net('egnn', dict(weights.DEFAULT_MODEL_CONFIG))
    assert isinstance(net, EGNN) and net.num_layers == weights.DEFAULT_MODEL_CONFIG['num_layers']
    spec = {k: tuple(s) for k, s, _, _ in weights.egnn_parameter_spec(net.num_layers)}
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == spec
    net.load_state_dict(weights.make_egnn_state_dict(5, num_layers=net.num_layers), strict=True)
    lib = capi.load_library()
    n = sum(int(np.prod(spec[k])) for k in capi.egnn_flat_key_order(net.num_layers))
    assert n == lib.td_egnn_num_weights(net.num_layers)
    with pytest.raises(NotImplementedError):
        EGNN(num_layers=2, hidden_dim=64, edge_feat_dim=4, num_r_gaussian=1)
    with pytest.raises(NotImplementedError):
        EGNN(num_layers=2, hidden_dim=128, edge_feat_dim=4, num_r_gaussian=1, cutoff_mode='hybrid')
    with pytest.raises(ValueError):
        get_refine_net('gcn', dict(weights.DEFAULT_MODEL_CONFIG))
    with pytest.raises(RuntimeError):
        net(torch.zeros(4, 128), torch.zeros(4, 3), torch.zeros(4, dtype=torch.bool), torch.zeros(4, dtype=torch.long))


def test_size_balanced_assignment_is_opt_in_and_deterministic():
    """The reference's i % N round-robin stays the default; LPT on node counts is the opt-in."""
    costs = [300, 600, 250, 500, 400, 450, 350, 550, 275, 575]
    assert workloads.partition_pockets(10, 4, 1) == [1, 5, 9]
    parts = workloads.lpt_assignment(costs, 4)
    assert sorted(i for p in parts for i in p) == list(range(10))                       # a partition
    assert parts == workloads.lpt_assignment(costs, 4)                                  # every rank computes the same table
    assert [workloads.partition_pockets(10, 4, r, costs=costs) for r in range(4)] == parts
    assert workloads.predicted_imbalance(costs, 4, balanced=True) <= workloads.predicted_imbalance(costs, 4) + 1e-12
    assert workloads.predicted_imbalance(costs, 4, balanced=True) < 1.12 < workloads.predicted_imbalance(costs, 4)
    # start_idx: the pockets before it are nobody's
    assert all(i >= 3 for p in workloads.lpt_assignment(costs, 4, start_idx=3) for i in p)


def test_native_options_live_on_the_module(state_dict):
    """set_native_option values survive a rebuild of the native handle and copy / pickle with the module."""
    import copy
    import pickle
    from targetdiff_amd.models import ScorePosNet3D
    m = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG), 27, 13)
    m.set_native_option('edge_key_split', 0)
    m.set_native_option('session_hop_levels', 2)
    for clone in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert clone._native_options == {'edge_key_split': 0, 'session_hop_levels': 2}
        assert clone._native_model is None


def test_unsorted_batch_is_refused_before_any_device_work():
    from targetdiff_amd.models import _check_graph_inputs, _check_sorted
    ok = torch.tensor([0, 0, 1, 1, 2])
    _check_graph_inputs(ok, ok, torch.tensor([0, 12, 3, 4, 5]), 13)
    _check_sorted(ok)
    with pytest.raises(ValueError, match='sorted'):
        _check_graph_inputs(torch.tensor([0, 1, 0]), ok, torch.tensor([0, 1, 2, 3, 4]), 13)
    with pytest.raises(ValueError, match='sorted'):
        _check_sorted(torch.tensor([1, 0]))
    with pytest.raises(ValueError, match=r'ligand_v must be in \[0, 13\)'):
        _check_graph_inputs(ok, ok, torch.tensor([0, 13, 2, 3, 4]), 13)


def test_radius_mode_warns_that_it_is_the_projects_rule():
    from targetdiff_amd.models import ScorePosNet3D
    with pytest.warns(UserWarning, match="no counterpart in the reference"):
        ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG, cutoff_mode='radius', r=5.0), 27, 13)


def test_round4_config_options_are_accepted_or_refused_like_the_reference():
    """model_mean_type 'noise' and time_emb_mode 'simple' construct (state_dict layout as the reference's: one more column of
    ligand_atom_emb); time_emb_mode 'sin' -- dead code in the reference's forward (torch.cat of [N_l, C] with [B, dim], :326-327) --
    constructs and refuses at forward, like the reference; the other architectures outside configs/training.yml raise."""
    from targetdiff_amd.models import ScorePosNet3D
    cfg = dict(weights.DEFAULT_MODEL_CONFIG)
    m = ScorePosNet3D(dict(cfg, time_emb_dim=8, time_emb_mode='simple', model_mean_type='noise'), 27, 13)
    assert m.ligand_atom_emb.weight.shape == (127, 14) and m.model_mean_type == 'noise'
    sd = weights.time_emb_state_dict(5)
    assert not m.load_state_dict(sd, strict=False).unexpected_keys
    # 'sin': constructed as the reference constructs it (same state_dict keys and shapes, so a checkpoint loads with strict=True);
    # forward refuses, where the reference's own forward fails (torch.cat of [N_l, C] with [B, dim])
    ms = ScorePosNet3D(dict(cfg, time_emb_dim=8, time_emb_mode='sin'), 27, 13)
    keys = {k: tuple(v.shape) for k, v in ms.state_dict().items() if k.startswith('time_emb') or k.startswith('ligand_atom_emb')}
    assert keys == {'time_emb.1.weight': (32, 8), 'time_emb.1.bias': (32,), 'time_emb.3.weight': (8, 32), 'time_emb.3.bias': (8,),
                    'ligand_atom_emb.weight': (127, 21), 'ligand_atom_emb.bias': (127,)}
    with pytest.raises(NotImplementedError, match='sin'):
        ms._time_bias(torch.zeros(2), 2)
    with pytest.raises(NotImplementedError):
        ScorePosNet3D(dict(cfg, time_emb_dim=8, time_emb_mode='other'), 27, 13)
    with pytest.raises(ValueError):
        ScorePosNet3D(dict(cfg, model_mean_type='x0'), 27, 13)


def test_bench_flop_bookkeeping_of_general_graphs():
    """bench.py's executed FLOPs: on a general graph the attention passes scale with the chunks per row, the node projections and
    the head do not (a k = 48 line once reported 1.12 of the fp32 peak because the whole step was doubled)."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    N, Nl, L = 10000, 400, 9
    base = bench.executed_flops_per_step(N, Nl, L, None)
    two = bench.executed_flops_per_step(N, Nl, L, None, 2 * bench.KEY_PASS_FLOP_EXECUTED, 2 * bench.KEY_PASS_FLOP_EXECUTED, 2)
    proj = L * (N * 6 * bench.GEMM128 + N * 2 * bench.GEMM128 + Nl * 4 * bench.GEMM128) + Nl * bench.HEAD_ROW
    assert base > proj > 0
    assert two == pytest.approx(2 * (base - proj) + proj)
    assert two < 2 * base
