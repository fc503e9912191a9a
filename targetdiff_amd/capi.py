"""ctypes binding of libtargetdiff_hip.so (C ABI: include/targetdiff_hip.h).

This is the binding a maintainer of the reference would add: torch tensors own all
device memory, the library only sees raw device pointers + sizes + the HIP stream of the current torch
stream.  There is no CPU fallback anywhere in this package: if the library is missing or a tensor is
not on a HIP device the call raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int32, c_int64, c_size_t, c_void_p

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libtargetdiff_hip.so')

TD_OK = 0
HIDDEN = 128
KNN = 32


class TdConfig(ctypes.Structure):
    _fields_ = [('hidden_dim', c_int32), ('n_heads', c_int32), ('knn', c_int32), ('num_layers', c_int32),
                ('num_r_gaussian', c_int32), ('edge_feat_dim', c_int32), ('protein_feat_dim', c_int32),
                ('ligand_num_classes', c_int32), ('num_timesteps', c_int32), ('cutoff_mode', c_int32), ('radius', c_float),
                ('max_num_neighbors', c_int32), ('model_mean_type', c_int32), ('num_blocks', c_int32), ('ew_net_type', c_int32),
                ('x2h_out_fc', c_int32), ('sync_twoup', c_int32), ('num_x2h', c_int32), ('num_h2x', c_int32), ('reserved', c_int32 * 1)]


class TdPropTape(ctypes.Structure):
    """td_prop_tape of include/targetdiff_hip.h: host-side record of a td_prop_forward_train"""
    _fields_ = [('model', c_void_p), ('weights_version', ctypes.c_uint64), ('N_p', c_int64), ('N_l', c_int64), ('B', c_int64),
                ('has_output_kind', c_int32), ('has_enc_node', c_int32), ('d_workspace', c_void_p), ('workspace_bytes', c_size_t)]


class TdPairProfile(ctypes.Structure):
    """td_pair_profile of include/targetdiff_hip.h"""
    _fields_ = [('z1', c_int32), ('z2', c_int32), ('cutoff', ctypes.c_double), ('n_edges', c_int32), ('reserved', c_int32),
                ('d_edges', c_void_p)]


class TdBondProfile(ctypes.Structure):
    """td_bond_profile of include/targetdiff_hip.h"""
    _fields_ = [('z1', c_int32), ('z2', c_int32), ('category', c_int32), ('n_edges', c_int32), ('d_edges', c_void_p)]


class TdGeometryProfile(ctypes.Structure):
    """td_geometry_profile of include/targetdiff_hip.h"""
    _fields_ = [('kind', c_int32), ('z', c_int32 * 4), ('category', c_int32), ('ring', c_int32), ('n_edges', c_int32), ('d_edges', c_void_p)]


class TdPropConfig(ctypes.Structure):
    """td_prop_config of include/targetdiff_hip.h"""
    _fields_ = [('hidden_dim', c_int32), ('num_layers', c_int32), ('knn', c_int32), ('num_r_gaussian', c_int32), ('cutoff', c_float),
                ('protein_feat_dim', c_int32), ('ligand_feat_dim', c_int32), ('enc_ligand_dim', c_int32), ('enc_node_dim', c_int32),
                ('enc_graph_dim', c_int32), ('output_dim', c_int32)]


CUTOFF_MODES = {'knn': 0, 'hybrid': 1, 'radius': 2}      # TD_CUTOFF_* (include/targetdiff_hip.h)
MAX_FANIN = 64
ABI_VERSION = 5


# every symbol include/targetdiff_hip.h declares: (restype, argtypes)
_P = c_void_p
# td_score_report, td_score_minimize and td_score_dock by side.  _SCORE_IN: the pack with the class table and class_aromatic, the pocket with
# N_p and n_kinds, the two cutoffs and rsum, the rotor inputs
_SCORE_IN = ([_P, _P, _P, c_int64, c_int64, c_int64, POINTER(c_int32), c_int32, POINTER(ctypes.c_uint8)] + [_P, _P, _P, _P, c_int64, c_int32] +
             [ctypes.c_double, ctypes.c_double, POINTER(ctypes.c_double)] + [_P, c_int64, _P])
_RELAX_IN = [POINTER(ctypes.c_double), c_int32, c_int32, ctypes.c_double]   # weights, max_steps, max_evals, max_shift
_RELAX_OUT = [_P] * 11                                                      # RELAX_KEYS
_DOCK_IN = [c_int32, c_int32, ctypes.c_double, ctypes.c_double, _P]         # n_chains, n_rounds, amplitude, temperature, draws
_DOCK_OUT = [_P] * 5                                                        # DOCK_KEYS beyond RELAX_KEYS
SIGNATURES = {
    'td_abi_version': (c_int32, []),
    'td_last_error': (c_char_p, []),
    'td_model_create': (c_int32, [POINTER(TdConfig), POINTER(c_float), c_size_t, POINTER(c_float), c_size_t,
                                  POINTER(c_void_p)]),
    'td_model_destroy': (None, [_P]),
    'td_model_num_weights': (c_size_t, [POINTER(TdConfig)]),
    'td_model_set_option': (c_int32, [_P, c_char_p, c_int32]),
    'td_model_get_option': (c_int32, [_P, c_char_p, POINTER(c_int32)]),
    'td_graph_build': (c_int32, [_P, _P, _P, _P, c_int64, c_int64, c_int32, _P, c_int32, _P]),
    'td_workspace_bytes': (c_size_t, [_P, c_int64, c_int64, c_int64]),
    'td_graph_ptr': (c_int32, [_P, c_int64, c_int64, _P, _P]),
    'td_knn': (c_int32, [_P, _P, c_int64, c_int64, c_int32, c_int32, _P, _P]),
    'td_refine_forward': (c_int32, [_P, _P, _P, _P, _P, c_int64, c_int64, c_int32, c_int32, _P, _P, _P, _P, _P,
                                    c_size_t, _P]),
    'td_model_forward': (c_int32, [_P, _P, _P, _P, c_int64, _P, _P, _P, c_int64, c_int64, c_int32, c_int32, _P, _P,
                                   _P, _P, _P, c_size_t, _P, _P]),
    'td_posterior_step': (c_int32, [_P, _P, _P, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'td_posterior_step_fixed': (c_int32, [_P, _P, _P, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'td_posterior_step_program': (c_int32, [_P, _P, _P, _P, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'td_renoise_step': (c_int32, [_P, _P, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'td_clash_shift': (c_int32, [_P, _P, _P, _P, c_int64, _P, c_float, c_float, _P, _P]),
    'td_clash_report': (c_int32, [_P, _P, _P, _P, c_int64, _P, _P, _P, _P, _P]),
    'td_quality_report': (c_int32, [_P, _P, _P, c_int64, c_int64, c_int64, POINTER(c_int32), c_int32, _P, _P, c_int32, _P, _P, _P, _P, _P, _P]),
    'td_bond_graph': (c_int32, [_P, _P, _P, c_int64, c_int64, c_int64, POINTER(c_int32), c_int32, _P, POINTER(ctypes.c_uint8), _P, c_int32, _P, _P, _P, _P,
                                _P, _P, _P]),
    'td_bond_list': (c_int32, [_P, _P, _P, c_int64, c_int64, c_int64, POINTER(c_int32), c_int32, POINTER(ctypes.c_uint8), _P, c_int64, _P, _P, _P, _P,
                               _P]),
    'td_ring_report': (c_int32, [_P, _P, _P, c_int64, c_int64, c_int64, POINTER(c_int32), c_int32, _P, POINTER(ctypes.c_uint8), _P, c_int64, _P, _P, _P,
                                 _P, _P, _P, _P, _P]),
    'td_fingerprint': (c_int32, [_P, _P, _P, c_int64, c_int64, c_int64, POINTER(c_int32), c_int32, POINTER(ctypes.c_uint8), c_int32, c_int32, _P, _P, _P,
                                 _P, _P]),
    'td_fingerprint_similarity': (c_int32, [_P, _P, _P, c_int64, c_int64, _P, _P, c_int64, _P, _P, _P, _P, _P, _P]),
    'td_geometry_report': (c_int32, [_P, _P, _P, c_int64, c_int64, c_int64, POINTER(c_int32), c_int32, _P, POINTER(ctypes.c_uint8), _P, c_int32, _P, c_int64,
                                     _P, POINTER(ctypes.c_double), _P, _P, _P, _P, _P, _P, _P, _P]),
    'td_pocket_report': (c_int32, [_P, _P, _P, c_int64, c_int64, c_int64, POINTER(c_int32), c_int32, _P, _P, _P, _P, c_int64, c_int32,
                                   ctypes.c_double, POINTER(ctypes.c_double), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'td_interaction_report': (c_int32, [_P, _P, _P, c_int64, c_int64, c_int64, POINTER(c_int32), c_int32, _P, _P, _P, _P, _P, c_int64, c_int32,
                                        ctypes.c_double, ctypes.c_double, ctypes.c_double, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                        _P, _P, _P, _P, _P]),
    'td_score_report': (c_int32, _SCORE_IN + [_P] * 4 + [_P]),              # protein_role_out, terms, n_pairs, n_rot; the stream
    'td_score_minimize': (c_int32, _SCORE_IN + _RELAX_IN + _RELAX_OUT + [_P]),
    'td_score_dock': (c_int32, _SCORE_IN + _RELAX_IN + _DOCK_IN + _RELAX_OUT + _DOCK_OUT + [_P]),
    'td_sasa_report': (c_int32, [_P, _P, _P, c_int64, c_int64, c_int64, POINTER(c_int32), c_int32, _P, _P, _P, c_int64, POINTER(ctypes.c_double),
                                 POINTER(ctypes.c_double), _P, c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'td_posterior_step_guided': (c_int32, [_P, _P, _P, _P, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'td_center_pos': (c_int32, [_P, _P, _P, _P, c_int64, _P, c_int32, c_int32, _P]),
    'td_perturb': (c_int32, [_P, _P, _P, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P]),
    'td_likelihood_terms': (c_int32, [_P, _P, _P, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'td_likelihood_prior': (c_int32, [_P, _P, c_int64, c_int64, _P, _P, _P, _P, _P]),
    'td_diffusion_loss': (c_int32, [_P, _P, _P, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, c_float, _P, _P, _P, _P, _P, _P]),
    'td_auroc': (c_int32, [_P, _P, c_int64, c_int32, _P, _P, _P]),
    'td_embed_ligand': (c_int32, [_P, _P, c_int64, _P, _P]),
    'td_v_inference': (c_int32, [_P, _P, c_int64, _P, _P]),
    'td_egnn_num_weights': (ctypes.c_size_t, [c_int32]),
    'td_egnn_create': (c_int32, [c_int32, c_int32, c_int32, c_int32, POINTER(c_float), ctypes.c_size_t, POINTER(c_void_p)]),
    'td_egnn_destroy': (None, [_P]),
    'td_egnn_workspace_bytes': (ctypes.c_size_t, [c_int64]),
    'td_egnn_forward': (c_int32, [_P, _P, _P, _P, _P, c_int64, c_int64, c_int32, _P, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    'td_prop_num_weights': (ctypes.c_size_t, [_P]),
    'td_prop_create': (c_int32, [_P, POINTER(c_float), ctypes.c_size_t, POINTER(c_void_p)]),
    'td_prop_destroy': (None, [_P]),
    'td_prop_workspace_bytes': (ctypes.c_size_t, [_P, c_int64, c_int64, c_int64]),
    'td_prop_forward': (c_int32, [_P, _P, _P, _P, c_int64, _P, _P, _P, c_int64, c_int64, _P, _P, _P, _P, c_int32, _P, _P, _P, _P,
                                  _P, ctypes.c_size_t, _P]),
    'td_prop_train_workspace_bytes': (ctypes.c_size_t, [_P, c_int64, c_int64, c_int64]),
    'td_prop_forward_train': (c_int32, [_P, _P, _P, _P, c_int64, _P, _P, _P, c_int64, c_int64, _P, _P, _P, _P, c_int32, _P, _P,
                                        ctypes.c_size_t, _P, _P]),
    'td_prop_backward': (c_int32, [_P, _P, c_int64, c_int64, c_int64, _P, _P, ctypes.c_size_t, _P]),
    'td_prop_set_weights': (c_int32, [_P, _P, ctypes.c_size_t, _P]),
    'td_session_create': (c_int32, [_P, _P, _P, _P, c_int64, _P, c_int64, c_int64, c_int32, _P, POINTER(c_void_p)]),
    'td_session_destroy': (None, [_P]),
    'td_session_forward': (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P]),
    'td_session_row_counts': (c_int32, [_P, POINTER(c_int32), c_int32, _P]),
    'td_session_step': (c_int32, [_P, _P, c_int32, _P]),
    'td_session_step_graph': (c_int32, [_P]),
    'td_step_io_size': (c_size_t, []),
    'td_session_set_program': (c_int32, [_P, _P, POINTER(c_int32), c_int32]),
    'td_session_set_guidance': (c_int32, [_P, _P, c_float, c_float]),
    'td_build_tag': (ctypes.c_char_p, []),
    'td_debug_fail_alloc': (c_int32, [c_int32]),
    'td_debug_node_stage': (c_int32, [_P, c_int32, c_int32, _P, c_int64, _P, _P, _P]),
    'td_debug_reductions': (c_int32, [_P, _P, _P]),
    'td_debug_wg_trace': (c_int32, [_P, c_int32]),
    'td_profile_begin': (c_int32, [ctypes.c_uint32]),
    'td_profile_end': (c_int32, [POINTER(c_float), POINTER(c_int32), c_int32]),
}

class StepIO(ctypes.Structure):
    """td_step_io of include/targetdiff_hip.h: the per-step arguments of td_session_step, all in device memory"""
    _fields_ = [('d_step', c_void_p), ('d_t_all', c_void_p), ('num_steps', c_int32), ('pos_only', c_int32),
                ('d_ligand_pos', c_void_p), ('d_ligand_v', c_void_p), ('d_noise', c_void_p), ('d_uniform', c_void_p),
                ('d_pos_traj', c_void_p), ('d_v_traj', c_void_p), ('d_v0_traj', c_void_p), ('d_vt_traj', c_void_p),
                ('d_ligand_graph_bias', c_void_p), ('d_fixed_mask', c_void_p), ('d_fixed_pos', c_void_p), ('d_fixed_v', c_void_p)]


def _fixed_ptrs(fixed_mask, fixed_pos, fixed_v, Nl):
    """Device pointers of the known-atom arguments (td_posterior_step_fixed): mask [N_l] bool / uint8, positions [N_l,3] fp32
    (centred), types [N_l] int64 -- or three None when there is no mask."""
    if fixed_mask is None:
        if fixed_pos is not None or fixed_v is not None:
            raise ValueError('fixed_pos / fixed_v without fixed_mask')
        return None, None, None
    if fixed_pos is None or fixed_v is None:
        raise ValueError('fixed_mask needs fixed_pos and fixed_v')
    if fixed_mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f'fixed_mask must be bool or uint8, got {fixed_mask.dtype}')
    if tuple(fixed_mask.shape) != (Nl,) or tuple(fixed_pos.shape) != (Nl, 3) or tuple(fixed_v.shape) != (Nl,):
        raise ValueError(f'fixed_mask / fixed_pos / fixed_v must be [{Nl}], [{Nl}, 3], [{Nl}] (got {tuple(fixed_mask.shape)}, '
                         f'{tuple(fixed_pos.shape)}, {tuple(fixed_v.shape)})')
    return (_ptr(fixed_mask, None, 'fixed_mask'), _ptr(fixed_pos, torch.float32, 'fixed_pos'),
            _ptr(fixed_v, torch.int64, 'fixed_v'))


CLASH_TILE = 1024       # TD_CLASH_TILE: protein atoms per LDS tile of the clash kernels (csrc/td_internal.h)
PROG_ROW = 12           # TD_PROG_ROW: floats per slot of a time program's coefficient table (schedule.ROW)


def _prog_row_ptr(row):
    if row.dtype != torch.float32 or row.numel() != PROG_ROW or not row.is_contiguous():
        raise ValueError(f'a program slot is {PROG_ROW} contiguous fp32 values')
    return _ptr(row, torch.float32, 'prog_row')


PROFILE_CLASSES = ('knn', 'gate', 'node_proj', 'x2h_k', 'x2h_v', 'h2x_k', 'h2x_v', 'compose', 'head', 'posterior')


def profile_begin(classes=PROFILE_CLASSES):
    mask = 0
    for c in classes:
        mask |= 1 << PROFILE_CLASSES.index(c)
    _check(load_library().td_profile_begin(mask), 'td_profile_begin')


def profile_end() -> dict:
    n = len(PROFILE_CLASSES)
    ms = (c_float * n)()
    cnt = (c_int32 * n)()
    _check(load_library().td_profile_end(ms, cnt, n), 'td_profile_end')
    return {name: {'ms': float(ms[i]), 'launches': int(cnt[i])} for i, name in enumerate(PROFILE_CLASSES)}


_lib = None


def build_tag() -> str:
    """td_build_tag(): names the sources the loaded library was built from; ties a measurement (bench line, PMC profile) to them."""
    return load_library().td_build_tag().decode()


def load_library(path: str = LIB_PATH):
    """dlopen the HIP library.  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(f'{path} not found: build it with `python -m targetdiff_amd.build` '
                           '(hipcc --offload-arch=gfx950).  There is no CPU fallback.')
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.td_abi_version() != ABI_VERSION:
        raise RuntimeError(f'{path} has ABI version {lib.td_abi_version()}, this binding needs {ABI_VERSION}: rebuild it '
                           '(python -m targetdiff_amd.build)')
    _lib = lib
    return lib


def _check(rc: int, what: str):
    if rc != TD_OK:
        msg = load_library().td_last_error()
        raise RuntimeError(f'{what} failed ({rc}): {msg.decode() if msg else "?"}')


def _ptr(t: torch.Tensor | None, dtype=None, what='tensor'):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f'{what} must live on a HIP device (got {t.device}); targetdiff_amd has no CPU path')
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f'{what} must be {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise ValueError(f'{what} must be contiguous')
    return c_void_p(t.data_ptr())


def _graph_bias_ptr(t, B):
    """[B][128] fp32 per-graph term of the ligand embedding (time embedding), or None"""
    if t is None:
        return None
    if t.dim() != 2 or t.shape[1] != HIDDEN or (B is not None and t.shape[0] != B):
        raise ValueError(f'ligand_graph_bias must be [B, {HIDDEN}] (got {tuple(t.shape)})')
    return _ptr(t, torch.float32, 'ligand_graph_bias')


def _stream(device=None):
    """HIP stream of torch's current stream ON `device` (the tensors' device, not the process-wide current device)."""
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _canonical_device(device=None) -> torch.device:
    d = torch.device('cuda') if device is None else torch.device(device)
    if d.type != 'cuda':
        raise RuntimeError(f'targetdiff_amd runs on HIP devices only (got {d}); there is no CPU path')
    return torch.device('cuda', torch.cuda.current_device()) if d.index is None else d


def _on(device):
    """Every library call runs with the tensors' device current: the library launches on / allocates from the current HIP
    device, and the reference CLI allows --device cuda:1 while the current device stays 0."""
    return torch.cuda.device(device)


# ----------------------------------------------------------------------------------------- weight blob
MLP_KEYS = ('net.0.weight', 'net.0.bias', 'net.1.weight', 'net.1.bias', 'net.3.weight', 'net.3.bias')


EW_NET_TYPES = {'global': 0, 'r': 1, 'm': 3}              # td_config.ew_net_type; anything else = 2 (e_w = 1)


def ew_net_code(ew_net_type) -> int:
    return EW_NET_TYPES.get(ew_net_type, 2)


def flat_key_order(num_layers: int, ew_net_type='global', x2h_out_fc=False, num_x2h=1, num_h2x=1):
    """Order of the reference state_dict tensors inside the flat blob td_model_create consumes
    (key names: SURVEY.md Appendix C; init_h_emb_layer and the schedule constants are not part of it).  Per layer: offsets; per x2h stage hk, hv, hq,
    [node_output (x2h_out_fc)], [x2h ew_net ('r': 80 + 1, 'm': 128 + 1)], xk, xv, xq, [h2x ew_net ('r')]; the global gate MLP only with ew_net_type 'global'."""
    keys = ['protein_atom_emb.weight', 'protein_atom_emb.bias', 'ligand_atom_emb.weight', 'ligand_atom_emb.bias',
            'refine_net.distance_expansion.offset']
    if ew_net_type == 'global':
        keys += [f'refine_net.edge_pred_layer.{k}' for k in MLP_KEYS]
    for l in range(num_layers):
        p = f'refine_net.base_block.{l}'
        keys.append(f'{p}.distance_expansion.offset')
        for i in range(num_x2h):
            for f in ('hk_func', 'hv_func', 'hq_func'):
                keys += [f'{p}.x2h_layers.{i}.{f}.{k}' for k in MLP_KEYS]
            if x2h_out_fc:
                keys += [f'{p}.x2h_layers.{i}.node_output.{k}' for k in MLP_KEYS]
            if ew_net_type in ('r', 'm'):
                keys += [f'{p}.x2h_layers.{i}.ew_net.0.weight', f'{p}.x2h_layers.{i}.ew_net.0.bias']
        for j in range(num_h2x):
            for f in ('xk_func', 'xv_func', 'xq_func'):
                keys += [f'{p}.h2x_layers.{j}.{f}.{k}' for k in MLP_KEYS]
            if ew_net_type == 'r':
                keys += [f'{p}.h2x_layers.{j}.ew_net.0.weight', f'{p}.h2x_layers.{j}.ew_net.0.bias']
    keys += ['v_inference.0.weight', 'v_inference.0.bias', 'v_inference.2.weight', 'v_inference.2.bias']
    return keys


def flatten_state_dict(sd, num_layers: int, ew_net_type='global', x2h_out_fc=False, num_x2h=1, num_h2x=1) -> np.ndarray:
    parts = [sd[k].detach().to('cpu', torch.float32).contiguous().reshape(-1).numpy()
             for k in flat_key_order(num_layers, ew_net_type, x2h_out_fc, num_x2h, num_h2x)]
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


SCHEDULE_ORDER = ('posterior_mean_c0_coef', 'posterior_mean_ct_coef', 'posterior_logvar', 'log_alphas_v',
                  'log_one_minus_alphas_v', 'log_alphas_cumprod_v', 'log_one_minus_alphas_cumprod_v')
# optional 8th array: needed by td_perturb / td_likelihood_prior (likelihood estimation), not by sampling
SCHEDULE_OPTIONAL = ('alphas_cumprod', 'sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod')
MEAN_TYPES = {'C0': 0, 'noise': 1}                        # td_config.model_mean_type


def _device_bound(fn):
    """Run a method of a handle-owning class with the handle's device current."""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *a, **k):
        for t in list(a) + list(k.values()):
            if torch.is_tensor(t) and t.is_cuda and t.device != self.device:
                raise RuntimeError(f'{fn.__name__}: tensor on {t.device}, but the native handle lives on {self.device}')
        with _on(self.device):
            return fn(self, *a, **k)
    return wrapped


class NativeModel:
    """Owns a td_model handle (packed weights on `device`) and a growable workspace."""

    def __init__(self, cfg: dict, state_dict, schedules: dict | None = None, device=None):
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise RuntimeError('no HIP device visible: targetdiff_amd needs an MI355X (gfx950); there is no CPU path')
        self.device = _canonical_device(device)
        mode = cfg.get('cutoff_mode', 'knn')
        if mode not in CUTOFF_MODES:
            raise ValueError(f'cutoff_mode must be one of {sorted(CUTOFF_MODES)}, got {mode!r}')
        self.cfg = TdConfig(hidden_dim=cfg['hidden_dim'], n_heads=cfg['n_heads'], knn=cfg['knn'],
                            num_layers=cfg['num_layers'], num_r_gaussian=cfg['num_r_gaussian'],
                            edge_feat_dim=cfg['edge_feat_dim'], protein_feat_dim=cfg['protein_feat_dim'],
                            ligand_num_classes=cfg['ligand_num_classes'], num_timesteps=cfg['num_timesteps'],
                            cutoff_mode=CUTOFF_MODES[mode], radius=float(cfg.get('radius', 0.0)),
                            max_num_neighbors=int(cfg.get('max_num_neighbors', 32)),
                            model_mean_type=MEAN_TYPES[cfg.get('model_mean_type', 'C0')], num_blocks=int(cfg.get('num_blocks', 1) or 1),
                            ew_net_type=ew_net_code(cfg.get('ew_net_type', 'global')), x2h_out_fc=int(bool(cfg.get('x2h_out_fc', False))),
                            sync_twoup=int(bool(cfg.get('sync_twoup', False))), num_x2h=int(cfg.get('num_x2h', 1) or 1),
                            num_h2x=int(cfg.get('num_h2x', 1) or 1))
        self.cutoff_mode, self.k = mode, int(cfg['knn'])
        self.default_graph = mode == 'knn' and self.k <= KNN       # the 32-slot fast path (and the caching session); k < 32
                                                                   # is the 32-NN row with the slots >= k masked
        self.num_classes = int(cfg['ligand_num_classes'])
        blob = flatten_state_dict(state_dict, cfg['num_layers'], cfg.get('ew_net_type', 'global'), bool(cfg.get('x2h_out_fc', False)),
                                  int(cfg.get('num_x2h', 1) or 1), int(cfg.get('num_h2x', 1) or 1))
        expect = self.lib.td_model_num_weights(ctypes.byref(self.cfg))
        if blob.size != expect:
            raise ValueError(f'weight blob has {blob.size} floats, library expects {expect}')
        sched_ptr, sched_n = None, 0
        if schedules is not None:
            # 7 arrays, + alphas_cumprod (8), + the two 'noise' arrays (10): the library takes these three lengths
            opt = SCHEDULE_OPTIONAL if all(o in schedules for o in SCHEDULE_OPTIONAL) else tuple(o for o in SCHEDULE_OPTIONAL[:1] if o in schedules)
            sch = np.ascontiguousarray(np.concatenate(
                [np.asarray(schedules[k], dtype=np.float32).reshape(-1) for k in SCHEDULE_ORDER + opt]))
            sched_ptr, sched_n = sch.ctypes.data_as(POINTER(c_float)), sch.size
        handle = c_void_p()
        with torch.cuda.device(self.device):
            _check(self.lib.td_model_create(ctypes.byref(self.cfg), blob.ctypes.data_as(POINTER(c_float)), blob.size,
                                            sched_ptr, sched_n, ctypes.byref(handle)), 'td_model_create')
        self.handle = handle
        self._ws = None

    def __del__(self):
        h, self.handle = getattr(self, 'handle', None), None
        if h and getattr(self, 'lib', None) is not None:
            self.lib.td_model_destroy(h)

    # ------------------------------------------------------------------------------------------
    @_device_bound
    def set_option(self, name: str, value: int):
        """Per-model switch (td_model_set_option; include/targetdiff_hip.h lists the names and their values).  Stored in the native
        handle; nothing is read from the environment."""
        _check(self.lib.td_model_set_option(self.handle, name.encode(), int(value)), 'td_model_set_option')

    def get_option(self, name: str) -> int:
        v = c_int32()
        _check(self.lib.td_model_get_option(self.handle, name.encode(), ctypes.byref(v)), 'td_model_get_option')
        return int(v.value)

    @_device_bound
    def graph_build(self, x: torch.Tensor, mask_ligand: torch.Tensor, node_ptr: torch.Tensor, width: int,
                    max_graph_nodes: int = 0) -> torch.Tensor:
        """The model's graph (its cutoff_mode) on a composed batch as a dense [N, width] table of in-neighbours, -1 padded."""
        N = x.shape[0]
        out = torch.empty(N, width, dtype=torch.int32, device=x.device)
        mask_u8 = mask_ligand.to(torch.uint8).contiguous()
        _check(self.lib.td_graph_build(self.handle, _ptr(x, torch.float32, 'x'), _ptr(mask_u8), _ptr(node_ptr, torch.int32, 'node_ptr'),
                                       N, node_ptr.numel() - 1, max_graph_nodes, _ptr(out), width, _stream(self.device)),
               'td_graph_build')
        return out

    def workspace(self, N: int, B: int, Nl: int) -> torch.Tensor:
        need = int(self.lib.td_workspace_bytes(self.handle, N, B, Nl))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    @_device_bound
    def graph_ptr(self, batch: torch.Tensor, B: int) -> torch.Tensor:
        ptr = torch.empty(B + 1, dtype=torch.int32, device=batch.device)
        _check(self.lib.td_graph_ptr(_ptr(batch, torch.int64, 'batch'), batch.numel(), B, _ptr(ptr), _stream(self.device)),
               'td_graph_ptr')
        return ptr

    @_device_bound
    def knn(self, x: torch.Tensor, node_ptr: torch.Tensor, k: int = KNN, max_graph_nodes: int = 0) -> torch.Tensor:
        N = x.shape[0]
        out = torch.empty(N, k, dtype=torch.int32, device=x.device)
        _check(self.lib.td_knn(_ptr(x, torch.float32, 'x'), _ptr(node_ptr, torch.int32, 'node_ptr'), N,
                               node_ptr.numel() - 1, k, max_graph_nodes, _ptr(out), _stream(self.device)), 'td_knn')
        return out

    @_device_bound
    def refine_forward(self, h, x, mask_ligand, node_ptr, fix_x=False, max_graph_nodes=0, want_graph=False):
        N, B = h.shape[0], node_ptr.numel() - 1
        out_h = torch.empty_like(h)
        out_x = torch.empty_like(x)
        if want_graph and not self.default_graph:
            raise ValueError('want_graph: the dense [N, 32] graph / gate outputs exist for the k = 32 kNN graph only (graph_build)')
        nbr = torch.empty(N, KNN, dtype=torch.int32, device=h.device) if want_graph else None
        ew = torch.empty(N, KNN, dtype=torch.float32, device=h.device) if want_graph else None
        ws = self.workspace(N, B, 0)
        mask_u8 = mask_ligand.to(torch.uint8).contiguous()
        _check(self.lib.td_refine_forward(
            self.handle, _ptr(h, torch.float32, 'h'), _ptr(x, torch.float32, 'x'), _ptr(mask_u8),
            _ptr(node_ptr, torch.int32, 'node_ptr'), N, B, int(bool(fix_x)), max_graph_nodes, _ptr(out_h), _ptr(out_x),
            _ptr(nbr), _ptr(ew), _ptr(ws), ws.numel(), _stream(self.device)), 'td_refine_forward')
        return out_h, out_x, nbr, ew

    @_device_bound
    def model_forward(self, protein_pos, protein_v, protein_ptr, ligand_pos, ligand_v, ligand_ptr, fix_x=False,
                      max_graph_nodes=0, want_final_h=True, out=None, ligand_graph_bias=None):
        Np, Nl, B = protein_pos.shape[0], ligand_pos.shape[0], protein_ptr.numel() - 1
        N, C = Np + Nl, self.num_classes
        dev = protein_pos.device
        if out is None:
            out = {}
        pred_pos = out.get('pred_ligand_pos')
        if pred_pos is None:
            pred_pos = torch.empty(Nl, 3, dtype=torch.float32, device=dev)
        pred_v = out.get('pred_ligand_v')
        if pred_v is None:
            pred_v = torch.empty(Nl, C, dtype=torch.float32, device=dev)
        lig_h = out.get('final_ligand_h')
        if lig_h is None:
            lig_h = torch.empty(Nl, HIDDEN, dtype=torch.float32, device=dev)
        final_h = torch.empty(N, HIDDEN, dtype=torch.float32, device=dev) if want_final_h else None
        ws = self.workspace(N, B, Nl)
        _check(self.lib.td_model_forward(
            self.handle, _ptr(protein_pos, torch.float32, 'protein_pos'), _ptr(protein_v, torch.float32, 'protein_v'),
            _ptr(protein_ptr, torch.int32, 'protein_ptr'), Np, _ptr(ligand_pos, torch.float32, 'ligand_pos'),
            _ptr(ligand_v, torch.int64, 'ligand_v'), _ptr(ligand_ptr, torch.int32, 'ligand_ptr'), Nl, B,
            int(bool(fix_x)), max_graph_nodes, _ptr(pred_pos), _ptr(pred_v), _ptr(lig_h), _ptr(final_h), _ptr(ws),
            ws.numel(), _graph_bias_ptr(ligand_graph_bias, B), _stream(self.device)), 'td_model_forward')
        return {'pred_ligand_pos': pred_pos, 'pred_ligand_v': pred_v, 'final_h': final_h, 'final_ligand_h': lig_h}

    @_device_bound
    def posterior_step(self, t, ligand_ptr, ligand_pos, ligand_v, pred_pos, pred_v, noise, uniform,
                       pos_next=None, v_next=None, log_v0=None, log_post=None, fixed_mask=None, fixed_pos=None, fixed_v=None,
                       prog_row=None, x0_shift=None):
        """One posterior update (td_posterior_step).  ``fixed_mask`` [N_l] bool with ``fixed_pos`` [N_l,3] (centred) and ``fixed_v``
        [N_l]: the flagged atoms take the forward-diffused copy of their known state instead (td_posterior_step_fixed).
        ``prog_row`` [schedule.ROW] fp32 on the device: a time program's slot, the step's coefficients come from it
        (td_posterior_step_program).  ``x0_shift`` [N_l,3] fp32: the step uses fl32(x0 + x0_shift) in place of the predicted x0
        (td_posterior_step_guided; clash guidance, ``guidance.clash_shift``); known atoms ignore it."""
        Nl, B = ligand_pos.shape[0], ligand_ptr.numel() - 1
        if pos_next is None:
            pos_next = torch.empty_like(ligand_pos)
        if v_next is None:
            v_next = torch.empty_like(ligand_v)
        fm, fp, fv = _fixed_ptrs(fixed_mask, fixed_pos, fixed_v, Nl)
        if x0_shift is not None and tuple(x0_shift.shape) != (Nl, 3):
            raise ValueError(f'x0_shift must be [{Nl}, 3] (got {tuple(x0_shift.shape)})')
        head = (self.handle, _ptr(t, torch.int32, 't'))
        body = (_ptr(ligand_ptr, torch.int32, 'ligand_ptr'), Nl, B,
                _ptr(ligand_pos, torch.float32, 'ligand_pos'), _ptr(ligand_v, torch.int64, 'ligand_v'),
                _ptr(pred_pos, torch.float32, 'pred_pos'), _ptr(pred_v, torch.float32, 'pred_v'),
                _ptr(noise, torch.float32, 'noise'), _ptr(uniform, torch.float32, 'uniform'), _ptr(pos_next),
                _ptr(v_next, torch.int64, 'v_next'), _ptr(log_v0), _ptr(log_post))
        prow = (_prog_row_ptr(prog_row) if prog_row is not None else None,)
        stream = (_stream(self.device),)
        # the entry point with the fewest optional pointers that takes the ones present
        if x0_shift is not None:
            name, args = 'td_posterior_step_guided', head + prow + body + (fm, fp, fv, _ptr(x0_shift, torch.float32, 'x0_shift')) + stream
        elif prog_row is not None:
            name, args = 'td_posterior_step_program', head + prow + body + (fm, fp, fv) + stream
        elif fm is not None:
            name, args = 'td_posterior_step_fixed', head + body + (fm, fp, fv) + stream
        else:
            name, args = 'td_posterior_step', head + body + stream
        _check(getattr(self.lib, name)(*args), name)
        return pos_next, v_next

    @_device_bound
    def renoise_step(self, prog_row, ligand_pos, ligand_v, noise, uniform=None, pos_next=None, v_next=None, log_v0=None, log_q=None):
        """One forward-process step of a time program (td_renoise_step): ``prog_row`` is the renoise slot's row of
        ``TimeProgram.tables`` on the device; ``uniform=None`` (pos_only) leaves the types alone."""
        Nl = ligand_pos.shape[0]
        if pos_next is None:
            pos_next = torch.empty_like(ligand_pos)
        if v_next is None:
            v_next = torch.empty_like(ligand_v)
        _check(self.lib.td_renoise_step(
            self.handle, _prog_row_ptr(prog_row), Nl, _ptr(ligand_pos, torch.float32, 'ligand_pos'),
            _ptr(ligand_v, torch.int64, 'ligand_v'), _ptr(noise, torch.float32, 'noise'),
            _ptr(uniform, torch.float32, 'uniform') if uniform is not None else None, _ptr(pos_next),
            _ptr(v_next, torch.int64, 'v_next'), _ptr(log_v0), _ptr(log_q), _stream(self.device)), 'td_renoise_step')
        return pos_next, v_next

    # ---- likelihood estimation / return_all (the other consumers of the denoiser)
    @_device_bound
    def perturb(self, t, ligand_ptr, ligand_pos, ligand_v, noise, uniform):
        Nl, B = ligand_pos.shape[0], ligand_ptr.numel() - 1
        pos_t, v_t = torch.empty_like(ligand_pos), torch.empty_like(ligand_v)
        _check(self.lib.td_perturb(self.handle, _ptr(t, torch.int32, 't'), _ptr(ligand_ptr, torch.int32, 'ligand_ptr'), Nl, B,
                                   _ptr(ligand_pos, torch.float32, 'ligand_pos'), _ptr(ligand_v, torch.int64, 'ligand_v'),
                                   _ptr(noise, torch.float32, 'noise'), _ptr(uniform, torch.float32, 'uniform'),
                                   _ptr(pos_t), _ptr(v_t), _stream(self.device)), 'td_perturb')
        return pos_t, v_t

    @_device_bound
    def likelihood_terms(self, t, ligand_ptr, pos_0, pos_t, v_0, v_t, pred_pos, pred_v):
        Nl, B = pos_0.shape[0], ligand_ptr.numel() - 1
        kl_pos = torch.empty(B, dtype=torch.float32, device=pos_0.device)
        kl_v = torch.empty(B, dtype=torch.float32, device=pos_0.device)
        _check(self.lib.td_likelihood_terms(
            self.handle, _ptr(t, torch.int32, 't'), _ptr(ligand_ptr, torch.int32, 'ligand_ptr'), Nl, B,
            _ptr(pos_0, torch.float32, 'pos_0'), _ptr(pos_t, torch.float32, 'pos_t'), _ptr(v_0, torch.int64, 'v_0'),
            _ptr(v_t, torch.int64, 'v_t'), _ptr(pred_pos, torch.float32, 'pred_pos'), _ptr(pred_v, torch.float32, 'pred_v'),
            _ptr(kl_pos), _ptr(kl_v), _stream(self.device)), 'td_likelihood_terms')
        return kl_pos, kl_v

    @_device_bound
    def likelihood_prior(self, ligand_ptr, pos_0, v_index):
        Nl, B = pos_0.shape[0], ligand_ptr.numel() - 1
        kl_pos = torch.empty(B, dtype=torch.float32, device=pos_0.device)
        kl_v = torch.empty(B, dtype=torch.float32, device=pos_0.device)
        _check(self.lib.td_likelihood_prior(self.handle, _ptr(ligand_ptr, torch.int32, 'ligand_ptr'), Nl, B,
                                            _ptr(pos_0, torch.float32, 'pos_0'), _ptr(v_index, torch.int64, 'v_index'),
                                            _ptr(kl_pos), _ptr(kl_v), _stream(self.device)), 'td_likelihood_prior')
        return kl_pos, kl_v

    @_device_bound
    def diffusion_loss(self, t, ligand_ptr, pos_0, pos_t, noise, v_0, v_t, pred_pos, pred_v, loss_v_weight, check=True):
        """The arithmetic of get_diffusion_loss after the network call (td_diffusion_loss; models/molopt_score_model.py:521-563), forward
        only.  ``noise`` may be None for model_mean_type 'C0'.  Returns a dict: 'loss_pos', 'loss_v', 'loss' (0-d views of one [3] tensor),
        'loss_pos_graph', 'loss_v_graph' [B], 'pred_pos_noise' [N_l, 3], 'ligand_v_recon' [N_l, C].  ``check`` looks at ``ligand_ptr`` on
        the host (one synchronisation): it must be ascending prefix offsets from 0 to N_l, since the kernel reads the atoms it names."""
        Nl, B, C = pos_0.shape[0], ligand_ptr.numel() - 1, self.num_classes
        dev = pos_0.device
        if tuple(pred_v.shape) != (Nl, C) or tuple(pred_pos.shape) != (Nl, 3) or tuple(pos_t.shape) != (Nl, 3) or t.numel() != B:
            raise ValueError(f'diffusion_loss: shapes do not fit {Nl} atoms, {B} graphs, {C} classes')
        if noise is not None and tuple(noise.shape) != (Nl, 3):
            raise ValueError(f'noise must be [{Nl}, 3] (got {tuple(noise.shape)})')
        if tuple(pos_0.shape) != (Nl, 3) or tuple(v_0.shape) != (Nl,) or tuple(v_t.shape) != (Nl,):
            raise ValueError(f'diffusion_loss: pos_0 must be [{Nl}, 3] and v_0 / v_t [{Nl}] (got {tuple(pos_0.shape)}, {tuple(v_0.shape)}, '
                             f'{tuple(v_t.shape)})')
        if check and B >= 0:
            p = ligand_ptr.tolist()
            if not p or p[0] != 0 or p[-1] != Nl or any(b < a for a, b in zip(p, p[1:])):
                raise ValueError(f'diffusion_loss: ligand_ptr must be ascending prefix offsets from 0 to N_l = {Nl}')
        eps = torch.empty(Nl, 3, dtype=torch.float32, device=dev)
        recon = torch.empty(Nl, C, dtype=torch.float32, device=dev)
        lp_g = torch.empty(B, dtype=torch.float32, device=dev)
        lv_g = torch.empty(B, dtype=torch.float32, device=dev)
        scalars = torch.empty(3, dtype=torch.float32, device=dev)
        _check(self.lib.td_diffusion_loss(
            self.handle, _ptr(t, torch.int32, 't'), _ptr(ligand_ptr, torch.int32, 'ligand_ptr'), Nl, B,
            _ptr(pos_0, torch.float32, 'pos_0'), _ptr(pos_t, torch.float32, 'pos_t'), _ptr(noise, torch.float32, 'noise'),
            _ptr(v_0, torch.int64, 'v_0'), _ptr(v_t, torch.int64, 'v_t'), _ptr(pred_pos, torch.float32, 'pred_pos'),
            _ptr(pred_v, torch.float32, 'pred_v'), float(loss_v_weight), _ptr(eps), _ptr(recon), _ptr(lp_g), _ptr(lv_g), _ptr(scalars),
            _stream(self.device)), 'td_diffusion_loss')
        return {'loss_pos': scalars[0], 'loss_v': scalars[1], 'loss': scalars[2], 'loss_pos_graph': lp_g, 'loss_v_graph': lv_g,
                'pred_pos_noise': eps, 'ligand_v_recon': recon}

    @_device_bound
    def embed_ligand(self, ligand_v):
        h = torch.empty(ligand_v.shape[0], HIDDEN, dtype=torch.float32, device=ligand_v.device)
        _check(self.lib.td_embed_ligand(self.handle, _ptr(ligand_v, torch.int64, 'ligand_v'), ligand_v.shape[0], _ptr(h),
                                        _stream(self.device)), 'td_embed_ligand')
        return h

    @_device_bound
    def v_inference(self, h):
        out = torch.empty(h.shape[0], self.num_classes, dtype=torch.float32, device=h.device)
        _check(self.lib.td_v_inference(self.handle, _ptr(h, torch.float32, 'h'), h.shape[0], _ptr(out), _stream(self.device)),
               'td_v_inference')
        return out

    @_device_bound
    def center_pos(self, protein_pos, protein_ptr, ligand_pos, ligand_ptr, offset=None, sign=-1):
        """In place.  offset=None: compute the protein centroids and subtract them (sign=-1)."""
        B = protein_ptr.numel() - 1
        compute = offset is None
        if compute:
            offset = torch.empty(B, 3, dtype=torch.float32, device=protein_ptr.device)
        _check(self.lib.td_center_pos(_ptr(protein_pos) if protein_pos is not None else None,
                                      _ptr(protein_ptr, torch.int32, 'protein_ptr'), _ptr(ligand_pos),
                                      _ptr(ligand_ptr, torch.int32, 'ligand_ptr'), B, _ptr(offset), int(compute), sign,
                                      _stream(self.device)), 'td_center_pos')
        return offset

    @_device_bound
    def debug_node_stage(self, layer: int, stage: int, h: torch.Tensor):
        """Test hook: node projections P [N,512] and query vectors q [N,128] of one attention stage."""
        N = h.shape[0]
        P = torch.empty(N, 4 * HIDDEN, dtype=torch.float32, device=h.device)
        q = torch.empty(N, HIDDEN, dtype=torch.float32, device=h.device)
        _check(self.lib.td_debug_node_stage(self.handle, layer, stage, _ptr(h, torch.float32, 'h'), N, _ptr(P), _ptr(q),
                                            _stream(self.device)), 'td_debug_node_stage')
        return P, q


AUROC_MAX_ROWS = 1 << 20      # td_auroc: pairs2 stays below 2^41


def auroc_counts(scores, labels):
    """``n_pos`` [C] and ``pairs2`` [C] int64 of td_auroc (include/targetdiff_hip.h) for ``scores`` [N, C] fp32 and ``labels`` [N] int64
    on a HIP device: per class the positives, and 2 #{pos > neg} + #{pos == neg} over its (positive, negative) pairs.  Raises ValueError
    for a NaN score or a label outside [0, C)."""
    if scores.dim() != 2 or labels.dim() != 1 or labels.shape[0] != scores.shape[0]:
        raise ValueError(f'auroc: scores [N, C] and labels [N] (got {tuple(scores.shape)}, {tuple(labels.shape)})')
    N, C = scores.shape
    if N > AUROC_MAX_ROWS:
        raise ValueError(f'auroc: {N} rows, the counts are built for at most {AUROC_MAX_ROWS}')
    if N and bool(torch.isnan(scores).any()):
        raise ValueError('auroc: a score is NaN')
    if N and bool(((labels < 0) | (labels >= C)).any()):
        raise ValueError(f'auroc: labels must be in [0, {C})')
    lib = load_library()
    dev = scores.device
    n_pos = torch.empty(C, dtype=torch.int64, device=dev)
    pairs2 = torch.empty(C, dtype=torch.int64, device=dev)
    with _on(dev):
        _check(lib.td_auroc(_ptr(scores, torch.float32, 'scores'), _ptr(labels, torch.int64, 'labels'), N, C, _ptr(n_pos), _ptr(pairs2),
                            _stream(dev)), 'td_auroc')
    return n_pos, pairs2


def auroc_from_counts(n_pos, pairs2):
    """get_auroc's numbers (scripts/train_diffusion.py:22-36) from td_auroc's counts, in float64: ``(weighted average, {class: auroc})``
    over the classes present; raises ValueError where a class holds every row (sklearn's roc_auc_score raises there as well)."""
    n_pos = [int(x) for x in n_pos]
    pairs2 = [int(x) for x in pairs2]
    N = sum(n_pos)
    per_class, avg = {}, 0.0
    for c, (n, p2) in enumerate(zip(n_pos, pairs2)):
        if n == 0:
            continue                                            # possible_classes = set(y_true)
        if N - n == 0:
            raise ValueError(f'auroc: class {c} holds every row; the one-vs-rest ROC is not defined with one class present')
        per_class[c] = float(np.float64(p2) / (2.0 * np.float64(n) * np.float64(N - n)))
        avg += per_class[c] * n
    if N == 0:
        raise ValueError('auroc: no rows')
    return avg / N, per_class


def auroc(scores, labels):
    """Atom-type AUROC of get_auroc (scripts/train_diffusion.py:22-36): ``(weighted average, {class: auroc})``; the N^2 comparisons run
    in td_auroc on the device as exact integers, the divisions here in float64."""
    n_pos, pairs2 = auroc_counts(scores, labels)
    return auroc_from_counts(n_pos.tolist(), pairs2.tolist())


class NativeSession:
    """Loop-invariant state of one sample_diffusion call (td_session): the centred protein is handed over once."""

    def __init__(self, native: NativeModel, protein_pos, protein_v, protein_ptr, ligand_ptr, num_ligand_atoms: int,
                 max_graph_nodes: int = 0):
        self.native = native
        self.lib = native.lib
        self.Nl = int(num_ligand_atoms)
        self.C = native.num_classes
        self.device = protein_pos.device
        handle = c_void_p()
        with _on(self.device):          # the session block is hipMalloc'ed on the current device
            _check(self.lib.td_session_create(
                native.handle, _ptr(protein_pos, torch.float32, 'protein_pos'), _ptr(protein_v, torch.float32, 'protein_v'),
                _ptr(protein_ptr, torch.int32, 'protein_ptr'), protein_pos.shape[0], _ptr(ligand_ptr, torch.int32, 'ligand_ptr'),
                self.Nl, protein_ptr.numel() - 1, max_graph_nodes, _stream(self.device), ctypes.byref(handle)),
                'td_session_create')
        self.handle = handle

    def __del__(self):
        h, self.handle = getattr(self, 'handle', None), None
        if h and getattr(self, 'lib', None) is not None:
            try:
                with _on(self.device):
                    self.lib.td_session_destroy(h)
            except Exception:            # interpreter shutdown: torch may already be gone
                self.lib.td_session_destroy(h)

    @_device_bound
    def forward(self, ligand_pos, ligand_v, out=None, ligand_graph_bias=None):
        out = out or {}
        dev = ligand_pos.device
        pred_pos = out.get('pred_ligand_pos')
        if pred_pos is None:
            pred_pos = torch.empty(self.Nl, 3, dtype=torch.float32, device=dev)
        pred_v = out.get('pred_ligand_v')
        if pred_v is None:
            pred_v = torch.empty(self.Nl, self.C, dtype=torch.float32, device=dev)
        lig_h = out.get('final_ligand_h')
        if lig_h is None:
            lig_h = torch.empty(self.Nl, HIDDEN, dtype=torch.float32, device=dev)
        _check(self.lib.td_session_forward(self.handle, _ptr(ligand_pos, torch.float32, 'ligand_pos'),
                                           _ptr(ligand_v, torch.int64, 'ligand_v'), _ptr(pred_pos), _ptr(pred_v),
                                           _ptr(lig_h), _graph_bias_ptr(ligand_graph_bias, None), _stream(self.device)),
               'td_session_forward')
        return {'pred_ligand_pos': pred_pos, 'pred_ligand_v': pred_v, 'final_h': None, 'final_ligand_h': lig_h}

    def make_step_io(self, step_index, t_all, ligand_pos, ligand_v, noise, uniform, pos_traj, v_traj, v0_traj=None,
                     vt_traj=None, pos_only=False, ligand_graph_bias=None, fixed_mask=None, fixed_pos=None, fixed_v=None) -> StepIO:
        """The argument block of :meth:`step`; the tensors must stay alive (and in place) for as long as it is used.
        ``fixed_mask`` / ``fixed_pos`` / ``fixed_v``: known atoms, see :meth:`NativeModel.posterior_step`."""
        S = int(t_all.shape[0])
        if step_index.numel() != 2 or pos_traj.shape[0] != S or v_traj.shape[0] != S:
            raise ValueError('step_index must hold 2 int32, the trajectories one slot per step')
        io = StepIO()           # ctypes zero-fills it, padding included: the library compares the whole block (memcmp) to re-capture
        io.d_step = _ptr(step_index, torch.int32, 'step_index').value
        io.d_t_all = _ptr(t_all, torch.int32, 't_all').value
        io.num_steps, io.pos_only = S, int(bool(pos_only))
        io.d_ligand_pos = _ptr(ligand_pos, torch.float32, 'ligand_pos').value
        io.d_ligand_v = _ptr(ligand_v, torch.int64, 'ligand_v').value
        io.d_noise = _ptr(noise, torch.float32, 'noise').value
        io.d_uniform = _ptr(uniform, torch.float32, 'uniform').value
        io.d_pos_traj = _ptr(pos_traj, torch.float32, 'pos_traj').value
        io.d_v_traj = _ptr(v_traj, torch.int64, 'v_traj').value
        io.d_v0_traj = _ptr(v0_traj, torch.float32, 'v0_traj').value if v0_traj is not None and v0_traj.numel() else None
        io.d_vt_traj = _ptr(vt_traj, torch.float32, 'vt_traj').value if vt_traj is not None and vt_traj.numel() else None
        gb = _graph_bias_ptr(ligand_graph_bias, int(t_all.shape[1]))
        io.d_ligand_graph_bias = gb.value if gb is not None else None
        fm, fp, fv = _fixed_ptrs(fixed_mask, fixed_pos, fixed_v, self.Nl)
        if fm is not None:
            io.d_fixed_mask, io.d_fixed_pos, io.d_fixed_v = fm.value, fp.value, fv.value
        return io

    def set_program(self, table, kinds):
        """Attach a time program (td_session_set_program): ``table`` [S, PROG_ROW] fp32 on the device (kept alive here), ``kinds``
        [S] host integers (0 denoise, 1 renoise).  ``table=None`` removes it.  Call k of :meth:`step` after this runs slot k."""
        if table is None:
            self._prog_table = None
            with _on(self.device):
                _check(self.lib.td_session_set_program(self.handle, None, None, 0), 'td_session_set_program')
            return
        kinds = [int(k) for k in kinds]
        if table.dtype != torch.float32 or tuple(table.shape) != (len(kinds), PROG_ROW) or not table.is_contiguous():
            raise ValueError(f'the program table must be contiguous fp32 [{len(kinds)}, {PROG_ROW}]')
        arr = (c_int32 * len(kinds))(*kinds)
        self._prog_table = table
        with _on(self.device):
            _check(self.lib.td_session_set_program(self.handle, _ptr(table, torch.float32, 'table'), arr, len(kinds)),
                   'td_session_set_program')

    def set_guidance(self, sigma, weight=1.0, max_shift=0.0):
        """Clash guidance for every denoise step from now on (td_session_set_guidance): ``sigma`` [N_p] fp32 contact radii of the
        session's protein atoms, all > 0 (checked here: the library does not read them on the host).  ``sigma=None`` removes it."""
        with _on(self.device):
            if sigma is None:
                _check(self.lib.td_session_set_guidance(self.handle, None, 0.0, 0.0), 'td_session_set_guidance')
                return
            if not bool((sigma > 0).all()):
                raise ValueError('clash guidance: every contact radius must be > 0')
            _check(self.lib.td_session_set_guidance(self.handle, _ptr(sigma, torch.float32, 'sigma'), float(weight), float(max_shift)),
                   'td_session_set_guidance')

    def step(self, io: StepIO, use_graph=True):
        """One reverse-diffusion step (denoiser + posterior update + trajectory record) as one replayable unit
        (td_session_step): captured into a hipGraph at the second call, replayed from then on."""
        with _on(self.device):
            _check(self.lib.td_session_step(self.handle, ctypes.byref(io), int(bool(use_graph)), _stream(self.device)),
                   'td_session_step')

    def last_step_was_graph(self) -> bool:
        return bool(self.lib.td_session_step_graph(self.handle))

    def row_counts(self):
        """(N, rows recomputed at layer 0, [receptive-field level sizes ...]) of the last forward; synchronises.

        Level k (1-based) is what the layer k - 1 from the end has to update when only ligand outputs are read."""
        n = self._counts()
        return int(n[0]), int(n[1]), [int(v) for v in n[2:6] if v >= 0]

    def forward_reach_rows(self):
        """Rows layer 1 recomputes (the ligand's one-hop forward reach), or None when that pruning is off."""
        v = int(self._counts()[6])
        return v if v >= 0 else None

    def shared_static_tables(self):
        """(rows of the static tables, distinct protein blocks of the batch) when the session keeps its static tables once per pocket
        (all samples of a pocket carry the same protein block; model option ``session_share_pockets``), else None."""
        n = self._counts()
        return (int(n[7]), int(n[8])) if n[7] >= 0 else None

    @_device_bound
    def _counts(self):
        n = (c_int32 * 10)()
        _check(self.lib.td_session_row_counts(self.handle, n, 10, _stream(self.device)), 'td_session_row_counts')
        return n

    def dirty_rows(self) -> int:
        return self.row_counts()[1]


# ----------------------------------------------------------------------------------------- standalone EGNN refine net
EGNN_LAYER_KEYS = ('edge_mlp.net.0.weight', 'edge_mlp.net.0.bias', 'edge_mlp.net.2.weight', 'edge_mlp.net.2.bias',
                   'edge_inf.0.weight', 'edge_inf.0.bias', 'x_mlp.0.weight', 'x_mlp.0.bias', 'x_mlp.2.weight',
                   'node_mlp.net.0.weight', 'node_mlp.net.0.bias', 'node_mlp.net.2.weight', 'node_mlp.net.2.bias')


def egnn_flat_key_order(num_layers: int):
    return [f'net.{l}.{k}' for l in range(num_layers) for k in EGNN_LAYER_KEYS]


def graph_ptr(batch: torch.Tensor, B: int) -> torch.Tensor:
    """CSR offsets of a sorted PyG ``batch`` vector (td_graph_ptr); no model handle needed."""
    lib = load_library()
    ptr = torch.empty(B + 1, dtype=torch.int32, device=batch.device)
    with _on(batch.device):
        _check(lib.td_graph_ptr(_ptr(batch, torch.int64, 'batch'), batch.numel(), B, _ptr(ptr), _stream(batch.device)),
               'td_graph_ptr')
    return ptr


def _clash_inputs(protein_pos, sigma, protein_ptr, ligand_ptr, pos, check=True):
    Np, Nl, B = protein_pos.shape[0], pos.shape[0], protein_ptr.numel() - 1
    if protein_pos.dim() != 2 or protein_pos.shape[1] != 3 or pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError(f'protein_pos / pos must be [N_p, 3] / [N_l, 3] (got {tuple(protein_pos.shape)}, {tuple(pos.shape)})')
    if tuple(sigma.shape) != (Np,):
        raise ValueError(f'sigma must be [{Np}] (got {tuple(sigma.shape)})')
    if ligand_ptr.numel() != B + 1 or B < 0:
        raise ValueError('protein_ptr and ligand_ptr must have the same length B + 1')
    if not check:     # a sampler's per-step call: the same offsets and radii were checked when it was set up
        return B
    if B > 0:         # the kernels index by these offsets: check them before anything runs (set-up / reporting path, one sync)
        pp, lp = protein_ptr.cpu(), ligand_ptr.cpu()
        if int(pp[0]) != 0 or int(lp[0]) != 0 or int(pp[-1]) != Np or int(lp[-1]) != Nl or bool((pp[1:] < pp[:-1]).any()) or \
                bool((lp[1:] < lp[:-1]).any()):
            raise ValueError('protein_ptr / ligand_ptr must be non-decreasing prefix offsets from 0 to N_p / N_l')
    if Np > 0 and not bool((sigma > 0).all()):
        raise ValueError('every contact radius must be > 0')
    return B


def clash_shift(protein_pos, sigma, protein_ptr, ligand_ptr, pos, weight=1.0, max_shift=0.0, out=None, check=True):
    """The clash-guidance shift [N_l, 3] of the points ``pos`` (td_clash_shift, include/targetdiff_hip.h); no model handle needed.
    ``check=False`` skips the host-side look at the offsets and radii (one synchronisation)."""
    lib = load_library()
    B = _clash_inputs(protein_pos, sigma, protein_ptr, ligand_ptr, pos, check)
    if out is None:
        out = torch.empty_like(pos)
    with _on(pos.device):
        _check(lib.td_clash_shift(_ptr(protein_pos, torch.float32, 'protein_pos'), _ptr(sigma, torch.float32, 'sigma'),
                                  _ptr(protein_ptr, torch.int32, 'protein_ptr'), _ptr(ligand_ptr, torch.int32, 'ligand_ptr'), B,
                                  _ptr(pos, torch.float32, 'pos'), float(weight), float(max_shift), _ptr(out, torch.float32, 'out'),
                                  _stream(pos.device)), 'td_clash_shift')
    return out


def clash_report(protein_pos, sigma, protein_ptr, ligand_ptr, pos):
    """Per graph: (pairs with d < sigma [B] int32, energy [B] fp32, smallest distance [B] fp32) (td_clash_report)."""
    lib = load_library()
    B = _clash_inputs(protein_pos, sigma, protein_ptr, ligand_ptr, pos)
    dev = pos.device
    count = torch.empty(B, dtype=torch.int32, device=dev)
    energy = torch.empty(B, dtype=torch.float32, device=dev)
    min_dist = torch.empty(B, dtype=torch.float32, device=dev)
    with _on(dev):
        _check(lib.td_clash_report(_ptr(protein_pos, torch.float32, 'protein_pos'), _ptr(sigma, torch.float32, 'sigma'),
                                   _ptr(protein_ptr, torch.int32, 'protein_ptr'), _ptr(ligand_ptr, torch.int32, 'ligand_ptr'), B,
                                   _ptr(pos, torch.float32, 'pos'), _ptr(count), _ptr(energy), _ptr(min_dist), _stream(dev)),
               'td_clash_report')
    return count, energy, min_dist


QUALITY_MAX_CLASSES, QUALITY_MAX_PROFILES, QUALITY_BINS = 64, 4, 128      # TD_QUALITY_* (csrc/td_internal.h)
QUALITY_ELEMENTS = (1, 6, 7, 8, 9, 15, 16, 17)                            # H C N O F P S Cl: the columns of the element counts


def _hist_edges(edges, bins, what, name='edges'):
    """The edges of one profile of a histogram of ``bins`` bins as contiguous float64 numpy: 1 .. bins - 1 of them, finite, ascending"""
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.float64).reshape(-1))
    if not 1 <= e.size <= bins - 1:
        raise ValueError(f'a {what} profile has 1 .. {bins - 1} edges (got {e.size})')
    if not np.isfinite(e).all() or bool((e[1:] < e[:-1]).any()):
        raise ValueError(f'the {name} of a {what} profile must be finite and ascending')
    return e


def _bond_ptr_input(bond_ptr, S, B):
    if bond_ptr is not None and (bond_ptr.dim() != 1 or bond_ptr.numel() != S * B + 1 or bond_ptr.dtype != torch.int64):
        raise ValueError(f'bond_ptr must be [{S * B + 1}] int64, as bond_graph returns it')


def _include_arg(include):
    """``include`` [S, B] bool / uint8 or None as the entry points' uint8 pointer"""
    if include is not None and include.dtype == torch.bool:
        include = include.view(torch.uint8)
    return _ptr(include, torch.uint8, 'include')


def _pack_args(pos, v, ligand_ptr, S, Nl, B, cz):
    """The leading arguments of every entry point over a pack: (d_pos, d_v, d_ligand_ptr, S, N_l, B, class table, K).  A binding forms
    them before it allocates anything, so a CPU tensor is refused first.  ``cz`` is the caller's: it outlives the call."""
    return (_ptr(pos, torch.float32, 'pos'), _ptr(v, torch.int64, 'v'), _ptr(ligand_ptr, torch.int32, 'ligand_ptr'), S, Nl, B,
            cz.ctypes.data_as(POINTER(c_int32)), cz.size)


def _profile_args(struct, prof, dev):
    """The checked profiles (their edges last) as the entry points' (array of ``struct``, P), the edges uploaded to ``dev``; the third
    value keeps both alive up to the call.  torch's allocator reuses the edges' memory in stream order: after the kernel."""
    edges = [torch.from_numpy(p[-1]).to(dev) for p in prof]
    parr = (struct * max(len(prof), 1))()
    for k, p in enumerate(prof):
        parr[k] = struct(*p[:-1], n_edges=p[-1].size, d_edges=edges[k].data_ptr())
    return ctypes.cast(parr, c_void_p), len(prof), (parr, edges)


def _quality_inputs(pos, v, ligand_ptr, class_z, include, profiles, check=True):
    """Shapes, the class table and the profiles of a quality_report call; with ``check`` the offsets and the classes are looked at on
    the host (one synchronisation), as _clash_inputs does.  Returns (S, N_l, B, class table as int32 numpy, [(z1, z2, cutoff, edges
    as float64 numpy)])."""
    if pos.dim() != 3 or pos.shape[2] != 3 or tuple(v.shape) != tuple(pos.shape[:2]):
        raise ValueError(f'pos / v must be [S, N_l, 3] / [S, N_l] (got {tuple(pos.shape)}, {tuple(v.shape)})')
    S, Nl, B = pos.shape[0], pos.shape[1], ligand_ptr.numel() - 1
    if ligand_ptr.dim() != 1 or B < 0:
        raise ValueError('ligand_ptr must be [B + 1]')
    cz = np.asarray(class_z, dtype=np.int64).reshape(-1)
    if not 1 <= cz.size <= QUALITY_MAX_CLASSES:
        raise ValueError(f'the class table must have 1 .. {QUALITY_MAX_CLASSES} entries (got {cz.size})')
    if not np.isin(cz, QUALITY_ELEMENTS).all():
        raise ValueError(f'atomic numbers {sorted(set(cz.tolist()) - set(QUALITY_ELEMENTS))} are outside the bond-length table '
                         f'{QUALITY_ELEMENTS}')
    if include is not None and (tuple(include.shape) != (S, B) or include.dtype not in (torch.bool, torch.uint8)):
        raise ValueError(f'include must be [{S}, {B}] bool or uint8')
    if len(profiles) > QUALITY_MAX_PROFILES:
        raise ValueError(f'at most {QUALITY_MAX_PROFILES} pair profiles (got {len(profiles)})')
    prof = []
    for z1, z2, cutoff, edges in profiles:
        e = _hist_edges(edges, QUALITY_BINS, 'pair')
        if any(z != 0 and z not in QUALITY_ELEMENTS for z in (int(z1), int(z2))):
            raise ValueError(f'a pair profile names elements of {QUALITY_ELEMENTS} or 0 for any (got {z1}, {z2})')
        if not float(cutoff) > 0.0:
            raise ValueError('the cutoff of a pair profile must be > 0')
        prof.append((int(z1), int(z2), float(cutoff), e))
    if check and B > 0:
        lp = ligand_ptr.cpu()
        if int(lp[0]) != 0 or int(lp[-1]) != Nl or bool((lp[1:] < lp[:-1]).any()):
            raise ValueError('ligand_ptr must be non-decreasing prefix offsets from 0 to N_l')
    if check and v.numel() and (int(v.min()) < 0 or int(v.max()) >= cz.size):
        raise ValueError(f'v must be in [0, {cz.size})')
    return S, Nl, B, cz.astype(np.int32), prof


def quality_report(pos, v, ligand_ptr, class_z, profiles=(), include=None, return_nr_bonds=True, check=True):
    """Stability and pair-distance counts of S frames of B molecules (td_quality_report, include/targetdiff_hip.h); no model handle
    needed.  ``pos`` [S, N_l, 3] fp32, ``v`` [S, N_l] int64, ``ligand_ptr`` [B + 1] int32, ``class_z`` the atomic number per class,
    ``profiles`` a sequence of (z1, z2, cutoff, edges), ``include`` [S, B] bool / uint8 or None.  Returns a dict of device tensors:
    nr_bonds [S, N_l] int32 (None without ``return_nr_bonds``), stable_atoms [S, B] int32, mol_stable [S, B] uint8, hist [S, P, 128]
    int64 and counts [S, 8] int64."""
    S, Nl, B, cz, prof = _quality_inputs(pos, v, ligand_ptr, class_z, include, profiles, check)
    lib = load_library()
    pack = _pack_args(pos, v, ligand_ptr, S, Nl, B, cz)
    dev = pos.device
    parr, P, _keep = _profile_args(TdPairProfile, prof, dev)
    out = dict(nr_bonds=torch.empty(S, Nl, dtype=torch.int32, device=dev) if return_nr_bonds else None,
               stable_atoms=torch.empty(S, B, dtype=torch.int32, device=dev), mol_stable=torch.empty(S, B, dtype=torch.uint8, device=dev),
               hist=torch.empty(S, P, QUALITY_BINS, dtype=torch.int64, device=dev), counts=torch.empty(S, 8, dtype=torch.int64, device=dev))
    with _on(dev):
        _check(lib.td_quality_report(*pack, _include_arg(include), parr, P, _ptr(out['nr_bonds']), _ptr(out['stable_atoms']),
                                     _ptr(out['mol_stable']), _ptr(out['hist']), _ptr(out['counts']), _stream(dev)), 'td_quality_report')
    return out


BOND_MAX_ATOMS, BOND_MAX_PROFILES, BOND_BINS = 512, 16, 128                 # TD_BOND_* (csrc/td_internal.h)


def _bond_inputs(pos, v, ligand_ptr, class_z, class_aromatic, include, profiles, check=True):
    """Shapes, the class table, the aromatic flags and the bond profiles of a bond_graph / bond_list call; with ``check`` the offsets,
    the classes and the molecule sizes are looked at on the host (one synchronisation).  Returns (S, N_l, B, class table as int32
    numpy, aromatic flags as uint8 numpy or None, [(z1, z2, category, edges as float64 numpy)])."""
    S, Nl, B, cz, _ = _quality_inputs(pos, v, ligand_ptr, class_z, include, (), check)
    aro = None
    if class_aromatic is not None:
        aro = np.ascontiguousarray(np.asarray(class_aromatic).reshape(-1) != 0, dtype=np.uint8)
        if aro.size != cz.size:
            raise ValueError(f'class_aromatic must have one flag per class ({cz.size}; got {aro.size})')
    if len(profiles) > BOND_MAX_PROFILES:
        raise ValueError(f'at most {BOND_MAX_PROFILES} bond profiles (got {len(profiles)})')
    prof = []
    for z1, z2, category, edges in profiles:
        e = _hist_edges(edges, BOND_BINS, 'bond')
        if any(z != 0 and z not in QUALITY_ELEMENTS for z in (int(z1), int(z2))):
            raise ValueError(f'a bond profile names elements of {QUALITY_ELEMENTS} or 0 for any (got {z1}, {z2})')
        if int(category) not in (0, 1, 2, 3, 4):
            raise ValueError(f'the category of a bond profile is 0 (any), 1, 2, 3 or 4 (got {category})')
        prof.append((int(z1), int(z2), int(category), e))
    if check and B > 0:
        sizes = ligand_ptr.cpu().to(torch.int64).diff()
        if int(sizes.max()) > BOND_MAX_ATOMS:
            raise ValueError(f'molecule {int(sizes.argmax())} has {int(sizes.max())} atoms: the bond graph takes at most {BOND_MAX_ATOMS}')
    return S, Nl, B, cz, aro, prof


def _aromatic_arg(aro):
    return None if aro is None else aro.ctypes.data_as(POINTER(ctypes.c_uint8))


def bond_graph(pos, v, ligand_ptr, class_z, class_aromatic=None, profiles=(), include=None, return_fragments=False, return_bond_ptr=False,
               check=True):
    """Bonds, fragments and bond-length counts of S frames of B molecules (td_bond_graph, include/targetdiff_hip.h); no model handle
    needed.  The pack as quality_report's; ``class_aromatic`` one flag per class or None; ``profiles`` a sequence of (z1, z2, category,
    edges).  Returns a dict of device tensors: n_bonds, n_fragments, largest_fragment [S, B] int32, fragment [S, N_l] int32 (None
    without ``return_fragments``), bond_hist [S, P, 128] int64 and bond_ptr [S * B + 1] int64 (None without ``return_bond_ptr``)."""
    S, Nl, B, cz, aro, prof = _bond_inputs(pos, v, ligand_ptr, class_z, class_aromatic, include, profiles, check)
    lib = load_library()
    pack = _pack_args(pos, v, ligand_ptr, S, Nl, B, cz)
    dev = pos.device
    parr, P, _keep = _profile_args(TdBondProfile, prof, dev)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    out = dict(n_bonds=i32(S, B), n_fragments=i32(S, B), largest_fragment=i32(S, B), fragment=i32(S, Nl) if return_fragments else None,
               bond_hist=torch.empty(S, P, BOND_BINS, dtype=torch.int64, device=dev),
               bond_ptr=torch.empty(S * B + 1, dtype=torch.int64, device=dev) if return_bond_ptr else None)
    with _on(dev):
        _check(lib.td_bond_graph(*pack, _include_arg(include), _aromatic_arg(aro), parr, P, _ptr(out['n_bonds']), _ptr(out['n_fragments']),
                                 _ptr(out['largest_fragment']), _ptr(out['fragment']), _ptr(out['bond_hist']), _ptr(out['bond_ptr']),
                                 _stream(dev)), 'td_bond_graph')
    return out


def bond_list(pos, v, ligand_ptr, class_z, class_aromatic, bond_ptr, check=True):
    """The bonds of a pack in ascending (frame, molecule, i, j) order (td_bond_list); ``bond_ptr`` [S * B + 1] int64 from bond_graph on
    the same pack.  Its last entry is read on the host to size the outputs: the one synchronisation of the path.  Returns a dict of
    device tensors: bond_atoms [nb, 2] int32 (indices along the pack's atom axis), bond_order and bond_category [nb] uint8 and
    bond_length [nb] float64."""
    S, Nl, B, cz, aro, _ = _bond_inputs(pos, v, ligand_ptr, class_z, class_aromatic, None, (), check)
    _bond_ptr_input(bond_ptr, S, B)
    lib = load_library()
    pack = _pack_args(pos, v, ligand_ptr, S, Nl, B, cz)
    _ptr(bond_ptr, torch.int64, 'bond_ptr')
    dev = pos.device
    nb = int(bond_ptr[-1])
    out = dict(bond_atoms=torch.empty(nb, 2, dtype=torch.int32, device=dev), bond_order=torch.empty(nb, dtype=torch.uint8, device=dev),
               bond_category=torch.empty(nb, dtype=torch.uint8, device=dev), bond_length=torch.empty(nb, dtype=torch.float64, device=dev))
    with _on(dev):
        _check(lib.td_bond_list(*pack, _aromatic_arg(aro), _ptr(bond_ptr), nb, _ptr(out['bond_atoms']), _ptr(out['bond_order']),
                                _ptr(out['bond_category']), _ptr(out['bond_length']), _stream(dev)), 'td_bond_list')
    return out


RING_BITS = 32                                                              # TD_RING_BITS (csrc/td_internal.h)


def ring_report(pos, v, ligand_ptr, class_z, class_aromatic=None, include=None, bond_ptr=None, return_atom_ring=True, check=True):
    """Ring sizes of the bond graph of S frames of B molecules (td_ring_report, include/targetdiff_hip.h); the pack, the class table
    and ``include`` as bond_graph's.  With ``bond_ptr`` [S * B + 1] int64 from bond_graph on the same pack the per-bond outputs are
    written too, aligned with bond_list's order; its last entry is read on the host to size them (one synchronisation).  Returns a
    dict of device tensors: ring_mask [S, B] int64 (the uint32 words, widened), n_ring_bonds and n_ring_atoms [S, B] int32, atom_ring
    [S, N_l] int32 (None without ``return_atom_ring``), ring_hist [S, 32] int64, and bond_ring [nb] int16 / bond_category [nb] uint8
    (the ring-aware category; both None without ``bond_ptr``)."""
    S, Nl, B, cz, aro, _ = _bond_inputs(pos, v, ligand_ptr, class_z, class_aromatic, include, (), check)
    _bond_ptr_input(bond_ptr, S, B)
    lib = load_library()
    pack = _pack_args(pos, v, ligand_ptr, S, Nl, B, cz)
    dev = pos.device
    nb = 0
    if bond_ptr is not None:
        _ptr(bond_ptr, torch.int64, 'bond_ptr')
        nb = int(bond_ptr[-1])
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    mask = i32(S, B)
    out = dict(n_ring_bonds=i32(S, B), n_ring_atoms=i32(S, B), atom_ring=i32(S, Nl) if return_atom_ring else None,
               ring_hist=torch.empty(S, RING_BITS, dtype=torch.int64, device=dev),
               bond_ring=torch.empty(nb, dtype=torch.int16, device=dev) if bond_ptr is not None else None,
               bond_category=torch.empty(nb, dtype=torch.uint8, device=dev) if bond_ptr is not None else None)
    with _on(dev):
        _check(lib.td_ring_report(*pack, _include_arg(include), _aromatic_arg(aro), _ptr(bond_ptr), nb, _ptr(mask), _ptr(out['n_ring_bonds']),
                                  _ptr(out['n_ring_atoms']), _ptr(out['atom_ring']), _ptr(out['ring_hist']), _ptr(out['bond_ring']),
                                  _ptr(out['bond_category']), _stream(dev)), 'td_ring_report')
    out['ring_mask'] = mask.to(torch.int64) & 0xffffffff              # torch has no arithmetic on uint32: the word, widened
    return out


GEOM_MAX_DEGREE, GEOM_MAX_PROFILES, GEOM_BINS = 8, 16, 128                  # TD_GEOM_* (csrc/td_internal.h)
GEOM_KINDS = {'angle': 1, 'torsion': 2}
GEOM_RINGS = {None: 0, 'any': 0, 'chain': 1, 'ring': 2}


def _geometry_profiles(profiles):
    """[(kind, (z, z, z, z), category, ring, cosine edges as float64 numpy)] of a geometry call, checked"""
    if len(profiles) > GEOM_MAX_PROFILES:
        raise ValueError(f'at most {GEOM_MAX_PROFILES} geometry profiles (got {len(profiles)})')
    prof = []
    for kind, z, category, ring, edges in profiles:
        kind = GEOM_KINDS.get(kind, kind)
        ring = GEOM_RINGS.get(ring, ring) if ring is None or isinstance(ring, str) else int(ring)
        if kind not in (1, 2):
            raise ValueError(f"the kind of a geometry profile is 'angle' (1) or 'torsion' (2) (got {kind!r})")
        z = tuple(int(x) for x in z)
        if len(z) != 2 + kind:
            raise ValueError(f'an angle names 3 elements and a torsion 4 (got {len(z)})')
        if any(x != 0 and x not in QUALITY_ELEMENTS for x in z):
            raise ValueError(f'a geometry profile names elements of {QUALITY_ELEMENTS} or 0 for any (got {z})')
        if int(category) not in (0, 1, 2, 3, 4) or ring not in (0, 1, 2):
            raise ValueError(f"category 0 (any) .. 4 and ring 0 / 'any', 1 / 'chain' or 2 / 'ring' (got {category}, {ring!r})")
        if kind == 1 and (int(category) != 0 or ring != 0):
            raise ValueError('an angle profile takes no category and no ring filter')
        prof.append((kind, z + (0,) * (4 - len(z)), int(category), ring, _hist_edges(edges, GEOM_BINS, 'geometry', 'cosine edges')))
    return prof


def geometry_report(pos, v, ligand_ptr, class_z, class_aromatic=None, profiles=(), include=None, clash_threshold=None, bond_ptr=None,
                    bond_ring=None, return_atom_clash=True, check=True):
    """Bond angles, torsions and internal clashes of S frames of B molecules (td_geometry_report, include/targetdiff_hip.h); the pack,
    the class table and ``include`` as bond_graph's.  ``profiles``: a sequence of (kind, elements, category, ring, edges): kind 'angle'
    or 'torsion', 3 or 4 atomic numbers (0: any), the central bond's category (0: any), ring 'any' / 'chain' / 'ring' (0 / 1 / 2) and
    ascending **cosine** edges; the bin is numpy.searchsorted(edges, c, 'left').  A ring filter needs ``bond_ptr`` of bond_graph and
    ``bond_ring`` of ring_report on the same pack.  ``clash_threshold``: [8, 8] float64 over H C N O F P S Cl, None: no clash pass.
    Returns a dict of device tensors: n_angles, n_torsions, n_degenerate, n_crowded [S, B] int32, n_clashes [S, B] int32 and atom_clash
    [S, N_l] int32 (None without a table / without ``return_atom_clash``), hist [S, P, 128] int64."""
    S, Nl, B, cz, aro, _ = _bond_inputs(pos, v, ligand_ptr, class_z, class_aromatic, include, (), check)
    prof = _geometry_profiles(profiles)
    need_ring = any(p[3] != 0 for p in prof)
    if need_ring and (bond_ptr is None or bond_ring is None):
        raise ValueError('a ring filter needs bond_ptr of bond_graph and bond_ring of ring_report on the same pack')
    _bond_ptr_input(bond_ptr, S, B)
    if bond_ring is not None and (bond_ptr is None or bond_ring.dim() != 1 or bond_ring.dtype != torch.int16):
        raise ValueError('bond_ring must be [n_bonds] int16, as ring_report returns it, and comes with bond_ptr')
    thr = None
    if clash_threshold is not None:
        thr = np.ascontiguousarray(np.asarray(clash_threshold, dtype=np.float64).reshape(-1))
        if thr.size != 64 or not np.isfinite(thr).all():
            raise ValueError('clash_threshold is a finite [8, 8] table over H C N O F P S Cl')
    lib = load_library()
    pack = _pack_args(pos, v, ligand_ptr, S, Nl, B, cz)
    dev = pos.device
    parr, P, _keep = _profile_args(TdGeometryProfile, prof, dev)
    nb = int(bond_ring.numel()) if bond_ring is not None else 0
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    out = dict(n_angles=i32(S, B), n_torsions=i32(S, B), n_degenerate=i32(S, B), n_crowded=i32(S, B),
               n_clashes=i32(S, B) if thr is not None else None, atom_clash=i32(S, Nl) if thr is not None and return_atom_clash else None,
               hist=torch.empty(S, P, GEOM_BINS, dtype=torch.int64, device=dev))
    with _on(dev):
        _check(lib.td_geometry_report(*pack, _include_arg(include), _aromatic_arg(aro), parr, P, _ptr(bond_ptr if bond_ring is not None else None), nb,
                                      _ptr(bond_ring), None if thr is None else thr.ctypes.data_as(POINTER(ctypes.c_double)),
                                      _ptr(out['n_angles']), _ptr(out['n_torsions']), _ptr(out['n_degenerate']), _ptr(out['n_crowded']),
                                      _ptr(out['n_clashes']), _ptr(out['atom_clash']), _ptr(out['hist']), _stream(dev)), 'td_geometry_report')
    return out


POCKET_MAX_KINDS, POCKET_ELEMENTS = 64, 6                                   # TD_POCKET_* (csrc/td_internal.h)


def _protein_inputs(pos, protein_pos, protein_elem, protein_kind=None, n_kinds=None, protein_role=None, ref_bits=None, ref_lead=(),
                    who=None, beside=(), what='the pocket', check=True):
    """The protein side of a pocket_report, interaction_report or sasa_report call: shapes, dtypes and devices of ``protein_pos``,
    ``protein_elem`` and, where the report takes them, ``protein_kind`` with ``n_kinds``, ``protein_role`` and the reference words
    ``ref_bits`` [*ref_lead, W] as ``who`` returns them; ``beside``: further tensors that must live on the device of the pack.  With
    ``check`` the elements, kinds and roles are looked at on the host (one synchronisation each).  Returns (N_p, W)."""
    if protein_pos.dim() != 2 or protein_pos.shape[1] != 3:
        raise ValueError(f'protein_pos must be [N_p, 3] (got {tuple(protein_pos.shape)})')
    Np = protein_pos.shape[0]
    W = (Np + 63) // 64
    per_atom = [protein_elem] if protein_kind is None else [protein_elem, protein_kind]
    names = 'protein_elem' if protein_kind is None else 'protein_elem / protein_kind'
    if any(tuple(t.shape) != (Np,) for t in per_atom):
        raise ValueError(f'{names} must be [{Np}] (got {", ".join(str(tuple(t.shape)) for t in per_atom)})')
    if protein_pos.dtype != torch.float32 or any(t.dtype != torch.int32 for t in per_atom):
        raise ValueError(f'protein_pos / {names} must be {" / ".join(["fp32"] + ["int32"] * len(per_atom))} (got '
                         f'{", ".join(str(t.dtype) for t in [protein_pos] + per_atom)})')
    if protein_role is not None and (tuple(protein_role.shape) != (Np,) or protein_role.dtype != torch.int32):
        raise ValueError(f'protein_role must be [{Np}] int32 (got {tuple(protein_role.shape)} {protein_role.dtype})')
    if any(t is not None and t.device != pos.device for t in [protein_pos, protein_role, ref_bits] + per_atom + list(beside)):
        raise ValueError(f'{what} must live on the device of the pack ({pos.device})')
    if protein_kind is not None and not 1 <= int(n_kinds) <= POCKET_MAX_KINDS:
        raise ValueError(f'n_kinds is 1 .. {POCKET_MAX_KINDS} (got {n_kinds})')
    if ref_bits is not None and (tuple(ref_bits.shape) != tuple(ref_lead) + (W,) or ref_bits.dtype != torch.int64):
        raise ValueError(f'ref_bits must be [{", ".join(str(n) for n in tuple(ref_lead) + (W,))}] int64 words, as {who} returns bits (got '
                         f'{tuple(ref_bits.shape)} {ref_bits.dtype})')
    if check and Np > 0:
        if int(protein_elem.min()) < -1 or int(protein_elem.max()) >= POCKET_ELEMENTS:
            raise ValueError(f'protein_elem must be in [-1, {POCKET_ELEMENTS}): an index over H C N O S Se, or -1')
        if protein_kind is not None and (int(protein_kind.min()) < -1 or int(protein_kind.max()) >= int(n_kinds)):
            raise ValueError(f'protein_kind must be in [-1, {int(n_kinds)})')
        if protein_role is not None and (int(protein_role.min()) < -1 or int(protein_role.max()) > (ROLE_DONOR | ROLE_ACCEPTOR)):
            raise ValueError('protein_role must be -1 or a sum of DONOR = 1 and ACCEPTOR = 2: the device decides which carbons are hydrophobic')
    return Np, W


def _allocators(dev):
    """(i32, z32, i64) of ``dev``: outputs by shape, int32 not initialised, int32 zeroed (an oversize molecule's atoms are not
    written) and int64 not initialised"""
    make = lambda fn, dtype: lambda *shape: fn(*shape, dtype=dtype, device=dev)
    return make(torch.empty, torch.int32), make(torch.zeros, torch.int32), make(torch.empty, torch.int64)


def _pocket_inputs(pos, protein_pos, protein_elem, protein_kind, n_kinds, contact_cutoff, clash_threshold, ref_bits, check=True):
    """The pocket's side of a pocket_report call: what _protein_inputs checks of the pocket, the kinds and the reference words, then
    the cutoff and the table.  Returns (N_p, W, the table as float64 numpy [48] or None)."""
    Np, W = _protein_inputs(pos, protein_pos, protein_elem, protein_kind, n_kinds, ref_bits=ref_bits, who='pocket_report', check=check)
    if not (np.isfinite(float(contact_cutoff)) and float(contact_cutoff) > 0.0):
        raise ValueError(f'the contact cutoff must be finite and > 0 (got {contact_cutoff})')
    thr = None
    if clash_threshold is not None:
        thr = np.asarray(clash_threshold, dtype=np.float64)
        if thr.shape not in ((8, POCKET_ELEMENTS), (8 * POCKET_ELEMENTS,)) or not np.isfinite(thr).all():
            raise ValueError(f'clash_threshold is a finite [8, {POCKET_ELEMENTS}] table: H C N O F P S Cl by H C N O S Se')
        thr = np.ascontiguousarray(thr.reshape(-1))
    return Np, W, thr


def pocket_report(pos, v, ligand_ptr, class_z, protein_pos, protein_elem, protein_kind, n_kinds, contact_cutoff, clash_threshold=None,
                  include=None, ref_bits=None, return_atoms=True, return_bits=True, check=True):
    """Contacts and clashes of S frames of B molecules with one pocket (td_pocket_report, include/targetdiff_hip.h); the pack, the
    class table and ``include`` as bond_graph's.  ``protein_pos`` [N_p, 3] fp32 in the frame of ``pos``, ``protein_elem`` [N_p] int32
    over H C N O S Se or -1, ``protein_kind`` [N_p] int32 in [0, n_kinds) or -1 (an atom with a -1 takes part nowhere).  A contact is
    a pair with d < ``contact_cutoff``, a clash one with d < ``clash_threshold`` [8, 6] (ligand element over H C N O F P S Cl by protein
    element; None: no clash pass), d the bond rule's float64 distance.  ``ref_bits`` [W] int64, W = ceil(N_p / 64): bit j & 63 of
    word j >> 6 marks protein atom j.  Returns a dict of device tensors: n_contacts, n_contact_atoms, n_pocket_atoms [S, B] int32,
    n_clashes, n_clash_atoms [S, B] int32 (None without a table), min_dist [S, B] float64, n_ref_common [S, B] int32 (None without
    ``ref_bits``), atom_contacts / atom_clash [S, N_l] int32 (None without ``return_atoms`` / a table), bits [S, B, W] int64 (None
    without ``return_bits``), and over the included molecules kind_hist [S, 8, n_kinds] int64 and pocket_freq [S, N_p] int32."""
    S, Nl, B, cz, _, _ = _bond_inputs(pos, v, ligand_ptr, class_z, None, include, (), check)
    Np, W, thr = _pocket_inputs(pos, protein_pos, protein_elem, protein_kind, n_kinds, contact_cutoff, clash_threshold, ref_bits, check)
    lib = load_library()
    pack = _pack_args(pos, v, ligand_ptr, S, Nl, B, cz)
    dev = pos.device
    i32, z32, _ = _allocators(dev)
    out = dict(n_contacts=i32(S, B), n_contact_atoms=i32(S, B), n_pocket_atoms=i32(S, B),
               n_clashes=i32(S, B) if thr is not None else None, n_clash_atoms=i32(S, B) if thr is not None else None,
               min_dist=torch.empty(S, B, dtype=torch.float64, device=dev),
               n_ref_common=(z32 if W == 0 else i32)(S, B) if ref_bits is not None else None,      # no words: nothing is in common
               atom_contacts=z32(S, Nl) if return_atoms else None, atom_clash=z32(S, Nl) if return_atoms and thr is not None else None,
               bits=torch.empty(S, B, W, dtype=torch.int64, device=dev) if return_bits else None,
               kind_hist=torch.empty(S, 8, int(n_kinds), dtype=torch.int64, device=dev), pocket_freq=i32(S, Np))
    with _on(dev):
        _check(lib.td_pocket_report(*pack, _include_arg(include), _ptr(protein_pos, torch.float32, 'protein_pos'),
                                    _ptr(protein_elem, torch.int32, 'protein_elem'), _ptr(protein_kind, torch.int32, 'protein_kind'), Np,
                                    int(n_kinds), float(contact_cutoff), None if thr is None else thr.ctypes.data_as(POINTER(ctypes.c_double)),
                                    _ptr(ref_bits, torch.int64, 'ref_bits'), _ptr(out['n_contacts']), _ptr(out['n_contact_atoms']),
                                    _ptr(out['n_pocket_atoms']), _ptr(out['n_clashes']), _ptr(out['n_clash_atoms']), _ptr(out['min_dist']),
                                    _ptr(out['n_ref_common']), _ptr(out['atom_contacts']), _ptr(out['atom_clash']), _ptr(out['bits']),
                                    _ptr(out['kind_hist']), _ptr(out['pocket_freq']), _stream(dev)), 'td_pocket_report')
    return out


ROLE_DONOR, ROLE_ACCEPTOR, ROLE_HYDROPHOBIC, INTERACTION_TYPES = 1, 2, 4, 3   # TD_ROLE_*, TD_INTERACTION_TYPES (csrc/td_internal.h)


def _interaction_inputs(pos, protein_pos, protein_elem, protein_kind, protein_role, n_kinds, cutoffs, ref_bits, check=True):
    """The pocket's side of an interaction_report call: what _protein_inputs checks of the pocket, the kinds, the roles and the
    reference words, then the three cutoffs.  Returns (N_p, W)."""
    Np, W = _protein_inputs(pos, protein_pos, protein_elem, protein_kind, n_kinds, protein_role, ref_bits, (INTERACTION_TYPES,),
                            'interaction_report', check=check)
    for name, c in zip(('hbond', 'hydrophobic', 'hetero'), cutoffs):
        if not (np.isfinite(float(c)) and float(c) > 0.0):
            raise ValueError(f'the {name} cutoff must be finite and > 0 (got {c})')
    return Np, W


def interaction_report(pos, v, ligand_ptr, class_z, protein_pos, protein_elem, protein_kind, protein_role, n_kinds, hbond_cutoff=3.5,
                       hydrophobic_cutoff=4.5, hetero_cutoff=1.75, include=None, ref_bits=None, return_atoms=True, return_bits=True,
                       check=True):
    """Hydrogen bonds and hydrophobic contacts of S frames of B molecules with one pocket (td_interaction_report,
    include/targetdiff_hip.h); the pack, the class table, ``include`` and the pocket as pocket_report's.  ``protein_role`` [N_p] int32:
    DONOR = 1, ACCEPTOR = 2, their sum, 0, or -1 (the atom takes part nowhere); the device adds HYDROPHOBIC = 4 to the carbons without
    an N or O closer than ``hetero_cutoff``.  Types: 0 the ligand donates, 1 the ligand accepts (d < ``hbond_cutoff``), 2 hydrophobic
    (d < ``hydrophobic_cutoff``).  ``ref_bits`` [3, W] int64, W = ceil(N_p / 64).  Returns a dict of device tensors: protein_role
    [N_p] int32; n_donated, n_accepted, n_hbonds, n_hydrophobic, n_hb_atoms, n_donors, n_acceptors, n_hydrophobic_atoms [S, B] int32;
    n_ref_common [S, B, 3] int32 (None without ``ref_bits``); atom_role, atom_hbonds, atom_hydrophobic [S, N_l] int32 (None without
    ``return_atoms``); bits [S, B, 3, W] int64 (None without ``return_bits``); and over the included molecules kind_hist
    [S, 3, n_kinds] int64 and pocket_freq [S, 3, N_p] int32."""
    S, Nl, B, cz, _, _ = _bond_inputs(pos, v, ligand_ptr, class_z, None, include, (), check)
    cutoffs = (hbond_cutoff, hydrophobic_cutoff, hetero_cutoff)
    Np, W = _interaction_inputs(pos, protein_pos, protein_elem, protein_kind, protein_role, n_kinds, cutoffs, ref_bits, check)
    lib = load_library()
    pack = _pack_args(pos, v, ligand_ptr, S, Nl, B, cz)
    dev = pos.device
    T = INTERACTION_TYPES
    i32, z32, _ = _allocators(dev)
    mol = ('n_donated', 'n_accepted', 'n_hbonds', 'n_hydrophobic', 'n_hb_atoms', 'n_donors', 'n_acceptors', 'n_hydrophobic_atoms')
    out = dict(protein_role=i32(Np), **{k: i32(S, B) for k in mol},
               n_ref_common=(z32 if W == 0 else i32)(S, B, T) if ref_bits is not None else None,   # no words: nothing is in common
               atom_role=z32(S, Nl) if return_atoms else None, atom_hbonds=z32(S, Nl) if return_atoms else None,
               atom_hydrophobic=z32(S, Nl) if return_atoms else None,
               bits=torch.empty(S, B, T, W, dtype=torch.int64, device=dev) if return_bits else None,
               kind_hist=torch.empty(S, T, int(n_kinds), dtype=torch.int64, device=dev), pocket_freq=i32(S, T, Np))
    with _on(dev):
        _check(lib.td_interaction_report(*pack, _include_arg(include), _ptr(protein_pos, torch.float32, 'protein_pos'),
                                         _ptr(protein_elem, torch.int32, 'protein_elem'), _ptr(protein_kind, torch.int32, 'protein_kind'),
                                         _ptr(protein_role, torch.int32, 'protein_role'), Np, int(n_kinds), *(float(c) for c in cutoffs),
                                         _ptr(ref_bits, torch.int64, 'ref_bits'), _ptr(out['protein_role']), *(_ptr(out[k]) for k in mol),
                                         _ptr(out['n_ref_common']), _ptr(out['atom_role']), _ptr(out['atom_hbonds']),
                                         _ptr(out['atom_hydrophobic']), _ptr(out['bits']), _ptr(out['kind_hist']), _ptr(out['pocket_freq']),
                                         _stream(dev)), 'td_interaction_report')
    return out


SCORE_TERMS, SCORE_FRAC_BITS = 5, 24                                        # TD_SCORE_* (csrc/td_internal.h)
SCORE_TERM_NAMES = ('gauss1', 'gauss2', 'repulsion', 'hydrophobic', 'hbond')
SCORE_MAX_RADIUS_SUM = 6.0


def _score_inputs(pos, protein_pos, protein_elem, protein_kind, protein_role, n_kinds, rsum, cutoff, hetero_cutoff, bond_ptr, bond_ring,
                  S, B, check=True):
    """The pocket's side of a score_report call (_protein_inputs), the two cutoffs, the radius-sum table and the rotor inputs.  Returns
    (N_p, the table as float64 numpy [48], n_bonds)."""
    Np, _ = _protein_inputs(pos, protein_pos, protein_elem, protein_kind, n_kinds, protein_role, who='score_report',
                            beside=(bond_ptr, bond_ring), what='the pocket and the bond arguments', check=check)
    for name, c in (('score', cutoff), ('hetero', hetero_cutoff)):
        if not (np.isfinite(float(c)) and float(c) > 0.0):
            raise ValueError(f'the {name} cutoff must be finite and > 0 (got {c})')
    if 512 * Np > 0x7fffffff:
        raise ValueError(f'512 N_p must fit 31 bits (N_p = {Np})')
    rs = np.asarray(rsum, dtype=np.float64)
    if rs.shape not in ((8, POCKET_ELEMENTS), (8 * POCKET_ELEMENTS,)):
        raise ValueError(f'rsum is an [8, {POCKET_ELEMENTS}] table of radius sums: H C N O F P S Cl by H C N O S Se')
    if not np.isfinite(rs).all() or not ((rs > 0.0) & (rs <= SCORE_MAX_RADIUS_SUM)).all():
        raise ValueError(f'every entry of rsum must be finite and in (0, {SCORE_MAX_RADIUS_SUM:g}]')
    if (bond_ptr is None) != (bond_ring is None):
        raise ValueError('bond_ptr of bond_graph and bond_ring of ring_report come together, or neither')
    _bond_ptr_input(bond_ptr, S, B)
    if bond_ring is not None and (bond_ring.dim() != 1 or bond_ring.dtype != torch.int16):
        raise ValueError('bond_ring must be [n_bonds] int16, as ring_report returns it')
    return Np, np.ascontiguousarray(rs.reshape(-1)), 0 if bond_ring is None else int(bond_ring.numel())


def _score_args(pack, aro, protein_pos, protein_elem, protein_kind, protein_role, Np, n_kinds, cutoff, hetero_cutoff, rs, bond_ptr, nb, bond_ring):
    """The arguments td_score_report, td_score_minimize and td_score_dock begin with (``_SCORE_IN``); ``pack`` of _pack_args, ``rs`` and
    ``nb`` of _score_inputs.  ``rs`` is the caller's: it outlives the call."""
    return (*pack, _aromatic_arg(aro), _ptr(protein_pos, torch.float32, 'protein_pos'), _ptr(protein_elem, torch.int32, 'protein_elem'),
            _ptr(protein_kind, torch.int32, 'protein_kind'), _ptr(protein_role, torch.int32, 'protein_role'), Np, int(n_kinds), float(cutoff),
            float(hetero_cutoff), rs.ctypes.data_as(POINTER(ctypes.c_double)), _ptr(bond_ptr, torch.int64, 'bond_ptr'), nb,
            _ptr(bond_ring, torch.int16, 'bond_ring') if nb else None)


def score_report(pos, v, ligand_ptr, class_z, class_aromatic, protein_pos, protein_elem, protein_kind, protein_role, n_kinds, rsum,
                 cutoff=8.0, hetero_cutoff=1.75, bond_ptr=None, bond_ring=None, check=True):
    """The five unweighted term sums of a Vina-style pair score of S frames of B molecules with one pocket, and their rotatable bonds
    (td_score_report, include/targetdiff_hip.h).  A score on this project's heuristic typing -- no hydrogens, roles from valence
    deficits, no intramolecular term -- and not AutoDock Vina's number: comparable between runs of this tool, not with published
    tables.  The pack, the class table and ``class_aromatic`` as bond_graph's; the pocket, ``protein_role`` and ``hetero_cutoff`` as
    interaction_report's.  ``rsum`` [8, 6] float64: R_l + R_p, ligand element over H C N O F P S Cl by protein element over H C N O S
    Se, every entry in (0, 6]; a pair counts when the bond rule's distance r < ``cutoff`` and its surface distance is r - rsum.
    ``bond_ptr`` [S * B + 1] int64 of bond_graph and ``bond_ring`` [n_bonds] int16 of ring_report on the same pack: with both the
    rotatable bonds are counted (order 1, in no ring, both ends with at least two bonded heavy atoms; amides are not excluded).
    Returns a dict of device tensors: protein_role [N_p] int32, terms [S, B, 5] int64 in units of 2^-24 (``SCORE_TERM_NAMES``),
    n_pairs [S, B] int32 and n_rot [S, B] int32 (None without the bond arguments).  An oversize molecule, refused under ``check``,
    gets -1 / INT64_MIN."""
    S, Nl, B, cz, aro, _ = _bond_inputs(pos, v, ligand_ptr, class_z, class_aromatic, None, (), check)
    Np, rs, nb = _score_inputs(pos, protein_pos, protein_elem, protein_kind, protein_role, n_kinds, rsum, cutoff, hetero_cutoff, bond_ptr,
                               bond_ring, S, B, check)
    lib = load_library()
    shared = _score_args(_pack_args(pos, v, ligand_ptr, S, Nl, B, cz), aro, protein_pos, protein_elem, protein_kind, protein_role, Np, n_kinds,
                         cutoff, hetero_cutoff, rs, bond_ptr, nb, bond_ring)
    dev = pos.device
    i32, _, i64 = _allocators(dev)
    out = dict(protein_role=i32(Np), terms=i64(S, B, SCORE_TERMS), n_pairs=i32(S, B), n_rot=i32(S, B) if bond_ptr is not None else None)
    with _on(dev):
        _check(lib.td_score_report(*shared, _ptr(out['protein_role']), _ptr(out['terms']), _ptr(out['n_pairs']), _ptr(out['n_rot']),
                                   _stream(dev)), 'td_score_report')
    return out


RELAX_MAX_STEPS, RELAX_MAX_SHIFT, RELAX_LIST_CAPACITY = 64, 3.0, 4096       # the conventions; TD_RELAX_LIST_CAPACITY (csrc/td_internal.h)
RELAX_KEYS = ('protein_role', 'n_rot', 'pos', 'terms_in', 'terms', 'n_pairs', 'n_steps', 'n_evals', 'status', 'transform', 'grad_in')
RELAX_CONVERGED, RELAX_OUT_OF_BUDGET, RELAX_AT_CAP = 1, 2, 4                  # the bits of status


def _relax_inputs(weights, max_steps, max_evals, max_shift):
    """The optimiser's side of a score_minimize call.  Returns (the weights as float64 numpy [5], max_steps, max_evals, max_shift);
    ``max_evals`` None: 4 max_steps + 1, the initial evaluation and four per step."""
    w = np.asarray(weights, dtype=np.float64)
    if w.shape != (SCORE_TERMS,) or not np.isfinite(w).all():
        raise ValueError(f'the weights are {SCORE_TERMS} finite numbers: {", ".join(SCORE_TERM_NAMES)}')
    if int(max_steps) != max_steps or int(max_steps) < 0 or int(max_steps) > 0x3fffffff:
        raise ValueError(f'max_steps must be an integer >= 0 (got {max_steps})')
    if max_evals is None:
        max_evals = 4 * int(max_steps) + 1
    if int(max_evals) != max_evals or int(max_evals) < 1 or int(max_evals) > 0x7fffffff:
        raise ValueError(f'max_evals must be an integer >= 1 (got {max_evals})')
    if not (np.isfinite(float(max_shift)) and float(max_shift) > 0.0):
        raise ValueError(f'max_shift must be finite and > 0 (got {max_shift})')
    return np.ascontiguousarray(w), int(max_steps), int(max_evals), float(max_shift)


def _relax_outputs(pos, S, B, Np, rotors):
    """the outputs ``RELAX_KEYS`` name, not initialised, on the device of ``pos``; n_rot only with the rotor inputs"""
    dev = pos.device
    i32, _, i64 = _allocators(dev)
    return dict(protein_role=i32(Np), n_rot=i32(S, B) if rotors else None, pos=torch.empty_like(pos), terms_in=i64(S, B, SCORE_TERMS),
                terms=i64(S, B, SCORE_TERMS), n_pairs=i32(S, B), n_steps=i32(S, B), n_evals=i32(S, B), status=i32(S, B),
                transform=torch.empty(S, B, 7, dtype=torch.float64, device=dev), grad_in=i64(S, B, 6))


def _call_with_capacity(lib, name, args, list_capacity):
    """call the entry point ``name``, or with a ``list_capacity`` its td_internal_*_capacity twin: the tests' door to the walk in global memory"""
    if list_capacity is None:
        return _check(getattr(lib, name)(*args), name)
    fn = getattr(lib, f'td_internal_{name[len("td_"):]}_capacity')
    fn.restype, fn.argtypes = c_int32, SIGNATURES[name][1] + [c_int32]
    _check(fn(*args, int(list_capacity)), name)


def score_minimize(pos, v, ligand_ptr, class_z, class_aromatic, protein_pos, protein_elem, protein_kind, protein_role, n_kinds, rsum, weights,
                   cutoff=8.0, hetero_cutoff=1.75, bond_ptr=None, bond_ring=None, max_steps=RELAX_MAX_STEPS, max_evals=None,
                   max_shift=RELAX_MAX_SHIFT, check=True, _list_capacity=None):
    """The rigid-body relaxation of S frames of B molecules in one pocket under ``inter = weights . terms`` of score_report
    (td_score_minimize, include/targetdiff_hip.h): one persistent workgroup per molecule runs BFGS with a backtracking line search on
    three translations and three rotations.  It is a local optimisation under this project's heuristic score, not AutoDock Vina's
    ``minimize``, and it is rigid-body only: three translations and three rotations, no torsions.  The arguments up to ``bond_ring``
    as score_report's (validated alike); ``weights`` five finite numbers; ``max_steps`` accepted steps, ``max_evals`` evaluations (None:
    4 max_steps + 1), ``max_shift`` the cap on the shift of the centre in Angstrom.
    Returns a dict of device tensors: protein_role [N_p] int32 and n_rot [S, B] int32 (of the input pose; None without the bond
    arguments) as score_report's, pos [S, N_l, 3] fp32 the relaxed poses, terms_in / terms [S, B, 5] int64 in units of 2^-24 at the
    input and at the relaxed pose, n_pairs [S, B] int32 at the relaxed pose, n_steps, n_evals, status [S, B] int32 (bits
    ``RELAX_CONVERGED``, ``RELAX_OUT_OF_BUDGET``, ``RELAX_AT_CAP``), transform [S, B, 7] float64 (the unit quaternion, then the shift of
    the centre) and grad_in [S, B, 6] int64, the gradient at the input pose in units of 2^-24.  An oversize molecule, refused under
    ``check``, keeps its positions and gets -1 / INT64_MIN."""
    S, Nl, B, cz, aro, _ = _bond_inputs(pos, v, ligand_ptr, class_z, class_aromatic, None, (), check)
    Np, rs, nb = _score_inputs(pos, protein_pos, protein_elem, protein_kind, protein_role, n_kinds, rsum, cutoff, hetero_cutoff, bond_ptr,
                               bond_ring, S, B, check)
    w, max_steps, max_evals, max_shift = _relax_inputs(weights, max_steps, max_evals, max_shift)
    lib = load_library()
    shared = _score_args(_pack_args(pos, v, ligand_ptr, S, Nl, B, cz), aro, protein_pos, protein_elem, protein_kind, protein_role, Np, n_kinds,
                         cutoff, hetero_cutoff, rs, bond_ptr, nb, bond_ring)
    dev = pos.device
    out = _relax_outputs(pos, S, B, Np, bond_ptr is not None)
    args = (*shared, w.ctypes.data_as(POINTER(ctypes.c_double)), max_steps, max_evals, max_shift, *(_ptr(out[k]) for k in RELAX_KEYS),
            _stream(dev))
    with _on(dev):
        _call_with_capacity(lib, 'td_score_minimize', args, _list_capacity)
    return out


DOCK_CHAINS, DOCK_ROUNDS, DOCK_AMPLITUDE, DOCK_TEMPERATURE = 16, 16, 2.0, 1.2   # the conventions
DOCK_MAX_CHAINS, DOCK_MAX_ROUNDS, DOCK_DRAWS = 64, 256, 7                       # TD_DOCK_* (csrc/td_internal.h)
DOCK_KEYS = RELAX_KEYS + ('best_chain', 'chain_terms', 'chain_transform', 'chain_accepts', 'chain_evals')


def _dock_inputs(n_chains, n_rounds, amplitude, temperature, seed, draws, S, B, device, check=True):
    """The search's side of a score_dock call.  Returns (n_chains, n_rounds, amplitude, temperature, the draws as a contiguous float64
    tensor [S, B, n_chains, n_rounds + 1, 7] on ``device``); ``draws`` None: torch.rand from a generator on the device seeded by ``seed``."""
    if int(n_chains) != n_chains or not 1 <= int(n_chains) <= DOCK_MAX_CHAINS:
        raise ValueError(f'n_chains must be an integer in 1 .. {DOCK_MAX_CHAINS} (got {n_chains})')
    if int(n_rounds) != n_rounds or not 0 <= int(n_rounds) <= DOCK_MAX_ROUNDS:
        raise ValueError(f'n_rounds must be an integer in 0 .. {DOCK_MAX_ROUNDS} (got {n_rounds})')
    if not (np.isfinite(float(amplitude)) and float(amplitude) > 0.0):
        raise ValueError(f'amplitude must be finite and > 0 (got {amplitude})')
    if not (np.isfinite(float(temperature)) and float(temperature) > 0.0):
        raise ValueError(f'temperature must be finite and > 0 (got {temperature})')
    shape = (S, B, int(n_chains), int(n_rounds) + 1, DOCK_DRAWS)
    if draws is None:
        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed))
        draws = torch.rand(shape, dtype=torch.float64, device=device, generator=gen)
    else:
        if not torch.is_tensor(draws) or draws.dtype != torch.float64 or tuple(draws.shape) != shape or draws.device != device:
            raise ValueError(f'draws is a float64 tensor {list(shape)} on the device of pos')
        draws = draws.contiguous()
        if check and draws.numel() and not bool(((draws >= 0.0) & (draws < 1.0)).all()):
            raise ValueError('draws must lie in [0, 1)')
    return int(n_chains), int(n_rounds), float(amplitude), float(temperature), draws


def score_dock(pos, v, ligand_ptr, class_z, class_aromatic, protein_pos, protein_elem, protein_kind, protein_role, n_kinds, rsum, weights,
               cutoff=8.0, hetero_cutoff=1.75, bond_ptr=None, bond_ring=None, max_steps=RELAX_MAX_STEPS, max_evals=None,
               max_shift=RELAX_MAX_SHIFT, n_chains=DOCK_CHAINS, n_rounds=DOCK_ROUNDS, amplitude=DOCK_AMPLITUDE, temperature=DOCK_TEMPERATURE,
               seed=0, draws=None, check=True, _list_capacity=None):
    """The docking search of S frames of B molecules in one pocket under ``inter = weights . terms`` of score_report (td_score_dock,
    include/targetdiff_hip.h): per molecule ``n_chains`` independent Monte-Carlo chains, one persistent workgroup each, run
    ``n_rounds`` + 1 rounds of a random rigid move (shift up to ``amplitude`` Angstrom per axis, a turn to match) followed by
    score_minimize's local optimisation, with a Metropolis rule at ``temperature`` on inter; a second small launch takes the best chain.
    Chain 0 starts with the plain relaxation of the input pose.  It is a rigid-body global search under this project's heuristic score,
    not AutoDock Vina's ``dock``: three translations and three rotations, no torsions.  No intramolecular term, no hydrogens; the search
    box is the ball of ``max_shift`` around the input centroid.  The arguments up to ``max_shift`` as score_minimize's (validated alike;
    ``max_steps`` and ``max_evals`` are one round's budget).  The uniforms are the caller's: ``draws`` float64
    [S, B, n_chains, n_rounds + 1, 7] in [0, 1) on the device, or None for torch.rand from a generator seeded by ``seed``.
    Returns score_minimize's dict for the winning pose (n_steps and n_evals summed over the chains), plus best_chain [S, B] int32,
    chain_terms [S, B, C, 5] int64 and chain_transform [S, B, C, 7] float64 (each chain's best), chain_accepts and chain_evals
    [S, B, C] int32, and ``draws``."""
    S, Nl, B, cz, aro, _ = _bond_inputs(pos, v, ligand_ptr, class_z, class_aromatic, None, (), check)
    Np, rs, nb = _score_inputs(pos, protein_pos, protein_elem, protein_kind, protein_role, n_kinds, rsum, cutoff, hetero_cutoff, bond_ptr,
                               bond_ring, S, B, check)
    w, max_steps, max_evals, max_shift = _relax_inputs(weights, max_steps, max_evals, max_shift)
    dev = pos.device
    C, n_rounds, amplitude, temperature, draws = _dock_inputs(n_chains, n_rounds, amplitude, temperature, seed, draws, S, B, dev, check)
    lib = load_library()
    shared = _score_args(_pack_args(pos, v, ligand_ptr, S, Nl, B, cz), aro, protein_pos, protein_elem, protein_kind, protein_role, Np, n_kinds,
                         cutoff, hetero_cutoff, rs, bond_ptr, nb, bond_ring)
    i32, _, i64 = _allocators(dev)
    out = dict(_relax_outputs(pos, S, B, Np, bond_ptr is not None), best_chain=i32(S, B), chain_terms=i64(S, B, C, SCORE_TERMS),
               chain_transform=torch.empty(S, B, C, 7, dtype=torch.float64, device=dev), chain_accepts=i32(S, B, C), chain_evals=i32(S, B, C))
    args = (*shared, w.ctypes.data_as(POINTER(ctypes.c_double)), max_steps, max_evals, max_shift, C, n_rounds, amplitude, temperature,
            _ptr(draws, torch.float64, 'draws'), *(_ptr(out[k]) for k in DOCK_KEYS), _stream(dev))
    with _on(dev):
        _call_with_capacity(lib, 'td_score_dock', args, _list_capacity)
    out['draws'] = draws
    return out


SASA_MAX_POINTS, SASA_CHUNK = 256, 512                                     # TD_SASA_* (csrc/td_internal.h)
SASA_CULL_REL, SASA_CULL_ABS = 1e-4, 1e-4                                   # TD_SASA_CULL_*: an occluder farther than (R_a + R_b) (1 + REL) + ABS is not looked at
SASA_COORD_MAX = 1.0e5                                                      # |coordinate| the binding admits: csrc/sasa.hip's cull is proved up to it
SASA_UNIT_TOL = 1.0e-6                                                      # | |u|^2 - 1 | the binding admits of a direction


def _sasa_inputs(pos, v, ligand_ptr, class_z, protein_pos, protein_elem, ligand_reach, protein_reach, dirs, include, check=True):
    """Everything a sasa_report call is given: the pack as _bond_inputs checks it, the pocket's shapes, dtypes and devices, the two
    reach tables and the directions; with ``check`` the elements, the directions and the coordinates are looked at on the host (one
    synchronisation each).  Returns (S, N_l, B, class table, N_p, W, P, ligand reaches [8], protein reaches [6] as float64 numpy)."""
    S, Nl, B, cz, _, _ = _bond_inputs(pos, v, ligand_ptr, class_z, None, include, (), check)
    Np, W = _protein_inputs(pos, protein_pos, protein_elem, beside=(dirs,), what='the pocket and the directions', check=check)
    if dirs.dim() != 2 or dirs.shape[1] != 3 or not 1 <= dirs.shape[0] <= SASA_MAX_POINTS:
        raise ValueError(f'dirs must be [P, 3] with 1 <= P <= {SASA_MAX_POINTS} (got {tuple(dirs.shape)})')
    if dirs.dtype != torch.float64:
        raise ValueError(f'dirs must be float64 (got {dirs.dtype})')
    if 512 * Np > 0x7fffffff or S * Np > 0x7fffffff or S * B * 8 > 0x7fffffff:
        raise ValueError(f'512 N_p, S N_p and 8 S B must fit 31 bits (S = {S}, B = {B}, N_p = {Np})')
    reach = []
    for name, r, size in (('ligand_reach', ligand_reach, 8), ('protein_reach', protein_reach, POCKET_ELEMENTS)):
        r = np.asarray(r, dtype=np.float64)
        if r.shape != (size,) or not np.isfinite(r).all() or not (r > 0.0).all():
            raise ValueError(f'{name} is [{size}], finite and > 0: van der Waals radius + probe per element')
        reach.append(np.ascontiguousarray(r))
    if check:
        if not bool(torch.isfinite(dirs).all()) or not float(((dirs * dirs).sum(1) - 1.0).abs().max()) <= SASA_UNIT_TOL:
            raise ValueError(f'dirs must be finite unit vectors (| |u|^2 - 1 | <= {SASA_UNIT_TOL})')
        for name, t in (('pos', pos), ('protein_pos', protein_pos)):
            if t.numel() and not float(t.abs().max()) <= SASA_COORD_MAX:
                raise ValueError(f'{name} must be finite with |coordinate| <= {SASA_COORD_MAX:g}')
    return S, Nl, B, cz, Np, W, dirs.shape[0], reach[0], reach[1]


def sasa_report(pos, v, ligand_ptr, class_z, protein_pos, protein_elem, ligand_reach, protein_reach, dirs, include=None,
                return_atoms=True, return_bits=True, check=True):
    """Solvent-accessible surface of S frames of B molecules, alone and in one pocket, as counts of sphere points (td_sasa_report,
    include/targetdiff_hip.h); the pack, the class table and ``include`` as bond_graph's.  ``protein_pos`` [N_p, 3] fp32 in the frame
    of ``pos``, ``protein_elem`` [N_p] int32 over H C N O S Se or -1 (the atom takes part nowhere).  ``ligand_reach`` [8] over H C N O
    F P S Cl and ``protein_reach`` [6]: van der Waals radius + probe, float64.  ``dirs`` [P, 3] float64 on the device, unit vectors, 1
    <= P <= 256.  Coordinates beyond ``SASA_COORD_MAX`` are refused.  Returns a dict of device tensors: free, bound [S, B, 8] int32 (the
    exposed points by ligand element, alone and in the pocket), pocket_buried [S, B, 6] int32 (the apo-exposed pocket points the
    molecule covers, by protein element), atom_free / atom_bound [S, N_l] int32 (None without ``return_atoms``), bits [S, B, W] int64
    (the protein atoms with a buried point; None without ``return_bits``), pocket_free [N_p] int32 and pocket_mask [N_p, 4] int64 (the
    pocket alone), and over the included molecules pocket_buried_sum [S, N_p] int64."""
    S, Nl, B, cz, Np, W, P, lr, pr = _sasa_inputs(pos, v, ligand_ptr, class_z, protein_pos, protein_elem, ligand_reach, protein_reach, dirs,
                                                  include, check)
    lib = load_library()
    pack = _pack_args(pos, v, ligand_ptr, S, Nl, B, cz)
    dev = pos.device
    i32, z32, i64 = _allocators(dev)
    out = dict(free=i32(S, B, 8), bound=i32(S, B, 8), pocket_buried=i32(S, B, POCKET_ELEMENTS),
               atom_free=z32(S, Nl) if return_atoms else None, atom_bound=z32(S, Nl) if return_atoms else None,
               bits=i64(S, B, W) if return_bits else None, pocket_free=i32(Np), pocket_mask=i64(Np, 4), pocket_buried_sum=i64(S, Np))
    f64p = lambda a: a.ctypes.data_as(POINTER(ctypes.c_double))
    with _on(dev):
        _check(lib.td_sasa_report(*pack, _include_arg(include), _ptr(protein_pos, torch.float32, 'protein_pos'),
                                  _ptr(protein_elem, torch.int32, 'protein_elem'), Np, f64p(lr), f64p(pr), _ptr(dirs, torch.float64, 'dirs'),
                                  P, _ptr(out['free']), _ptr(out['bound']), _ptr(out['pocket_buried']), _ptr(out['atom_free']),
                                  _ptr(out['atom_bound']), _ptr(out['bits']), _ptr(out['pocket_free']), _ptr(out['pocket_mask']),
                                  _ptr(out['pocket_buried_sum']), _stream(dev)), 'td_sasa_report')
    return out


FP_BITS, FP_WORDS, FP_MAX_RADIUS, FP_MAX_ROUNDS = 2048, 32, 4, 16           # TD_FP_* (csrc/td_internal.h)


def _fingerprint_inputs(pos, v, ligand_ptr, class_z, class_aromatic, radius, key_rounds, check=True):
    """_bond_inputs plus the two round counts of a fingerprint call.  Returns (S, N_l, B, class table, aromatic flags, radius,
    key_rounds)."""
    radius, key_rounds = int(radius), int(key_rounds)
    if not 0 <= radius <= FP_MAX_RADIUS or not radius <= key_rounds <= FP_MAX_ROUNDS:
        raise ValueError(f'0 <= radius <= {FP_MAX_RADIUS} and radius <= key_rounds <= {FP_MAX_ROUNDS} (got {radius}, {key_rounds})')
    S, Nl, B, cz, aro, _ = _bond_inputs(pos, v, ligand_ptr, class_z, class_aromatic, None, (), check)
    return S, Nl, B, cz, aro, radius, key_rounds


def fingerprint(pos, v, ligand_ptr, class_z, class_aromatic=None, radius=2, key_rounds=8, return_atom_keys=False, check=True):
    """Fingerprints of the bond graph of S frames of B molecules (td_fingerprint, include/targetdiff_hip.h); the pack and the class
    table as bond_graph's.  This is not RDKit's RDKFingerprint: it is a circular, Morgan-style fingerprint over this project's bond
    graph, whose orders come from the bond-length table; its similarities are comparable between runs of this tool, not with published
    tables.  Returns a dict of device tensors: fp_words [S, B, 32] int64 (word w, bit k: fingerprint bit 64 w + k, after ``radius``
    rounds), n_bits [S, B] int32, key [S, B] int64 (after ``key_rounds`` rounds) and atom_key [S, N_l] int64 (None without
    ``return_atom_keys``; 0 for an atom of no class)."""
    S, Nl, B, cz, aro, radius, key_rounds = _fingerprint_inputs(pos, v, ligand_ptr, class_z, class_aromatic, radius, key_rounds, check)
    lib = load_library()
    pack = _pack_args(pos, v, ligand_ptr, S, Nl, B, cz)
    dev = pos.device
    out = dict(fp_words=torch.empty(S, B, FP_WORDS, dtype=torch.int64, device=dev), n_bits=torch.empty(S, B, dtype=torch.int32, device=dev),
               key=torch.empty(S, B, dtype=torch.int64, device=dev),
               atom_key=torch.zeros(S, Nl, dtype=torch.int64, device=dev) if return_atom_keys else None)
    with _on(dev):
        _check(lib.td_fingerprint(*pack, _aromatic_arg(aro), radius, key_rounds, _ptr(out['fp_words']), _ptr(out['n_bits']), _ptr(out['key']),
                                  _ptr(out['atom_key']), _stream(dev)), 'td_fingerprint')
    return out


def fingerprint_similarity(fp_words, n_bits, key, include=None, q_words=None, q_bits=None, return_common=False):
    """The molecules of every frame compared (td_fingerprint_similarity): ``fp_words`` [S, B, 32] int64, ``n_bits`` [S, B] int32 and
    ``key`` [S, B] int64 as fingerprint returns them, ``include`` [S, B] bool / uint8 or None; a query set ``q_words`` [Q, 32] int64 with
    its ``q_bits`` [Q] int32 (one frame of another fingerprint call).  Returns a dict of device tensors: sim_sum and sim_max [S, B]
    float64 (Tanimoto similarity to the other included molecules: summed in ascending order, and the largest), first_equal [S, B] int32
    (the first included molecule with the same key, -1 when not included), common [S, B, B] int32 (None without ``return_common``),
    and with a query set query_common [S, B, Q] int32 and query_sim [S, B, Q] float64 = c / (n_bits + q_bits - c), 0 for an empty
    union (one float64 division per entry, formed by torch from the kernel's integers); both None without one."""
    if fp_words.dim() != 3 or fp_words.shape[2] != FP_WORDS or fp_words.dtype != torch.int64:
        raise ValueError(f'fp_words must be [S, B, {FP_WORDS}] int64 (got {tuple(fp_words.shape)} {fp_words.dtype})')
    S, B = fp_words.shape[:2]
    if tuple(n_bits.shape) != (S, B) or n_bits.dtype != torch.int32 or tuple(key.shape) != (S, B) or key.dtype != torch.int64:
        raise ValueError(f'n_bits / key must be [{S}, {B}] int32 / int64')
    if include is not None and (tuple(include.shape) != (S, B) or include.dtype not in (torch.bool, torch.uint8)):
        raise ValueError(f'include must be [{S}, {B}] bool or uint8')
    Q = 0
    if (q_words is None) != (q_bits is None):
        raise ValueError('a query set is q_words and q_bits together')
    if q_words is not None:
        if q_words.dim() != 2 or q_words.shape[1] != FP_WORDS or q_words.dtype != torch.int64:
            raise ValueError(f'q_words must be [Q, {FP_WORDS}] int64 (got {tuple(q_words.shape)} {q_words.dtype})')
        Q = q_words.shape[0]
        if tuple(q_bits.shape) != (Q,) or q_bits.dtype != torch.int32:
            raise ValueError(f'q_bits must be [{Q}] int32')
    lib = load_library()
    _ptr(fp_words, torch.int64, 'fp_words')           # a CPU tensor is refused before anything is allocated
    dev = fp_words.device
    out = dict(sim_sum=torch.empty(S, B, dtype=torch.float64, device=dev), sim_max=torch.empty(S, B, dtype=torch.float64, device=dev),
               first_equal=torch.empty(S, B, dtype=torch.int32, device=dev),
               common=torch.empty(S, B, B, dtype=torch.int32, device=dev) if return_common else None,
               query_common=torch.empty(S, B, Q, dtype=torch.int32, device=dev) if Q else None, query_sim=None)
    with _on(dev):
        _check(lib.td_fingerprint_similarity(_ptr(fp_words), _ptr(n_bits, torch.int32, 'n_bits'), _ptr(key, torch.int64, 'key'), S, B,
                                             _include_arg(include), _ptr(q_words, torch.int64, 'q_words') if Q else None, Q,
                                             _ptr(out['sim_sum']), _ptr(out['sim_max']), _ptr(out['first_equal']), _ptr(out['common']),
                                             _ptr(out['query_common']), _stream(dev)), 'td_fingerprint_similarity')
    if Q:
        c = out['query_common'].to(torch.int64)
        union = n_bits.to(torch.int64)[:, :, None] + q_bits.to(device=dev, dtype=torch.int64)[None, None, :] - c
        out['query_sim'] = torch.where(union > 0, c.to(torch.float64) / union.clamp(min=1).to(torch.float64), torch.zeros((), dtype=torch.float64, device=dev))
    return out


def protein_centroids(protein_pos: torch.Tensor, protein_ptr: torch.Tensor) -> torch.Tensor:
    """Per-graph centroid [B, 3] of the protein atoms (td_center_pos's offset: one block reduction per graph, so the
    result is run-to-run reproducible, unlike an atomics-based scatter_mean)."""
    lib = load_library()
    B = protein_ptr.numel() - 1
    scratch = protein_pos.detach().clone().contiguous().float()
    offset = torch.empty(B, 3, dtype=torch.float32, device=protein_pos.device)
    with _on(protein_pos.device):
        _check(lib.td_center_pos(_ptr(scratch), _ptr(protein_ptr, torch.int32, 'protein_ptr'), None,
                                 _ptr(protein_ptr, torch.int32, 'protein_ptr'), B, _ptr(offset), 1, -1,
                                 _stream(protein_pos.device)), 'td_center_pos')
    return offset


class NativeEgnn:
    """Owns a td_egnn handle: the EGNN refine net of models/egnn.py with packed weights on the current HIP device."""

    def __init__(self, num_layers: int, state_dict, hidden_dim=HIDDEN, edge_feat_dim=4, k=KNN, device=None, prefix=''):
        self.lib = load_library()
        self.device = _canonical_device(device)
        self.num_layers = int(num_layers)
        blob = np.ascontiguousarray(np.concatenate(
            [state_dict[prefix + key].detach().cpu().numpy().astype(np.float32).reshape(-1)
             for key in egnn_flat_key_order(self.num_layers)]))
        handle = c_void_p()
        with torch.cuda.device(self.device):
            _check(self.lib.td_egnn_create(self.num_layers, hidden_dim, edge_feat_dim, k, blob.ctypes.data_as(POINTER(c_float)),
                                           blob.size, ctypes.byref(handle)), 'td_egnn_create')
        self.handle = handle
        self._ws = None

    def __del__(self):
        h, self.handle = getattr(self, 'handle', None), None
        if h and getattr(self, 'lib', None) is not None:
            self.lib.td_egnn_destroy(h)

    @_device_bound
    def forward(self, h, x, mask_ligand, node_ptr, return_all=False, max_graph_nodes=0):
        N, B, L = h.shape[0], node_ptr.numel() - 1, self.num_layers
        out_h, out_x = torch.empty_like(h), torch.empty_like(x)
        all_h = torch.empty(L, N, HIDDEN, dtype=torch.float32, device=h.device) if return_all else None
        all_x = torch.empty(L, N, 3, dtype=torch.float32, device=h.device) if return_all else None
        need = int(self.lib.td_egnn_workspace_bytes(N))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=h.device)
        mask_u8 = mask_ligand.to(torch.uint8).contiguous()
        _check(self.lib.td_egnn_forward(
            self.handle, _ptr(h, torch.float32, 'h'), _ptr(x, torch.float32, 'x'), _ptr(mask_u8),
            _ptr(node_ptr, torch.int32, 'node_ptr'), N, B, max_graph_nodes, _ptr(out_h), _ptr(out_x), _ptr(all_h), _ptr(all_x),
            _ptr(self._ws), self._ws.numel(), _stream(self.device)), 'td_egnn_forward')
        return out_h, out_x, all_h, all_x


# ----------------------------------------------------------------------------------------- binding-affinity predictor
PROP_HIDDEN = 256
PROP_LAYER_KEYS = ('edge_mlp.net.0.weight', 'edge_mlp.net.0.bias', 'edge_mlp.net.2.weight', 'edge_mlp.net.2.bias',
                   'edge_inf.0.weight', 'edge_inf.0.bias', 'node_mlp.net.0.weight', 'node_mlp.net.0.bias',
                   'node_mlp.net.2.weight', 'node_mlp.net.2.bias')


def prop_flat_key_order(num_layers: int, enc_node_dim: int = 0):
    """The order td_prop_create reads the state_dict of PropPredNet / PropPredNetEnc in (include/targetdiff_hip.h)."""
    keys = ['protein_atom_emb.weight', 'protein_atom_emb.bias', 'ligand_atom_emb.weight', 'ligand_atom_emb.bias',
            'encoder.distance_expansion.offset']
    keys += [f'encoder.net.{l}.{k}' for l in range(num_layers) for k in PROP_LAYER_KEYS]
    if enc_node_dim > 0:
        keys += ['enc_node_layer.0.weight', 'enc_node_layer.0.bias', 'enc_node_layer.2.weight', 'enc_node_layer.2.bias']
    keys += ['out_block.0.weight', 'out_block.0.bias', 'out_block.2.weight', 'out_block.2.bias']
    return keys


class NativeProp:
    """Owns a td_prop handle: PropPredNet / PropPredNetEnc (models/property_pred/prop_model.py) with packed weights on a HIP device."""

    def __init__(self, cfg: dict, state_dict, device=None):
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise RuntimeError('no HIP device visible: targetdiff_amd needs an MI355X (gfx950); there is no CPU path')
        self.device = _canonical_device(device)
        self.cfg = TdPropConfig(**{k: cfg[k] for k, _ in TdPropConfig._fields_})
        blob = np.ascontiguousarray(np.concatenate(
            [state_dict[k].detach().cpu().numpy().astype(np.float32).reshape(-1)
             for k in prop_flat_key_order(self.cfg.num_layers, self.cfg.enc_node_dim)]))
        expect = int(self.lib.td_prop_num_weights(ctypes.byref(self.cfg)))
        if blob.size != expect:
            raise ValueError(f'weight blob has {blob.size} floats, library expects {expect}')
        handle = c_void_p()
        with torch.cuda.device(self.device):
            _check(self.lib.td_prop_create(ctypes.byref(self.cfg), blob.ctypes.data_as(POINTER(c_float)), blob.size,
                                           ctypes.byref(handle)), 'td_prop_create')
        self.handle = handle
        self._ws = None

    def __del__(self):
        h, self.handle = getattr(self, 'handle', None), None
        if h and getattr(self, 'lib', None) is not None:
            self.lib.td_prop_destroy(h)

    @_device_bound
    def forward(self, protein_pos, protein_feat, protein_ptr, ligand_pos, ligand_feat, ligand_ptr, output_kind=None,
                enc_ligand=None, enc_node=None, enc_graph=None, want_layers=False, want_final_h=False, want_graph=False,
                max_graph_nodes=0):
        """Inputs sorted by complex (``*_ptr``: [B+1] int32 offsets).  Returns (out [B, 1 or O], h_layers [L, N, 256] | None,
        final_h [N, 256] | None, nbr [N, knn] | None); node rows in the composed order (per complex protein, then ligand)."""
        Np, Nl, B = protein_pos.shape[0], ligand_pos.shape[0], protein_ptr.numel() - 1
        N, dev, c = Np + Nl, protein_pos.device, self.cfg
        out = torch.empty(B, 1 if output_kind is not None else c.output_dim, dtype=torch.float32, device=dev)
        h_layers = torch.empty(c.num_layers, N, PROP_HIDDEN, dtype=torch.float32, device=dev) if want_layers else None
        final_h = torch.empty(N, PROP_HIDDEN, dtype=torch.float32, device=dev) if want_final_h else None
        nbr = torch.empty(N, c.knn, dtype=torch.int32, device=dev) if want_graph else None
        need = int(self.lib.td_prop_workspace_bytes(self.handle, Np, Nl, B))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)

        def opt(t, dtype, what, rows, cols):
            if t is None:
                return None
            if tuple(t.shape) != (rows, cols):
                raise ValueError(f'{what}: expected shape {(rows, cols)}, got {tuple(t.shape)}')
            return _ptr(t, dtype, what)
        kind = None
        if output_kind is not None:
            if tuple(output_kind.shape) != (B,):
                raise ValueError(f'output_kind: expected shape {(B,)}, got {tuple(output_kind.shape)}')
            kind = _ptr(output_kind, torch.int64, 'output_kind')
        _check(self.lib.td_prop_forward(
            self.handle, _ptr(protein_pos, torch.float32, 'protein_pos'), _ptr(protein_feat, torch.float32, 'protein_feat'),
            _ptr(protein_ptr, torch.int32, 'protein_ptr'), Np, _ptr(ligand_pos, torch.float32, 'ligand_pos'),
            _ptr(ligand_feat, torch.float32, 'ligand_feat'), _ptr(ligand_ptr, torch.int32, 'ligand_ptr'), Nl, B,
            opt(enc_ligand, torch.float32, 'enc_ligand_feature', Nl, c.enc_ligand_dim),
            opt(enc_node, torch.float32, 'enc_node_feature', N, c.enc_node_dim),
            opt(enc_graph, torch.float32, 'enc_graph_feature', B, c.enc_graph_dim), kind, max_graph_nodes, _ptr(out),
            _ptr(h_layers), _ptr(final_h), _ptr(nbr), _ptr(self._ws), self._ws.numel(), _stream(self.device)), 'td_prop_forward')
        return out, h_layers, final_h, nbr

    def num_weights(self) -> int:
        return int(self.lib.td_prop_num_weights(ctypes.byref(self.cfg)))

    @_device_bound
    def set_weights(self, flat: torch.Tensor):
        """Re-pack the weights from ``flat`` (device, fp32, prop_flat_key_order) on the device (td_prop_set_weights)."""
        _check(self.lib.td_prop_set_weights(self.handle, _ptr(flat, torch.float32, 'weights'), flat.numel(), _stream(self.device)),
               'td_prop_set_weights')

    @_device_bound
    def forward_train(self, protein_pos, protein_feat, protein_ptr, ligand_pos, ligand_feat, ligand_ptr, output_kind=None,
                      enc_ligand=None, enc_node=None, enc_graph=None, max_graph_nodes=0):
        """td_prop_forward_train: as ``forward`` (no optional outputs); returns (out, tape).  The tape owns its workspace tensor, so
        any number of tapes can wait for their backward."""
        Np, Nl, B = protein_pos.shape[0], ligand_pos.shape[0], protein_ptr.numel() - 1
        N, dev, c = Np + Nl, protein_pos.device, self.cfg
        out = torch.empty(B, 1 if output_kind is not None else c.output_dim, dtype=torch.float32, device=dev)
        ws = torch.empty(int(self.lib.td_prop_train_workspace_bytes(self.handle, Np, Nl, B)), dtype=torch.uint8, device=dev)

        def opt(t, what, rows, cols):
            if t is None:
                return None
            if tuple(t.shape) != (rows, cols):
                raise ValueError(f'{what}: expected shape {(rows, cols)}, got {tuple(t.shape)}')
            return _ptr(t, torch.float32, what)
        kind = None
        if output_kind is not None:
            if tuple(output_kind.shape) != (B,):
                raise ValueError(f'output_kind: expected shape {(B,)}, got {tuple(output_kind.shape)}')
            kind = _ptr(output_kind, torch.int64, 'output_kind')
        tape = TdPropTape()
        _check(self.lib.td_prop_forward_train(
            self.handle, _ptr(protein_pos, torch.float32, 'protein_pos'), _ptr(protein_feat, torch.float32, 'protein_feat'),
            _ptr(protein_ptr, torch.int32, 'protein_ptr'), Np, _ptr(ligand_pos, torch.float32, 'ligand_pos'),
            _ptr(ligand_feat, torch.float32, 'ligand_feat'), _ptr(ligand_ptr, torch.int32, 'ligand_ptr'), Nl, B,
            opt(enc_ligand, 'enc_ligand_feature', Nl, c.enc_ligand_dim), opt(enc_node, 'enc_node_feature', N, c.enc_node_dim),
            opt(enc_graph, 'enc_graph_feature', B, c.enc_graph_dim), kind, max_graph_nodes, _ptr(out), _ptr(ws), ws.numel(),
            ctypes.byref(tape), _stream(self.device)), 'td_prop_forward_train')
        return out, (tape, ws, (Np, Nl, B))

    @_device_bound
    def backward(self, tape, grad_out: torch.Tensor) -> torch.Tensor:
        """td_prop_backward: the gradient of every weight, flat in prop_flat_key_order (the offset slot is zero)."""
        rec, ws, (Np, Nl, B) = tape
        grad = torch.empty(self.num_weights(), dtype=torch.float32, device=self.device)
        _check(self.lib.td_prop_backward(self.handle, ctypes.byref(rec), Np, Nl, B, _ptr(grad_out, torch.float32, 'grad_out'),
                                         _ptr(grad), grad.numel(), _stream(self.device)), 'td_prop_backward')
        return grad
