"""td_model_set_option / td_model_get_option on the MI355X (``-m gpu``): the defaults, the value rules of the three kinds of option
(flag, clamped, ranged), the read-only and unknown names, and -- what the step kernels see -- the per-layer switches the library derives
from the options: setting an option and putting it back, in any order and around other options' changes, must leave the forward's bits
where an untouched model has them, and an option must select the same kernels whenever it is set.

Model and batch are those of tests/test_gpu_step_variants.py: pockets of 60 / 45 / 38 atoms with ligands of 1 / 5 / 130 atoms -- one
graph below, one at and one above a workgroup's rows."""
import pytest
import torch

from oracle import weights
from targetdiff_amd import workloads

pytestmark = pytest.mark.gpu

T = 4
POCKETS = [(101, 60, 3.0, 9.0), (102, 45, 3.0, 8.0), (103, 38, 3.0, 8.0)]
SIZES = [1, 5, 130]
# TdOptions (csrc/td_internal.h)
DEFAULTS = dict(h2x_fused=1, node_proj_split=1, edge_key_split=1, edge_first_layer_f16=1, edge_second_layer_f16=1, session_hop_levels=4,
                session_forward_reach=1, edge_row_dealing=2, node_proj_bpipe=0, node_proj_async=1, session_share_pockets=1,
                session_step_lists=1)
FLAGS = [k for k in DEFAULTS if k not in ('session_hop_levels', 'edge_row_dealing')]
# the options mirrored into the per-layer weight structs, each with a value that is not its default
MIRRORED = dict(node_proj_split=0, node_proj_bpipe=1, node_proj_async=0, edge_key_split=0, edge_first_layer_f16=0, edge_second_layer_f16=0,
                edge_row_dealing=0)
KEYS = ('pred_ligand_pos', 'pred_ligand_v', 'final_h', 'final_ligand_h')

_CACHE = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


def _native():
    """a fresh native handle with the shipped options"""
    from targetdiff_amd.models import ScorePosNet3D
    if 'sd' not in _CACHE:
        _CACHE['sd'] = weights.make_state_dict(2021)
    m = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG, num_diffusion_timesteps=T), 27, 13)
    assert not m.load_state_dict(_CACHE['sd'], strict=False).unexpected_keys
    m = m.to(_dev()).eval()
    return m._native(_dev())


def _forward(nat):
    dev = _dev()
    if 'batch' not in _CACHE:
        b = workloads.pack_samples([workloads.synthetic_pocket(*p) for p in POCKETS], 1, SIZES)
        lpos, lv = workloads.init_ligand(b, generator=torch.Generator().manual_seed(91))
        b = b.to(dev)
        pptr, lptr = nat.graph_ptr(b.protein_element_batch, 3), nat.graph_ptr(b.ligand_element_batch, 3)
        ppos, lpos = b.protein_pos.clone(), lpos.to(dev).float()
        nat.center_pos(ppos, pptr, lpos, lptr)
        _CACHE['batch'] = (ppos, b.protein_atom_feature.float(), pptr, lpos, lv.to(dev), lptr)
    out = nat.model_forward(*_CACHE['batch'])
    torch.cuda.synchronize()
    return {k: out[k].clone() for k in KEYS}


def _untouched():
    if 'want' not in _CACHE:
        _CACHE['want'] = _forward(_native())
    return _CACHE['want']


def _same(got, want, what):
    for k in KEYS:
        assert torch.equal(got[k], want[k]), f'{what}: {k} differs'


def test_defaults_and_value_rules():
    nat = _native()
    for name, value in DEFAULTS.items():
        assert nat.get_option(name) == value, name
    assert nat.get_option('fold_dead_units') >= 0 and nat.get_option('fold_fp32_mlps') >= 0
    for name in FLAGS:          # a flag: any non-zero value is 1
        for v in (5, -3):
            nat.set_option(name, 0)
            nat.set_option(name, v)
            assert nat.get_option(name) == 1, (name, v)
        nat.set_option(name, 0)
        assert nat.get_option(name) == 0, name
        nat.set_option(name, DEFAULTS[name])
    nat.set_option('edge_row_dealing', -1)
    assert nat.get_option('edge_row_dealing') == 0
    nat.set_option('edge_row_dealing', 7)
    assert nat.get_option('edge_row_dealing') == 2
    nat.set_option('session_hop_levels', 2)
    for v in (0, 5):
        with pytest.raises(RuntimeError, match='session_hop_levels'):
            nat.set_option('session_hop_levels', v)
        assert nat.get_option('session_hop_levels') == 2
    nat.set_option('session_hop_levels', 4)
    for name in ('fold_dead_units', 'fold_fp32_mlps'):
        with pytest.raises(RuntimeError, match='read-only'):
            nat.set_option(name, 1)
    with pytest.raises(RuntimeError, match='unknown option'):
        nat.set_option('no_such_option', 1)
    with pytest.raises(RuntimeError, match='unknown option'):
        nat.get_option('no_such_option')
    for name, value in DEFAULTS.items():
        assert nat.get_option(name) == value, name
    _same(_forward(nat), _untouched(), 'after the value rules')


@pytest.mark.parametrize('name', sorted(MIRRORED))
def test_toggle_and_restore(name):
    nat = _native()
    nat.set_option(name, MIRRORED[name])
    assert nat.get_option(name) == MIRRORED[name]
    _forward(nat)            # (the other variant runs; its bits may differ)
    nat.set_option(name, DEFAULTS[name])
    _same(_forward(nat), _untouched(), f'{name} set and restored')


@pytest.mark.parametrize('restore', [('edge_first_layer_f16', 'edge_key_split'), ('edge_key_split', 'edge_first_layer_f16')],
                         ids=['last_set_first', 'first_set_first'])
def test_restore_order_does_not_matter(restore):
    nat = _native()
    nat.set_option('edge_key_split', 0)
    nat.set_option('edge_first_layer_f16', 0)
    for name in restore:
        nat.set_option(name, 1)
    _same(_forward(nat), _untouched(), f'edge_key_split, edge_first_layer_f16 set to 0 and restored as {restore}')


@pytest.mark.parametrize('name,other', [('edge_second_layer_f16', 'edge_first_layer_f16'), ('edge_row_dealing', 'edge_key_split')])
def test_an_option_selects_the_same_kernels_whenever_it_is_set(name, other):
    first = _native()
    first.set_option(name, 0)
    want = _forward(first)
    before = _native()          # the option set before another option's set / restore cycle ...
    before.set_option(name, 0)
    before.set_option(other, 0)
    before.set_option(other, 1)
    _same(_forward(before), want, f'{name} = 0 before a cycle of {other}')
    after = _native()           # ... and after it
    after.set_option(other, 0)
    after.set_option(other, 1)
    after.set_option(name, 0)
    _same(_forward(after), want, f'{name} = 0 after a cycle of {other}')
