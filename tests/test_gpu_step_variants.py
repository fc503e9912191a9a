"""Every variant of the step update, in both of its forms, on the MI355X (``-m gpu``): known atoms on / off x time program on / off x
clash guidance on / off x pos_only on / off.  Each case runs four steps that end on clean data three ways -- the stateless entry points
(td_posterior_step* / td_renoise_step), a session launch by launch, a session replaying its captured graph -- and asserts that the four
trajectories agree bit for bit.  The files of the single features cover their own combinations; this one covers the cross product, so
that an argument that reaches one form's kernel in the wrong place shows as a difference.  The stateless side is tied to the CPU
restatements by those files: nothing here is about absolute values.

Shape: three graphs with 1, 5 and 130 ligand atoms -- a one-atom graph, an ordinary one and one that spans two 128-atom workgroups, so
that the step index is handed over by the last of several workgroups.  The mask flags atoms of the first and the last graph only.
"""
import pytest
import torch

from oracle import draws, weights
from targetdiff_amd import workloads
from targetdiff_amd.guidance import ClashGuidance
from targetdiff_amd.schedule import DENOISE, RENOISE, TimeProgram

pytestmark = pytest.mark.gpu

T = 4                       # levels of the model: four unit steps end at t = 0
POCKETS = [(101, 60, 3.0, 9.0), (102, 45, 3.0, 8.0), (103, 38, 3.0, 8.0)]
SIZES = [1, 5, 130]
KNOWN = [0, 6, 70, 127, 128, 135]            # the one atom of graph 0; graph 2 on both sides of the workgroup boundary, its last atom
# four slots, the last one onto clean data: a pure descent, and one with jumps and a renoise slot in the middle
DESCENT = TimeProgram.from_levels(T, [3, 2, 1, 0, -1])
RESAMPLED = TimeProgram(T, [DENOISE, RENOISE, DENOISE, DENOISE], [3, 1, 2, 0], [1, 2, 0, -1])

_CACHE = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')


def _model():
    if 'model' not in _CACHE:
        from targetdiff_amd.models import ScorePosNet3D
        m = ScorePosNet3D(dict(weights.DEFAULT_MODEL_CONFIG, num_diffusion_timesteps=T), 27, 13)
        assert not m.load_state_dict(weights.make_state_dict(2021), strict=False).unexpected_keys
        _CACHE['model'] = m.to(_dev()).eval()
    return _CACHE['model']


def _batch(dev):
    if 'batch' not in _CACHE:
        b = workloads.pack_samples([workloads.synthetic_pocket(*p) for p in POCKETS], 1, SIZES)
        g = torch.Generator().manual_seed(91)
        init_pos, init_v = workloads.init_ligand(b, generator=g)
        n = init_pos.shape[0]
        mask = torch.zeros(n, dtype=torch.bool)
        mask[KNOWN] = True
        assert not bool(mask[SIZES[0]:SIZES[0] + SIZES[1]].any())
        cen = torch.stack([b.protein_pos[b.protein_element_batch == k].mean(0) for k in range(3)])
        fixed = dict(fixed_mask=mask.to(dev), fixed_pos=(cen[b.ligand_element_batch] + 1.2 * torch.randn(n, 3, generator=g)).to(dev),
                     fixed_v=torch.randint(0, 13, (n,), generator=g).to(dev))
        sigma = (3.5 + 1.5 * torch.rand(b.protein_pos.shape[0], generator=g)).to(dev)
        b = b.to(dev)
        args = (b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch, init_pos.to(dev), init_v.to(dev),
                b.ligand_element_batch)
        _CACHE['batch'] = (args, fixed, sigma)
    return _CACHE['batch']


def _on_side_stream(dev, fn):
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        out = fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    return out


@pytest.mark.parametrize('pos_only', [False, True])
@pytest.mark.parametrize('guided', [False, True])
@pytest.mark.parametrize('prog', [False, True])
@pytest.mark.parametrize('mask', [False, True])
def test_stateless_eager_and_graph_agree(mask, prog, guided, pos_only):
    dev = _dev()
    args, fixed, sigma = _batch(dev)
    kw = dict(fixed) if mask else {}
    program = None
    if prog:
        program = RESAMPLED if guided else DESCENT          # the renoise slot: with and without known atoms, with and without pos_only
        kw['time_program'] = program
    if guided:
        kw['guidance'] = ClashGuidance(radius=sigma, weight=1.0, max_shift=1.0)

    def run(use_session, use_graph):
        s = _model().begin_sampling(*args, center_pos_mode='protein', noise_source=draws.Source(5100, dev), use_session=use_session,
                                    use_graph=use_graph, pos_only=pos_only, **kw)
        replayed = []
        while not s.done:
            s.step()
            replayed.append(bool(s.session.last_step_was_graph()) if s.session is not None else False)
        return s.finish(), replayed

    stateless, _ = run(False, None)
    eager, rep_e = run(True, False)
    graph, rep_g = _on_side_stream(dev, lambda: run(True, True))
    assert len(stateless['pos_traj']) == 4 and not any(rep_e)
    # the first denoise step is issued launch by launch and captured, renoise slots are always one eager launch
    want = [k > 0 and (program is None or program.kind[k] == DENOISE) for k in range(4)]
    assert rep_g == want, rep_g
    for name, other in (('session, launch by launch', eager), ('session, captured graph', graph)):
        for key in ('pos_traj', 'v_traj', 'v0_traj', 'vt_traj'):
            assert len(other[key]) == len(stateless[key]) == (0 if pos_only and key in ('v0_traj', 'vt_traj') else 4), (name, key)
            for k, (x, y) in enumerate(zip(stateless[key], other[key])):
                assert torch.equal(x, y), f'stateless vs {name}: {key} differs at step {k}'
