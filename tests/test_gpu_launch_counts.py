"""What one denoiser evaluation launches, per profile class (td_profile_begin / td_profile_end: one count per launch scope of csrc/plan.cpp,
forward.cpp and session.cpp).  The host code that issues a step's launches is shared by the stateless entry points and the sampling session;
these literals pin its sequence for every architecture option, graph mode and session kind, so that a change of that host code which adds,
drops or doubles a launch shows here and not only as a number somewhere else.  The literals were read from the library before the block
loop, the layer loop and the x2h stage were written once (EXPERIMENTS.md, "Denoiser host path").  Launches without a profile scope (the
row restore, the receptive-field levels of the fallback, the memcpys) are not seen here."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ('knn', 'gate', 'node_proj', 'x2h_k', 'x2h_v', 'h2x_k', 'h2x_v', 'compose', 'head', 'posterior')


def _counts(knn, gate, node_proj, x2h_k, x2h_v, h2x_k, h2x_v, compose=1, head=1, posterior=0):
    return dict(zip(KEYS, (knn, gate, node_proj, x2h_k, x2h_v, h2x_k, h2x_v, compose, head, posterior)))


# (name, model config over configs/training.yml, native options, call) -> launches per class.
# The default entry, from the layer count L = 9 (one stage of each kind per layer, run_backbone): one graph search and one global gate per
# block; node_proj = L + 1 scopes: the x2h projections of layer 0 alone, one pair launch per layer l < L - 1 (h2x of layer l with x2h of
# layer l + 1) and the last layer's h2x projections alone; one x2h key pass and one value pass per layer; the h2x stage is one fused launch
# per layer, counted as h2x_k (h2x_v counts the separate coordinate pass of h2x_fused = 0 and of the general graphs' fp32 first layer).
L = 9
STATELESS = [
    ('default', {}, {}, 'forward', _counts(1, 1, L + 1, L, L, L, 0)),
    # fix_x: no h2x stage, so nothing pairs: one projection launch per layer
    ('fix_x', {}, {}, 'fix_x', _counts(1, 1, 9, 9, 9, 0, 0)),
    # td_refine_forward: no compose, no head
    ('refine', {}, {}, 'refine', _counts(1, 1, 10, 9, 9, 9, 0, compose=0, head=0)),
    ('sync_twoup', dict(sync_twoup=True), {}, 'forward', _counts(1, 1, 9, 9, 9, 9, 0)),
    ('ew_r_out_fc', dict(ew_net_type='r', x2h_out_fc=True), {}, 'forward', _counts(1, 18, 19, 9, 9, 9, 0)),
    ('ew_none', dict(ew_net_type='none'), {}, 'forward', _counts(1, 18, 10, 9, 9, 9, 0)),
    ('stages_2_2', dict(num_x2h=2, num_h2x=2), {}, 'forward', _counts(1, 1, 36, 18, 18, 18, 0)),
    ('stages_1_3_r', dict(num_x2h=1, num_h2x=3, ew_net_type='r', x2h_out_fc=True), {}, 'forward', _counts(1, 36, 45, 9, 9, 27, 0)),
    ('blocks2', dict(num_blocks=2), {}, 'forward', _counts(2, 2, 20, 18, 18, 18, 0)),
    ('knn48', dict(knn=48), {}, 'forward', _counts(1, 1, 10, 9, 9, 9, 0)),
    ('hybrid', dict(cutoff_mode='hybrid'), {}, 'forward', _counts(1, 1, 10, 9, 9, 9, 0)),
    ('radius_cap24', dict(cutoff_mode='radius', r=5.0, max_num_neighbors=24), {}, 'forward', _counts(1, 1, 10, 9, 9, 9, 0)),
    ('radius_cap40', dict(cutoff_mode='radius', r=6.0, max_num_neighbors=40), {}, 'forward', _counts(1, 1, 10, 9, 9, 9, 0)),
    ('out_fc_sync_hybrid', dict(x2h_out_fc=True, sync_twoup=True, cutoff_mode='hybrid'), {}, 'forward', _counts(1, 1, 18, 9, 9, 9, 0)),
    ('h2x_unfused', {}, dict(h2x_fused=0), 'forward', _counts(1, 1, 10, 9, 9, 9, 9)),
    ('h2x_unfused_knn48', dict(knn=48), dict(h2x_fused=0), 'forward', _counts(1, 1, 10, 9, 9, 9, 9)),
]

# the second of two session steps (td_session_step issues its launches one by one while a profile is open); posterior = the step's update
SESSION = [
    ('default', {}, {}, _counts(1, 1, 10, 9, 9, 9, 0, posterior=1)),                                         # caching, forward reach on
    ('step_lists_0', {}, dict(session_step_lists=0), _counts(1, 1, 10, 9, 9, 9, 0, posterior=1)),
    ('knn48', dict(knn=48), {}, _counts(1, 1, 10, 9, 9, 9, 0, posterior=1)),                                 # chunked caching
    ('hybrid', dict(cutoff_mode='hybrid'), {}, _counts(1, 1, 10, 9, 9, 9, 0, posterior=1)),
    ('ew_r_out_fc', dict(ew_net_type='r', x2h_out_fc=True), {}, _counts(1, 18, 19, 9, 9, 9, 0, posterior=1)),  # a session that does not cache
    ('blocks2', dict(num_blocks=2), {}, _counts(2, 2, 20, 18, 18, 18, 0, posterior=1)),
]


def _dev():
    return torch.device('cuda:0')


_state_dicts = {}


def _model(over, options):
    import warnings
    from oracle import weights
    from oracle.make_golden import SEED
    from targetdiff_amd.models import ScorePosNet3D
    cfg = dict(weights.DEFAULT_MODEL_CONFIG)
    cfg.update(over)
    key = tuple(sorted(over.items()))
    if key not in _state_dicts:
        _state_dicts[key] = weights.make_state_dict(SEED, cfg)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')            # cutoff_mode='radius' warns that the reference has no such graph
        m = ScorePosNet3D(cfg, 27, 13)
    assert not m.load_state_dict(_state_dicts[key], strict=False).unexpected_keys
    m = m.to(_dev()).eval()
    nat = m._native(_dev())
    for name, value in options.items():
        nat.set_option(name, value)
    return m


def _profiled(fn):
    from targetdiff_amd import capi
    torch.cuda.synchronize()
    capi.profile_begin()
    try:
        fn()
    finally:
        prof = capi.profile_end()
    return {k: prof[k]['launches'] for k in KEYS}


@pytest.mark.parametrize('name,over,options,call,want', STATELESS, ids=[e[0] for e in STATELESS])
def test_launches_of_a_stateless_forward(name, over, options, call, want):
    from oracle.make_golden import small_batch
    dev = _dev()
    b, lpos, lv = small_batch()
    b = b.to(dev)
    model = _model(over, options)
    args = (b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch, lpos.to(dev), lv.to(dev), b.ligand_element_batch)
    if call == 'refine':
        # the refine_net seam on a composed batch: protein rows first inside every graph (compose_context order)
        batch = torch.cat([b.protein_element_batch, b.ligand_element_batch])
        order = torch.sort(batch, stable=True).indices
        x = torch.cat([b.protein_pos, lpos.to(dev)])[order].contiguous()
        mask = torch.cat([torch.zeros_like(b.protein_element_batch), torch.ones_like(b.ligand_element_batch)])[order].bool()
        h = torch.randn(x.shape[0], 128, generator=torch.Generator().manual_seed(5)).to(dev)
        fn = lambda: model.refine_net(h, x, mask, batch[order].contiguous())
    else:
        fn = lambda: model(*args, fix_x=(call == 'fix_x'))
    fn()                      # (the first call of a model also does the one-time kernel set-up)
    got = _profiled(fn)
    print('COUNTS stateless', name, got)
    assert got == want, (name, got)


@pytest.mark.parametrize('name,over,options,want', SESSION, ids=[e[0] for e in SESSION])
def test_launches_of_a_session_step(name, over, options, want):
    """The loop body of sample_diffusion, two steps, the second one counted; and the two steps' trajectory against use_session=False."""
    from oracle import draws
    from oracle.make_golden import small_batch
    dev = _dev()
    b, lpos, lv = small_batch()
    b = b.to(dev)
    model = _model(over, options)
    args = (b.protein_pos, b.protein_atom_feature.float(), b.protein_element_batch, lpos.to(dev), lv.to(dev), b.ligand_element_batch)
    kw = dict(num_steps=2, center_pos_mode='protein')
    smp = model.begin_sampling(*args, noise_source=draws.Source(9100, dev), **kw)
    assert smp.session is not None
    smp.step()
    got = _profiled(smp.step)
    assert smp.done
    out = smp.finish()
    print('COUNTS session', name, got)
    assert got == want, (name, got)
    ref = model.sample_diffusion(*args, noise_source=draws.Source(9100, dev), use_session=False, **kw)
    for key in ('pos_traj', 'v_traj'):
        assert torch.equal(torch.stack(out[key]), torch.stack(ref[key])), (name, key)
