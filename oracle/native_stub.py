"""A recording stand-in for the native layer (TEST INFRASTRUCTURE): capi's method surface on torch CPU tensors, its arithmetic from
the oracle restatement, every call logged.  It lets the mirror class run where there is no GPU, so that the seam between a driver
and ``targetdiff_amd.models.ScorePosNet3D`` can be checked on its own: argument names / order / dtypes / devices, the members read,
the dictionary keys, list lengths, dtypes and de-centring expected back.  Used by tests/test_reference_driver_with_mirror.py and
oracle/check_with_reference.py."""
import torch

from oracle import restatement as R


def _batch_of(ptr):
    n = (ptr[1:] - ptr[:-1]).long()
    return torch.repeat_interleave(torch.arange(n.numel()), n)


class RecordingNative:
    """capi.NativeModel's surface on torch CPU tensors; every call is logged as (name, shapes / dtypes of the arguments)."""

    def __init__(self, sd, cfg, num_classes, log):
        self.sd, self.cfg, self.num_classes, self.log = sd, cfg, num_classes, log
        self.sched = R.diffusion_schedules(cfg)

    def _rec(self, name, **tensors):
        self.log.append((name, {k: (tuple(v.shape), str(v.dtype), v.device.type) for k, v in tensors.items() if torch.is_tensor(v)}))

    def graph_ptr(self, batch, B):
        self._rec('graph_ptr', batch=batch)
        assert batch.dtype == torch.int64
        return torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(batch, minlength=B).cumsum(0)]).to(torch.int32)

    def center_pos(self, protein_pos, protein_ptr, ligand_pos, ligand_ptr, offset=None, sign=-1):
        self._rec('center_pos', protein_pos=protein_pos, ligand_pos=ligand_pos)
        assert offset is None and sign == -1
        bp, bl = _batch_of(protein_ptr), _batch_of(ligand_ptr)
        p, l, off = R.center_positions(protein_pos, ligand_pos, bp, bl)
        protein_pos.copy_(p)
        ligand_pos.copy_(l)
        return off

    def model_forward(self, protein_pos, protein_v, protein_ptr, ligand_pos, ligand_v, ligand_ptr, fix_x=False, max_graph_nodes=0,
                      want_final_h=True, out=None, ligand_graph_bias=None):
        self._rec('model_forward', protein_pos=protein_pos, protein_v=protein_v, ligand_pos=ligand_pos, ligand_v=ligand_v)
        assert protein_v.dtype == torch.float32 and ligand_v.dtype == torch.int64
        return R.model_forward(self.sd, self.cfg, protein_pos, protein_v, _batch_of(protein_ptr), ligand_pos, ligand_v,
                               _batch_of(ligand_ptr), fix_x=fix_x)

    def posterior_step(self, t, ligand_ptr, ligand_pos, ligand_v, pred_pos, pred_v, noise, uniform, pos_next=None, v_next=None,
                       log_v0=None, log_post=None):
        self._rec('posterior_step', t=t, noise=noise, uniform=uniform)
        assert t.dtype == torch.int32 and t.numel() == ligand_ptr.numel() - 1
        pos, v, l0, lp = R.posterior_step(self.sched, t.long(), ligand_pos, ligand_v, pred_pos, pred_v, _batch_of(ligand_ptr), noise,
                                          uniform, self.num_classes)
        pos_next.copy_(pos)
        v_next.copy_(v)
        if log_v0 is not None:
            log_v0.copy_(l0)
            log_post.copy_(lp)
        return pos_next, v_next


class StubSession:
    """capi.NativeSession: the sampling session is an optimisation of model_forward, bit-identical by construction."""

    def __init__(self, native, protein_pos, protein_v, protein_ptr, ligand_ptr, num_ligand_atoms, max_graph_nodes):
        native._rec('session_create', protein_pos=protein_pos, protein_v=protein_v)
        self.a = (native, protein_pos, protein_v, protein_ptr, ligand_ptr)

    def forward(self, ligand_pos, ligand_v, out=None, ligand_graph_bias=None):
        n, pp, pv, pptr, lptr = self.a
        return n.model_forward(pp, pv, pptr, ligand_pos, ligand_v, lptr)

    # td_session_step: forward + posterior update on the state held in `io` (current positions / types updated in place, slot s of
    # the trajectories filled, the step index advanced)
    def make_step_io(self, step_index, t_all, ligand_pos, ligand_v, noise, uniform, pos_traj, v_traj, v0_traj=None, vt_traj=None,
                     pos_only=False, ligand_graph_bias=None):
        assert ligand_graph_bias is None               # time_emb_dim == 0 in this configuration
        return dict(step=step_index, t_all=t_all, pos=ligand_pos, v=ligand_v, noise=noise, uniform=uniform, pos_traj=pos_traj,
                    v_traj=v_traj, v0_traj=v0_traj, vt_traj=vt_traj, pos_only=pos_only)

    def step(self, io, use_graph=True):
        n, pp, pv, pptr, lptr = self.a
        s = int(io['step'][0])
        preds = n.model_forward(pp, pv, pptr, io['pos'], io['v'], lptr)
        full = not io['pos_only']
        v_next = io['v_traj'][s] if full else torch.empty_like(io['v'])
        n.posterior_step(io['t_all'][s], lptr, io['pos'], io['v'], preds['pred_ligand_pos'], preds['pred_ligand_v'], io['noise'],
                         io['uniform'], pos_next=io['pos_traj'][s], v_next=v_next, log_v0=io['v0_traj'][s] if full else None,
                         log_post=io['vt_traj'][s] if full else None)
        io['pos'].copy_(io['pos_traj'][s])
        if full:
            io['v'].copy_(io['v_traj'][s])
        else:
            io['v_traj'][s].copy_(io['v'])
        io['step'][0] += 1


def route_draws(monkeypatch):
    """Route the sampler's draws through torch.randn_like / rand_like (which oracle.make_golden_r2.counter_draws patches), in the
    reference's order: the sampler refills fixed buffers in place (normal_ / uniform_), and the mirror draws its per-step uniforms
    with torch.rand(N_l, K) where the reference calls torch.rand_like (inside log_sample_categorical)."""
    from targetdiff_amd import models

    def draw(self, s):
        self._noise.copy_(torch.randn_like(self.lpos))
        if not self.pos_only:
            self._uniform.copy_(torch.rand(self.Nl, self.C, dtype=torch.float32))
    monkeypatch.setattr(models.ReverseSampler, '_draw', draw)
    monkeypatch.setattr(torch, 'rand', lambda *size, **kw: torch.rand_like(torch.empty(*size, dtype=kw.get('dtype', torch.float32))))
