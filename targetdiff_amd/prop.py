"""Mirror of the reference's binding-affinity predictor (models/property_pred/prop_model.py PropPredNet / PropPredNetEnc,
models/property_pred/prop_egnn.py EnEquiEncoder / EnBaseLayer): same class names, constructor arguments and ``state_dict`` keys, so
a reference checkpoint loads with ``strict=True``; the arithmetic runs in libtargetdiff_hip.so (td_prop_forward).

Built for what configs/prop/*.yml give: hidden 256, 64 Gaussians, ReLU, no LayerNorm, no coordinate update (get_encoder passes
update_x=False), edge_dim 0, k <= 64, any number of layers and any enc_ligand_dim / enc_node_dim / enc_graph_dim >= 0.  Anything
else raises NotImplementedError.  There is no CPU path.

Training: ``get_loss`` (prop_model.py:76-95, 167-212) and ``forward(..., differentiable=True)`` run td_prop_forward_train and, on
``backward()``, td_prop_backward, which hands every parameter its gradient; the optimizer is torch's.  Gradients flow to parameters
only: an input that requires grad raises NotImplementedError.  After ``optimizer.step()`` the next call re-packs the weights on the
device (td_prop_set_weights) instead of building a new handle.

Composed order (compose_context_prop, models/common.py:140-153, argsorts the concatenated batch vector): the project's rule is the
stable one -- per complex its protein atoms, then its ligand atoms, each in input order; unsorted batch vectors are handled the same
way.  Only the k-NN tie rule (ascending (d^2, index)) and the order of floating-point sums depend on it.
"""
from __future__ import annotations

import torch
from torch import nn

from . import capi


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


class _Holder(nn.Module):
    def forward(self, *a, **k):
        raise RuntimeError('parameter holder: the arithmetic runs in libtargetdiff_hip.so')


class _Offsets(_Holder):
    """GaussianSmearing(start, stop, num_gaussians, fixed_offset=False) (models/common.py:7-19): the ``offset`` buffer."""

    def __init__(self, start, stop, num_gaussians):
        super().__init__()
        self.start, self.stop, self.num_gaussians = start, stop, num_gaussians
        offset = torch.linspace(start, stop, num_gaussians)
        self.coeff = -0.5 / (offset[1] - offset[0]).item() ** 2
        self.register_buffer('offset', offset)


class _Mlp2(_Holder):
    """models/common.py:60-80 with num_layer=2, norm=False, ReLU: keys net.0 / net.2."""

    def __init__(self, in_dim, out_dim, hidden_dim, act_last=False):
        super().__init__()
        layers = [nn.Linear(in_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, out_dim)]
        if act_last:
            layers.append(nn.ReLU())
        self.net = nn.Sequential(*layers)


class _Seq(nn.Sequential):
    def forward(self, *a, **k):
        raise RuntimeError('parameter holder: the arithmetic runs in libtargetdiff_hip.so')


def _supported(hidden_dim, edge_feat_dim, num_r_gaussian, act_fn, norm, update_x, k=48):
    if (hidden_dim, edge_feat_dim, num_r_gaussian, act_fn, bool(norm), bool(update_x)) != (256, 0, 64, 'relu', False, False) or \
            not 1 <= int(k) <= capi.MAX_FANIN:
        raise NotImplementedError(
            'the HIP affinity encoder is built for hidden_dim 256, edge_feat_dim 0, num_r_gaussian 64, act_fn "relu", norm False, '
            f'update_x False and 1 <= k <= {capi.MAX_FANIN}; got hidden_dim {hidden_dim}, edge_feat_dim {edge_feat_dim}, '
            f'num_r_gaussian {num_r_gaussian}, act_fn {act_fn!r}, norm {norm}, update_x {update_x}, k {k}')


class EnBaseLayer(_Holder):
    """models/property_pred/prop_egnn.py:8-26 (parameters only)."""

    def __init__(self, hidden_dim, edge_feat_dim, num_r_gaussian, update_x=True, act_fn='relu', norm=False):
        super().__init__()
        _supported(hidden_dim, edge_feat_dim, num_r_gaussian, act_fn, norm, update_x)
        self.r_min, self.r_max = 0., 10. ** 2
        self.hidden_dim, self.num_r_gaussian, self.edge_feat_dim = hidden_dim, num_r_gaussian, edge_feat_dim
        self.update_x, self.act_fn, self.norm = update_x, act_fn, norm
        if num_r_gaussian > 1:
            self.r_expansion = _Offsets(self.r_min, self.r_max, num_r_gaussian)      # built by the reference, never used
        self.edge_mlp = _Mlp2(2 * hidden_dim + edge_feat_dim + num_r_gaussian, hidden_dim, hidden_dim, act_last=True)
        self.edge_inf = _Seq(nn.Linear(hidden_dim, 1), nn.Sigmoid())
        self.node_mlp = _Mlp2(2 * hidden_dim, hidden_dim, hidden_dim)


class EnEquiEncoder(_Holder):
    """models/property_pred/prop_egnn.py:48-83 (parameters only; PropPredNet runs it inside td_prop_forward)."""

    def __init__(self, num_layers, hidden_dim, edge_feat_dim, num_r_gaussian, k=32, cutoff=10.0, update_x=True, act_fn='relu',
                 norm=False):
        super().__init__()
        _supported(hidden_dim, edge_feat_dim, num_r_gaussian, act_fn, norm, update_x, k)
        self.num_layers, self.hidden_dim, self.edge_feat_dim, self.num_r_gaussian = num_layers, hidden_dim, edge_feat_dim, num_r_gaussian
        self.update_x, self.act_fn, self.norm, self.k, self.cutoff = update_x, act_fn, norm, k, cutoff
        self.distance_expansion = _Offsets(0.0, cutoff, num_r_gaussian)
        self.net = nn.ModuleList([EnBaseLayer(hidden_dim, edge_feat_dim, num_r_gaussian, update_x=update_x, act_fn=act_fn, norm=norm)
                                  for _ in range(num_layers)])


def get_encoder(config):
    """models/property_pred/prop_model.py:10-24."""
    if _get(config, 'name') in ('egnn', 'egnn_enc'):
        return EnEquiEncoder(num_layers=_get(config, 'num_layers'), edge_feat_dim=_get(config, 'edge_dim'),
                             hidden_dim=_get(config, 'hidden_dim'), num_r_gaussian=_get(config, 'num_r_gaussian'),
                             act_fn=_get(config, 'act_fn'), norm=_get(config, 'norm'), update_x=False, k=_get(config, 'knn'),
                             cutoff=_get(config, 'cutoff'))
    raise ValueError(_get(config, 'name'))


def _sort_by_complex(batch):
    """Stable order of a batch vector (a no-op permutation when it is sorted) and the CSR offsets of the sorted vector."""
    order = torch.sort(batch, stable=True).indices
    return order, batch[order]


class _PropBase(nn.Module):
    enc_ligand_dim = enc_node_dim = enc_graph_dim = 0

    def _init_common(self, config, protein_atom_feature_dim, ligand_atom_feature_dim, output_dim, graph_in):
        self.config = config
        self.hidden_dim = _get(config, 'hidden_channels')
        if self.hidden_dim != capi.PROP_HIDDEN:
            raise NotImplementedError(f'hidden_channels must be {capi.PROP_HIDDEN} for the HIP path, got {self.hidden_dim}')
        self.output_dim = output_dim
        self.protein_atom_feature_dim, self.ligand_atom_feature_dim = protein_atom_feature_dim, ligand_atom_feature_dim
        self.protein_atom_emb = nn.Linear(protein_atom_feature_dim, self.hidden_dim)
        self.ligand_atom_emb = nn.Linear(ligand_atom_feature_dim + self.enc_ligand_dim, self.hidden_dim)
        self.encoder = get_encoder(_get(config, 'encoder'))
        if self.enc_node_dim > 0:
            self.enc_node_layer = _Seq(nn.Linear(self.hidden_dim + self.enc_node_dim, self.hidden_dim), nn.ReLU(),
                                       nn.Linear(self.hidden_dim, self.hidden_dim))
        self.out_block = _Seq(nn.Linear(graph_in, self.hidden_dim), _ShiftedSoftplus(), nn.Linear(self.hidden_dim, output_dim))
        self._native = None
        self._native_key = None

    def native_config(self):
        enc = self.encoder
        return dict(hidden_dim=self.hidden_dim, num_layers=enc.num_layers, knn=int(enc.k), num_r_gaussian=enc.num_r_gaussian,
                    cutoff=float(enc.cutoff), protein_feat_dim=self.protein_atom_feature_dim,
                    ligand_feat_dim=self.ligand_atom_feature_dim, enc_ligand_dim=self.enc_ligand_dim, enc_node_dim=self.enc_node_dim,
                    enc_graph_dim=self.enc_graph_dim, output_dim=self.output_dim)

    def _flat_keys(self):
        return capi.prop_flat_key_order(self.encoder.num_layers, self.enc_node_dim)

    def native(self, device) -> capi.NativeProp:
        """The td_prop handle on `device`.  A new handle when the device, a tensor's storage or a buffer changed; when only parameter
        values changed (an optimizer step), the same handle, re-packed on the device from a device copy of the parameters."""
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError(f'targetdiff_amd runs on HIP devices only (got {device}); there is no CPU path')
        sd = self.state_dict()
        named = dict(self.named_parameters())
        is_param = [k in named for k in sd]
        key = (str(device),) + tuple((t.data_ptr(), None if p else t._version) for t, p in zip(sd.values(), is_param))
        versions = tuple(t._version for t, p in zip(sd.values(), is_param) if p)
        if self._native is None or key != self._native_key:
            self._native = capi.NativeProp(self.native_config(), sd, device=device)
            self._native_key, self._native_versions = key, versions
        elif versions != self._native_versions:
            flat = torch.cat([sd[k].reshape(-1) for k in self._flat_keys()]).to(device=device, dtype=torch.float32).contiguous()
            self._native.set_weights(flat)
            self._native_versions = versions
        return self._native

    def _check_inputs(self, tensors):
        for name, t in tensors.items():
            if torch.is_tensor(t) and t.requires_grad:
                raise NotImplementedError(f'{name} requires grad: the HIP affinity predictor gives gradients to its parameters only '
                                          '(positions and input features are constants)')

    def _run(self, protein_pos, protein_atom_feature, ligand_pos, ligand_atom_feature, batch_protein, batch_ligand, output_kind,
             enc_ligand_feature=None, enc_node_feature=None, enc_graph_feature=None, return_extra=False, differentiable=False):
        if differentiable:
            if return_extra:
                raise ValueError('return_extra is not available with differentiable=True')
            self._check_inputs(dict(protein_pos=protein_pos, protein_atom_feature=protein_atom_feature, ligand_pos=ligand_pos,
                                    ligand_atom_feature=ligand_atom_feature, enc_ligand_feature=enc_ligand_feature,
                                    enc_node_feature=enc_node_feature, enc_graph_feature=enc_graph_feature))
        with torch.no_grad():
            return self._run_native(protein_pos, protein_atom_feature, ligand_pos, ligand_atom_feature, batch_protein, batch_ligand,
                                    output_kind, enc_ligand_feature, enc_node_feature, enc_graph_feature, return_extra, differentiable)

    def _run_native(self, protein_pos, protein_atom_feature, ligand_pos, ligand_atom_feature, batch_protein, batch_ligand, output_kind,
                    enc_ligand_feature, enc_node_feature, enc_graph_feature, return_extra, differentiable):
        dev = protein_pos.device
        native = self.native(dev)
        B = int(max(int(batch_protein.max()) if batch_protein.numel() else -1,
                    int(batch_ligand.max()) if batch_ligand.numel() else -1)) + 1
        op, bp = _sort_by_complex(batch_protein)
        ol, bl = _sort_by_complex(batch_ligand)
        pptr = capi.graph_ptr(bp.contiguous(), B)
        lptr = capi.graph_ptr(bl.contiguous(), B)

        def f32(t, order=None):
            if t is None:
                return None
            t = t.float()
            return (t[order] if order is not None else t).contiguous()
        enc_node = f32(enc_node_feature)          # rows in composed order already (the order the library composes in)
        kind = output_kind.to(torch.int64).contiguous() if output_kind is not None else None
        if differentiable:
            args = dict(protein_pos=f32(protein_pos, op), protein_feat=f32(protein_atom_feature, op), protein_ptr=pptr,
                        ligand_pos=f32(ligand_pos, ol), ligand_feat=f32(ligand_atom_feature, ol), ligand_ptr=lptr, output_kind=kind,
                        enc_ligand=f32(enc_ligand_feature, ol), enc_node=enc_node, enc_graph=f32(enc_graph_feature))
            keys = [k for k in self._flat_keys() if k != 'encoder.distance_expansion.offset']
            named = dict(self.named_parameters())
            with torch.enable_grad():
                return _PropTrain.apply(native, args, self._flat_slices(), keys, *[named[k] for k in keys])
        out, h_layers, final_h, nbr = native.forward(
            f32(protein_pos, op), f32(protein_atom_feature, op), pptr, f32(ligand_pos, ol), f32(ligand_atom_feature, ol), lptr,
            output_kind=kind, enc_ligand=f32(enc_ligand_feature, ol), enc_node=enc_node, enc_graph=f32(enc_graph_feature),
            want_layers=return_extra, want_final_h=return_extra, want_graph=return_extra)
        if return_extra:
            return out, {'h_layers': h_layers, 'final_h': final_h, 'nbr': nbr}
        return out

    def _flat_slices(self):
        sd = self.state_dict()
        sl, o = {}, 0
        for k in self._flat_keys():
            n = sd[k].numel()
            sl[k] = (o, o + n, tuple(sd[k].shape))
            o += n
        return sl

    def _enc_features(self, batch):
        return None, None, None

    def get_loss(self, batch, pos_noise_std, return_pred=False):
        """prop_model.py:76-95 / 167-212: MSE of the prediction for ``batch.kind`` against ``batch.y``, positions jittered by
        N(0, pos_noise_std^2) (protein noise drawn first, then ligand noise, with torch.randn_like on the data's device).  Under grad
        mode the prediction is differentiable (HIP forward and backward); under torch.no_grad() it is the plain forward."""
        enc_ligand, enc_node, enc_graph = self._enc_features(batch)
        differentiable = torch.is_grad_enabled()
        if differentiable:
            self._check_inputs(dict(protein_pos=batch.protein_pos, ligand_pos=batch.ligand_pos,
                                    protein_atom_feature=batch.protein_atom_feature, ligand_atom_feature_full=batch.ligand_atom_feature_full,
                                    enc_ligand_feature=enc_ligand, enc_node_feature=enc_node, enc_graph_feature=enc_graph))
        protein_noise = torch.randn_like(batch.protein_pos) * pos_noise_std
        ligand_noise = torch.randn_like(batch.ligand_pos) * pos_noise_std
        pred = self._run(batch.protein_pos + protein_noise, batch.protein_atom_feature.float(), batch.ligand_pos + ligand_noise,
                         batch.ligand_atom_feature_full.float(), batch.protein_element_batch, batch.ligand_element_batch, batch.kind,
                         enc_ligand, enc_node, enc_graph, differentiable=differentiable)
        loss = nn.MSELoss()(pred.view(-1), batch.y)
        if return_pred:
            return loss, pred
        return loss

    @staticmethod
    def composed_order(batch_protein, batch_ligand):
        """Index into cat([protein rows, ligand rows]) of every composed row, in the project's order (stable argsort)."""
        return torch.sort(torch.cat([batch_protein, batch_ligand]), stable=True).indices


class _PropTrain(torch.autograd.Function):
    """The model's output as a function of its parameters: td_prop_forward_train forward, td_prop_backward backward."""

    @staticmethod
    def forward(ctx, native, args, slices, keys, *params):
        out, tape = native.forward_train(**args)
        ctx.native, ctx.tape, ctx.slices, ctx.keys = native, tape, slices, keys
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        if ctx.tape is None:
            raise RuntimeError('the HIP affinity predictor\'s tape was used already (backward twice without retain_graph)')
        flat = ctx.native.backward(ctx.tape, grad_out.float().contiguous())
        ctx.tape = None
        grads = [flat[ctx.slices[k][0]:ctx.slices[k][1]].view(ctx.slices[k][2]) for k in ctx.keys]
        return (None, None, None, None) + tuple(grads)


class _ShiftedSoftplus(_Holder):
    """models/common.py:156-162 (parameterless)."""


class PropPredNet(_PropBase):
    """models/property_pred/prop_model.py:27-75: ``forward(...)`` -> [B, 3], or [B, 1] when ``output_kind`` is given."""

    def __init__(self, config, protein_atom_feature_dim, ligand_atom_feature_dim, output_dim=3):
        super().__init__()
        self._init_common(config, protein_atom_feature_dim, ligand_atom_feature_dim, output_dim, _get(config, 'hidden_channels'))

    def forward(self, protein_pos, protein_atom_feature, ligand_pos, ligand_atom_feature, batch_protein, batch_ligand, output_kind,
                return_extra=False, differentiable=False):
        return self._run(protein_pos, protein_atom_feature, ligand_pos, ligand_atom_feature, batch_protein, batch_ligand, output_kind,
                         return_extra=return_extra, differentiable=differentiable)


class PropPredNetEnc(_PropBase):
    """models/property_pred/prop_model.py:98-165, with the optional diffusion-model features ``enc_ligand_feature`` [N_l, El],
    ``enc_node_feature`` [N_p + N_l, En] (e.g. ``final_h`` of ScorePosNet3D.fetch_embedding, composed order) and
    ``enc_graph_feature`` [B, Eg]."""

    def __init__(self, config, protein_atom_feature_dim, ligand_atom_feature_dim, enc_ligand_dim, enc_node_dim, enc_graph_dim,
                 enc_feature_type=None, output_dim=1):
        super().__init__()
        for name, v in (('enc_ligand_dim', enc_ligand_dim), ('enc_node_dim', enc_node_dim), ('enc_graph_dim', enc_graph_dim)):
            if int(v) < 0:
                raise ValueError(f'{name} must be >= 0, got {v}')
        self.enc_ligand_dim, self.enc_node_dim, self.enc_graph_dim = int(enc_ligand_dim), int(enc_node_dim), int(enc_graph_dim)
        self.enc_feature_type = enc_feature_type
        self._init_common(config, protein_atom_feature_dim, ligand_atom_feature_dim, output_dim,
                          _get(config, 'hidden_channels') + self.enc_graph_dim)

    def forward(self, protein_pos, protein_atom_feature, ligand_pos, ligand_atom_feature, batch_protein, batch_ligand, output_kind,
                enc_ligand_feature, enc_node_feature, enc_graph_feature, return_extra=False, differentiable=False):
        if enc_ligand_feature is None and self.enc_ligand_dim > 0:
            raise ValueError(f'enc_ligand_dim is {self.enc_ligand_dim}: enc_ligand_feature is needed (ligand_atom_emb takes it)')
        if enc_graph_feature is None and self.enc_graph_dim > 0:
            raise ValueError(f'enc_graph_dim is {self.enc_graph_dim}: enc_graph_feature is needed (out_block takes it)')
        if enc_node_feature is not None and self.enc_node_dim == 0:
            raise ValueError('enc_node_feature given, but the model has no enc_node_layer (enc_node_dim 0)')
        return self._run(protein_pos, protein_atom_feature, ligand_pos, ligand_atom_feature, batch_protein, batch_ligand, output_kind,
                         enc_ligand_feature, enc_node_feature, enc_graph_feature, return_extra=return_extra, differentiable=differentiable)

    def _enc_features(self, batch):
        """prop_model.py:172-194: which batch fields feed enc_ligand_feature / enc_node_feature / enc_graph_feature."""
        t = self.enc_feature_type
        if t == 'nll_all':
            return None, None, batch.nll_all
        if t == 'nll':
            return None, None, batch.nll
        if t == 'final_h':
            return None, batch.final_h, None
        if t == 'pred_ligand_v':
            return batch.pred_ligand_v, None, None
        if t == 'pred_v_entropy_pre':
            return batch.pred_v_entropy, None, None
        if t == 'pred_v_entropy_post':
            return None, None, _graph_sum(batch.pred_v_entropy, batch.ligand_element_batch, batch.kind.shape[0])
        if t == 'full':
            graph = torch.cat([batch.nll_all, _graph_sum(batch.pred_v_entropy, batch.ligand_element_batch, batch.kind.shape[0])], -1)
            return torch.cat([batch.pred_ligand_v, batch.pred_v_entropy], -1), batch.final_h, graph
        raise NotImplementedError(f'enc_feature_type {t!r}')


def _graph_sum(x, batch, B):
    """scatter(x, batch, dim=0, reduce='sum') with B rows, as a one-hot product (no float atomics: the same sum every run)."""
    onehot = (batch.view(1, -1) == torch.arange(B, device=batch.device).view(-1, 1)).to(x.dtype)
    return onehot @ x


def get_model(config, protein_atom_feat_dim, ligand_atom_feat_dim):
    """utils/misc_prop.py:45-64."""
    model_cfg = _get(config, 'model')
    if _get(_get(model_cfg, 'encoder'), 'name') == 'egnn_enc':
        return PropPredNetEnc(model_cfg, protein_atom_feature_dim=protein_atom_feat_dim, ligand_atom_feature_dim=ligand_atom_feat_dim,
                              enc_ligand_dim=_get(model_cfg, 'enc_ligand_dim'), enc_node_dim=_get(model_cfg, 'enc_node_dim'),
                              enc_graph_dim=_get(model_cfg, 'enc_graph_dim'), enc_feature_type=_get(model_cfg, 'enc_feature_type'),
                              output_dim=1)
    return PropPredNet(model_cfg, protein_atom_feature_dim=protein_atom_feat_dim, ligand_atom_feature_dim=ligand_atom_feat_dim,
                       output_dim=3)
