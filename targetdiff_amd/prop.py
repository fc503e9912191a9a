"""Mirror of the reference's binding-affinity predictor (models/property_pred/prop_model.py PropPredNet / PropPredNetEnc,
models/property_pred/prop_egnn.py EnEquiEncoder / EnBaseLayer): same class names, constructor arguments and ``state_dict`` keys, so
a reference checkpoint loads with ``strict=True``; the arithmetic runs in libtargetdiff_hip.so (td_prop_forward).

Built for what configs/prop/*.yml give: hidden 256, 64 Gaussians, ReLU, no LayerNorm, no coordinate update (get_encoder passes
update_x=False), edge_dim 0, k <= 64, any number of layers and any enc_ligand_dim / enc_node_dim / enc_graph_dim >= 0.  Anything
else raises NotImplementedError.  There is no CPU path.

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

    def native(self, device) -> capi.NativeProp:
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError(f'targetdiff_amd runs on HIP devices only (got {device}); there is no CPU path')
        key = (str(device),) + tuple((t.data_ptr(), t._version) for t in self.state_dict().values())
        if self._native is None or key != self._native_key:
            self._native = capi.NativeProp(self.native_config(), self.state_dict(), device=device)
            self._native_key = key
        return self._native

    @torch.no_grad()
    def _run(self, protein_pos, protein_atom_feature, ligand_pos, ligand_atom_feature, batch_protein, batch_ligand, output_kind,
             enc_ligand_feature=None, enc_node_feature=None, enc_graph_feature=None, return_extra=False):
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
        out, h_layers, final_h, nbr = native.forward(
            f32(protein_pos, op), f32(protein_atom_feature, op), pptr, f32(ligand_pos, ol), f32(ligand_atom_feature, ol), lptr,
            output_kind=kind, enc_ligand=f32(enc_ligand_feature, ol), enc_node=enc_node, enc_graph=f32(enc_graph_feature),
            want_layers=return_extra, want_final_h=return_extra, want_graph=return_extra)
        if return_extra:
            return out, {'h_layers': h_layers, 'final_h': final_h, 'nbr': nbr}
        return out

    @staticmethod
    def composed_order(batch_protein, batch_ligand):
        """Index into cat([protein rows, ligand rows]) of every composed row, in the project's order (stable argsort)."""
        return torch.sort(torch.cat([batch_protein, batch_ligand]), stable=True).indices


class _ShiftedSoftplus(_Holder):
    """models/common.py:156-162 (parameterless)."""


class PropPredNet(_PropBase):
    """models/property_pred/prop_model.py:27-75: ``forward(...)`` -> [B, 3], or [B, 1] when ``output_kind`` is given."""

    def __init__(self, config, protein_atom_feature_dim, ligand_atom_feature_dim, output_dim=3):
        super().__init__()
        self._init_common(config, protein_atom_feature_dim, ligand_atom_feature_dim, output_dim, _get(config, 'hidden_channels'))

    def forward(self, protein_pos, protein_atom_feature, ligand_pos, ligand_atom_feature, batch_protein, batch_ligand, output_kind,
                return_extra=False):
        return self._run(protein_pos, protein_atom_feature, ligand_pos, ligand_atom_feature, batch_protein, batch_ligand, output_kind,
                         return_extra=return_extra)


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
                enc_ligand_feature, enc_node_feature, enc_graph_feature, return_extra=False):
        if enc_ligand_feature is None and self.enc_ligand_dim > 0:
            raise ValueError(f'enc_ligand_dim is {self.enc_ligand_dim}: enc_ligand_feature is needed (ligand_atom_emb takes it)')
        if enc_graph_feature is None and self.enc_graph_dim > 0:
            raise ValueError(f'enc_graph_dim is {self.enc_graph_dim}: enc_graph_feature is needed (out_block takes it)')
        if enc_node_feature is not None and self.enc_node_dim == 0:
            raise ValueError('enc_node_feature given, but the model has no enc_node_layer (enc_node_dim 0)')
        return self._run(protein_pos, protein_atom_feature, ligand_pos, ligand_atom_feature, batch_protein, batch_ligand, output_kind,
                         enc_ligand_feature, enc_node_feature, enc_graph_feature, return_extra=return_extra)


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
