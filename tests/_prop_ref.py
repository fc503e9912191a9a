"""Binding-affinity predictor: seeded weights, the fixture complexes and a float64 CPU restatement of PropPredNet / PropPredNetEnc
(models/property_pred/prop_model.py, prop_egnn.py), written from the reference's arithmetic, not imported from it.

tools/make_golden_prop.py builds tests/golden/prop_*.npz with the real reference from the same weights and inputs; the fixtures hold
inputs and outputs only, the weights are regenerated here from (seed, gain).
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

PROTEIN_FEAT_DIM = 27          # utils/transforms_prop.py:15-20: 6 elements + 20 amino acids + backbone
# utils/transforms_prop.py:35-67: 8 elements + ATOM_FEATS of datasets/protein_ligand.py:14 = AtomicNumber 1, Aromatic 1, Degree 6,
# NumHs 6, Hybridization len(rdkit HybridizationType.values) = 8 (UNSPECIFIED, S, SP, SP2, SP3, SP3D, SP3D2, OTHER)
LIGAND_FEAT_DIM = 8 + 1 + 1 + 6 + 6 + 8
LIGAND_ELEMENTS = ('H', 'C', 'N', 'O', 'F', 'P', 'S', 'Cl')
ATOMIC_NUMBER = {'H': 1, 'C': 6, 'N': 7, 'O': 8, 'F': 9, 'P': 15, 'S': 16, 'Cl': 17, 'Br': 35}

MODEL_CONFIG = dict(hidden_channels=256, encoder=dict(name='egnn', num_layers=6, hidden_dim=256, edge_dim=0, num_r_gaussian=64,
                                                      act_fn='relu', norm=False, cutoff=10.0, knn=48))


def enc_config(enc_ligand_dim=0, enc_node_dim=128, enc_graph_dim=0, enc_feature_type='final_h'):
    """configs/prop/pdbbind_general_egnn_enc_final_h.yml (model section), with the three enc_* widths as given."""
    cfg = dict(MODEL_CONFIG, enc_ligand_dim=enc_ligand_dim, enc_node_dim=enc_node_dim, enc_graph_dim=enc_graph_dim,
               enc_feature_type=enc_feature_type)
    cfg['encoder'] = dict(MODEL_CONFIG['encoder'], name='egnn_enc')
    return cfg


def make_state_dict(spec, seed: int, gain: float = 1.0, bias_gain: float = 1.0):
    """Seeded weights for the (key, shape) list `spec` (the reference's state_dict order): every Linear weight and bias
    U(-gain / sqrt(fan_in), gain / sqrt(fan_in)) (nn.Linear's range at gain 1; biases at bias_gain times it); the Gaussian offsets
    are the buffers' own linspace values."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    fan = {}
    for key, shape in spec:
        if key.endswith('.weight'):
            fan[key[:-len('weight')]] = shape[1]
    for key, shape in spec:
        if key.endswith('offset'):
            stop = 100.0 if 'r_expansion' in key else 10.0             # r_max = 10 ** 2 (prop_egnn.py:12); cutoff 10
            sd[key] = torch.linspace(0.0, stop, shape[0])
            continue
        f = fan[key.rsplit('.', 1)[0] + '.']
        a = gain / np.sqrt(f) * (bias_gain if key.endswith('.bias') else 1.0)
        sd[key] = ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * a).float()
    return sd


def ligand_features(elements, seed):
    """ligand_atom_feature_full (utils/transforms_prop.py:50-67) for the given elements, with seeded aromatic / degree / NumHs /
    hybridization values (RDKit is not available to derive them)."""
    rng = np.random.RandomState(seed)
    n = len(elements)
    f = np.zeros((n, LIGAND_FEAT_DIM), np.float32)
    for i, e in enumerate(elements):
        if e in LIGAND_ELEMENTS:                 # an element outside the list (1h36's Br) has an all-zero element one-hot
            f[i, LIGAND_ELEMENTS.index(e)] = 1
        f[i, 8] = ATOMIC_NUMBER[e] / 100.
        f[i, 9] = rng.randint(2)
        f[i, 10 + rng.randint(1, 5)] = 1
        f[i, 16 + rng.randint(0, 4)] = 1
        f[i, 22 + rng.randint(1, 7)] = 1
    return f


def synthetic_complex(seed, n_protein, n_ligand, r_out):
    from targetdiff_amd import workloads
    p = workloads.synthetic_pocket(seed, n_protein, 2.5, r_out)
    rng = np.random.RandomState(seed + 1000)
    lpos = rng.normal(0, 1.5, size=(n_ligand, 3)).astype(np.float32)
    elements = [LIGAND_ELEMENTS[i] for i in rng.choice([1, 1, 1, 2, 3, 6], size=n_ligand)]
    return (np.asarray(p.pos, np.float32), np.asarray(p.feat, np.float32), lpos, ligand_features(elements, seed))


def complex_1h36(seed=0, jitter=0.0):
    """The 1h36 pocket (tests/golden/pocket_1h36.npz) with its docked ligand (ligand_1h36_docked.npz); `jitter` moves the ligand atoms
    by N(0, jitter^2) per coordinate (seeded)."""
    with np.load(os.path.join(GOLDEN, 'pocket_1h36.npz')) as z:
        ppos, pfeat = z['pos'].astype(np.float32), z['feat'].astype(np.float32)
    with np.load(os.path.join(GOLDEN, 'ligand_1h36_docked.npz')) as z:
        lpos, elements = z['pos'].astype(np.float32), [str(e) for e in z['elements']]
    if jitter:
        lpos = lpos + np.random.RandomState(seed).normal(0, jitter, size=lpos.shape).astype(np.float32)
    return ppos, pfeat, lpos, ligand_features(elements, 11)


def batch_of(complexes):
    """Concatenate (ppos, pfeat, lpos, lfeat) tuples into the reference's inputs (numpy), batch vectors sorted."""
    cat = lambda i: np.concatenate([c[i] for c in complexes]).astype(np.float32)
    bp = np.concatenate([np.full(len(c[0]), b, np.int64) for b, c in enumerate(complexes)])
    bl = np.concatenate([np.full(len(c[2]), b, np.int64) for b, c in enumerate(complexes)])
    return dict(protein_pos=cat(0), protein_feat=cat(1), ligand_pos=cat(2), ligand_feat=cat(3), batch_protein=bp, batch_ligand=bl)


def fixture_complexes():
    """The three complexes of the prop fixtures: 1h36 + docked ligand, a synthetic pocket, and one with fewer than k + 1 = 49 nodes."""
    return [complex_1h36(), synthetic_complex(301, 110, 14, 9.0), synthetic_complex(302, 24, 7, 5.0)]


def spec_of(fixture):
    return [(k, tuple(s)) for k, s in json.loads(str(fixture['state_dict_spec']))]


# ------------------------------------------------------------------------------------------ float64 restatement
def knn_table(pos32, batch, k):
    """Each node's k nearest same-complex nodes, ascending (d2, index), d2 = (dx*dx + dy*dy) + dz*dz in fp32; -1 padded."""
    N = pos32.shape[0]
    out = np.full((N, k), -1, np.int64)
    x = torch.from_numpy(np.ascontiguousarray(pos32, np.float32))
    for b in np.unique(batch):
        idx = np.nonzero(batch == b)[0]
        xs = x[idx]
        dx = xs[None, :, 0] - xs[:, None, 0]
        dy = xs[None, :, 1] - xs[:, None, 1]
        dz = xs[None, :, 2] - xs[:, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d2.fill_diagonal_(float('inf'))
        kk = min(k, len(idx) - 1)
        if kk > 0:
            order = torch.sort(d2, dim=1, stable=True).indices[:, :kk].numpy()
            out[idx, :kk] = idx[order]
    return out


def composed_order(batch_protein, batch_ligand):
    """The project's compose rule: stable sort of cat([batch_protein, batch_ligand])."""
    return np.argsort(np.concatenate([batch_protein, batch_ligand]), kind='stable')


def restate(sd, cfg, inp, output_kind=None, enc_ligand=None, enc_node=None, enc_graph=None, trace=None):
    """PropPredNet(Enc).forward in float64.  Returns dict(out, h_layers [L, N, 256], final_h, nbr, order, rbf [E, 64], out_pre [B, 256]
    = the pre-activations of out_block.0).  A list given as `trace` receives, for every ReLU, (key of the Linear before it, that
    Linear's input, its output = the ReLU's pre-activation, the ReLU's output)."""
    d = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    W = {k: v.double() for k, v in sd.items()}
    lin = lambda x, p: x @ W[p + '.weight'].T + W[p + '.bias']
    hp = lin(d(inp['protein_feat']), 'protein_atom_emb')
    lf = d(inp['ligand_feat'])
    if enc_ligand is not None:
        lf = torch.cat([lf, d(enc_ligand)], -1)
    hl = lin(lf, 'ligand_atom_emb')
    order = composed_order(inp['batch_protein'], inp['batch_ligand'])
    h = torch.cat([hp, hl])[order]
    pos32 = np.concatenate([inp['protein_pos'], inp['ligand_pos']]).astype(np.float32)[order]
    batch = np.concatenate([inp['batch_protein'], inp['batch_ligand']])[order]
    enc = cfg['encoder']
    nbr = knn_table(pos32, batch, enc['knn'])
    dst, slot = np.nonzero(nbr >= 0)
    src = nbr[dst, slot]
    pos = d(pos32)
    length = torch.linalg.norm(pos[dst] - pos[src], dim=1)
    offset = W['encoder.distance_expansion.offset']
    coeff = -0.5 / (offset[1] - offset[0]).item() ** 2
    rbf = torch.exp(coeff * (length.view(-1, 1) - offset.view(1, -1)) ** 2)
    def relu_of(x, p):
        z = lin(x, p)
        a = torch.relu(z)
        if trace is not None:
            trace.append((p, x, z, a))
        return a
    layers = []
    for l in range(enc['num_layers']):
        p = f'encoder.net.{l}.'
        m = relu_of(relu_of(torch.cat([rbf, h[dst], h[src]], -1), p + 'edge_mlp.net.0'), p + 'edge_mlp.net.2')
        e = torch.sigmoid(lin(m, p + 'edge_inf.0'))
        mi = torch.zeros_like(h).index_add_(0, torch.from_numpy(dst), m * e)
        h = h + lin(relu_of(torch.cat([mi, h], -1), p + 'node_mlp.net.0'), p + 'node_mlp.net.2')
        layers.append(h)
    if enc_node is not None:
        h = lin(relu_of(torch.cat([h, d(enc_node)], -1), 'enc_node_layer.0'), 'enc_node_layer.2')
    B = int(batch.max()) + 1
    pre = torch.zeros(B, h.shape[1], dtype=torch.float64).index_add_(0, torch.from_numpy(batch), h)
    if enc_graph is not None:
        pre = torch.cat([pre, d(enc_graph)], -1)
    out_pre = lin(pre, 'out_block.0')
    # ShiftedSoftplus (models/common.py:156-162): its shift is torch.log(torch.tensor(2.0)).item(), log 2 rounded to fp32, 1.9e-9 above
    # log 2 -- in the float64 run as well
    y = torch.nn.functional.softplus(out_pre) - float(np.float32(np.log(2.0)))
    y = lin(y, 'out_block.2')
    if output_kind is not None:
        y = y[torch.arange(B), torch.as_tensor(output_kind) - 1].view(-1, 1)
    return dict(out=y, h_layers=torch.stack(layers), final_h=h, nbr=nbr, order=order, rbf=rbf, out_pre=out_pre)


def rel_err(a, b):
    """max |a - b| / max(1, max |b|) (pooled sums over hundreds of nodes are large: a relative measure)."""
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b))))) if a.size else 0.0
