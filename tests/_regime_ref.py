"""Input regimes for the attention and EGNN layers, and the rule that compares a HIP result with float64 (pure CPU, deterministic).

The parity tests elsewhere vary weights, graph modes, pack shapes and session state; the data the kernels read is always unit-scale features on a
Gaussian cloud.  Here the DATA varies: feature scale (tiny, large, one scale per row, exact zeros, one spiking channel), geometry (every neighbour
beyond the last Gaussian centre, coincident atoms as real edges, coordinates 500 A from the origin, a lattice with exact distance ties) and the
sharpness of the attention (the last Linear of the query MLPs times s).  Every expected value is oracle/restatement.py in float64.

The pack is fixed: (protein, ligand) sizes (1,1), (3,2), (20,14), (60,12), (5,40) in compose order (per graph the protein rows, then the ligand
rows), 158 nodes: rows with a single in-edge, rows with fewer than k in-edges, full rows at k = 32, rows of two chunks at k = 48, a ligand-heavy
graph.

The comparison rule is the one of tests/test_gpu_weight_regimes.py: with r64 = max |restatement fp32 - restatement float64| and
d64 = max |HIP - float64|, pass when d64 <= max(floor, factor * r64), floor = TOL_FWD, factor = 2.  Where the input rows differ by orders of
magnitude (`large`, `mixed`) the rule is applied per decade of the input row's max |h| and 2^-22 * (the group's max |h|) is added to the floor:
one rounding of the fp32 result h + update, with a factor 4 of slack.
"""
import functools
import math

import numpy as np
import torch

from _tol import TOL_FWD, close, maxdiff

SIZES = ((1, 1), (3, 2), (20, 14), (60, 12), (5, 40))
BIG = 3                                   # the 72-node graph
FEATURES = ('unit', 'tiny', 'large', 'mixed', 'zero', 'spike')
GEOMETRIES = ('cloud', 'far', 'coincident', 'offset', 'lattice')
SHARPNESS = (1, 30, 300)
GRAPHS = {'knn32': {}, 'knn48': {'knn': 48}, 'hybrid': {'cutoff_mode': 'hybrid'}}
VARIANTS = ((1, 1, 1), (1, 0, 1), (1, 0, 0), (0, 0, 0))        # (edge_key_split, edge_first_layer_f16, edge_second_layer_f16)
FAR_SCALE = 16.0                        # at x 8 the cloud's closest ligand pair of the 72-node graph is still 6.2 A apart; at x 16, 12.3 A
LAST_CENTRE = 10.0                        # A, the last Gaussian centre of the distance expansion

# 6 feature regimes on the cloud, the 4 other geometries at unit scale, 2 sharpened models on 3 inputs: 16, not the cross product
CASES = tuple([(f, 'cloud', 1) for f in FEATURES] + [('unit', g, 1) for g in GEOMETRIES[1:]]
              + [(f, g, s) for s in SHARPNESS[1:] for f, g in (('unit', 'cloud'), ('unit', 'coincident'), ('mixed', 'cloud'))])
GROUPED = ('large', 'mixed')              # feature regimes whose h is compared per decade of the input rows


def case_id(case):
    return '%s-%s-s%d' % case


# ------------------------------------------------------------------------------------------ the pack
class Pack:
    def __init__(self, sizes=SIZES, big=BIG):
        self.sizes, self.big = tuple(sizes), big
        mask, batch, ptr = [], [], [0]
        for g, (n_p, n_l) in enumerate(self.sizes):
            mask += [False] * n_p + [True] * n_l
            batch += [g] * (n_p + n_l)
            ptr.append(ptr[-1] + n_p + n_l)
        self.mask = torch.tensor(mask)
        self.batch = torch.tensor(batch)
        self.ptr = ptr
        self.N = ptr[-1]

    def protein_rows(self, g):
        return range(self.ptr[g], self.ptr[g] + self.sizes[g][0])

    def ligand_rows(self, g):
        return range(self.ptr[g] + self.sizes[g][0], self.ptr[g + 1])

    def split(self, x):
        """(protein rows, protein batch, ligand rows, ligand batch) of a composed [N, ...] tensor"""
        return x[~self.mask], self.batch[~self.mask], x[self.mask], self.batch[self.mask]


PACK = Pack()
EGNN_PACK = Pack((SIZES[BIG], SIZES[0]), big=0)          # the EGNN layer: the 72-node graph and the (1, 1) graph
EGNN_FEATURES = ('unit', 'tiny', 'large')                # `large` at x 1e2 there: outputs of about 5e2, finite


# ------------------------------------------------------------------------------------------ regimes
def features(regime, pack=PACK, seed=11, large=1e3):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(pack.N, 128, generator=g)
    if regime == 'unit':
        return h
    if regime == 'tiny':
        return h * 1e-6
    if regime == 'large':
        return h * large
    if regime == 'mixed':                  # one scale per row, log-uniform over nine decades, shuffled
        e = torch.linspace(-6.0, 3.0, pack.N, dtype=torch.float64)[torch.randperm(pack.N, generator=g)]
        return h * (10.0 ** e).float().unsqueeze(1)
    if regime == 'zero':                   # every third row, and the whole (1, 1) graph
        h[::3] = 0.0
        h[pack.ptr[0]:pack.ptr[1]] = 0.0
        return h
    if regime == 'spike':
        h = h * 0.01
        h[:, 7] = 50.0
        return h
    raise ValueError(regime)


def zero_rows(pack=PACK):
    rows = set(range(0, pack.N, 3)) | set(range(pack.ptr[0], pack.ptr[1]))
    return sorted(rows)


def _cloud(pack, seed):
    g = torch.Generator().manual_seed(seed)
    xs = []
    for n_p, n_l in pack.sizes:
        xs += [torch.randn(n_p, 3, generator=g) * 4.0, torch.randn(n_l, 3, generator=g) * 1.5]
    return torch.cat(xs)


def _lattice(pack, seed):
    """1.5 A cubic lattice, protein atoms on lattice points, ligand atoms on body centres (multiples of 0.75 A: exact in fp32, so distances tie exactly)"""
    g = torch.Generator().manual_seed(seed)
    xs = []
    for n_p, n_l in pack.sizes:
        m = max(2, math.ceil(max(n_p, n_l) ** (1.0 / 3.0) - 1e-9))
        grid = torch.stack(torch.meshgrid(*[torch.arange(m)] * 3, indexing='ij'), -1).reshape(-1, 3).float()
        c = (m - 1) / 2.0
        xs += [(grid[torch.randperm(m ** 3, generator=g)[:n_p]] - c) * 1.5, (grid[torch.randperm(m ** 3, generator=g)[:n_l]] + 0.5 - c) * 1.5]
    return torch.cat(xs)


def coincident_pairs(pack=PACK):
    """(moved row, row it is put on): ligand on ligand, ligand on protein, protein on protein, all in the 72-node graph"""
    p, l = pack.protein_rows(pack.big), pack.ligand_rows(pack.big)
    return ((l[1], l[0]), (l[2], p[0]), (p[2], p[1]))


def geometry(regime, pack=PACK, seed=5):
    if regime == 'lattice':
        return _lattice(pack, seed)
    x = _cloud(pack, seed)
    if regime == 'cloud':
        return x
    if regime == 'far':
        return x * FAR_SCALE
    if regime == 'offset':
        return x + 500.0
    if regime == 'coincident':
        for a, b in coincident_pairs(pack):
            x[a] = x[b]
        return x
    raise ValueError(regime)


def sharpened(sd, s):
    """the query MLPs' last Linear (weight and bias) times s: logits s times as large, same keys and values"""
    if s == 1:
        return sd
    out = dict(sd)
    for k, v in sd.items():
        if ('.hq_func.net.3.' in k) or ('.xq_func.net.3.' in k):
            out[k] = v * float(s)
    return out


@functools.lru_cache(maxsize=None)
def base_state_dict():
    from oracle import weights
    return weights.make_state_dict(2021)


def layer_config(graph, num_layers=1):
    from oracle import weights
    return dict(weights.DEFAULT_MODEL_CONFIG, num_layers=num_layers, **GRAPHS[graph])


# ------------------------------------------------------------------------------------------ references
@functools.lru_cache(maxsize=None)
def refine_reference(case, graph):
    """One attention layer (num_layers = 1) in fp32 and float64 on the same graph; computed once per (case, graph), never modified."""
    from oracle import restatement as R
    feat, geom, s = case
    sd = sharpened(base_state_dict(), s)
    h, x = features(feat), geometry(geom)
    out = {'h': h, 'x': x, 'sd': sd, 'cfg': layer_config(graph)}
    for name, dtype in (('f32', torch.float32), ('f64', torch.float64)):
        col = {}
        for fix_x in (False, True):
            o = R.refine_forward(sd, out['cfg'], h, x, PACK.mask, PACK.batch, fix_x=fix_x, dtype=dtype, collect=None if fix_x else col)
            out[name + ('_fix' if fix_x else '')] = o
        out[name + '_nbr'], out[name + '_ew'] = col['nbr'], col['e_w']
    return out


def edge_lengths(x, nbr):
    """float64 lengths of the table's edges; pads are nan"""
    x = x.double()
    d = (x.unsqueeze(1) - x[nbr.clamp(min=0)]).norm(dim=-1)
    return torch.where(nbr >= 0, d, torch.full_like(d, float('nan')))


def layer0_logits(sd, cfg, h, x, nbr, mask, dtype=torch.float64):
    """the x2h logits of layer 0 [N, k, heads], recomputed from the restatement's pieces; pads are nan"""
    from oracle import restatement as R
    p = 'refine_net.base_block.0'
    heads = cfg['n_heads']
    dh = cfg['hidden_dim'] // heads
    h, x = h.to(dtype), x.to(dtype)
    etype = R.edge_types(nbr, mask)
    dist = (x.unsqueeze(1) - x[nbr.clamp(min=0)]).norm(dim=-1)
    gfeat = R.gaussian_smearing(dist, sd[f'{p}.distance_expansion.offset'].to(dtype))
    kv = R._kv_input(h, nbr, etype, gfeat, slice(0, h.shape[0]))
    kk = R._mlp(sd, f'{p}.x2h_layers.0.hk_func', kv, dtype).view(h.shape[0], nbr.shape[1], heads, dh)
    q = R._mlp(sd, f'{p}.x2h_layers.0.hq_func', h, dtype).view(h.shape[0], 1, heads, dh)
    lg = (q * kk / math.sqrt(dh)).sum(-1)
    return torch.where((nbr >= 0).unsqueeze(-1), lg, torch.full_like(lg, float('nan'))), q.reshape(h.shape[0], -1)


# ------------------------------------------------------------------------------------------ the rule
def decade_groups(h_in):
    """rows of the input grouped by the decade of their max |h|: {decade or None for an all-zero row: (row indices, the group's max |h|)}"""
    m = h_in.detach().cpu().double().abs().amax(dim=1)
    groups = {}
    for i, v in enumerate(m.tolist()):
        groups.setdefault(None if v == 0.0 else math.floor(math.log10(v)), []).append(i)
    return {d: (torch.tensor(rows), float(m[rows].max())) for d, rows in groups.items()}


def _cpu(t):
    return t.detach().cpu() if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))


def figures(f32, f64, h_in=None, factor=2.0, floor=TOL_FWD):
    """[(decade or None, rows, floor, r64, tolerance)] of the rule: one entry, or one per decade group of `h_in`"""
    f32, f64 = _cpu(f32), _cpu(f64)
    if h_in is None:
        parts = [(None, slice(None), floor)]
    else:
        parts = [(d, rows, floor + 2.0 ** -22 * gmax) for d, (rows, gmax) in sorted(decade_groups(h_in).items(), key=lambda kv: (kv[0] is None, kv[0]))]
    out = []
    for d, rows, fl in parts:
        r64 = maxdiff(f32[rows], f64[rows])
        out.append((d, rows, fl, r64, max(fl, factor * r64)))
    return out


def check(got, f32, f64, what, h_in=None, factor=2.0, floor=TOL_FWD):
    """d64 <= max(floor, factor * r64) through _tol.close; with `h_in` per decade group of the input rows, the floor raised by 2^-22 * the group's
    max |h|.  A float64 result that is not finite, or a result that is not finite where the float64 one is, fails outright.  Returns the
    largest d64 / max(r64, floor / factor) it saw (the `ratio to the fp32 restatement's own error`, floored so that it stays finite)."""
    got, f32, f64 = _cpu(got), _cpu(f32), _cpu(f64)
    assert got.shape == f64.shape == f32.shape, (what, got.shape, f32.shape, f64.shape)
    assert bool(torch.isfinite(f64).all()), (what, 'the float64 reference is not finite')
    assert bool(torch.isfinite(got).all()), (what, 'not finite where the float64 reference is')
    if got.numel() == 0:
        return 0.0
    worst = 0.0
    for d, rows, fl, r64, tol in figures(f32, f64, h_in, factor, floor):
        d64 = close(got[rows], f64[rows], tol, what if h_in is None else (what, 'decade', d))
        worst = max(worst, d64 / max(r64, fl / factor))
    return worst


@functools.lru_cache(maxsize=None)
def egnn_reference(feat, geom):
    """One EGNN layer (it rebuilds its graph per layer) in fp32 and float64."""
    from oracle import restatement as R
    from oracle import weights
    sd = weights.make_egnn_state_dict(2021, num_layers=1)
    P = EGNN_PACK
    h, x = features(feat, P, large=1e2), geometry(geom, P)
    out = {'h': h, 'x': x, 'sd': sd}
    for name, dtype in (('f32', torch.float32), ('f64', torch.float64)):
        col = {}
        out[name] = R.egnn_forward(sd, h, x, P.mask, P.batch, num_layers=1, k=32, dtype=dtype, collect=col)
        out[name + '_nbr'] = col['nbr'][0]
    return out


def model_inputs(geom, pack=PACK, seed=77):
    """The pack through the whole model: one-hot protein features (an element of 6 and a residue of 20), random ligand types, positions as given."""
    g = torch.Generator().manual_seed(seed)
    x = geometry(geom, pack)
    ppos, pb, lpos, lb = pack.split(x)
    pv = torch.zeros(len(pb), 27)
    pv[torch.arange(len(pb)), torch.randint(0, 6, (len(pb),), generator=g)] = 1.0
    pv[torch.arange(len(pb)), 6 + torch.randint(0, 20, (len(pb),), generator=g)] = 1.0
    lv = torch.randint(0, 13, (len(lb),), generator=g)
    return ppos.contiguous(), pv, pb, lpos.contiguous(), lv, lb


@functools.lru_cache(maxsize=None)
def model_reference(geom):
    from oracle import restatement as R
    inp = model_inputs(geom)
    return {name: R.model_forward(base_state_dict(), None, *inp, dtype=dtype) for name, dtype in (('f32', torch.float32), ('f64', torch.float64))}
