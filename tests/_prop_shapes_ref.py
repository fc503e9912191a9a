"""Binding-affinity predictor over its whole supported range: the case table of tests/test_gpu_prop_shapes.py,
tests/test_prop_shapes_host.py and tools/make_golden_prop_shapes.py.  Seeded, pure numpy / torch; the arithmetic is
_prop_ref.restate and _prop_grad_ref.restate_grads.

A case is (name, model kind, knn, num_layers, widths, complexes, geometry, loss form) plus the weights' (seed, gain, bias_gain).
  kind       'net' = PropPredNet, 'enc' = PropPredNetEnc (enc_feature_type 'full')
  widths     (enc_ligand_dim, enc_node_dim, enc_graph_dim, output_dim); the enc_* widths are 0 for 'net'
  complexes  ((n_protein, n_ligand), ...): complex b of the batch, cut from 1h36 + its docked ligand (_prop_ref.complex_1h36): the
             n_protein pocket atoms nearest to a seeded point next to the ligand, n_ligand seeded ligand atoms, all jittered.
             (0, 0) is a complex index that no atom carries.
  geometry   None, or the name of a rule in GEOMETRY that replaces the positions (features stay)
  loss       'kind' = get_loss's MSE of out[kind] against seeded y; 'up' = sum(out * U), U a seeded upstream gradient [B, O]

Which branch each group reaches is listed in DESIGN.md (affinity section).
"""
from __future__ import annotations

import collections
import functools
import zlib

import numpy as np
import torch

import _prop_grad_ref as PG
import _prop_ref as P

Case = collections.namedtuple('Case', 'name kind knn layers widths complexes geometry loss seed gain bias_gain')

TOL_GRAD = 1e-4          # tests/test_gpu_prop_train.py
LARGE = ('red_cap', 'red_scan1025', 'red_scan2049', 'red_grid')          # the fixture keeps norms and projections only


# ------------------------------------------------------------------------------------------ complexes
@functools.lru_cache(maxsize=None)
def _source():
    ppos, pfeat, lpos, lfeat = P.complex_1h36()
    return ppos, pfeat, lpos, lfeat


def cut(seed, n_protein, n_ligand):
    """(ppos, pfeat, lpos, lfeat) with exactly n_protein / n_ligand atoms, cut from 1h36 + docked ligand: seeded ligand atoms (file
    order kept), the pocket atoms nearest to a seeded point next to the ligand (file order kept), every atom moved by N(0, 0.2^2)."""
    ppos, pfeat, lpos, lfeat = _source()
    rng = np.random.RandomState(seed)
    lsel = np.sort(rng.permutation(len(lpos))[:n_ligand])
    centre = lpos.mean(0) + rng.normal(0, 2.0, size=3)
    psel = np.sort(np.argsort(np.linalg.norm(ppos - centre, axis=1), kind='stable')[:n_protein])
    jp = rng.normal(0, 0.2, size=(n_protein, 3)).astype(np.float32)
    jl = rng.normal(0, 0.2, size=(n_ligand, 3)).astype(np.float32)
    return ppos[psel] + jp, pfeat[psel], lpos[lsel] + jl, lfeat[lsel]


def _place(c, pts):
    """The complex `c` with its atoms (protein, then ligand) at the rows of `pts`."""
    ppos, pfeat, lpos, lfeat = c
    pts = np.asarray(pts, np.float32)
    assert len(pts) == len(ppos) + len(lpos)
    return pts[:len(ppos)].copy(), pfeat, pts[len(ppos):].copy(), lfeat


def _grid(n, spacing, rng):
    side = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing='ij'), -1).reshape(-1, 3).astype(np.float64) * spacing
    return g[rng.permutation(len(g))[:n]]


def geo_lattice(cs, rng):
    """complex 0 (64 atoms) on a 4 x 4 x 4 lattice at 1.5 A, atoms assigned to lattice points in seeded order: every distance is
    shared by many pairs and exact in fp32, so the k-th neighbour is decided by index."""
    return [_place(cs[0], _grid(64, 1.5, rng))] + cs[1:]


def geo_coincident(cs, rng):
    """complex 0: ligand atom 0 on protein atom 3, ligand atom 5 on ligand atom 2 (d = 0)."""
    ppos, pfeat, lpos, lfeat = cs[0]
    lpos = lpos.copy()
    lpos[0] = ppos[3]
    lpos[5] = lpos[2]
    return [(ppos, pfeat, lpos, lfeat)] + cs[1:]


def geo_sparse(cs, rng):
    """every complex on a 13 A grid, each atom moved by at most 0.4 A per coordinate: nearest-neighbour spacing >= 12.2 A."""
    out = []
    for c in cs:
        n = len(c[0]) + len(c[2])
        out.append(_place(c, _grid(n, 13.0, rng) + rng.uniform(-0.4, 0.4, size=(n, 3))))
    return out


HUB_AT = 4               # composed row (inside complex 0) of the hub atom


def _with_hub(c, shell):
    pts = np.insert(np.asarray(shell, np.float64), HUB_AT, 0.0, axis=0) + np.array([3.0, -2.0, 5.0])
    return _place(c, pts)


def geo_hub12(cs, rng):
    """complex 0 (13 atoms): the 12 vertices of an icosahedron of circumradius 3 A (edge 3.155 A) around one atom at the centre.  At
    k = 1 the centre is the only neighbour of all 12."""
    phi = (1 + 5 ** 0.5) / 2
    v = np.array([(0, s1, s2 * phi) for s1 in (-1, 1) for s2 in (-1, 1)], np.float64)
    v = np.concatenate([v, v[:, [1, 2, 0]], v[:, [2, 0, 1]]])
    v *= 3.0 / np.linalg.norm(v[0])
    return [_with_hub(cs[0], v[rng.permutation(12)])] + cs[1:]


def geo_hub220(cs, rng):
    """complex 0 (221 atoms): 220 atoms spread evenly (a Fibonacci spiral) over a sphere of radius 3 A around one atom at the centre.
    A quarter of the sphere (~55 atoms) is nearer to a sphere atom than the centre is, so at k = 64 the centre is a neighbour of
    all 220: the longest reverse-adjacency list a k <= 64 graph of this size can have."""
    n = 220
    i = np.arange(n) + 0.5
    z = 1 - 2 * i / n
    t = np.pi * (1 + 5 ** 0.5) * i
    v = 3.0 * np.stack([np.sqrt(1 - z * z) * np.cos(t), np.sqrt(1 - z * z) * np.sin(t), z], -1)
    return [_with_hub(cs[0], v[rng.permutation(n)])] + cs[1:]


GEOMETRY = dict(lattice=geo_lattice, coincident=geo_coincident, sparse=geo_sparse, hub12=geo_hub12, hub220=geo_hub220)


# ------------------------------------------------------------------------------------------ the table
# A case's seed is 3000 + its position i in the table, unless the seed rule moved it.  Candidates are the table seed, then
# 5000 + 100 t + i for t = 0 .. 23 (t up to 118 for fan_k33, fan_k63, layers_2_k48 and hub_k64, which found no seed below TOL_GRAD / 4 in
# the first 25; t up to 319 for layers_7_k48).  A candidate is admissible if the reference's fp32 gradients stay within TOL_GRAD / 2 of
# its float64 ones under every one of 1 + ORDERS evaluation orders (see ORDERS below; tools/make_golden_prop_shapes.py refuses the
# others); of the admissible ones the first with kink_exposure <= TOL_GRAD / 4 (see KINK_WINDOW below) is taken, else the one with the
# smallest exposure.  At seven layers 2 of 320 candidates are admissible (10711: r = 5.5e-6; 22411: r = 3.6e-5); the candidate with the
# smallest exposure of the first 120, 13911, is 2.0e-4 away in fp32 under one of the orders, and the GPU, one more order, was 2.2e-4 away.
RESEEDED = {'fan_k16': 5103, 'fan_k17': 5204, 'fan_k33': 6305, 'fan_k47': 5206, 'fan_k63': 5407, 'fan_k64': 7208, 'layers_1_k48': 5209,
            'layers_2_k48': 11310, 'layers_7_k48': 10711, 'rows_n32': 5120, 'widths_3_17_65_o5': 5022, 'red_1024': 5426, 'red_1025': 5027,
            'red_cap': 5528, 'red_scan1025': 5129, 'red_scan2049': 6630, 'red_grid': 5831, 'hub_k64': 10533, 'coincident_k5': 5035,
            'lattice_k48': 6637, 'coincident_k48': 5438}
# What the rule could not remove: the exposure of the seed taken (rounded up), for the cases that stay above TOL_GRAD / 4.  The window
# is a worst case: on these no unit flipped under any of the 1 + ORDERS fp32 orders, but one whose rounding does flip the most exposed
# unit moves one row of one gradient by this much.
KINK_RESIDUAL = {'fan_k33': 1.2e-4, 'fan_k63': 5.6e-5, 'layers_2_k48': 8.3e-5, 'layers_7_k48': 8.9e-4, 'red_cap': 4.2e-5, 'red_grid': 6.3e-5}


def _cases():
    t = []
    add = lambda name, kind, knn, layers, widths, complexes, geometry=None, loss='kind', seed=0, gain=1.0, bias_gain=1.0: t.append(
        Case(name, kind, knn, layers, widths, tuple(complexes), geometry, loss, RESEEDED.get(name, seed or 3000 + len(t)), gain, bias_gain))
    net = (0, 0, 0, 3)
    # ---- fan-in: one complex with fewer than k + 1 nodes, one with exactly k + 1, one with more
    for k, layers in ((1, 1), (5, 2), (15, 1), (16, 3), (17, 2), (33, 3), (47, 1), (63, 2), (64, 1)):
        below = (max(k // 2 - 2, 0), 1) if k > 1 else (1, 0)
        add(f'fan_k{k}', 'net', k, layers, net, [below, (k + 1 - min(3, k), min(3, k)), (k + 6, 4)], loss='kind' if k % 2 else 'up')
    for layers in (1, 2, 7):
        add(f'layers_{layers}_k48', 'net', 48, layers, net, [(26, 4), (45, 4), (54, 6)], loss='up' if layers == 2 else 'kind')
    # ---- rows: N in {1, 2, 3, 4, 5, 15, 16, 17, 32}, B in {1, 2, 5}
    add('rows_n1', 'net', 64, 1, net, [(1, 0)], loss='up')                                  # a lone one-node complex
    add('rows_n2', 'net', 5, 1, net, [(1, 1)])
    add('rows_n3', 'net', 5, 2, net, [(0, 1), (1, 1)], loss='up')                           # complex 0 has no protein atoms
    add('rows_n4', 'net', 1, 1, net, [(3, 1)])
    add('rows_n5', 'net', 16, 1, net, [(1, 0), (0, 1), (1, 0), (0, 1), (1, 0)], loss='up')  # no edge anywhere
    add('rows_n15', 'net', 17, 1, net, [(10, 2), (2, 1)])
    add('rows_n16', 'net', 5, 2, net, [(1, 0), (5, 2), (0, 1), (4, 2), (1, 0)], loss='up')  # first, middle, last: one node
    add('rows_n17', 'net', 15, 1, net, [(6, 2), (1, 0), (0, 0), (5, 1), (0, 2)])            # index 2: no atom at all
    add('rows_n32', 'net', 33, 2, net, [(20, 4), (7, 1)], loss='up')
    # ---- widths: K1 + K2 of the embeddings (27, 30 + El), enc_node_layer.0 (256 + En) and out_block.0 (256 + Eg)
    for (El, En, Eg, O), cx in (((1, 3, 17, 2), [(12, 3), (6, 2)]), ((3, 17, 65, 5), [(9, 2), (0, 0), (14, 3)]),
                                ((17, 65, 0, 1), [(16, 0), (5, 4)]), ((65, 0, 1, 1), [(10, 5)]), ((0, 1, 3, 2), [(0, 3), (13, 3)])):
        add(f'widths_{El}_{En}_{Eg}_o{O}', 'enc', 5 if O != 5 else 17, 2 if O == 2 else 1, (El, En, Eg, O), cx, loss='up')
    # ---- reductions (one layer): split-K chunk boundaries and cap, the scan's per, the grid-stride loop
    add('red_1024', 'net', 16, 1, net, [(50, 14)])                                          # N k = 64 * 16 = 1024: one chunk
    add('red_1025', 'net', 5, 1, net, [(120, 10), (70, 5)], loss='up')                      # N k = 205 * 5 = 1025: two chunks
    add('red_cap', 'net', 64, 1, net, [(500, 15), (500, 15)], loss='up')                    # N k = 1030 * 64 = 65920 > 65536
    add('red_scan1025', 'net', 4, 1, net, [(400, 10), (400, 10), (195, 10)])                # per = 2
    add('red_scan2049', 'net', 4, 1, net, [(400, 10)] * 4 + [(399, 10)], loss='up')         # per = 3
    add('red_grid', 'net', 4, 1, net, [(400, 10)] * 39 + [(386, 10)])                       # N = 16386 > 16384, N % 4 = 2
    # ---- hubs: one node in every other node's neighbour list
    add('hub_k1', 'net', 1, 1, net, [(10, 3), (5, 2)], 'hub12', loss='up')
    add('hub_k64', 'net', 64, 1, net, [(206, 15), (30, 4)], 'hub220')
    # ---- geometry regimes, two layers
    for k in (5, 48):
        add(f'lattice_k{k}', 'net', k, 2, net, [(56, 8), (10, 3)], 'lattice', loss='up' if k == 5 else 'kind')
        add(f'coincident_k{k}', 'net', k, 2, net, [(40, 8), (12, 3)], 'coincident', loss='kind' if k == 5 else 'up')
        add(f'sparse_k{k}', 'net', k, 2, net, [(20, 4), (6, 2)], 'sparse', loss='up' if k == 5 else 'kind')
    # ---- softplus threshold: out_block.0 pre-activations on both sides of 20 (weights at 3x, biases at 6x, as prop_grad_gain)
    add('ssp_gain3', 'net', 16, 2, net, [(30, 5), (12, 3), (3, 1)], seed=3101, gain=3.0, bias_gain=6.0)
    return collections.OrderedDict((c.name, c) for c in t)


CASES = _cases()
GAIN_CASES = ('ssp_gain3',)


# ------------------------------------------------------------------------------------------ a case's model, weights and inputs
def config(case):
    enc = dict(P.MODEL_CONFIG['encoder'], knn=case.knn, num_layers=case.layers, name='egnn' if case.kind == 'net' else 'egnn_enc')
    cfg = dict(hidden_channels=256, encoder=enc)
    if case.kind == 'enc':
        El, En, Eg, _ = case.widths
        cfg.update(enc_ligand_dim=El, enc_node_dim=En, enc_graph_dim=Eg, enc_feature_type='full')
    return cfg


def build_model(case, module):
    """PropPredNet / PropPredNetEnc of `module` (targetdiff_amd.prop, or the reference's prop_model through `wrap`)."""
    cfg, O = config(case), case.widths[3]
    if case.kind == 'net':
        return module.PropPredNet(cfg, P.PROTEIN_FEAT_DIM, P.LIGAND_FEAT_DIM, output_dim=O)
    return module.PropPredNetEnc(cfg, P.PROTEIN_FEAT_DIM, P.LIGAND_FEAT_DIM, cfg['enc_ligand_dim'], cfg['enc_node_dim'],
                                 cfg['enc_graph_dim'], cfg['enc_feature_type'], output_dim=O)


@functools.lru_cache(maxsize=None)
def spec(name):
    from targetdiff_amd import prop
    return tuple((k, tuple(v.shape)) for k, v in build_model(CASES[name], prop).state_dict().items())


def weights(case):
    return P.make_state_dict(list(spec(case.name)), case.seed, case.gain, case.bias_gain)


def complexes(case):
    cs = [cut(case.seed * 100 + b, n_p, n_l) for b, (n_p, n_l) in enumerate(case.complexes)]
    if case.geometry is not None:
        cs = GEOMETRY[case.geometry](cs, np.random.RandomState(case.seed + 7))
    return cs


def inputs(case):
    """(inp, out_kind [B] or None, y [B], enc {ligand, node, graph}, up [B, O] or None).  enc['node'] rows are in composed order."""
    inp = P.batch_of(complexes(case))
    B, (El, En, Eg, O) = len(case.complexes), case.widths
    n_l, n = len(inp['batch_ligand']), len(inp['batch_ligand']) + len(inp['batch_protein'])
    rng = np.random.RandomState(case.seed + 11)
    y = rng.normal(6.0, 1.5, size=B).astype(np.float32)
    enc = {}
    if case.kind == 'enc':
        feat = lambda rows, cols: rng.normal(size=(rows, cols)).astype(np.float32) if cols else None
        enc = {'ligand': feat(n_l, El), 'node': feat(n, En), 'graph': feat(B, Eg)}
    if case.loss == 'up':
        return inp, None, y, enc, PG.upstream(case.seed + 13, B, O)
    return inp, (1 + np.arange(B) % O).astype(np.int64), y, enc, None


def load(name):
    """(case, cfg, sd32, inp, out_kind, y, enc, up)"""
    case = CASES[name]
    return (case, config(case), weights(case)) + inputs(case)


def inputs_crc(inp, enc):
    crc = 0
    for k in sorted(inp):
        crc = zlib.crc32(np.ascontiguousarray(inp[k]).tobytes(), crc)
    for k in sorted(enc):
        if enc[k] is not None:
            crc = zlib.crc32(np.ascontiguousarray(enc[k]).tobytes(), crc)
    return np.int64(crc)


def restate(name):
    """The float64 restatement's forward of a case (with rbf and the out_block.0 pre-activations)."""
    case, cfg, sd32, inp, out_kind, y, enc, up = load(name)
    return P.restate(sd32, cfg, inp, output_kind=out_kind, enc_ligand=enc.get('ligand'), enc_node=enc.get('node'),
                     enc_graph=enc.get('graph'))


@functools.lru_cache(maxsize=4)
def restate_grads(name, order='sorted'):
    """(loss, out, {key: gradient}) of _prop_grad_ref.restate_grads for a case, computed once; `order` names a permutation of the
    atoms (PERMUTATIONS)."""
    case, cfg, sd32, inp, out_kind, y, enc, up = load(name)
    inp, enc = PERMUTATIONS[order](inp, enc)
    return PG.restate_grads(sd32, cfg, inp, out_kind, y, enc, up)


# ------------------------------------------------------------------------------------------ ReLU kinks
# A ReLU whose pre-activation z is within fp32 rounding of zero is on in one correct fp32 evaluation and off in another (a different
# order of the sum is enough); the weight gradient of that unit then differs by that one edge's (or node's) whole term, da * x.  Such a
# flip is no error of either evaluation, but it is far larger than rounding: a case in which it can exceed the bound tests nothing.
# KINK_WINDOW: z counts as "within rounding" when |z| <= KINK_WINDOW * (sum_k |W_uk x_k| + |b_u|), with KINK_WINDOW = 2 u, u = 2^-24
# the fp32 unit roundoff.  The error of a K-term fp32 dot product grows like sqrt(K) u times the terms' rms, which for K <= 576 terms
# of mixed sign is well below u times the sum of their magnitudes; 2 u leaves room for the rounding the inputs carry.  No window makes
# every case of this size free of such units (at 32 u nearly every case has one), so the rule is a choice among seeds, made on the CPU
# before any GPU run: a case takes, of its table seed and 24 fixed others, the first whose exposure is at most TOL_GRAD / 4, else the
# one with the smallest, among those whose fp32 reference run stays within r <= TOL_GRAD / 2 (RESEEDED; KINK_RESIDUAL lists what is left).
KINK_WINDOW = 2.0 ** -23


def kink_exposure(name):
    """The largest change, relative to the tensor's max |g| as the GPU test measures it, that flipping one ReLU within KINK_WINDOW
    of zero makes to a weight or bias gradient; float64, from the restatement's trace.  (exposure, key of the Linear, units near zero)."""
    case, cfg, sd32, inp, out_kind, y, enc, up = load(name)
    sd = {k: v.detach().double().requires_grad_(PG.is_param(k)) for k, v in sd32.items()}
    trace = []
    loss, _ = PG.restate_loss(sd, cfg, inp, out_kind, y, enc, up, trace=trace)
    keys = sorted({t[0] for t in trace})
    wanted = [sd[k + s] for k in keys for s in ('.weight', '.bias')] + [t[3] for t in trace]
    grads = torch.autograd.grad(loss, wanted, allow_unused=True)
    gmax = {k + s: (0.0 if g is None else float(g.abs().max())) for (k, s), g in
            zip([(k, s) for k in keys for s in ('.weight', '.bias')], grads)}
    worst, where, count = 0.0, None, 0
    for (key, x, z, a), da in zip(trace, grads[2 * len(keys):]):
        if da is None or z.numel() == 0 or gmax[key + '.weight'] == 0.0:
            continue
        with torch.no_grad():
            W, b = sd[key + '.weight'], sd[key + '.bias']
            near = z.abs() <= KINK_WINDOW * (x.abs() @ W.abs().T + b.abs())
            if not bool(near.any()):
                continue
            per_unit = torch.maximum(x.abs().max(1, keepdim=True).values / gmax[key + '.weight'],
                                     torch.full((1, 1), 1.0 / (gmax[key + '.bias'] or float('inf')), dtype=torch.float64))
            e = float((da.abs() * per_unit)[near].max())
            count += int(near.sum())
            if e > worst:
                worst, where = e, key
    return worst, where, count


# ------------------------------------------------------------------------------------------ equivalent evaluation orders
# Renumbering the 256 hidden units consistently in every weight gives the same function and the same gradients (renumbered), but every
# fp32 dot product then adds its terms in another order: one more correct fp32 evaluation of the same case.  r of the fixture is the
# largest distance from float64 over the reference's fp32 run as it is and under ORDERS such renumberings, so a seed is kept only if
# no fp32 evaluation order among them flips a ReLU that matters -- the GPU's order is one more of the same kind.
ORDERS = 8
HID = 256


def _index(key, shape, p):
    """(row index, column index or None) such that the renumbered tensor is W[rows][:, cols]."""
    ident = lambda n: np.arange(n)
    rows = p if shape[0] == HID else ident(shape[0])
    if len(shape) == 1:
        return rows, None
    n_in = shape[1]
    if key.endswith('atom_emb.weight'):
        cols = ident(n_in)
    elif key.endswith('edge_mlp.net.0.weight'):
        cols = np.concatenate([ident(n_in - 2 * HID), n_in - 2 * HID + p, n_in - HID + p])
    elif key.endswith('node_mlp.net.0.weight'):
        cols = np.concatenate([p, HID + p])
    else:                                          # 256 hidden inputs, then (enc_node_layer.0, out_block.0) the enc_* feature columns
        cols = np.concatenate([p, HID + ident(n_in - HID)])
    return rows, cols


def renumber_hidden(sd, order):
    """The state dict with its hidden units renumbered by the seeded permutation `order` (>= 1); buffers unchanged."""
    p = np.random.RandomState(900 + order).permutation(HID)
    out = {}
    for k, v in sd.items():
        if not PG.is_param(k):
            out[k] = v
            continue
        rows, cols = _index(k, tuple(v.shape), p)
        out[k] = (v[rows] if cols is None else v[rows][:, cols]).contiguous()
    return out


def original_numbering(grads, order):
    """Gradients of a renumbered model, back in the original numbering."""
    p = np.random.RandomState(900 + order).permutation(HID)
    out = {}
    for k, g in grads.items():
        rows, cols = _index(k, tuple(g.shape), p)
        o = torch.zeros_like(g)
        if cols is None:
            o[rows] = g
        else:
            o[torch.as_tensor(rows)[:, None], torch.as_tensor(cols)[None, :]] = g
        out[k] = o
    return out


# ------------------------------------------------------------------------------------------ permutations of the atoms
def _permuted(inp, enc, pp, lp):
    out = dict(protein_pos=inp['protein_pos'][pp], protein_feat=inp['protein_feat'][pp], batch_protein=inp['batch_protein'][pp],
               ligand_pos=inp['ligand_pos'][lp], ligand_feat=inp['ligand_feat'][lp], batch_ligand=inp['batch_ligand'][lp])
    e = dict(enc)
    if e.get('ligand') is not None:
        e['ligand'] = e['ligand'][lp]
    if e.get('node') is not None:
        # enc_node_feature rows follow the composed order: the row of composed position c of the permuted batch is the row the same
        # atom had in the sorted batch
        n_p = len(pp)
        atom = np.concatenate([pp, n_p + lp])[P.composed_order(out['batch_protein'], out['batch_ligand'])]
        e['node'] = e['node'][np.argsort(P.composed_order(inp['batch_protein'], inp['batch_ligand']))[atom]]
    return out, e


def shuffled(inp, enc):
    """`unsorted` of tests/test_gpu_prop_train.py: protein and ligand atoms in seeded random order, across and inside complexes.  The
    composed order inside a complex changes with it, and so do the order of every sum and the index that decides a k-NN tie."""
    r = np.random.RandomState(13)
    return _permuted(inp, enc, r.permutation(len(inp['batch_protein'])), r.permutation(len(inp['batch_ligand'])))


def _interleave(batch, r):
    """A permutation that mixes the complexes but keeps every complex's atoms in their order."""
    mixed = batch[r.permutation(len(batch))]
    out = np.empty(len(batch), np.int64)
    for b in np.unique(batch):
        out[mixed == b] = np.nonzero(batch == b)[0]
    return out


def interleaved(inp, enc):
    """The atoms of different complexes interleaved (unsorted batch vectors), every complex's own atoms still in their order: the
    composed batch, and so every bit of the result, is that of the sorted batch."""
    r = np.random.RandomState(13)
    return _permuted(inp, enc, _interleave(inp['batch_protein'], r), _interleave(inp['batch_ligand'], r))


PERMUTATIONS = dict(sorted=lambda inp, enc: (inp, enc), shuffled=shuffled, interleaved=interleaved)


# ------------------------------------------------------------------------------------------ the fixture's per-case entries
def summarize(case, grads):
    """{key: gradient} -> (keys, norm [P], proj [P, 16]) in the model's parameter order (PG.directions)."""
    keys = [k for k, _ in spec(case.name) if PG.is_param(k)]
    norm = np.array([float(grads[k].detach().double().norm()) for k in keys], np.float64)
    proj = np.stack([(PG.directions(k, grads[k].shape) @ grads[k].detach().double().reshape(-1)).numpy() for k in keys])
    return keys, norm, proj


def distance(g32, g64):
    """r of tools/make_golden_prop_grad.py: the largest of |norm32 - norm64| / norm64, max |proj32 - proj64| / norm64 and, for tensors
    of at most PG.SMALL elements, max |g32 - g64| / max |g64|, over the tensors whose float64 gradient is not zero."""
    r = 0.0
    for k, a in g64.items():
        a, b = a.detach().double().reshape(-1), g32[k].detach().double().reshape(-1)
        n = float(a.norm())
        if n == 0.0:
            continue
        d = PG.directions(k, a.shape)
        r = max(r, abs(float(b.norm()) - n) / n, float((d @ b - d @ a).abs().max()) / n)
        if a.numel() <= PG.SMALL:
            r = max(r, float((a - b).abs().max() / a.abs().max()))
    return r
