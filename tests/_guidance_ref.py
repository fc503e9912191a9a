"""Clash guidance ("Clash guidance"): plain-torch statements of the rule (TEST INFRASTRUCTURE).  The reference has
no such mode; the yardstick is the energy itself in float64 with autograd.

    E_g = 1/2 sum_i sum_j max(0, sigma_j - d_ij)^2,   d_ij = |x_i - p_j|                  (i: ligand atoms, j: protein atoms of graph g)
    D_i = -w grad_{x_i} E_g = w sum_j max(0, sigma_j - d_ij) (x_i - p_j) / d_ij           (pairs with d_ij < 1e-6 add nothing)
    |D_i| > max_shift > 0:  D_i <- D_i max_shift / |D_i|

Everything here takes ONE graph (protein [P,3], sigma [P], points [L,3]); `per_graph` walks a pack.
"""
import torch

D_MIN = 1e-6


def energy(protein, sigma, x):
    """E_g in the dtype of its inputs (use float64), differentiable in x"""
    if protein.shape[0] == 0 or x.shape[0] == 0:
        return x.sum() * 0
    d = (x[:, None, :] - protein[None, :, :]).pow(2).sum(-1).sqrt()
    return 0.5 * (sigma[None, :] - d).clamp(min=0).pow(2).sum()


def shift_autograd(protein, sigma, x, w=1.0):
    """-w grad E by autograd, float64.  (sqrt has no gradient at d = 0: callers keep coincident pairs out of this one.)"""
    xx = x.double().clone().requires_grad_(True)
    e = energy(protein.double(), sigma.double(), xx)
    (g,) = torch.autograd.grad(e, xx, allow_unused=True)
    return torch.zeros_like(xx) if g is None else -w * g


def cap(delta, max_shift):
    if not max_shift > 0:
        return delta
    n = delta.pow(2).sum(-1, keepdim=True).sqrt()
    scale = torch.where(n > max_shift, max_shift / n.clamp(min=1e-300 if delta.dtype == torch.float64 else 1e-30), torch.ones_like(n))
    return delta * scale


def shift_closed(protein, sigma, x, w=1.0, max_shift=0.0, dtype=torch.float64):
    """the closed form in `dtype` (float64: the yardstick; float32: the error any plain fp32 evaluation makes)"""
    p, s, x = protein.to(dtype), sigma.to(dtype), x.to(dtype)
    if p.shape[0] == 0 or x.shape[0] == 0:
        return torch.zeros_like(x)
    diff = x[:, None, :] - p[None, :, :]
    d = diff.pow(2).sum(-1).sqrt()
    pen = (s[None, :] - d).clamp(min=0)
    f = torch.where(d >= D_MIN, pen / d.clamp(min=D_MIN), torch.zeros_like(d))
    return cap(w * (f[..., None] * diff).sum(1), max_shift)


def report(protein, sigma, x, dtype=torch.float64):
    """(pairs with d < sigma, E_g, min d) of one graph; min d = inf without pairs"""
    p, s, x = protein.to(dtype), sigma.to(dtype), x.to(dtype)
    if p.shape[0] == 0 or x.shape[0] == 0:
        return 0, 0.0, float('inf')
    d = (x[:, None, :] - p[None, :, :]).pow(2).sum(-1).sqrt()
    pen = (s[None, :] - d).clamp(min=0)
    return int((d < s[None, :]).sum()), float(0.5 * pen.pow(2).sum()), float(d.min())


def min_gap(protein, sigma, x):
    """smallest | d_ij - sigma_j | in float64: counts are exact for inputs that keep this above 1e-4"""
    if protein.shape[0] == 0 or x.shape[0] == 0:
        return float('inf')
    d = (x.double()[:, None, :] - protein.double()[None, :, :]).pow(2).sum(-1).sqrt()
    return float((d - sigma.double()[None, :]).abs().min())


def per_graph(fn, protein, sigma, pptr, x, lptr, *a, **k):
    """fn on every graph of a pack (pptr / lptr: python lists of prefix offsets); returns the list of results"""
    return [fn(protein[pptr[g]:pptr[g + 1]], sigma[pptr[g]:pptr[g + 1]], x[lptr[g]:lptr[g + 1]], *a, **k) for g in range(len(pptr) - 1)]


# ------------------------------------------------------------------------------------------ the pack of the kernel test
def make_pack(tile, seed=20261, max_shift=1.0):
    """One pack of 4 graphs for tests/test_gpu_guidance.py: protein sizes {1, tile - 1, tile, tile + 77}, ligand sizes {0, 1, 5, 37}
    in this pairing, so that every tile boundary has ligand atoms to go wrong on and the empty ligand sits beside a one-atom protein.
    Proteins fill a ball at about 0.035 atoms / A^3 (a radius-3.25 sphere then holds about five of them), radii are drawn in
    [2.5, 4] A, ligand points lie in the inner half of the ball.  Graph 3 (two tiles) holds three special atoms: `coincident` sits on a protein
    atom of the second tile, `outside` lies 0.01 A beyond every contact sphere (its shift is exactly zero), `capped` has the longest uncapped shift of
    its graph (above `max_shift`).  Ligand points are redrawn until no d_ij is within 1e-4 A of sigma_j (float64), so that the
    pair counts do not hang on a rounding.  Everything is fp32 on return; offsets are python lists."""
    g = torch.Generator().manual_seed(seed)
    psizes, lsizes = [1, tile - 1, tile, tile + 77], [0, 1, 5, 37]
    prot, sig, lig = [], [], []

    def ball(n, radius):
        u = torch.randn(n, 3, generator=g, dtype=torch.float64)
        u = u / u.norm(dim=-1, keepdim=True)
        return u * radius * torch.rand(n, 1, generator=g, dtype=torch.float64).pow(1.0 / 3.0)

    for P, L in zip(psizes, lsizes):
        R = max(2.0, (3.0 * P / (4.0 * 3.141592653589793 * 0.035)) ** (1.0 / 3.0))
        p = ball(P, R).float()
        s = (2.5 + 1.5 * torch.rand(P, generator=g, dtype=torch.float64)).float()
        x = ball(L, 0.5 * R).float()
        for _ in range(100):
            if L == 0:
                break
            d = (x.double()[:, None, :] - p.double()[None, :, :]).pow(2).sum(-1).sqrt()
            bad = ((d - s.double()[None, :]).abs() < 2e-4).any(dim=1)
            if not bool(bad.any()):
                break
            x[bad] = ball(int(bad.sum()), 0.5 * R).float()
        prot.append(p); sig.append(s); lig.append(x)
    special = {}
    p, s, x = prot[3], sig[3], lig[3]
    x[3] = p[tile + 5]                                                                        # d = 0 exactly
    x[7] = torch.tensor([float((p[:, 0].double() + s.double()).max()) + 0.01, 0.0, 0.0])      # x - p_jx >= sigma_j + 0.01 for every j
    raw = shift_closed(p, s, x, 1.0, 0.0).norm(dim=-1)
    l0 = sum(lsizes[:3])
    special = dict(graph=3, coincident=l0 + 3, coincident_protein=sum(psizes[:3]) + tile + 5, outside=l0 + 7, capped=l0 + int(raw.argmax()))
    pptr = [0]
    lptr = [0]
    for P, L in zip(psizes, lsizes):
        pptr.append(pptr[-1] + P)
        lptr.append(lptr[-1] + L)
    return dict(protein=torch.cat(prot).contiguous(), sigma=torch.cat(sig).contiguous(), x=torch.cat(lig).contiguous(), pptr=pptr,
                lptr=lptr, special=special, max_shift=max_shift)
