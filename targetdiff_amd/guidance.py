"""Pocket-clash guidance of the sampler ("Clash guidance"; the reference has no such mode).

Every denoise step shifts the denoiser's predicted ligand ``x0`` out of the protein atoms' contact spheres before the posterior update
uses it:

    E_g = 1/2 sum_i sum_j max(0, sigma_j - d_ij)^2,   d_ij = |x0_i - p_j|        (graph g: its ligand atoms i, its protein atoms j)
    D_i = -w grad E_g = w sum_j max(0, sigma_j - d_ij) (x0_i - p_j) / d_ij       (pairs with d_ij < 1e-6 add nothing)

``D_i`` is scaled to length ``max_shift`` when it is longer, and the step uses ``fl32(x0_i + D_i)``.  No network gradient is involved.
The arithmetic runs in libtargetdiff_hip.so (csrc/guidance.hip); this module holds the setting, its checks and thin wrappers.

    from targetdiff_amd.guidance import ClashGuidance, clash_report
    out = model.sample_diffusion(..., guidance=ClashGuidance(radius=3.0))
    count, energy, min_dist = clash_report(protein_pos, batch_protein, out['pos'], batch_ligand, radius=3.0)
"""
from __future__ import annotations

import math

import torch

# Defaults (DESIGN.md section 3 gives the reasoning; none of them is a measurement of sample quality):
DEFAULT_RADIUS = 3.0        # Angstrom: below the 3.4 A sum of two carbon van-der-Waals radii, at the short end of heavy-atom contacts
DEFAULT_WEIGHT = 1.0        # one isolated overlapping pair is resolved exactly by one shift
DEFAULT_MAX_SHIFT = 1.0     # Angstrom: less than a covalent bond, so no single step tears a ligand apart


class ClashGuidance:
    """Setting of the clash guidance: ``radius`` -- one contact radius (float, Angstrom) for every protein atom, or a 1-D tensor with
    one radius per protein atom of the call it is passed to; ``weight`` -- w >= 0 (0 computes the shift and adds zeros);
    ``max_shift`` -- cap on the length of one atom's shift per step in Angstrom (0: no cap).  Raises ValueError for anything else."""

    def __init__(self, radius=DEFAULT_RADIUS, weight=DEFAULT_WEIGHT, max_shift=DEFAULT_MAX_SHIFT):
        if torch.is_tensor(radius):
            if radius.dim() != 1 or not radius.is_floating_point():
                raise ValueError(f'radius must be a float or a 1-D floating-point tensor [N_p] (got shape {tuple(radius.shape)}, {radius.dtype})')
            if radius.numel() and not bool((torch.isfinite(radius) & (radius > 0)).all()):
                raise ValueError('every contact radius must be finite and > 0')
            self.radius = radius.detach().to(torch.float32)
        else:
            if isinstance(radius, bool) or not isinstance(radius, (int, float)):
                raise ValueError(f'radius must be a float or a 1-D tensor, got {type(radius).__name__}')
            if not (math.isfinite(radius) and radius > 0):
                raise ValueError(f'radius must be finite and > 0 (got {radius})')
            self.radius = float(radius)
        for name, val in (('weight', weight), ('max_shift', max_shift)):
            if isinstance(val, bool) or not isinstance(val, (int, float)) or not math.isfinite(val) or val < 0:
                raise ValueError(f'{name} must be a finite number >= 0 (got {val!r})')
        self.weight, self.max_shift = float(weight), float(max_shift)

    def __repr__(self):
        r = self.radius if isinstance(self.radius, float) else f'tensor[{self.radius.numel()}]'
        return f'ClashGuidance(radius={r}, weight={self.weight}, max_shift={self.max_shift})'

    @property
    def per_atom(self) -> bool:
        return torch.is_tensor(self.radius)

    def radii(self, num_protein_atoms: int, device=None) -> torch.Tensor:
        """The [N_p] fp32 radii for a call with ``num_protein_atoms`` protein atoms."""
        if self.per_atom:
            if self.radius.numel() != int(num_protein_atoms):
                raise ValueError(f'guidance has {self.radius.numel()} radii, the call has {int(num_protein_atoms)} protein atoms')
            return self.radius.to(device).contiguous()
        return torch.full((int(num_protein_atoms),), self.radius, dtype=torch.float32, device=device)

    def replicated(self, num_pocket_atoms: int, num_samples: int) -> 'ClashGuidance':
        """For a pack of ``num_samples`` copies of one pocket (sample_diffusion_ligand): a scalar radius serves any pack as it is,
        one radius per atom of the pocket is repeated per sample."""
        if not self.per_atom:
            return self
        if self.radius.numel() != int(num_pocket_atoms):
            raise ValueError(f'guidance has {self.radius.numel()} radii, the pocket has {int(num_pocket_atoms)} atoms')
        return ClashGuidance(self.radius.repeat(int(num_samples)), self.weight, self.max_shift)

    @classmethod
    def parse(cls, text: str) -> 'ClashGuidance':
        """``RADIUS[:WEIGHT[:MAX_SHIFT]]`` (tools/batch_sample.py --clash-guidance); missing fields take the defaults."""
        parts = str(text).split(':')
        if not 1 <= len(parts) <= 3:
            raise ValueError(f'clash guidance is RADIUS[:WEIGHT[:MAX_SHIFT]], got {text!r}')
        try:
            vals = [float(p) for p in parts]
        except ValueError:
            raise ValueError(f'clash guidance is RADIUS[:WEIGHT[:MAX_SHIFT]] in numbers, got {text!r}') from None
        return cls(*vals)


def check_guidance(guidance, num_protein_atoms: int, unsorted_ligand: bool):
    """Argument checks of the ``guidance`` keyword (ScorePosNet3D.sample_diffusion); None when none was given."""
    if guidance is None:
        return None
    if not isinstance(guidance, ClashGuidance):
        raise ValueError(f'guidance must be a targetdiff_amd.guidance.ClashGuidance, got {type(guidance).__name__}')
    if guidance.per_atom and guidance.radius.numel() != int(num_protein_atoms):
        raise ValueError(f'guidance has {guidance.radius.numel()} radii, the call has {int(num_protein_atoms)} protein atoms')
    if unsorted_ligand:
        raise ValueError('guidance with an unsorted batch_ligand: that path keeps its state in input order and has no guided form')
    return guidance


def _packed(protein_pos, batch_protein, pos, batch_ligand, radius):
    from . import capi
    if batch_protein.numel() > 1 and bool((batch_protein[1:] < batch_protein[:-1]).any()) or \
            batch_ligand.numel() > 1 and bool((batch_ligand[1:] < batch_ligand[:-1]).any()):
        raise ValueError('batch_protein / batch_ligand must be sorted by graph id (PyG batch vectors are)')
    B = 0
    for b in (batch_protein, batch_ligand):
        if b.numel():
            B = max(B, int(b.max().item()) + 1)
    g = radius if isinstance(radius, ClashGuidance) else ClashGuidance(radius, 0.0, 0.0)
    sigma = g.radii(protein_pos.shape[0], protein_pos.device)
    pptr = capi.graph_ptr(batch_protein.contiguous(), B)
    lptr = capi.graph_ptr(batch_ligand.contiguous(), B)
    return protein_pos.contiguous().float(), sigma, pptr, lptr, pos.contiguous().float()


def clash_shift(protein_pos, batch_protein, pos, batch_ligand, radius=DEFAULT_RADIUS, weight=DEFAULT_WEIGHT,
                max_shift=DEFAULT_MAX_SHIFT) -> torch.Tensor:
    """The shift [N_l, 3] the guidance would add to the points ``pos`` (td_clash_shift).  ``protein_pos`` and ``pos`` share a frame;
    ``batch_*`` are sorted graph ids; ``radius`` as in :class:`ClashGuidance`."""
    from . import capi
    ClashGuidance(1.0, weight, max_shift)           # the checks of the two numbers
    return capi.clash_shift(*_packed(protein_pos, batch_protein, pos, batch_ligand, radius), weight=weight, max_shift=max_shift)


def clash_report(protein_pos, batch_protein, pos, batch_ligand, radius=DEFAULT_RADIUS):
    """What a user asks of finished poses (td_clash_report): per graph ``(count, energy, min_dist)`` -- the number of protein-ligand
    pairs closer than the protein atom's radius ([B] int32), the energy E_g ([B] fp32) and the smallest protein-ligand distance
    ([B] fp32, inf for a graph without pairs).  ``protein_pos`` and ``pos`` share a frame (the sampler returns de-centred poses:
    pass the pocket as it was given)."""
    from . import capi
    return capi.clash_report(*_packed(protein_pos, batch_protein, pos, batch_ligand, radius))
