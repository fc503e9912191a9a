"""Sampling time programs: which noise levels the sampler visits, and in which direction ("Time programs").

A level is ``l`` in ``{-1, 0, ..., T-1}``; ``-1`` is clean data.  A program is a list of steps, each either

* DENOISE ``t -> s`` with ``s < t``: one denoiser call at time ``t`` and a draw from the posterior ``q(x_s | x_t, x_0)`` that is exact
  for the pair ``(t, s)``, positions and categorical types alike; or
* RENOISE ``s -> t`` with ``t > s``: no denoiser call, a draw from the forward process ``q(x_t | x_s)`` (the resampling jump of
  RePaint, one draw for the whole jump).

The reference's sampler (models/molopt_score_model.py:633-703) is the program ``T-1 -> T-2 -> ... -> -1`` of unit DENOISE steps, and
a program of unit steps reproduces it bit for bit: those slots take the model's own per-``t`` table entries.  Every other slot's
coefficients are computed here in float64 from the model's float64 schedule tables and rounded to fp32 once (``TimeProgram.tables``),
the way the reference's constructor rounds its tables (:248-267).

Sample QUALITY under strides or jumps is not assessed anywhere in this project (the tree holds no trained weights); what is checked
is that each step computes the stated distribution's draw.
"""
from __future__ import annotations

import numpy as np

DENOISE, RENOISE = 0, 1

# columns of the per-slot coefficient table (fp32, ROW floats per slot; TD_PROG_* of include/targetdiff_hip.h)
ROW = 12
C0, CT, LOGVAR, LOG_A, LOG_1MA, LOG_CA, LOG_1MCA, ABAR_TO, LAST, RHO, LOG_R, LOG_1MR = range(ROW)


def _log1m(a):
    return np.log(1.0 - np.exp(a) + 1e-40)


class TimeProgram:
    """Immutable list of steps ``(kind, t_from, t_to)`` over the levels of a ``T``-step diffusion."""

    __slots__ = ('T', 'kind', 't_from', 't_to')

    def __init__(self, T, kind, t_from, t_to):
        T = int(T)
        kind = np.asarray(kind, dtype=np.int32).reshape(-1).copy()
        t_from = np.asarray(t_from, dtype=np.int32).reshape(-1).copy()
        t_to = np.asarray(t_to, dtype=np.int32).reshape(-1).copy()
        if T < 1:
            raise ValueError(f'T = {T}')
        if not (len(kind) == len(t_from) == len(t_to)):
            raise ValueError('kind, t_from and t_to must have one entry per step')
        if len(kind):
            if int(t_from[0]) != T - 1:
                raise ValueError(f'a program starts at level T - 1 = {T - 1} (the sampler\'s initial state), not at {int(t_from[0])}')
            if (t_from[1:] != t_to[:-1]).any():
                k = int(np.nonzero(t_from[1:] != t_to[:-1])[0][0]) + 1
                raise ValueError(f'step {k} starts at level {int(t_from[k])}, the step before it ends at {int(t_to[k - 1])}')
            lv = np.concatenate([t_from, t_to])
            if lv.min() < -1 or lv.max() > T - 1:
                raise ValueError(f'levels must lie in [-1, {T - 1}]')
            if not np.isin(kind, (DENOISE, RENOISE)).all():
                raise ValueError('kind must be DENOISE (0) or RENOISE (1)')
            down, up = kind == DENOISE, kind == RENOISE
            if (t_to[down] >= t_from[down]).any():
                raise ValueError('a denoise step goes strictly down')
            if (t_to[up] <= t_from[up]).any():
                raise ValueError('a renoise step goes strictly up')
        for a in (kind, t_from, t_to):
            a.setflags(write=False)
        object.__setattr__(self, 'T', T)
        object.__setattr__(self, 'kind', kind)
        object.__setattr__(self, 't_from', t_from)
        object.__setattr__(self, 't_to', t_to)

    def __setattr__(self, name, value):
        raise AttributeError('TimeProgram is immutable')

    def __len__(self):
        return int(self.kind.shape[0])

    def __eq__(self, other):
        return (isinstance(other, TimeProgram) and self.T == other.T and np.array_equal(self.kind, other.kind) and
                np.array_equal(self.t_from, other.t_from) and np.array_equal(self.t_to, other.t_to))

    def __hash__(self):
        return hash((self.T, self.kind.tobytes(), self.t_from.tobytes(), self.t_to.tobytes()))

    def __repr__(self):
        return (f'TimeProgram(T={self.T}, steps={len(self)}, denoise={self.num_denoise}, renoise={self.num_renoise}, '
                f'ends_at={int(self.t_to[-1]) if len(self) else self.T - 1})')

    @property
    def num_denoise(self):
        return int((self.kind == DENOISE).sum())

    @property
    def num_renoise(self):
        return int((self.kind == RENOISE).sum())

    @property
    def levels(self):
        """The level after each step."""
        return self.t_to

    # ---------------------------------------------------------------------------------------- constructors
    @classmethod
    def from_levels(cls, T, levels):
        """A pure descent through ``levels`` (the first must be T - 1, strictly decreasing, the last may be -1)."""
        lv = np.asarray(list(levels), dtype=np.int64).reshape(-1)
        if lv.size < 1:
            raise ValueError('from_levels needs at least the starting level')
        return cls(T, np.full(lv.size - 1, DENOISE), lv[:-1], lv[1:])

    @classmethod
    def reference(cls, T, num_steps=None):
        """The reference's chain: ``num_steps`` unit steps from T - 1 (all T of them by default, down to clean data)."""
        n = int(T) if num_steps is None else int(num_steps)
        if not 0 <= n <= T:
            raise ValueError(f'num_steps = {n} outside [0, {T}]')
        return cls.from_levels(T, np.arange(T - 1, T - 2 - n, -1))

    @classmethod
    def strided(cls, T, K):
        """K denoiser calls: levels ``round(linspace(T-1, 0, K))`` made unique, then clean data; K = 1 is ``[T-1, -1]``."""
        K = int(K)
        if K < 1:
            raise ValueError(f'K = {K}')
        lv = [T - 1] if K == 1 else np.round(np.linspace(T - 1, 0, K)).astype(np.int64).tolist()
        uniq = [lv[0]]
        for x in lv[1:]:
            if x < uniq[-1]:
                uniq.append(x)
        return cls.from_levels(T, uniq + [-1])

    def with_resampling(self, jump_length, resamplings):
        """RePaint's schedule on a pure descent of n denoise steps (positions 0 .. n along it): after the denoise step that completes
        position i, for every i that is a multiple of ``jump_length`` with 0 < i < n, re-noise back ``jump_length`` positions and
        descend again, ``resamplings - 1`` times.  Length: n + (r - 1) * floor((n - 1) / j) * (j + 1)."""
        j, r = int(jump_length), int(resamplings)
        if j < 1 or r < 1:
            raise ValueError('jump_length and resamplings must be at least 1')
        if self.num_renoise:
            raise ValueError('with_resampling applies to a pure descent (a program without renoise steps)')
        n = len(self)
        if n == 0:
            return self
        L = [int(self.t_from[0])] + [int(x) for x in self.t_to]
        kind, a, b = [], [], []

        def add(k, x, y):
            kind.append(k), a.append(x), b.append(y)
        for i in range(1, n + 1):
            add(DENOISE, L[i - 1], L[i])
            if i % j == 0 and i < n:
                for _ in range(r - 1):
                    add(RENOISE, L[i], L[i - j])
                    for k in range(i - j + 1, i + 1):
                        add(DENOISE, L[k - 1], L[k])
        return TimeProgram(self.T, kind, a, b)

    # ---------------------------------------------------------------------------------------- coefficients
    def tables(self, model):
        """The per-slot coefficient table, float32 ``[len(self), ROW]`` (numpy).  ``model``: a ``ScorePosNet3D`` of this package (its
        float64 schedule tables ``_sched64`` and, for unit steps, its own fp32 per-t tables)."""
        if int(model.num_timesteps) != self.T:
            raise ValueError(f'the program is for T = {self.T}, the model has {int(model.num_timesteps)} levels')
        A64, Lc64 = model._sched64['alphas_cumprod'], model._sched64['log_alphas_cumprod_v']
        A = lambda l: 1.0 if l < 0 else float(A64[l])
        Lc = lambda l: 0.0 if l < 0 else float(Lc64[l])
        own = lambda name: model.get_parameter(name).detach().cpu().numpy()
        m = {k: own(k) for k in ('posterior_mean_c0_coef', 'posterior_mean_ct_coef', 'posterior_logvar', 'log_alphas_v',
                                 'log_one_minus_alphas_v', 'log_alphas_cumprod_v', 'log_one_minus_alphas_cumprod_v', 'alphas_cumprod')}
        out = np.zeros((len(self), ROW), dtype=np.float32)
        for i, (k, f, to) in enumerate(zip(self.kind.tolist(), self.t_from.tolist(), self.t_to.tolist())):
            row = out[i]
            if k == RENOISE:
                s, t = f, to
                row[RHO] = np.float32(A(t) / A(s))
                l_r = Lc(t) - Lc(s)
                row[LOG_R], row[LOG_1MR] = np.float32(l_r), np.float32(_log1m(l_r))
                continue
            t, s = f, to
            if s == t - 1:          # a unit step: the model's own entries, the reference's clamp t - 1 -> 0 at t == 0 included (:403-405)
                p = max(t - 1, 0)
                row[C0], row[CT], row[LOGVAR] = m['posterior_mean_c0_coef'][t], m['posterior_mean_ct_coef'][t], m['posterior_logvar'][t]
                row[LOG_A], row[LOG_1MA] = m['log_alphas_v'][t], m['log_one_minus_alphas_v'][t]
                row[LOG_CA], row[LOG_1MCA] = m['log_alphas_cumprod_v'][p], m['log_one_minus_alphas_cumprod_v'][p]
                row[ABAR_TO] = m['alphas_cumprod'][p]
                row[LAST] = 1.0 if t == 0 else 0.0
                continue
            At, As = A(t), A(s)
            alpha = At / As
            beta = 1.0 - alpha
            row[C0] = np.float32(beta * np.sqrt(As) / (1.0 - At))
            row[CT] = np.float32((1.0 - As) * np.sqrt(alpha) / (1.0 - At))
            var = np.float32(beta * (1.0 - As) / (1.0 - At))
            row[LOGVAR] = 0.0 if s < 0 else np.float32(np.log(var))          # s == -1: no noise is added, the entry is not read
            l_a = Lc(t) - Lc(s)
            row[LOG_A], row[LOG_1MA] = np.float32(l_a), np.float32(_log1m(l_a))
            row[LOG_CA], row[LOG_1MCA] = np.float32(Lc(s)), np.float32(_log1m(Lc(s)))
            row[ABAR_TO] = np.float32(As)
            row[LAST] = 1.0 if s < 0 else 0.0
        return out

    def denoiser_times(self):
        """Per slot, the time the denoiser runs at (``t_from`` of a denoise step; a renoise slot holds its ``t_to``, unused)."""
        return np.where(self.kind == DENOISE, self.t_from, self.t_to).astype(np.int32)
