"""Proposal moves of the ensemble sampler (``kmc_config.move`` in ``include/kissmcmc_hip.h``).

``move=None`` everywhere is the reference's stretch move with ``a_scale`` (``src/samplers.jl:250-260``).  ``DEMove`` is the
opt-in differential-evolution move (ter Braak 2006; emcee's ``DEMove``), which the reference does not have; ``DESnookerMove``
the DE snooker update (ter Braak & Vrugt 2008; emcee's ``DESnookerMove``).  A list of 2 to 4 ``(move, weight)`` pairs of the two
is a mixture: every half-step uses one member for all its walkers (emcee's recipe for multimodal targets is
``[(DEMove(), 0.8), (DESnookerMove(), 0.2)]``).
"""
from __future__ import annotations

import math

from . import _lib


class DEMove:
    """Differential evolution: ``y = x + g (x_j - x_k)`` with two distinct partners ``j != k`` drawn uniformly from the
    complementary half, ``g = gamma0 (1 + sigma v)`` and ``v`` uniform in (-1, 1); accepted when ``p1 - p0 >= log u``.

    ``gamma0=None`` is ``2.38 / sqrt(2 ndim)``.  ``sigma`` is the relative jitter of ``g``, in [0, 1); 0 means none.
    One GPU with double rows, two launches per generation: not with island mode, P2P, shards, dealt sub-ensembles,
    ``dtype="f32"`` or device blobs (``KmcError`` with ``ERR_UNSUPPORTED``).  The stream is DESIGN.md section 2's."""

    def __init__(self, gamma0=None, sigma: float = 1e-5):
        if gamma0 is not None:
            gamma0 = float(gamma0)
            if not (math.isfinite(gamma0) and gamma0 > 0.0):
                raise ValueError("DEMove: gamma0 must be a finite number > 0 (or None for 2.38 / sqrt(2 ndim))")
        sigma = float(sigma)
        if not (math.isfinite(sigma) and 0.0 <= sigma < 1.0):
            raise ValueError("DEMove: sigma must be in [0, 1)")
        self.gamma0 = gamma0
        self.sigma = sigma

    def gamma0_for(self, ndim: int) -> float:
        """gamma0 as the kernels use it for ``ndim`` dimensions."""
        return self.gamma0 if self.gamma0 is not None else 2.38 / math.sqrt(2.0 * int(ndim))

    def apply(self, cfg) -> None:
        """Write this move into a ``kmc_config`` (``_lib.Config``)."""
        cfg.move = _lib.MOVE_DE
        cfg.de_gamma0 = 0.0 if self.gamma0 is None else self.gamma0
        cfg.de_sigma = self.sigma

    def apply_member(self, cfg, i: int) -> None:
        """Write this move into member ``i`` of a mixture."""
        setattr(cfg, f"mix_move{i}", _lib.MOVE_DE)
        setattr(cfg, f"mix_gamma{i}", 0.0 if self.gamma0 is None else self.gamma0)
        setattr(cfg, f"mix_sigma{i}", self.sigma)

    def __repr__(self):
        return f"DEMove(gamma0={self.gamma0!r}, sigma={self.sigma!r})"


class DESnookerMove:
    """The DE snooker update: three distinct partners ``z, z1, z2`` drawn uniformly from the complementary half,
    ``d = x - z``, ``s = gamma (d . (z1 - z2)) / (d . d)`` and ``y = x + d s``; accepted when
    ``(ndim - 1) log|1 + s| + p1 - p0 >= log u``.  The two sums over the row run in one fixed order.

    ``gamma`` defaults to 1.7.  Needs ``ndim >= 2`` and at least 6 walkers; otherwise restricted like ``DEMove``."""

    def __init__(self, gamma: float = 1.7):
        gamma = float(gamma)
        if not (math.isfinite(gamma) and gamma > 0.0):
            raise ValueError("DESnookerMove: gamma must be a finite number > 0")
        self.gamma = gamma

    def apply(self, cfg) -> None:
        """Write this move into a ``kmc_config`` (``_lib.Config``)."""
        cfg.move = _lib.MOVE_SNOOKER
        cfg.snooker_gamma = self.gamma

    def apply_member(self, cfg, i: int) -> None:
        """Write this move into member ``i`` of a mixture."""
        setattr(cfg, f"mix_move{i}", _lib.MOVE_SNOOKER)
        setattr(cfg, f"mix_gamma{i}", self.gamma)
        setattr(cfg, f"mix_sigma{i}", 0.0)

    def __repr__(self):
        return f"DESnookerMove(gamma={self.gamma!r})"


def mixture_weights(weights):
    """The weights as the library normalises them: in double, in list order."""
    total = 0.0
    for w in weights:
        total += w
    return [w / total for w in weights]


def apply_move(move, cfg) -> None:
    """``move=None``: the stretch move (the zeroed default of the config); a ``DEMove`` or ``DESnookerMove``: written into ``cfg``;
    a list of 2 to 4 ``(move, weight)`` pairs of those: a mixture (weights finite and > 0, normalised by the library)."""
    if move is None:
        return
    if isinstance(move, (DEMove, DESnookerMove)):
        move.apply(cfg)
        return
    if not isinstance(move, (list, tuple)):
        raise TypeError(f"move must be None (the stretch move), a DEMove, a DESnookerMove or a list of (move, weight) pairs; got {type(move).__name__}")
    pairs = list(move)
    if not (2 <= len(pairs) <= _lib.MIX_MAX):
        raise ValueError(f"a move mixture has 2 to {_lib.MIX_MAX} (move, weight) pairs; got {len(pairs)}")
    members = []
    for pair in pairs:
        if not (isinstance(pair, (list, tuple)) and len(pair) == 2):
            raise TypeError("a move mixture is a list of (move, weight) pairs")
        m, w = pair
        if m is None:
            raise ValueError("a stretch member (None) in a move mixture is not supported yet: members are DEMove and DESnookerMove")
        if not isinstance(m, (DEMove, DESnookerMove)):
            raise TypeError(f"a mixture member must be a DEMove or a DESnookerMove; got {type(m).__name__}")
        w = float(w)
        if not (math.isfinite(w) and w > 0.0):
            raise ValueError("move mixture: weights must be finite and > 0")
        members.append((m, w))
    if not math.isfinite(sum(w for _, w in members)):
        raise ValueError("move mixture: the weights' sum must be finite")
    cfg.move = _lib.MOVE_MIX
    cfg.mix_count = len(members)
    for i, (m, w) in enumerate(members):
        m.apply_member(cfg, i)
        setattr(cfg, f"mix_weight{i}", w)
