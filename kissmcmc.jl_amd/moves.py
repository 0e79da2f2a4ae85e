"""Proposal moves of the ensemble sampler (``kmc_config.move`` in ``include/kissmcmc_hip.h``).

``move=None`` everywhere is the reference's stretch move with ``a_scale`` (``src/samplers.jl:250-260``).  ``DEMove`` is the
opt-in differential-evolution move (ter Braak 2006; emcee's ``DEMove``), which the reference does not have.
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

    def __repr__(self):
        return f"DEMove(gamma0={self.gamma0!r}, sigma={self.sigma!r})"


def apply_move(move, cfg) -> None:
    """``move=None``: the stretch move (the zeroed default of the config); a ``DEMove``: written into ``cfg``."""
    if move is None:
        return
    if not isinstance(move, DEMove):
        raise TypeError(f"move must be None (the stretch move) or a DEMove; got {type(move).__name__}")
    move.apply(cfg)
