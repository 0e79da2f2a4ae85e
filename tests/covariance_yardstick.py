"""The yardstick of the posterior covariance (kmc_*_covariance, kmc_cov_plan, kmc_cov_correlation; the definitions are in
include/kissmcmc_hip.h): numpy, math.fsum and fractions only, nothing of the product.

`sums` gives the column sums and the centred cross products with EXACT sums of EXACT products: a centred value is formed in float64 as
the definition writes it (one rounded subtraction of the mean it is given -- the device's own), the product of two of them is split
without error into its rounded value and the rounding error (Dekker's TwoProduct over Veltkamp's split), and math.fsum adds both halves
of every term, returning the correctly rounded exact sum.  `sums_fraction` is the same in rationals, for the test of the split itself.
`correlation` and `plan` restate the host stage and the plan operation for operation: they must agree with the library bit for bit.

Chains are [sample][walker][dim], the layout of Sampler.chain()."""
import math
from fractions import Fraction

import numpy as np

TILE_COLS, STRIP_TILES, ROWS_PER_WAVE_BLOCK, MAX_COLS = 16, 8, 64, 1024


def walkers_of(nwalkers, walkers=None):
    if walkers is None:
        return np.arange(nwalkers)
    w = np.asarray(walkers)
    return np.flatnonzero(w) if w.dtype == np.bool_ else np.unique(w.astype(np.int64))


def rows_of(chain, logp=None, first=0, walkers=None):
    """x[n][C] in float64: the rows (sample >= first, walker selected); the log-densities, when given, are the last column."""
    chain = np.asarray(chain)
    cols = chain.astype(np.float64)                                                # (a float32 chain widens exactly)
    if logp is not None:
        cols = np.concatenate([cols, np.asarray(logp, dtype=np.float64)[:, :, None]], axis=2)
    return cols[first:][:, walkers_of(chain.shape[1], walkers)].reshape(-1, cols.shape[2])


def two_product(a, b):
    """(p, e) with p = fl(a b) and p + e = a b exactly (Dekker 1971; no overflow, no underflow in e: |a b| in about [1e-290, 1e300])."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    p = a * b
    k = 134217729.0                                                                # 2^27 + 1
    ah = k * a - (k * a - a)
    bh = k * b - (k * b - b)
    al, bl = a - ah, b - bh
    return p, al * bl - (((p - ah * bh) - al * bh) - ah * bl)


def _fsum(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return math.fsum(v.tolist()) if np.isfinite(v).all() else float(np.sum(v))


def sums(x, mean=None):
    """Of the rows x[n][C]: `col_sum[C]` (exact, rounded once), `col_abs[C]` = sum |x|, and -- centred on `mean` (the column sums over n
    when None) -- `cross[C][C]` = sum_r d[r][a] d[r][b] with d = fl(x - mean) (exact products, exact sum, rounded once) and
    `cross_abs[C][C]` = sum |d_a d_b|.  A column with NaN or inf in it gets numpy's sums (IEEE: inf, or NaN)."""
    x = np.asarray(x, dtype=np.float64)
    n, C = x.shape
    col_sum = np.array([_fsum(x[:, c]) for c in range(C)])
    col_abs = np.array([_fsum(np.abs(x[:, c])) for c in range(C)])
    mean = col_sum / n if mean is None else np.asarray(mean, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x - mean[None, :]
        cross, cross_abs = np.empty((C, C)), np.empty((C, C))
        for a in range(C):
            p, e = two_product(d[:, a:a + 1], d[:, a:])
            for b in range(a, C):
                cross[a, b] = cross[b, a] = _fsum(np.concatenate([p[:, b - a], e[:, b - a]]))
                cross_abs[a, b] = cross_abs[b, a] = _fsum(np.abs(p[:, b - a]))
    return {"n": n, "col_sum": col_sum, "col_abs": col_abs, "mean": mean, "cross": cross, "cross_abs": cross_abs}


def sums_fraction(x, mean):
    """`cross[C][C]` of :func:`sums` in rationals, rounded once (finite data)."""
    x = np.asarray(x, dtype=np.float64)
    d = (x - np.asarray(mean, dtype=np.float64)[None, :]).tolist()
    C = x.shape[1]
    return np.array([[float(sum(Fraction(r[a]) * Fraction(r[b]) for r in d)) for b in range(C)] for a in range(C)])


def correlation(cov):
    """kmc_cov_correlation, operation for operation: (corr, std)."""
    cov = np.asarray(cov, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        std = np.sqrt(np.diag(cov))
        corr = cov / (std[:, None] * std[None, :])
    var = np.diag(cov)
    one = (var > 0.0) & np.isfinite(var)
    corr[np.flatnonzero(one), np.flatnonzero(one)] = 1.0
    return corr, std


def plan(ncols):
    """kmc_cov_plan: dict tile_cols, strip_tiles, nstrips, rows_per_wave_block."""
    ntiles = (ncols + TILE_COLS - 1) // TILE_COLS
    nstrips = 1 if ntiles <= 2 else sum((ntiles - ta + STRIP_TILES - 1) // STRIP_TILES for ta in range(ntiles))
    return {"tile_cols": TILE_COLS, "strip_tiles": STRIP_TILES, "nstrips": nstrips, "rows_per_wave_block": ROWS_PER_WAVE_BLOCK}
