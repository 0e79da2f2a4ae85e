"""The yardstick of the rank-normalised convergence diagnostics (kmc_*_rank_scores, kmc_*_rank_convergence; the definitions are in
include/kissmcmc_hip.h): numpy and the standard library only, nothing of the product.

Ranks by np.sort and np.searchsorted on zero-canonicalised values; the normal score in two forms -- element by element through
statistics.NormalDist().inv_cdf, and `inv_cdf`, a vectorised restatement of the same operation order (Wichura's AS 241, PPND16) that
must agree with it bit for bit; the fold, the indicators and the quantiles by the rule of kmc.quantile_ranks; the statistics through
convergence_yardstick.raw / stats on the transformed columns.

Chains are [sample][walker][dim], the layout of Sampler.chain()."""
import math
import statistics

import numpy as np

import convergence_yardstick as cy

HAS_NAN = 4
_ND = statistics.NormalDist()


def pooled(chain, logp=None, first=0, walkers=None, split=True):
    """x[ncols][m][h] in float64, the draws that belong to a chain (chain j = half * nw + k), and m, h."""
    x, h, m = cy.chains_of(chain, logp, first, walkers, split)
    return np.ascontiguousarray(x.transpose(2, 1, 0)), m, h


def rank2_of(values):
    """#{y < x} + #{y <= x} + 1 for every x of a 1-D array, by value: -0.0 ties with +0.0, infinities are ordinary values."""
    v = np.asarray(values, dtype=np.float64).ravel() + 0.0
    s = np.sort(v)
    return (np.searchsorted(s, v, side="left") + np.searchsorted(s, v, side="right") + 1).astype(np.int64)


def p_of(rank2, S):
    """(rank2 / 2 - 0.375) / (S + 0.25): everything before the division is exact."""
    return (np.asarray(rank2, dtype=np.int64).astype(np.float64) * 0.5 - 0.375) / (float(S) + 0.25)


def scores_scalar(rank2, S):
    """z element by element through statistics.NormalDist().inv_cdf."""
    p = p_of(rank2, S)
    return np.array([_ND.inv_cdf(v) for v in p.ravel().tolist()]).reshape(p.shape)


def _horner(coef, r):
    acc = coef[0] * r + coef[1]
    for c in coef[2:]:
        acc = acc * r + c
    return acc


_A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4, 1.3731693765509461125e+4,
      1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0)
_B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4, 5.3941960214247511077e+3,
      6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0)
_C = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0, 3.64784832476320460504e+0,
      5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0)
_D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1, 6.89767334985100004550e-1,
      1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0)
_E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2, 2.96560571828504891230e-1,
      1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0)
_F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4, 1.48753612908506148525e-2,
      1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0)


def central(p):
    """Where |p - 0.5| <= 0.425: the branch of +, -, *, / alone, whose bits are the same everywhere."""
    return np.abs(np.asarray(p, dtype=np.float64) - 0.5) <= 0.425


def inv_cdf(p):
    """statistics._normal_dist_inv_cdf(p, 0, 1) restated on arrays in the same operation order.  numpy's +, -, *, / and sqrt are the
    IEEE operations; the logarithm of the tail branches is math.log element by element (numpy's own log need not round like libm's)."""
    p = np.asarray(p, dtype=np.float64)
    shape = p.shape
    p = p.ravel()
    q = p - 0.5
    z = np.empty_like(p)
    mid = np.abs(q) <= 0.425
    r = 0.180625 - q[mid] * q[mid]
    z[mid] = (_horner(_A, r) * q[mid]) / _horner(_B, r)
    tail = ~mid
    pt, qt = p[tail], q[tail]
    r = np.where(qt <= 0.0, pt, 1.0 - pt)
    r = np.sqrt(-np.array([math.log(v) for v in r.tolist()], dtype=np.float64))
    near = r <= 5.0
    rn, rf = r[near] - 1.6, r[~near] - 5.0
    x = np.empty_like(r)
    x[near] = _horner(_C, rn) / _horner(_D, rn)
    x[~near] = _horner(_E, rf) / _horner(_F, rf)
    z[tail] = np.where(qt < 0.0, -x, x)
    return z.reshape(shape)


def scores(rank2, S):
    return inv_cdf(p_of(rank2, S))


def quantile(sorted_col, q):
    """x_lo + frac (x_hi - x_lo) with h = q (S - 1), lo = floor(h), hi = min(lo + 1, S - 1), frac = h - lo; x_lo where frac == 0."""
    S = sorted_col.size
    hq = float(q) * float(S - 1)
    lo = math.floor(hq)
    hi = min(lo + 1, S - 1)
    frac = hq - lo
    x_lo, x_hi = float(sorted_col[lo]), float(sorted_col[hi])
    with np.errstate(invalid="ignore"):
        return x_lo if frac == 0.0 else float(np.float64(x_lo) + np.float64(frac) * (np.float64(x_hi) - np.float64(x_lo)))


def transforms(chain, logp=None, first=0, walkers=None, split=True):
    """dict: m, h, S, nan_count[ncols], nan_count_folded[ncols], median, q05, q95 [ncols], rank2, z, rank2_folded, z_folded, i05, i95
    [ncols][m][h].  A column with a NaN: rank2 = 0, z = NaN, quantiles NaN, folded counts S."""
    x, m, h = pooled(chain, logp, first, walkers, split)
    ncols, S = x.shape[0], m * h
    out = {"m": m, "h": h, "S": S, "nan_count": np.isnan(x).reshape(ncols, -1).sum(axis=1).astype(np.int64)}
    for k in ("median", "q05", "q95"):
        out[k] = np.full(ncols, np.nan)
    for k in ("rank2", "rank2_folded"):
        out[k] = np.zeros((ncols, m, h), dtype=np.int64)
    for k in ("z", "z_folded", "i05", "i95"):
        out[k] = np.full((ncols, m, h), np.nan)
    out["nan_count_folded"] = np.full(ncols, S, dtype=np.int64)
    for c in range(ncols):
        if out["nan_count"][c]:
            continue
        v = x[c].ravel() + 0.0
        s = np.sort(v)
        out["median"][c], out["q05"][c], out["q95"][c] = quantile(s, 0.5), quantile(s, 0.05), quantile(s, 0.95)
        out["rank2"][c] = rank2_of(v).reshape(m, h)
        out["z"][c] = scores(out["rank2"][c], S)
        out["i05"][c] = (v <= out["q05"][c]).astype(np.float64).reshape(m, h)
        out["i95"][c] = (v <= out["q95"][c]).astype(np.float64).reshape(m, h)
        with np.errstate(invalid="ignore"):
            f = np.abs(v - out["median"][c]) + 0.0
        out["nan_count_folded"][c] = int(np.isnan(f).sum())
        if out["nan_count_folded"][c] == 0:
            out["rank2_folded"][c] = rank2_of(f).reshape(m, h)
            out["z_folded"][c] = scores(out["rank2_folded"][c], S)
    return out


def as_chain(cols):
    """[ncols][m][h] -> a chain [h][m][ncols] of m unsplit walkers."""
    return np.ascontiguousarray(np.asarray(cols, dtype=np.float64).transpose(2, 1, 0))


def statistics_of(z, z_folded, i05, i95, max_lag=None):
    """The statistics of the four transformed column sets ([ncols][m][h] each; NaN columns are replaced by zeros and reported NaN by
    the caller): (stats dict over the 4 ncols columns, raw dict), through convergence_yardstick."""
    t = np.concatenate([np.nan_to_num(np.asarray(a, dtype=np.float64), nan=0.0) for a in (z, z_folded, i05, i95)], axis=0)
    return cy.convergence(as_chain(t), split=False, max_lag=max_lag)


def combine(st, ncols, nan_count, nan_count_folded):
    """rhat, rhat_bulk, rhat_folded, ess_bulk, ess_tail, ess_q05, ess_q95, T[4][ncols], flags from the stats of the 4 ncols columns."""
    g = lambda k, t: np.array(st[k][t * ncols:(t + 1) * ncols], dtype=np.float64 if k != "T" else np.int64)
    out = {"rhat_bulk": g("rhat", 0), "rhat_folded": g("rhat", 1), "ess_bulk": g("ess", 0), "ess_q05": g("ess", 2), "ess_q95": g("ess", 3),
           "T": np.stack([g("T", t) for t in range(4)])}
    fl = np.stack([np.asarray(st["flags"][t * ncols:(t + 1) * ncols]) for t in range(4)])
    flags = fl[0] | fl[1] | fl[2] | fl[3]
    for c in range(ncols):
        if nan_count[c]:
            for k in ("rhat_bulk", "rhat_folded", "ess_bulk", "ess_q05", "ess_q95"):
                out[k][c] = np.nan
            out["T"][:, c] = 0
            flags[c] = HAS_NAN
        elif nan_count_folded[c]:
            out["rhat_folded"][c] = np.nan
            out["T"][1, c] = 0
            flags[c] = fl[0, c] | fl[2, c] | fl[3, c] | HAS_NAN
    with np.errstate(invalid="ignore"):
        out["rhat"] = np.where(np.isnan(out["rhat_bulk"]) | np.isnan(out["rhat_folded"]), np.nan, np.maximum(out["rhat_bulk"], out["rhat_folded"]))
        out["ess_tail"] = np.where(np.isnan(out["ess_q05"]) | np.isnan(out["ess_q95"]), np.nan, np.minimum(out["ess_q05"], out["ess_q95"]))
    out["flags"] = flags.astype(np.int32)
    return out


def rank_convergence(chain, logp=None, first=0, walkers=None, split=True, max_lag=None):
    """The whole thing from the chain: (combined dict with median, q05, q95 added, transforms dict)."""
    t = transforms(chain, logp, first, walkers, split)
    st, _ = statistics_of(t["z"], t["z_folded"], t["i05"], t["i95"], max_lag)
    out = combine(st, t["z"].shape[0], t["nan_count"], t["nan_count_folded"])
    out.update(median=t["median"], q05=t["q05"], q95=t["q95"])
    return out, t
