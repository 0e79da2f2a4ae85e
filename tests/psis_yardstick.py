"""A numpy restatement of PSIS-LOO as ``include/kissmcmc_hip.h`` defines it (steps 1 to 6), for the tests: from a matrix ``l[n][J]`` every
output of ``kmc.loo``.  ``longdouble=True`` runs the same operations in ``np.longdouble``: the distance between the two modes is the
yardstick's own error on an input, from which the tests take their tolerance.  Sums are numpy's (pairwise), not the library's order.
"""
from __future__ import annotations

import math

import numpy as np

LOG_DBL_MIN = float(np.log(np.finfo(np.float64).tiny))
TEN_EPS = 10.0 * float(np.finfo(np.float64).eps)


def tail_length(n, r_eff=1.0):
    return int(math.ceil(min(0.2 * n, 3.0 * math.sqrt(n / r_eff))))


def pairwise_tree(v):
    """The data-density contract's tree: neighbours are added level by level, an odd last element passes up."""
    v = list(np.asarray(v, dtype=np.float64))
    while len(v) > 1:
        half = len(v) // 2
        nxt = [v[2 * i] + v[2 * i + 1] for i in range(half)]
        if len(v) & 1:
            nxt.append(v[-1])
        v = nxt
    return float(v[0])


def shift_and_tail(col, M):
    """Steps 1 and 2 in float64 (exact but for the one subtraction): ``m, xc, x, tail mask``; ``None`` for a NaN observation."""
    col = np.asarray(col, dtype=np.float64)
    if np.isnan(col).any():
        return None
    m = col.min()
    if not np.isfinite(m):
        return None
    with np.errstate(invalid="ignore"):
        x = m - col
    xs = np.sort(x)
    xc = max(LOG_DBL_MIN, xs[col.size - M - 1])
    return m, xc, x, x > xc


def gpdfit(e, ft=np.float64, dropped=None):
    """Step 3 on the ascending exceedances ``e``: ``(k, sigma)``.  ``dropped`` (a list) receives the mask of the weights dropped."""
    e = np.asarray(e, dtype=ft)
    nt = e.size
    m_est = 30 + int(math.floor(math.sqrt(nt)))
    i = np.arange(1, m_est + 1, dtype=ft)
    b = (ft(1) - np.sqrt(ft(m_est) / (i - ft(0.5)))) / (ft(3) * e[int(nt / 4 + 0.5) - 1]) + ft(1) / e[nt - 1]
    kap = np.log1p(-b[:, None] * e[None, :]).mean(axis=1)
    L = ft(nt) * (np.log(-b / kap) - kap - ft(1))
    w = ft(1) / np.exp(L[None, :] - L[:, None]).sum(axis=1)
    keep = w >= ft(TEN_EPS)
    if dropped is not None:
        dropped.append(~keep)
    w = w[keep] / w[keep].sum()
    bbar = (w * b[keep]).sum()
    kbar = np.log1p(-bbar * e).mean()
    return (ft(nt) * kbar + ft(5)) / (ft(nt) + ft(10)), -kbar / bbar


def smooth(x_tail, xc, ft=np.float64, dropped=None):
    """Steps 3 and 4 on the ascending tail: ``(k, sigma, s)``."""
    x = np.asarray(x_tail, dtype=ft)
    nt = x.size
    if nt <= 4:
        return ft(np.inf), ft(np.nan), x.copy()
    with np.errstate(all="ignore"):
        exc = np.exp(ft(xc))
        k, sigma = gpdfit(np.exp(x) - exc, ft, dropped)
        if not np.isfinite(k):
            return k, sigma, x.copy()
        if not (np.isfinite(sigma) and sigma > 0):
            return k, sigma, np.full(nt, np.nan, dtype=ft)
        p = (np.arange(1, nt + 1, dtype=ft) - ft(0.5)) / ft(nt)
        s = np.minimum(ft(0), np.log(sigma * np.expm1(-k * np.log1p(-p)) / k + exc))
    return k, sigma, s


def loo_column(col, M, ft=np.float64, dropped=None):
    """Steps 1 to 5 for one observation: dict ``m, xc, n_tail, tail, k, sigma, elpd``."""
    st = shift_and_tail(col, M)
    nan = ft(np.nan)
    if st is None:
        return {"m": nan, "xc": nan, "n_tail": -1, "tail": np.zeros(0), "k": nan, "sigma": nan, "elpd": nan}
    m, xc, x, mask = st
    tail = np.sort(x[mask])
    k, sigma, s = smooth(tail, xc, ft, dropped)
    with np.errstate(all="ignore"):
        W = np.exp(x[~mask].astype(ft)).sum() + np.exp(s).sum()
        N = ft(col.size - tail.size) + np.exp(s - tail.astype(ft)).sum()
        elpd = ft(m) + np.log(N / W)
    return {"m": m, "xc": xc, "n_tail": tail.size, "tail": tail, "k": k, "sigma": sigma, "elpd": elpd}


def lppd_column(col, ft=np.float64):
    col = np.asarray(col, dtype=ft)
    M = col.max()
    with np.errstate(all="ignore"):
        return M + (np.log(np.exp(col - M).sum()) - np.log(ft(col.size)))


def totals(elpd_j, lppd_j, pareto_k):
    """Step 6 in float64, in the library's order."""
    el, lp, kh = (np.asarray(a, dtype=np.float64) for a in (elpd_j, lppd_j, pareto_k))
    J = el.size
    pl = lp - el
    elpd = pairwise_tree(el)
    with np.errstate(all="ignore"):
        dv = el - elpd / float(J)
        se = float(np.sqrt(float(J) * pairwise_tree(dv * dv) / float(J - 1))) if J > 1 else float("nan")
    kc = (int((kh <= 0.5).sum()), int(((kh > 0.5) & (kh <= 0.7)).sum()), int(((kh > 0.7) & (kh <= 1.0)).sum()), int((kh > 1.0).sum()))
    return {"elpd_loo": elpd, "se": se, "p_loo": pairwise_tree(pl), "looic": -2.0 * elpd, "lppd": pairwise_tree(lp),
            "n_nan": int(np.isnan(el).sum()), "k_counts": kc, "p_loo_j": pl}


def loo(l, r_eff=1.0, longdouble=False, lppd_j=None, dropped=None):
    """Every output of ``kmc.loo`` from the matrix ``l[n][J]``.  ``lppd_j``: taken as given (the library's own) when not None."""
    l = np.asarray(l, dtype=np.float64)
    n, J = l.shape
    ft = np.longdouble if longdouble else np.float64
    M = tail_length(n, r_eff)
    cols = [loo_column(l[:, j], M, ft, dropped) for j in range(J)]
    lp = np.array([lppd_column(l[:, j], ft) for j in range(J)], dtype=ft) if lppd_j is None else np.asarray(lppd_j, dtype=ft)
    out = {"n": n, "tail_len": M, "elpd_loo_j": np.array([c["elpd"] for c in cols], dtype=ft), "pareto_k": np.array([c["k"] for c in cols], dtype=ft),
           "n_tail_j": np.array([c["n_tail"] for c in cols], dtype=np.int64), "m_j": np.array([c["m"] for c in cols], dtype=np.float64),
           "xc_j": np.array([c["xc"] for c in cols], dtype=np.float64), "tails": [c["tail"] for c in cols], "lppd_j": lp}
    t = totals(out["elpd_loo_j"].astype(np.float64), lp.astype(np.float64), out["pareto_k"].astype(np.float64))
    out["p_loo_j"] = lp - out["elpd_loo_j"]
    t.pop("p_loo_j")
    out.update(t)
    return out
