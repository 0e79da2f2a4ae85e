"""Yardstick of the pointwise log-likelihood read-outs (kmc.waic, kmc.pointwise_loglike, kmc.waic_stats, kmc.pointwise_plan): numpy and
``math`` only, no device.

* the term matrix ``l[r][j]`` of arithmetic-only term bodies, operation by operation as the C++ body writes them (bit-equal to the device
  compiled with contraction off);
* the per-observation statistics: ``M`` exactly, ``S1``, ``E`` and ``V`` as the exactly rounded sums (``math.fsum``) of their exact
  terms -- ``exp`` is ``math.exp``, the squares of ``V`` are carried error-free (two-sum of the difference, Dekker product);
* the host stage with ``math.log`` / ``math.sqrt`` (the C library's, as in ``kmc_waic_stats``; ``np.log``'s vector form may differ in
  the last bit) and the data-density contract's pairwise tree, in the operation order of ``include/kissmcmc_hip.h``;
* the plan.
"""
import math

import numpy as np

from covariance_yardstick import two_product

U = 2.0 ** -53

REG_TERM = "double mu = x[0]; for (int k = 1; k < n; ++k) mu += x[k] * d[k - 1]; double r = d[n - 1] - mu; return -0.5 * p[0] * r * r;"
# -inf below a threshold the observation carries, a NaN through a NaN in the observation
CUT_TERM = "double r = d[1] - x[1]; return x[0] < d[0] ? -INFINITY : -0.5 * p[0] * r * r;"


def rows_of(thetas, first_sample=0, thin=1, walkers=None):
    """``thetas[walker][sample][dim]`` -> the selected rows ``[n, dim]`` in the library's order: sample by sample, walkers ascending."""
    th = np.asarray(thetas, dtype=np.float64)
    if walkers is not None:
        th = th[np.asarray(walkers)]
    th = th[:, first_sample::thin]
    return np.ascontiguousarray(th.transpose(1, 0, 2)).reshape(-1, th.shape[2])


def reg_matrix(X, D, p0):
    """REG_TERM for every row of ``X [n, ndim]`` and observation of ``D [J, ndim]``."""
    X, D = np.asarray(X, dtype=np.float64), np.asarray(D, dtype=np.float64)
    nd = X.shape[1]
    mu = np.repeat(X[:, :1], D.shape[0], axis=1)
    for k in range(1, nd):
        mu = mu + X[:, k:k + 1] * D[None, :, k - 1]
    r = D[None, :, nd - 1] - mu
    return ((-0.5 * p0) * r) * r


def cut_matrix(X, D, p0):
    """CUT_TERM (ndim 2, two columns)."""
    X, D = np.asarray(X, dtype=np.float64), np.asarray(D, dtype=np.float64)
    r = D[None, :, 1] - X[:, 1:2]
    with np.errstate(invalid="ignore"):
        v = ((-0.5 * p0) * r) * r
    return np.where(X[:, :1] < D[None, :, 0], -np.inf, v)


def two_sum(a, b):
    """(s, e) with s = fl(a + b) and s + e = a + b exactly (Knuth)."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def col_max(l):
    """``M_j``: the largest term; NaN when a term is NaN."""
    return np.max(l, axis=0)


def fsum_cols(t):
    out = np.empty(t.shape[1])
    for j in range(t.shape[1]):
        col = t[:, j]
        if np.isfinite(col).all():
            out[j] = math.fsum(col.tolist())
        else:                                        # fsum refuses inf - inf; the IEEE answer is what plain addition gives
            with np.errstate(invalid="ignore"):
                out[j] = np.add.reduce(col)
    return out


def exact_stats(l, centre=None):
    """``[4, J]``: M, S1, E, V of the matrix ``l [n, J]``; V about ``centre`` (default: the exact S1 / n), with its terms
    (l - centre)^2 carried error-free for the finite ones."""
    l = np.asarray(l, dtype=np.float64)
    n, J = l.shape
    M = col_max(l)
    S1 = fsum_cols(l)
    c = S1 / n if centre is None else np.asarray(centre, dtype=np.float64)
    E, V = np.empty(J), np.empty(J)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(J):
            col = l[:, j]
            if M[j] == -np.inf:
                E[j] = 0.0
            else:
                a = col - M[j]
                e = [math.exp(v) if v == v and v != np.inf else v for v in a.tolist()]
                E[j] = math.fsum(e) if all(math.isfinite(v) for v in e) else float(np.add.reduce(np.array(e)))
            if np.isfinite(col).all() and np.isfinite(c[j]):
                hi, lo = two_sum(col, -c[j])
                p, err = two_product(hi, hi)
                V[j] = math.fsum(p.tolist() + err.tolist() + (2.0 * hi * lo).tolist())
            else:
                d = col - c[j]
                V[j] = np.add.reduce(d * d)
    return np.stack([M, S1, E, V])


def pairwise(v):
    """The data-density contract's tree: each level adds neighbours, an odd last element passes up."""
    v = [float(x) for x in v]
    while len(v) > 1:
        nxt = [v[i] + v[i + 1] for i in range(0, len(v) - 1, 2)]
        if len(v) & 1:
            nxt.append(v[-1])
        v = nxt
    return v[0]


def _log(x):
    if x != x:
        return x
    if x == 0.0:
        return -math.inf
    return math.log(x) if x > 0.0 else math.nan


def host_stage(stats, n):
    """``kmc_waic_stats`` restated: dict of the totals and the three arrays."""
    st = np.asarray(stats, dtype=np.float64)
    J = st.shape[1]
    M, S1, E, V = (st[i].tolist() for i in range(4))
    logn, nm1 = math.log(float(n)), float(n - 1)
    lp = [M[j] + (_log(E[j]) - logn) for j in range(J)]
    pw = [V[j] / nm1 for j in range(J)]
    el = [lp[j] - pw[j] for j in range(J)]
    lppd, p_waic, elpd = pairwise(lp), pairwise(pw), pairwise(el)
    centre = elpd / float(J)
    dev = [el[j] - centre for j in range(J)]
    ss = pairwise([d * d for d in dev])
    if J == 1:
        se = math.nan                                # J * ss / 0: 0 / 0, or NaN / 0
    else:
        q = float(J) * ss / float(J - 1)
        se = math.sqrt(q) if q == q else q
    return {"lppd": lppd, "p_waic": p_waic, "elpd_waic": elpd, "se": se, "waic": -2.0 * elpd,
            "n_high": sum(1 for v in pw if v > 0.4), "n_nan": sum(1 for v in S1 if v != v), "n": int(n),
            "lppd_j": np.array(lp), "p_waic_j": np.array(pw), "elpd_j": np.array(el)}


TARGET_WAVES, MIN_RUN = 4096, 16


def plan(n, J):
    """``kmc_pointwise_plan`` restated."""
    lanes, slots = 64, 1
    if J < 64:
        lanes = 1
        while lanes < J:
            lanes *= 2
        slots = 64 // lanes
    max_runs = max(1, TARGET_WAVES // ((J + 63) // 64))
    run_len = max(MIN_RUN, -(-n // max_runs))
    nruns = -(-n // run_len)
    return {"run_len": run_len, "nruns": nruns, "lanes_per_run": lanes, "slots": slots, "nwaves": -(-nruns // slots)}


def planned_sums(terms, n, J):
    """The sum of ``terms [n, J]`` in the library's order: every run from 0.0 in row order, the runs from 0.0 in run order."""
    p = plan(n, J)
    total = np.zeros(J)
    for r in range(p["nruns"]):
        acc = np.zeros(J)
        for k in range(r * p["run_len"], min(n, (r + 1) * p["run_len"])):
            acc = acc + terms[k]
        total = total + acc
    return total
