"""The yardstick of the covariance-shaped Metropolis proposal (MVNormalStep, TunedStep; the definition is in
include/kissmcmc_hip.h): plain Python and numpy, nothing of the product.

`cholesky_lower` and `delta` restate the two fixed operation orders operation for operation (numpy's elementwise products and sums
are rounded one by one, never fused), so they must agree with the library bit for bit.  `metropolis` is the reference's loop
(src/samplers.jl:96-126) line by line for many chains, fed the stream's normals and accept uniforms and a log-density from outside
(the tests pass the CPU oracle's `metropolis_draw` and `logpdf`).  `tune_boundaries`, `covariance_two_pass` and `tuned_factor`
restate the tuning rule."""
import math

import numpy as np


def cholesky_lower(a):
    """(L, bad): row by row, j = 0..i within a row, s = a[i][j] - sum_k L[i][k] L[j][k] with k ascending and every operation rounded;
    `bad` is the first pivot that is not finite and positive (L is then None), else -1.  Only the lower triangle of `a` is read."""
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[0]
    L = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1):
            s = float(a[i, j])
            for k in range(j):
                t = float(L[i, k]) * float(L[j, k])
                s = s - t
            if j < i:
                L[i, j] = s / float(L[j, j])
            else:
                if not (math.isfinite(s) and s > 0.0):
                    return None, i
                L[i, i] = math.sqrt(s)
    return L, -1


def delta(L, z):
    """delta[..., i] = ((L[i][0] z[0] + L[i][1] z[1]) + ...) + L[i][i] z[i]: j ascending, every j <= i, each product and each sum rounded.
    `z` is [..., ndim]; the leading axes are independent."""
    L = np.asarray(L, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    d = np.empty_like(z)
    for i in range(L.shape[0]):
        s = L[i, 0] * z[..., 0]
        for j in range(1, i + 1):
            s = s + L[i, j] * z[..., j]
        d[..., i] = s
    return d


def tune_boundaries(nburnin, rounds):
    """b_r = floor(r nburnin / (R + 1)), r = 1..R, equal ones collapsed."""
    out = []
    for r in range(1, rounds + 1):
        b = (r * nburnin) // (rounds + 1)
        if not out or out[-1] != b:
            out.append(b)
    return out


def covariance_two_pass(x):
    """np.cov(x.T) restated: the mean first, then the centred cross products, divisor n - 1.  x is [n][ndim]."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    mean = x.sum(axis=0) / n
    c = x - mean
    return (c.T @ c) / (n - 1)


def default_scale(ndim):
    return 2.38 / math.sqrt(ndim)


def tuned_factor(states, scale):
    """(L, bad) of one tuning boundary: C = (scale scale) Sigma entry by entry, L = cholesky_lower(C)."""
    return cholesky_lower((scale * scale) * covariance_two_pass(states))


def metropolis(logpdf, draw, theta0, L, niter, nburnin, nthin, rounds=0, scale=None):
    """Many chains of src/samplers.jl:96-126 with the proposal theta + L z.  `logpdf(x)` -> float for one state, `draw(it, c)` ->
    (normals[ndim], uniform).  With `rounds` > 0 L is replaced at the tuning boundaries (a failed factorisation keeps the previous one).
    Returns a dict like run_chains', plus `margin` = the smallest |p1 - p0 - log u| met, `states_at` = {boundary: states} and
    `chol` = the L in force at the end."""
    x = np.array(theta0, dtype=np.float64)
    nc, nd = x.shape
    L = np.array(L, dtype=np.float64)
    p0 = np.array([logpdf(v) for v in x])
    nacc = np.zeros(nc, dtype=np.int64)
    chain, chain_logp = [], []
    margin = math.inf
    bounds = tune_boundaries(nburnin, rounds) if rounds > 0 else []
    if scale is None:
        scale = default_scale(nd)
    skipped = 0
    states_at = {}
    for it in range(niter):
        if it in bounds:
            states_at[it] = x.copy()
            Ln, bad = tuned_factor(x, scale)
            if bad >= 0:
                skipped += 1
            else:
                L = Ln
        n = it + 1 - nburnin                                              # :96
        z = np.empty((nc, nd))
        lu = np.empty(nc)
        for c in range(nc):
            zc, u = draw(it, c)
            z[c] = zc
            lu[c] = math.log(u)
        y = x + delta(L, z)                                               # :98
        for c in range(nc):
            p1 = logpdf(y[c])                                             # :99
            d = p1 - p0[c] - lu[c]
            if math.isfinite(d):
                margin = min(margin, abs(d))
            if p1 - p0[c] > lu[c]:                                        # :101
                x[c] = y[c]
                p0[c] = p1
                nacc[c] += n > 0                                          # :105
        if n > 0 and n % nthin == 0:                                      # :108, :112
            chain.append(x.copy())
            chain_logp.append(p0.copy())
    ns = len(chain)
    return dict(chain=np.array(chain).reshape(ns, nc, nd), chain_logp=np.array(chain_logp).reshape(ns, nc), naccept=nacc,
                final_pos=x, final_logp=p0, margin=margin, states_at=states_at, chol=L, tune_skipped=skipped)


def simulate_tuned(rng, mean, cov, nchains, step0, rounds, nburnin, niter, scale=None):
    """The tuning rule on a Gaussian target N(mean, cov) with numpy's own generator, vectorised over chains started at the mean:
    returns the final states, the last L and the acceptance fraction after burn-in."""
    mean = np.asarray(mean, dtype=np.float64)
    nd = mean.size
    P = np.linalg.inv(cov)
    lp = lambda v: -0.5 * np.einsum("ci,ij,cj->c", v - mean, P, v - mean)
    x = np.tile(mean, (nchains, 1))
    p0 = lp(x)
    L = np.diag(np.broadcast_to(np.asarray(step0, dtype=np.float64), (nd,)))
    bounds = tune_boundaries(nburnin, rounds)
    if scale is None:
        scale = default_scale(nd)
    nacc = 0
    for it in range(niter):
        if it in bounds:
            Ln, bad = tuned_factor(x, scale)
            if bad < 0:
                L = Ln
        y = x + rng.standard_normal((nchains, nd)) @ L.T
        p1 = lp(y)
        acc = p1 - p0 > np.log(rng.random(nchains))
        x[acc], p0[acc] = y[acc], p1[acc]
        if it >= nburnin:
            nacc += int(acc.sum())
    return x, L, nacc / max(1, (niter - nburnin) * nchains)


# the shape of the statistical test of the tuning rule (tests/test_gpu_mvnormal_step.py; tests/test_mvnormal_step_cpu.py shows the bounds
# for the rule itself): MvNormal2 with correlation rho, chains started at the mean
STAT = dict(nchains=4096, step0=0.05, rounds=4, nburnin=2000, niter=2400, rho=0.95, mean=(0.5, -0.25))


def stat_bounds(x, L, mean, cov, scale):
    """The three checks of the statistical test on final states x [n][2] (independent draws) and the last factor L, each as its largest
    |error| / standard error: the mean (se = sigma / sqrt(n)), every entry of the sample covariance (se^2 = (S_ii S_jj + S_ij^2) / (n - 1))
    and L L^T against scale^2 Sigma (the same se, scaled)."""
    n = x.shape[0]
    sd = np.sqrt(np.diag(cov))
    rm = np.max(np.abs(x.mean(axis=0) - mean) / (sd / np.sqrt(n)))
    se = np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov ** 2) / (n - 1))
    rc = np.max(np.abs(covariance_two_pass(x) - cov) / se)
    rl = np.max(np.abs(L @ L.T - scale * scale * cov) / (scale * scale * se))
    return rm, rc, rl
