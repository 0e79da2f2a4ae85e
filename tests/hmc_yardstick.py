"""The yardstick of the HMC step of the many-chain Metropolis sampler (kmc.HMCStep; the definition is in include/kissmcmc_hip.h):
plain Python and numpy, nothing of the product.

The rule is restated operation for operation -- numpy's elementwise products and sums are rounded one by one, never fused -- with the
five gradients of the menu densities in the operation order of kmc_hmc.hpp.  `metropolis` is the reference's loop
(src/samplers.jl:96-126) for many chains at once, fed the draws of an iteration and a log-density from outside: the tests pass the
CPU oracle's `metropolis_draw`, `philox4x32_10` and `logpdf` (`oracle_draws`, `oracle_logpdf`), or numpy's own generator.

Parameters are the C ABI's (`pdf.params()`): `digest` turns them into what the kernels take, as the library does."""
import math

import numpy as np


def digest(density, params):
    p = [float(v) for v in params] + [0.0] * 6
    if density == "gaussian_iso":
        return [p[0], 1.0 / p[1]]
    if density == "rosenbrock":
        return [p[0], p[1], 1.0 / p[2]]
    return p[:6]


# ---- the gradients: p digested, x [nchains][ndim] ----
def grad_gaussian_iso(p, x):
    t = (x - p[0]) * p[1]
    return -(t * p[1])


def grad_exponential(p, x):
    return np.full_like(x, -p[0])


def grad_rosenbrock(p, x):
    a, b, s = p[0], p[1], p[2]
    n = x.shape[1]
    g = np.empty_like(x)
    for k in range(n):
        acc = np.zeros(x.shape[0])
        if k >= 1:
            d = x[:, k] - x[:, k - 1] * x[:, k - 1]
            acc = (2.0 * b) * d
        if k <= n - 2:
            d = x[:, k + 1] - x[:, k] * x[:, k]
            acc = acc - ((4.0 * b) * x[:, k]) * d
            acc = acc - 2.0 * (a - x[:, k])
        g[:, k] = -(acc * s)
    return g


def grad_lognormal(p, x):
    g = np.zeros_like(x)
    ok = x > 0.0
    with np.errstate(all="ignore"):
        lx = np.log(np.where(ok, x, 1.0))
        t = (lx - p[0]) / p[1]
        v = -((1.0 + t / p[1]) / np.where(ok, x, 1.0))
    g[ok] = v[ok]
    return g


def grad_mvnormal2(p, x):
    d0, d1 = x[:, 0] - p[0], x[:, 1] - p[1]
    return np.stack([-(p[2] * d0 + p[3] * d1), -(p[3] * d0 + p[4] * d1)], axis=1)


GRADS = dict(gaussian_iso=grad_gaussian_iso, exponential=grad_exponential, rosenbrock=grad_rosenbrock, lognormal=grad_lognormal,
             mvnormal2=grad_mvnormal2)


def grad_of(density, params):
    p = digest(density, params)
    return lambda x: GRADS[density](p, np.atleast_2d(np.asarray(x, dtype=np.float64)))


# ---- the rule ----
def jitter_factor(j, jitter):
    """f = 1.0 + jitter * (((double)j + 0.5) * 2^-11 - 1.0); j: the low 12 bits of w3 of Philox block 0."""
    return 1.0 + jitter * ((np.asarray(j, dtype=np.float64) + 0.5) * 2.0 ** -11 - 1.0)


def kinetic(m):
    s = m[:, 0] * m[:, 0]
    for i in range(1, m.shape[1]):
        s = s + m[:, i] * m[:, i]
    return 0.5 * s


def leapfrog(grad, x, m, step, f, nleap):
    """nleap leapfrog steps from (x, m) [nchains][ndim]; step a scalar or [ndim], f [nchains].  Returns (y, m)."""
    e = np.atleast_1d(np.asarray(step, dtype=np.float64))[None, :] * np.asarray(f, dtype=np.float64)[:, None]
    h = 0.5 * e
    y, m = np.array(x, dtype=np.float64), np.array(m, dtype=np.float64)
    with np.errstate(all="ignore"):
        g = grad(y)
        for _ in range(nleap):
            m = m + h * g
            y = y + e * m
            g = grad(y)
            m = m + h * g
    return y, m


def metropolis(logpdf, grad, draws, theta0, step, nleap, jitter, niter, nburnin, nthin):
    """Many chains of src/samplers.jl:96-126 with the HMC proposal.  `logpdf(X)` -> [nchains] log-densities of rows, `grad(X)` ->
    [nchains][ndim], `draws(it)` -> (z [nchains][ndim], u [nchains], j [nchains]).  Returns the dict mvnormal_step_yardstick.metropolis
    returns (`margin` = the smallest finite |(p1 - K1) - (p0 - K0) - log u| met), plus `nonfinite` = the proposals whose log-density
    was not finite and `nonfinite_accepted` = how many of those were accepted."""
    x = np.array(theta0, dtype=np.float64)
    nc, nd = x.shape
    step = np.ascontiguousarray(np.broadcast_to(np.asarray(step, dtype=np.float64), (nd,)))
    p0 = np.asarray(logpdf(x), dtype=np.float64).copy()
    nacc = np.zeros(nc, dtype=np.int64)
    chain, chain_logp = [], []
    margin = math.inf
    nonfinite = nonfinite_accepted = 0
    for it in range(niter):
        n = it + 1 - nburnin                                              # :96
        z, u, j = draws(it)
        lu = np.array([math.log(v) for v in u])
        f = jitter_factor(j, jitter)
        m0 = np.array(z, dtype=np.float64)
        K0 = kinetic(m0)
        y, m1 = leapfrog(grad, x, m0, step, f, nleap)
        with np.errstate(all="ignore"):
            p1 = np.asarray(logpdf(y), dtype=np.float64)
            K1 = kinetic(m1)
            lhs = (p1 - K1) - (p0 - K0)
            d = lhs - lu
            acc = lhs > lu                                                # :101, strict; NaN compares false
        fin = np.isfinite(d)
        if fin.any():
            margin = min(margin, float(np.min(np.abs(d[fin]))))
        bad = ~np.isfinite(p1)
        nonfinite += int(bad.sum())
        nonfinite_accepted += int((bad & acc).sum())
        x[acc] = y[acc]
        p0[acc] = p1[acc]
        if n > 0:
            nacc += acc                                                   # :105
        if n > 0 and n % nthin == 0:                                      # :108, :112
            chain.append(x.copy())
            chain_logp.append(p0.copy())
    ns = len(chain)
    return dict(chain=np.array(chain).reshape(ns, nc, nd), chain_logp=np.array(chain_logp).reshape(ns, nc), naccept=nacc,
                final_pos=x, final_logp=p0, margin=margin, states_at={}, chol=np.diag(step), tune_skipped=0,
                nonfinite=nonfinite, nonfinite_accepted=nonfinite_accepted)


# ---- the library's stream and log-densities, from the CPU oracle ----
def oracle_draws(oracle, seed, nchains, ndim):
    """draws(it) from the Metropolis stream: the normals and the uniform from oracle.metropolis_draw, j = w3 & 0xFFF of Philox block 0
    (key {seed_lo ^ 0x4d455452, seed_hi}, counter {it_lo, it_hi, chain, 0})."""
    key = ((seed & 0xFFFFFFFF) ^ 0x4d455452, (seed >> 32) & 0xFFFFFFFF)

    def draws(it):
        z, u, j = np.empty((nchains, ndim)), np.empty(nchains), np.empty(nchains, dtype=np.int64)
        for c in range(nchains):
            z[c], u[c] = oracle.metropolis_draw(seed, it, c, ndim)
            j[c] = oracle.philox4x32_10((it & 0xFFFFFFFF, (it >> 32) & 0xFFFFFFFF, c, 0), key)[3] & 0xFFF
        return z, u, j
    return draws


def oracle_logpdf(oracle, density_id, params):
    return lambda X: oracle.logpdf_batch(density_id, params, np.atleast_2d(X))


def numpy_draws(rng, nchains, ndim):
    return lambda it: (rng.standard_normal((nchains, ndim)), 1.0 - rng.random(nchains), rng.integers(0, 4096, nchains))


# the shape of the statistical test (tests/test_hmc_cpu.py on the rule itself, tests/test_gpu_hmc.py on the device): an 8-D
# GaussianIso(mu, sigma), chains started at the mean
STAT = dict(nchains=4096, ndim=8, eps=0.585, nleap=4, jitter=0.3, niter=300, nburnin=100)


def stat_errors(x, mu, sigma):
    """The largest |mean - mu| and |variance - sigma^2| over the dimensions of final states x [n][ndim], in standard errors
    (sigma / sqrt(n) and sigma^2 sqrt(2 / (n - 1)): independent Gaussian draws)."""
    n = x.shape[0]
    rm = np.max(np.abs(x.mean(axis=0) - mu)) / (sigma / np.sqrt(n))
    rv = np.max(np.abs(x.var(axis=0, ddof=1) - sigma ** 2)) / (sigma ** 2 * np.sqrt(2.0 / (n - 1)))
    return float(rm), float(rv)
