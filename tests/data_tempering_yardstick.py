"""numpy restatement of likelihood tempering (kmc_config.temper_mode = KMC_TEMPER_LIKELIHOOD, DESIGN.md sections 2 and 4d): the
yardstick of tests/test_gpu_data_tempering.py, checked itself by tests/test_data_tempering_cpu.py.  The loop of
tempering_yardstick.emcee_tempered -- the same draws, walker words, partners, mixture choice, sweep schedule and swap stream -- with a
log-density that returns the two values of the data-density value contract, `(pri, S)`:

    tempered value   q = pri + (beta * S)          the product rounded, then the sum
    accept           stretch, snooker: (t1 + q1) - q0 >= log u;  DE: q1 - q0 >= log u;  never when pri1 == -inf
    swap             (beta_t - beta_{t+1}) * (S_{t+1,w} - S_{t,w}) >= log u
    stored           logp = pri + S on every rung; S and pri next to it, exchanged with their row

`loglike_sum` adds up S of the stored states in the order the sweep kernel does for ensembles of up to 256 walkers (one workgroup per
rung: a xor butterfly over each wave's 64 lanes, absent lanes 0.0, then (w0 + w1) + (w2 + w3), then one add into the running sum), so
that it can be compared bit for bit; `logp_sum` is kept as tempering_yardstick keeps it."""
import math

import numpy as np

import de_yardstick as yd
import snooker_yardstick as sy
import tempering_yardstick as ty


def data_logpdf(term_fn, prior_fn=None):
    """`X [n, nd] -> (pri [n], S [n])` from a term function `X -> [n, ndata]` (the body's operation order) and a prior function:
    S is the contract's pairwise tree over the terms."""
    from test_data_density_cpu import pairwise

    def f(X):
        X = np.asarray(X, dtype=np.float64)
        S = pairwise(term_fn(X))
        pri = np.zeros(X.shape[0]) if prior_fn is None else np.asarray(prior_fn(X), dtype=np.float64)
        return pri, S
    return f


def block_sum256(v):
    """The sweep kernel's sum of one workgroup's values (kmc_kernels.hpp: block_sum256), len(v) <= 256."""
    a = np.zeros(256)
    a[:len(v)] = v
    a = a.reshape(4, 64)
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        a = a + a[:, idx ^ off]
    w = a[:, 0]
    return (w[0] + w[1]) + (w[2] + w[3])


def posterior(pri, S):
    """The stored log-density: -inf when the prior is, else pri + S (the value contract)."""
    with np.errstate(invalid="ignore"):
        return np.where(pri == -np.inf, -np.inf, pri + S)


def sweep(pos, logp, like, prior, betas, seed, n):
    """Swap sweep number n, in place, decided on S; returns the accepted exchanges per pair [T - 1]."""
    T, nw = logp.shape
    acc_n = np.zeros(T - 1, dtype=np.int64)
    for t in ty.swap_pairs(n, T):
        lu = np.array([math.log(v) for v in ty.swap_u(seed, n, t, nw)])
        acc = (betas[t] - betas[t + 1]) * (like[t + 1] - like[t]) >= lu
        for a in (pos, logp, like, prior):
            a[t, acc], a[t + 1, acc] = a[t + 1, acc].copy(), a[t, acc].copy()
        acc_n[t] = int(acc.sum())
    return acc_n


def _half_step(logpdf2, pos, logp, like, prior, nacc, beta, t, seed, gen, half, count, member, a_scale):
    """One half-step of rung t, in place (tempering_yardstick._half_step with the tempered value q in the accept test)."""
    nw, nd = pos.shape
    h = nw // 2
    step = 2 * gen + half
    act = np.arange(half * h, half * h + h)
    words = act + t * nw
    oth0 = (1 - half) * h
    x = pos[act]
    ok = np.ones(h, dtype=bool)
    if member is None:
        partner, z, u = ty.draws_stretch(seed, step, words, h, a_scale)
        xo = pos[oth0 + partner]
        y = ty.fma(z[:, None], x - xo, xo)
        t1 = np.array([(nd - 1) * math.log(v) for v in z])
    elif isinstance(member, sy.DE):
        g0 = yd.default_gamma0(nd) if member.gamma0 is None else float(member.gamma0)
        j, k, u, g = yd.draws(seed, step, words, h, g0, member.sigma)
        y = x + g[:, None] * (pos[oth0 + j] - pos[oth0 + k])
        t1 = None
    else:
        z, z1, z2, u = sy.draws_snooker(seed, step, words, h)
        y, s = sy.snooker_proposal(x, pos[oth0 + z], pos[oth0 + z1], pos[oth0 + z2], float(member.gamma))
        with np.errstate(invalid="ignore", over="ignore"):
            a1 = np.abs(1.0 + s)
        ok = np.isfinite(s) & np.isfinite(a1) & (a1 > 0.0)
        t1 = np.array([sy.HASTINGS_DIMS(nd) * math.log(v) if o else 0.0 for v, o in zip(a1, ok)])
        y = np.where(ok[:, None], y, x)
    pri1, S1 = logpdf2(y)
    lu = np.array([math.log(v) for v in u])
    with np.errstate(invalid="ignore"):
        q1 = pri1 + (beta * S1)
        q0 = prior[act] + (beta * like[act])
        if t1 is None:
            acc = (q1 - q0) >= lu
        else:
            acc = ok & (((t1 + q1) - q0) >= lu)
        acc = acc & (pri1 != -np.inf)
        p1 = pri1 + S1
    pos[act[acc]] = y[acc]
    logp[act[acc]] = p1[acc]
    like[act[acc]] = S1[acc]
    prior[act[acc]] = pri1[acc]
    if count:
        nacc[act[acc]] += 1


def emcee_data_tempered(logpdf2, theta0, betas, ngen, nburnin=0, nthin=1, seed=0, a_scale=2.0, move=None, swap_every=1, start=None):
    """The likelihood-tempered sampler.  `logpdf2(X [n, ndim]) -> (pri [n], S [n])`; everything else as
    tempering_yardstick.emcee_tempered.  Returns every rung's pos, logp, loglike, logprior, nacc, nswap, logp_sum, loglike_sum, rung
    0's chain and chain_logp, and the generation reached.  `start`: a dict this function returned (a checkpoint; loglike and logprior
    are evaluated again from its positions, as the library does)."""
    betas = np.asarray(betas, dtype=np.float64)
    T = betas.size
    if start is None:
        th = np.asarray(theta0, dtype=np.float64)
        pos = np.array(np.broadcast_to(th, (T,) + th.shape[-2:]), dtype=np.float64)
        nacc = np.zeros(pos.shape[:2], dtype=np.int64)
        nswap, logp_sum, like_sum, gen0 = np.zeros(T - 1, dtype=np.int64), np.zeros(T), np.zeros(T), 0
    else:
        pos, nacc = np.array(start["pos"]), np.array(start["nacc"])
        nswap, logp_sum, like_sum, gen0 = np.array(start["nswap"]), np.array(start["logp_sum"]), np.array(start["loglike_sum"]), int(start["generation"])
    both = [logpdf2(pos[t]) for t in range(T)]
    prior, like = np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    logp = posterior(prior, like) if start is None else np.array(start["logp"])
    _, nw, nd = pos.shape
    if move is None or isinstance(move, (sy.DE, sy.Snooker)):
        members, cum = [move], [1.0]
    else:
        members = [m for m, _ in move]
        _, cum = sy.mix_weights([float(w) for _, w in move])
    ns = max(0, (ngen - nburnin) // nthin)
    chain, chain_logp = np.zeros((ns, nw, nd)), np.zeros((ns, nw))
    for gen in range(gen0, ngen):
        count = gen + 1 - nburnin > 0
        for half in (0, 1):
            m = members[sy.mix_choice(seed, 2 * gen + half, cum) if len(members) > 1 else 0]
            for t in range(T):
                _half_step(logpdf2, pos[t], logp[t], like[t], prior[t], nacc[t], float(betas[t]), t, seed, gen, half, count, m, a_scale)
        n = gen + 1 - nburnin
        if n > 0 and n % nthin == 0 and n // nthin - 1 < ns:           # the sample is the state BEFORE this generation's sweep
            chain[n // nthin - 1] = pos[0]
            chain_logp[n // nthin - 1] = logp[0]
            logp_sum += logp.sum(axis=1)
            if nw <= 256:
                for t in range(T):
                    like_sum[t] = like_sum[t] + block_sum256(like[t])
            else:
                like_sum += like.sum(axis=1)
        if swap_every > 0 and (gen + 1) % swap_every == 0:
            acc_n = sweep(pos, logp, like, prior, betas, seed, (gen + 1) // swap_every - 1)
            if count:
                nswap += acc_n
    return dict(pos=pos, logp=logp, loglike=like, logprior=prior, nacc=nacc, nswap=nswap, logp_sum=logp_sum, loglike_sum=like_sum,
                chain=chain, chain_logp=chain_logp, generation=ngen)


# ---- the conjugate model of the evidence tests (test_data_tempering_cpu.py, test_gpu_data_tempering.py) ------------------------
# y_j = theta_0 + theta_1 z_j + noise of precision p; prior N(0, s^2 I); both bodies NORMALISED, so Z is the evidence.
EV_TERM = "double mu = x[0] + x[1] * d[0]; double r = d[1] - mu; return -0.5 * p[0] * r * r + p[3];"
EV_PRIOR = "return -0.5 * p[1] * (x[0] * x[0] + x[1] * x[1]) - p[2];"


class EvidenceModel:
    """200 observations, p = 1, s = 0.3 and a ladder of 23 geometric rungs down to 1e-3 plus the prior rung: chosen so that the
    trapezoid of the ANALYTIC <S>_beta over the ladder is within 0.05 nat of the exact log Z (test_data_tempering_cpu.py computes it:
    0.030)."""
    n, s, p = 200, 0.3, 1.0
    nw, G, nburn, start_seed = 64, 1200, 400, 3

    def __init__(self):
        rng = np.random.default_rng(7)
        z = rng.standard_normal(self.n)
        self.y = 0.3 - 0.2 * z + rng.standard_normal(self.n) / math.sqrt(self.p)
        self.A = np.column_stack([np.ones(self.n), z])
        self.D = np.column_stack([z, self.y])
        self.params = [self.p, 1.0 / self.s ** 2, math.log(2.0 * math.pi * self.s ** 2), 0.5 * math.log(self.p / (2.0 * math.pi))]
        b = 1e-3 ** (np.arange(23, dtype=np.float64) / 22.0)
        b[0], b[-1] = 1.0, 1e-3
        self.betas = np.append(b, 0.0)
        self.theta0 = np.array([0.3, -0.2]) + 0.05 * np.random.default_rng(self.start_seed).standard_normal((self.nw, 2))

    def term_fn(self, X):
        P = self.params
        mu = X[:, 0:1] + X[:, 1:2] * self.D[None, :, 0]
        r = self.D[None, :, 1] - mu
        return -0.5 * P[0] * r * r + P[3]

    def prior_fn(self, X):
        P = self.params
        return -0.5 * P[1] * (X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1]) - P[2]

    def mean_loglike(self, beta):
        """<S>_beta under the Gaussian posterior at beta: precision I / s^2 + beta p A'A."""
        A, y, p = self.A, self.y, self.p
        cov = np.linalg.inv(np.eye(2) / self.s ** 2 + beta * p * A.T @ A)
        r = y - A @ (cov @ (beta * p * A.T @ y))
        return self.n * self.params[3] - 0.5 * p * (r @ r + np.trace(A @ cov @ A.T))

    def log_z(self):
        """log N(y; 0, I / p + s^2 A A')."""
        C = np.eye(self.n) / self.p + self.s ** 2 * self.A @ self.A.T
        _, ld = np.linalg.slogdet(C)
        return -0.5 * (self.y @ np.linalg.solve(C, self.y)) - 0.5 * ld - 0.5 * self.n * math.log(2.0 * math.pi)
