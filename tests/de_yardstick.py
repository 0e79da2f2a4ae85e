"""numpy restatement of the differential-evolution move (KMC_MOVE_DE): the yardstick of
tests/test_gpu_de_move.py, checked itself by tests/test_de_move_cpu.py.  Everything but the log-density and math.log is
integer or separately rounded double arithmetic, as the kernels do it."""
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
DE_KEY = 0x44454D56      # "DEMV"


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays of counters (uint64 holding 32-bit words); key words may be scalars."""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & M32 for v in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & M32, np.uint64(k1) & M32
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0 = M0 * c0
        p1 = M1 * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & M32, n2, p0 & M32
        k0, k1 = (k0 + W0) & M32, (k1 + W1) & M32
    return c0, c1, c2, c3


def default_gamma0(ndim):
    return 2.38 / math.sqrt(2.0 * ndim)


def draws(seed, step, walkers, nhalf, gamma0, sigma):
    """(j, k, u_acc, g) of walkers `walkers` (global indices) at `step` = 2 generation + half."""
    w = np.asarray(walkers, dtype=np.uint64)
    s_lo, s_hi = np.uint64(step & 0xFFFFFFFF), np.uint64(step >> 32)
    k0, k1 = (seed & 0xFFFFFFFF) ^ DE_KEY, seed >> 32
    b0 = philox4x32_10(s_lo, s_hi, w, 0, k0, k1)
    b1 = philox4x32_10(s_lo, s_hi, w, 1, k0, k1)
    h = np.uint64(nhalf)
    j = (b0[0] * h) >> np.uint64(32)
    kp = (b0[1] * (h - np.uint64(1))) >> np.uint64(32)
    k = kp + (kp >= j).astype(np.uint64)
    kk = (b0[2] << np.uint64(20)) | (b0[3] >> np.uint64(12))
    u = (kk.astype(np.float64) + 0.5) * 2.0 ** -52
    v = 2.0 * ((b1[0].astype(np.float64) + 0.5) * 2.0 ** -32) - 1.0
    g = gamma0 * (1.0 + sigma * v)
    return j.astype(np.int64), k.astype(np.int64), u, g


def emcee_de(logpdf, theta0, ngen, nburnin=0, nthin=1, seed=0, gamma0=None, sigma=1e-5, logp0=None):
    """The sampler with the DE move.  `logpdf(X [n, ndim]) -> [n]`.  Returns the arrays the GPU tests compare."""
    pos = np.array(theta0, dtype=np.float64)
    nw, nd = pos.shape
    h = nw // 2
    g0 = default_gamma0(nd) if gamma0 is None else float(gamma0)
    logp = np.array(logpdf(pos) if logp0 is None else logp0, dtype=np.float64)
    nacc = np.zeros(nw, dtype=np.int64)
    ns = max(0, (ngen - nburnin) // nthin)
    chain, chain_logp = np.zeros((ns, nw, nd)), np.zeros((ns, nw))
    for gen in range(ngen):
        for half in (0, 1):
            act = np.arange(half * h, half * h + h)
            oth0 = (1 - half) * h
            j, k, u, g = draws(seed, 2 * gen + half, act, h, g0, sigma)
            x = pos[act]
            y = x + g[:, None] * (pos[oth0 + j] - pos[oth0 + k])
            p1 = np.asarray(logpdf(y), dtype=np.float64)
            lu = np.array([math.log(v) for v in u])
            acc = (p1 - logp[act]) >= lu
            pos[act[acc]] = y[acc]
            logp[act[acc]] = p1[acc]
            if gen + 1 - nburnin > 0:
                nacc[act[acc]] += 1
        n = gen + 1 - nburnin
        if n > 0 and n % nthin == 0 and n // nthin - 1 < ns:
            chain[n // nthin - 1] = pos
            chain_logp[n // nthin - 1] = logp
    return dict(pos=pos, logp=logp, nacc=nacc, chain=chain, chain_logp=chain_logp,
                sum=chain.sum(axis=(0, 1)), sumsq=(chain * chain).sum(axis=(0, 1)), n=ns * nw)
