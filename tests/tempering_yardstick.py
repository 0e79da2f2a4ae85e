"""numpy restatement of parallel tempering (kmc_config.ntemps >= 2, DESIGN.md sections 2 and 4d): the yardstick of
tests/test_gpu_tempering.py, checked itself by tests/test_tempering_cpu.py.  A ladder of `len(betas)` ensembles; rung t samples
exp(betas[t] logpdf) with the stretch move, DE, the snooker move or a mixture, its draws keyed by the walker word t nwalkers + w,
partners from the complementary half of the same rung; stored log-densities are untempered; neighbouring rungs exchange walkers of
the same index in sweeps.  Built on de_yardstick / snooker_yardstick (the DE family's draws and the order T); the stretch move's
draws and its fused multiply-adds are restated here.  Everything that feeds a stored position is integer or exactly rounded double
arithmetic in the kernels' order; only the log-density and math.log (against the device's log_pos_normal) are to rounding."""
import math

import numpy as np

import de_yardstick as yd
import snooker_yardstick as sy
from de_yardstick import philox4x32_10

TEMPER_KEY = 0x54454D50     # "TEMP"


def _split(a):
    c = 134217729.0 * a                      # 2^27 + 1 (Veltkamp)
    hi = c - (c - a)
    return hi, a - hi


def fma(a, b, c):
    """a * b + c with one rounding, for arrays of moderate magnitude: Dekker's exact product p + e = a b, Knuth's exact sum
    s + t = p + c, and s + (t + e) -- correctly rounded unless the exact value lies within 2^-53 ulp of a rounding boundary
    (never met; tests/test_tempering_cpu.py holds it to the oracle's C fma bit for bit over whole runs)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    return s + (t + e)


def draws_stretch(seed, step, words, nhalf, a_scale):
    """(partner, z, u_acc) of the walker words `words` at `step` = 2 generation + half: DESIGN.md section 2's stream, the 64-bit
    walker counter in counter words 2 and 3."""
    w = np.asarray(words, dtype=np.uint64)
    s_lo, s_hi = np.uint64(step & 0xFFFFFFFF), np.uint64(step >> 32)
    b = philox4x32_10(s_lo, s_hi, w & yd.M32, w >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)
    partner = (b[0] * np.uint64(nhalf)) >> np.uint64(32)
    c0 = math.sqrt(1.0 / a_scale)
    c1 = math.sqrt(a_scale) - math.sqrt(1.0 / a_scale)
    uz = (b[1].astype(np.float64) + 0.5) * 2.0 ** -32
    t = fma(uz, c1, c0)
    kk = (b[2] << np.uint64(20)) | (b[3] >> np.uint64(12))
    u = (kk.astype(np.float64) + 0.5) * 2.0 ** -52
    return partner.astype(np.int64), t * t, u


def swap_pairs(sweep, ntemps):
    """Lower rungs t of the pairs (t, t + 1) of sweep number `sweep`: t = sweep (mod 2), so no rung is in two pairs."""
    return list(range(sweep % 2, ntemps - 1, 2))


def swap_u(seed, sweep, t, nwalkers):
    b = philox4x32_10(np.uint64(sweep & 0xFFFFFFFF), np.uint64(sweep >> 32), np.arange(nwalkers, dtype=np.uint64), t,
                      (seed & 0xFFFFFFFF) ^ TEMPER_KEY, seed >> 32)
    kk = (b[2] << np.uint64(20)) | (b[3] >> np.uint64(12))
    return (kk.astype(np.float64) + 0.5) * 2.0 ** -52


def sweep(pos, logp, betas, seed, n):
    """Swap sweep number n over pos [T, nw, nd], logp [T, nw], in place; returns the accepted exchanges per pair [T - 1]."""
    T, nw = logp.shape
    acc_n = np.zeros(T - 1, dtype=np.int64)
    for t in swap_pairs(n, T):
        lu = np.array([math.log(v) for v in swap_u(seed, n, t, nw)])
        acc = (betas[t] - betas[t + 1]) * (logp[t + 1] - logp[t]) >= lu
        pos[t, acc], pos[t + 1, acc] = pos[t + 1, acc].copy(), pos[t, acc].copy()
        logp[t, acc], logp[t + 1, acc] = logp[t + 1, acc].copy(), logp[t, acc].copy()
        acc_n[t] = int(acc.sum())
    return acc_n


def _half_step(logpdf, pos, logp, nacc, beta, t, seed, gen, half, count, member, a_scale):
    """One half-step of rung t (its arrays pos [nw, nd], logp, nacc), in place."""
    nw, nd = pos.shape
    h = nw // 2
    step = 2 * gen + half
    act = np.arange(half * h, half * h + h)
    words = act + t * nw                                   # the walker word of the draws
    oth0 = (1 - half) * h
    x = pos[act]
    ok = np.ones(h, dtype=bool)
    if member is None:                                     # the stretch move
        partner, z, u = draws_stretch(seed, step, words, h, a_scale)
        xo = pos[oth0 + partner]
        y = fma(z[:, None], x - xo, xo)
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
    p1 = np.asarray(logpdf(y), dtype=np.float64)
    lu = np.array([math.log(v) for v in u])
    with np.errstate(invalid="ignore"):
        if t1 is None:
            acc = (beta * p1 - beta * logp[act]) >= lu
        else:
            acc = ok & (((t1 + beta * p1) - beta * logp[act]) >= lu)
    pos[act[acc]] = y[acc]
    logp[act[acc]] = p1[acc]
    if count:
        nacc[act[acc]] += 1


def emcee_tempered(logpdf, theta0, betas, ngen, nburnin=0, nthin=1, seed=0, a_scale=2.0, move=None, swap_every=1, start=None):
    """The tempered sampler.  `logpdf(X [n, ndim]) -> [n]`; `theta0` [nw, nd] (every rung starts there) or [T, nw, nd]; `move` None
    (stretch), a snooker_yardstick.DE / .Snooker or a list of (member, weight) pairs.  `start`: a dict this function returned -- go on
    from its generation (a checkpoint).  Returns every rung's pos [T, nw, nd], logp, nacc [T, nw], nswap [T - 1], logp_sum [T], rung 0's
    chain and chain_logp, and the generation reached."""
    betas = np.asarray(betas, dtype=np.float64)
    T = betas.size
    if start is None:
        th = np.asarray(theta0, dtype=np.float64)
        pos = np.array(np.broadcast_to(th, (T,) + th.shape[-2:]), dtype=np.float64)
        logp = np.stack([np.asarray(logpdf(pos[t]), dtype=np.float64) for t in range(T)])
        nacc = np.zeros(logp.shape, dtype=np.int64)
        nswap = np.zeros(T - 1, dtype=np.int64)
        logp_sum = np.zeros(T)
        gen0 = 0
    else:
        pos, logp, nacc = np.array(start["pos"]), np.array(start["logp"]), np.array(start["nacc"])
        nswap, logp_sum, gen0 = np.array(start["nswap"]), np.array(start["logp_sum"]), int(start["generation"])
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
            m = members[sy.mix_choice(seed, 2 * gen + half, cum) if len(members) > 1 else 0]   # a function of (seed, step) alone
            for t in range(T):
                _half_step(logpdf, pos[t], logp[t], nacc[t], float(betas[t]), t, seed, gen, half, count, m, a_scale)
        n = gen + 1 - nburnin
        if n > 0 and n % nthin == 0 and n // nthin - 1 < ns:           # the sample is the state BEFORE this generation's sweep
            chain[n // nthin - 1] = pos[0]
            chain_logp[n // nthin - 1] = logp[0]
            logp_sum += logp.sum(axis=1)
        if swap_every > 0 and (gen + 1) % swap_every == 0:
            acc_n = sweep(pos, logp, betas, seed, (gen + 1) // swap_every - 1)
            if count:
                nswap += acc_n
    return dict(pos=pos, logp=logp, nacc=nacc, nswap=nswap, logp_sum=logp_sum, chain=chain, chain_logp=chain_logp, generation=ngen)
