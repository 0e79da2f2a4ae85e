"""numpy restatement of the adaptive ladder (kmc_config.adapt, DESIGN.md sections 2 and 4d): the yardstick of
tests/test_gpu_adaptive_ladder.py, checked itself by tests/test_adaptive_ladder_cpu.py.  The loops of
tempering_yardstick.emcee_tempered and data_tempering_yardstick.emcee_data_tempered -- their half-steps and their `sweep` as they
are -- with the ladder's state around the sweep:

    a sweep after generation g < adapt_until adds its accepted exchanges per pair into round_acc
    after the odd sweep n of such a generation: (betas, S) <- kissmcmc_jl_amd.tempering.adapt_ladder(betas, S, round_acc / nwalkers,
    k = (n - 1) / 2, lag, time), `skipped` counts the rounds it refused, round_acc is zeroed either way

S_j = log(1 / beta_j - 1 / beta_{j-1}) is computed once from the caller's ladder (math.log: the library's std::log) and is state from
then on.  Everything that was exact or to rounding in the two yardsticks stays so; the ladder adds one `exp` per rung and update that
is to rounding (S itself is exact arithmetic on both sides)."""
import math

import numpy as np

import data_tempering_yardstick as dy
import snooker_yardstick as sy
import tempering_yardstick as ty


def initial_S(betas):
    b = np.asarray(betas, dtype=np.float64)
    return np.array([math.log(1.0 / b[j] - 1.0 / b[j - 1]) for j in range(1, b.size - 1)])


class Ladder:
    """The ladder's state: betas, S, round_acc, skipped (a checkpoint carries all four)."""

    def __init__(self, betas, adapt=None, nburnin=0, start=None):
        from kissmcmc_jl_amd.tempering import ADAPT_LAG, ADAPT_TIME
        self.on = adapt is not None and adapt is not False
        a = {} if adapt in (None, False, True) else dict(adapt)
        self.lag, self.time = float(a.get("lag", ADAPT_LAG)), float(a.get("time", ADAPT_TIME))
        self.until = int(nburnin if a.get("until") is None else a["until"])
        if start is not None and "S" in start:
            self.betas, self.S = np.array(start["betas"], dtype=np.float64), np.array(start["S"], dtype=np.float64)
            self.round_acc, self.skipped = np.array(start["round_acc"], dtype=np.int64), int(start["skipped"])
        else:
            self.betas = np.array(betas, dtype=np.float64)
            self.S = initial_S(self.betas)
            self.round_acc, self.skipped = np.zeros(self.betas.size - 1, dtype=np.int64), 0
        self.history = []                     # (generation, betas) after every committed or refused update

    def after_sweep(self, gen, n, acc_n, nwalkers):
        """What the sweep kernel's tail does after sweep n of generation gen accepted acc_n [T - 1] exchanges."""
        from kissmcmc_jl_amd.tempering import adapt_ladder
        if not self.on or gen >= self.until:
            return
        self.round_acc += acc_n
        if n % 2 == 1:
            A = self.round_acc.astype(np.float64) / float(nwalkers)
            self.betas, self.S, skipped = adapt_ladder(self.betas, self.S, A, (n - 1) // 2, self.lag, self.time)
            self.skipped += skipped
            self.round_acc[:] = 0
            self.history.append((gen, self.betas.copy()))

    def out(self):
        return dict(betas=self.betas.copy(), S=self.S.copy(), round_acc=self.round_acc.copy(), skipped=self.skipped)


def _members(move):
    if move is None or isinstance(move, (sy.DE, sy.Snooker)):
        return [move], [1.0]
    return [m for m, _ in move], sy.mix_weights([float(w) for _, w in move])[1]


def emcee_tempered(logpdf, theta0, betas, ngen, nburnin=0, nthin=1, seed=0, a_scale=2.0, move=None, swap_every=1, start=None, adapt=None):
    """tempering_yardstick.emcee_tempered with `adapt` (None / False: off -- then its results bit for bit --, True, or a dict with any of
    lag, time, until).  Returns what it returns, plus betas (the ladder at the end), S, round_acc, skipped, and `history`."""
    lad = Ladder(betas, adapt, nburnin, start)
    T = lad.betas.size
    if start is None:
        th = np.asarray(theta0, dtype=np.float64)
        pos = np.array(np.broadcast_to(th, (T,) + th.shape[-2:]), dtype=np.float64)
        logp = np.stack([np.asarray(logpdf(pos[t]), dtype=np.float64) for t in range(T)])
        nacc = np.zeros(logp.shape, dtype=np.int64)
        nswap, logp_sum, gen0 = np.zeros(T - 1, dtype=np.int64), np.zeros(T), 0
    else:
        pos, logp, nacc = np.array(start["pos"]), np.array(start["logp"]), np.array(start["nacc"])
        nswap, logp_sum, gen0 = np.array(start["nswap"]), np.array(start["logp_sum"]), int(start["generation"])
    _, nw, nd = pos.shape
    members, cum = _members(move)
    ns = max(0, (ngen - nburnin) // nthin)
    chain, chain_logp = np.zeros((ns, nw, nd)), np.zeros((ns, nw))
    for gen in range(gen0, ngen):
        count = gen + 1 - nburnin > 0
        for half in (0, 1):
            m = members[sy.mix_choice(seed, 2 * gen + half, cum) if len(members) > 1 else 0]
            for t in range(T):
                ty._half_step(logpdf, pos[t], logp[t], nacc[t], float(lad.betas[t]), t, seed, gen, half, count, m, a_scale)
        n = gen + 1 - nburnin
        if n > 0 and n % nthin == 0 and n // nthin - 1 < ns:
            chain[n // nthin - 1] = pos[0]
            chain_logp[n // nthin - 1] = logp[0]
            logp_sum += logp.sum(axis=1)
        if swap_every > 0 and (gen + 1) % swap_every == 0:
            sw = (gen + 1) // swap_every - 1
            acc_n = ty.sweep(pos, logp, lad.betas, seed, sw)
            if count:
                nswap += acc_n
            lad.after_sweep(gen, sw, acc_n, nw)
    return dict(pos=pos, logp=logp, nacc=nacc, nswap=nswap, logp_sum=logp_sum, chain=chain, chain_logp=chain_logp, generation=ngen,
                history=lad.history, **lad.out())


def emcee_data_tempered(logpdf2, theta0, betas, ngen, nburnin=0, nthin=1, seed=0, a_scale=2.0, move=None, swap_every=1, start=None, adapt=None):
    """data_tempering_yardstick.emcee_data_tempered with `adapt`, as above."""
    lad = Ladder(betas, adapt, nburnin, start)
    T = lad.betas.size
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
    logp = dy.posterior(prior, like) if start is None else np.array(start["logp"])
    _, nw, nd = pos.shape
    members, cum = _members(move)
    ns = max(0, (ngen - nburnin) // nthin)
    chain, chain_logp = np.zeros((ns, nw, nd)), np.zeros((ns, nw))
    for gen in range(gen0, ngen):
        count = gen + 1 - nburnin > 0
        for half in (0, 1):
            m = members[sy.mix_choice(seed, 2 * gen + half, cum) if len(members) > 1 else 0]
            for t in range(T):
                dy._half_step(logpdf2, pos[t], logp[t], like[t], prior[t], nacc[t], float(lad.betas[t]), t, seed, gen, half, count, m, a_scale)
        n = gen + 1 - nburnin
        if n > 0 and n % nthin == 0 and n // nthin - 1 < ns:
            chain[n // nthin - 1] = pos[0]
            chain_logp[n // nthin - 1] = logp[0]
            logp_sum += logp.sum(axis=1)
            if nw <= 256:
                for t in range(T):
                    like_sum[t] = like_sum[t] + dy.block_sum256(like[t])
            else:
                like_sum += like.sum(axis=1)
        if swap_every > 0 and (gen + 1) % swap_every == 0:
            sw = (gen + 1) // swap_every - 1
            acc_n = dy.sweep(pos, logp, like, prior, lad.betas, seed, sw)
            if count:
                nswap += acc_n
            lad.after_sweep(gen, sw, acc_n, nw)
    return dict(pos=pos, logp=logp, loglike=like, logprior=prior, nacc=nacc, nswap=nswap, logp_sum=logp_sum, loglike_sum=like_sum,
                chain=chain, chain_logp=chain_logp, generation=ngen, history=lad.history, **lad.out())
