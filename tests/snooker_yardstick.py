"""numpy restatement of the snooker move (KMC_MOVE_SNOOKER) and of the DE / snooker mixtures (KMC_MOVE_MIX), DESIGN.md section 2:
the yardstick of tests/test_gpu_snooker_move.py, checked itself by tests/test_snooker_move_cpu.py.  Everything that feeds a stored
position is integer or separately rounded double arithmetic in the kernels' order -- the two sums of the snooker proposal in the
fixed order T below; only the log-density and math.log (against the device's log_pos_normal) are to rounding."""
import math

import numpy as np

import de_yardstick as yd
from de_yardstick import philox4x32_10

MIX_KEY = 0x4D495856     # "MIXV"


class DE:
    def __init__(self, gamma0=None, sigma=1e-5):
        self.gamma0, self.sigma = gamma0, sigma


class Snooker:
    def __init__(self, gamma=1.7):
        self.gamma = gamma


def T(v):
    """The reduction order of the snooker sums over the last axis: the pairwise tree over the terms in index order, padded with
    +0.0 to a power of two (at least 2), and + 0.0 at the root (how far a row is padded then changes no bit)."""
    v = np.asarray(v, dtype=np.float64)
    n = v.shape[-1]
    p = 2
    while p < n:
        p *= 2
    a = np.zeros(v.shape[:-1] + (p,))
    a[..., :n] = v
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0] + 0.0


def draws_snooker(seed, step, walkers, nhalf):
    """(z, z1, z2, u_acc) of walkers `walkers` (global indices) at `step` = 2 generation + half: the DE key family, blocks 2 and 3.
    z = floor(w0 h / 2^32); z1 from the h - 1 others; z2 from the h - 2 others (skipping the smaller, then the larger)."""
    assert nhalf >= 3
    w = np.asarray(walkers, dtype=np.uint64)
    s_lo, s_hi = np.uint64(step & 0xFFFFFFFF), np.uint64(step >> 32)
    k0, k1 = (seed & 0xFFFFFFFF) ^ yd.DE_KEY, seed >> 32
    b2 = philox4x32_10(s_lo, s_hi, w, 2, k0, k1)
    b3 = philox4x32_10(s_lo, s_hi, w, 3, k0, k1)
    h = np.uint64(nhalf)
    one, sh = np.uint64(1), np.uint64(32)
    z = (b2[0] * h) >> sh
    z1 = (b2[1] * (h - one)) >> sh
    z1 = z1 + (z1 >= z).astype(np.uint64)
    lo, hi = np.minimum(z, z1), np.maximum(z, z1)
    z2 = (b2[2] * (h - np.uint64(2))) >> sh
    z2 = z2 + (z2 >= lo).astype(np.uint64)
    z2 = z2 + (z2 >= hi).astype(np.uint64)
    kk = (b3[2] << np.uint64(20)) | (b3[3] >> np.uint64(12))
    u = (kk.astype(np.float64) + 0.5) * 2.0 ** -52
    return z.astype(np.int64), z1.astype(np.int64), z2.astype(np.int64), u


def mix_weights(weights):
    """Normalised in double, in list order; the cumulative weights in the same order."""
    total = 0.0
    for w in weights:
        total += w
    p = [w / total for w in weights]
    cum, c = [], 0.0
    for v in p:
        c += v
        cum.append(c)
    return p, cum


def mix_choices(seed, steps, cum):
    """Members of the half-steps `steps` (array): the first whose cumulative weight exceeds u_mix = (w0 + 1/2) 2^-32 of Philox key
    {seed_lo ^ "MIXV", seed_hi}, counter {step_lo, step_hi, 0, 0}; the last member catches rounding."""
    st = np.asarray(steps, dtype=np.uint64)
    b = philox4x32_10(st & yd.M32, st >> np.uint64(32), 0, 0, (seed & 0xFFFFFFFF) ^ MIX_KEY, seed >> 32)
    u = (b[0].astype(np.float64) + 0.5) * 2.0 ** -32
    out = np.full(st.shape, len(cum) - 1, dtype=np.int64)
    for i in range(len(cum) - 2, -1, -1):
        out[cum[i] > u] = i
    return out


def mix_choice(seed, step, cum):
    return int(mix_choices(seed, [step], cum)[0])


def snooker_proposal(x, xz, x1, x2, gamma):
    """(y, s): d = x - z, s = gamma (T(d (z1 - z2)) / T(d d)), y = x + d s -- each operation rounded on its own."""
    d = x - xz
    n2 = T(d * d)
    q = T(d * (x1 - x2))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = gamma * (q / n2)
        y = x + d * s[:, None]
    return y, s


HASTINGS_DIMS = lambda nd: nd - 1      # (tests/test_snooker_move_cpu.py replaces this to see the stationary test fail)


def emcee_moves(logpdf, theta0, ngen, nburnin=0, nthin=1, seed=0, move=None, logp0=None):
    """The sampler with `move` a Snooker, a DE or a list of (member, weight) pairs of them.  `logpdf(X [n, ndim]) -> [n]`.
    Returns the arrays the GPU tests compare, and `members`: the member index of every half-step."""
    pos = np.array(theta0, dtype=np.float64)
    nw, nd = pos.shape
    h = nw // 2
    if isinstance(move, (DE, Snooker)):
        members, cum = [move], [1.0]
    else:
        members = [m for m, _ in move]
        _, cum = mix_weights([float(w) for _, w in move])
    logp = np.array(logpdf(pos) if logp0 is None else logp0, dtype=np.float64)
    nacc = np.zeros(nw, dtype=np.int64)
    ns = max(0, (ngen - nburnin) // nthin)
    chain, chain_logp = np.zeros((ns, nw, nd)), np.zeros((ns, nw))
    used = []
    for gen in range(ngen):
        for half in (0, 1):
            step = 2 * gen + half
            act = np.arange(half * h, half * h + h)
            oth0 = (1 - half) * h
            m = members[mix_choice(seed, step, cum) if len(members) > 1 else 0]
            used.append(members.index(m))
            x = pos[act]
            if isinstance(m, DE):
                g0 = yd.default_gamma0(nd) if m.gamma0 is None else float(m.gamma0)
                j, k, u, g = yd.draws(seed, step, act, h, g0, m.sigma)
                y = x + g[:, None] * (pos[oth0 + j] - pos[oth0 + k])
                t1 = np.zeros(h)
                ok = np.ones(h, dtype=bool)
            else:
                z, z1, z2, u = draws_snooker(seed, step, act, h)
                y, s = snooker_proposal(x, pos[oth0 + z], pos[oth0 + z1], pos[oth0 + z2], float(m.gamma))
                with np.errstate(invalid="ignore", over="ignore"):
                    a1 = np.abs(1.0 + s)
                ok = np.isfinite(s) & np.isfinite(a1) & (a1 > 0.0)
                t1 = np.array([HASTINGS_DIMS(nd) * math.log(v) if o else 0.0 for v, o in zip(a1, ok)])
                y = np.where(ok[:, None], y, x)          # (a rejected proposal's density is evaluated somewhere harmless)
            p1 = np.asarray(logpdf(y), dtype=np.float64)
            lu = np.array([math.log(v) for v in u])
            with np.errstate(invalid="ignore"):
                acc = ok & (((t1 + p1) - logp[act]) >= lu) if not isinstance(m, DE) else (p1 - logp[act]) >= lu
            pos[act[acc]] = y[acc]
            logp[act[acc]] = p1[acc]
            if gen + 1 - nburnin > 0:
                nacc[act[acc]] += 1
        n = gen + 1 - nburnin
        if n > 0 and n % nthin == 0 and n // nthin - 1 < ns:
            chain[n // nthin - 1] = pos
            chain_logp[n // nthin - 1] = logp
    return dict(pos=pos, logp=logp, nacc=nacc, chain=chain, chain_logp=chain_logp,
                sum=chain.sum(axis=(0, 1)), sumsq=(chain * chain).sum(axis=(0, 1)), n=ns * nw, members=np.array(used))
