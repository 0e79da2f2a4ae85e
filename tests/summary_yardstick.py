"""numpy restatement of the posterior summaries (kmc_sampler_order_stats / kmc_sampler_chain_argmax; include/kissmcmc_hip.h):
the key transform, an MSD radix select written the slow way, np.sort-based order statistics, the arg-max rule with its tie-break,
and the adversarial arrays the tests run through both."""
import numpy as np

SIGN = np.uint64(1 << 63)
DIGIT_BITS = 8


def keys(x):
    """double -> 64-bit key whose unsigned order is the value order: all bits flipped when the sign bit is set, else the sign bit
    flipped.  -inf < ... < -0.0 < +0.0 < ... < +inf; NaNs by bit pattern beyond the infinities."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b & SIGN != 0, ~b, b ^ SIGN)


def unkeys(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k & SIGN != 0, k ^ SIGN, ~k).view(np.float64)


def radix_select(x, rank):
    """The element of 0-based `rank` of the 1-D array x in key order, digit by digit from the top: histogram the next digit of the
    elements under the current prefix, take the digit where the cumulative count crosses the residual rank."""
    k = keys(np.ravel(x))
    assert 0 <= rank < k.size
    prefix, rem = np.uint64(0), int(rank)
    for p in range(64 // DIGIT_BITS):
        shift = np.uint64(64 - DIGIT_BITS * (p + 1))
        under = k if p == 0 else k[(k >> (shift + np.uint64(DIGIT_BITS))) == (prefix >> (shift + np.uint64(DIGIT_BITS)))]
        hist = np.bincount(((under >> shift) & np.uint64(255)).astype(np.int64), minlength=256)
        cum = np.cumsum(hist)
        d = int(np.searchsorted(cum, rem, side="right"))
        rem -= int(cum[d] - hist[d])
        prefix |= np.uint64(d) << shift
    return unkeys(np.array([prefix]))[0]


def sort_by_key(x):
    """x in key order (np.sort alone leaves -0.0 and +0.0 in input order: they compare equal)."""
    x = np.ravel(np.asarray(x, dtype=np.float64))
    return x[np.argsort(keys(x), kind="stable")]


def order_stats(chain, ranks, logp=None, first_sample=0, walkers=None):
    """chain [sample][walker][dim] -> (theta[len(ranks), ndim], logp[len(ranks)] | None, N) over the samples >= first_sample of the
    walkers `walkers` (a boolean mask, indices, or None)."""
    chain = np.asarray(chain, dtype=np.float64)
    w = np.arange(chain.shape[1]) if walkers is None else (np.flatnonzero(walkers) if np.asarray(walkers).dtype == np.bool_ else np.unique(walkers))
    sel = chain[first_sample:, w].reshape(-1, chain.shape[2])
    ranks = np.asarray(ranks, dtype=np.int64)
    th = np.stack([sort_by_key(sel[:, d])[ranks] for d in range(sel.shape[1])], axis=1)
    lp = None if logp is None else sort_by_key(np.asarray(logp)[first_sample:, w])[ranks]
    return th, lp, sel.shape[0]


def argmax(chain, logp, first_sample=0, walkers=None):
    """(theta, logp, sample, walker) of the largest log-density; ties to the smallest sample, then the smallest walker; NaN ignored."""
    logp = np.asarray(logp, dtype=np.float64)
    ok = np.zeros(logp.shape, dtype=bool)
    w = np.arange(logp.shape[1]) if walkers is None else (np.flatnonzero(walkers) if np.asarray(walkers).dtype == np.bool_ else np.unique(walkers))
    ok[first_sample:, w] = True
    ok &= ~np.isnan(logp)
    best = logp[ok].max()
    k, wk = np.argwhere(ok & (logp == best))[0]         # row-major: the first is the smallest (sample, walker)
    return np.asarray(chain)[k, wk], logp[k, wk], int(k), int(wk)


def quantile(sorted_x, q):
    """The interpolation formula of kmc.quantile_ranks on a sorted 1-D array."""
    n = sorted_x.size
    h = q * (n - 1)
    lo = int(np.floor(h))
    hi = min(lo + 1, n - 1)
    frac = h - lo
    return sorted_x[lo] if frac == 0 else sorted_x[lo] + frac * (sorted_x[hi] - sorted_x[lo])


def adversarial(n=3000, seed=0):
    """name -> 1-D array of n doubles, each hard on the select in its own way."""
    rng = np.random.default_rng(seed)
    one = 1.2345678901234567
    mags = np.concatenate([10.0 ** rng.uniform(-300, 300, n // 2 - 8), np.array([0.0, np.inf, 5e-324, 2.2e-308, 1e-310, 1.0, 2.0 ** -1074, 1.7e308])])
    special = np.concatenate([mags, -mags])
    rng.shuffle(special)
    dup = np.where(rng.random(n) < 0.9, 0.75, rng.standard_normal(n))
    return {
        "all_equal": np.full(n, one),
        "one_ulp_apart": rng.permutation(np.where(np.arange(n) % 2 == 0, one, np.nextafter(one, 2.0))),
        "specials": special,                             # +-0.0, +-inf, denormals, negatives of every magnitude
        "ascending": np.sort(rng.standard_normal(n)),
        "descending": np.sort(rng.standard_normal(n))[::-1].copy(),
        "heavy_duplicate": dup,
    }
