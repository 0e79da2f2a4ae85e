"""CPU: the adaptive ladder's rule (kissmcmc_jl_amd.tempering.adapt_ladder; include/kissmcmc_hip.h above kmc_sampler_get_ladder) and
its numpy yardstick (tests/adaptive_ladder_yardstick.py): the rule against ptemcee's formula, the guard, the operation order, the
yardstick with adaptation off against the two tempering yardsticks, what the rule is for, and the library's refusals (validation
needs no device)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import adaptive_ladder_yardstick as ay
import data_tempering_yardstick as dy
import snooker_yardstick as sy
import tempering_yardstick as ty
from tempering_yardstick import fma

EPS = 2.0 ** -52


def ptemcee_betas(betas, A, k, lag, time):
    """ptemcee's _get_ladder_adjustment in its betas form, restated independently of adapt_ladder: no S, no log."""
    betas = np.array(betas, dtype=np.float64)
    kappa = lag / (k + lag) / time
    dS = kappa * (A[:-1] - A[1:])
    deltaTs = np.diff(1.0 / betas[:-1]) * np.exp(dS)
    betas[1:-1] = 1.0 / (np.cumsum(deltaTs) + 1.0)
    return betas


def random_ladder(rng, T, last_zero):
    """A valid ladder whose gaps in 1 / beta are exp(S_j) with |S_j| <= 2, and a last rung below the others (or 0)."""
    tau = 1.0 + np.cumsum(np.exp(rng.uniform(-2.0, 2.0, T - 2)))
    b = np.concatenate(([1.0], 1.0 / tau, [0.0 if last_zero else rng.uniform(0.1, 0.9) / tau[-1]]))
    assert np.all(np.diff(b) < 0)
    return b


@pytest.mark.parametrize("T", [3, 4, 7, 64])
@pytest.mark.parametrize("last_zero", [False, True])
def test_one_update_is_ptemcees_formula(kmc, T, last_zero):
    """betas' against deltaTs = diff(1 / betas[:-1]) * exp(dS), betas[1:-1] = 1 / (cumsum(deltaTs) + 1), to T * 4 * 2^-52 relative: two
    exp / log roundings per term, summed over at most T terms.  adapt_ladder goes through S = log(gap), so log's rounding reaches a
    term multiplied by |S|: the ladders drawn here keep |S_j| <= 2 and |dS_j| <= 1/2 (time = 2), where the count of two roundings per
    term holds -- |S| 2^-53 from the log, |S'| 2^-53 from the sum, 2^-53 from exp stay below 4 * 2^-52 together with the reference's
    own three.  The last rung is 0 (the likelihood mode's prior rung: ptemcee exactly) or finite."""
    from kissmcmc_jl_amd.tempering import adapt_ladder
    rng = np.random.default_rng(100 * T + last_zero)
    moved = 0
    for _ in range(50):
        b = random_ladder(rng, T, last_zero)
        A = rng.integers(0, 257, T - 1) / 256.0
        k, lag, time = int(rng.integers(0, 5000)), 1000.0, 2.0
        b1, S1, skipped = adapt_ladder(b, ay.initial_S(b), A, k, lag, time)
        want = ptemcee_betas(b, A, k, lag, time)
        if skipped:                                      # (the finite last rung's guard: ptemcee would have let the ladder cross)
            assert not last_zero and not want[-2] > want[-1]
            np.testing.assert_array_equal(b1, b)
            continue
        moved += 1
        assert b1[0] == 1.0 and b1[-1] == b[-1] and np.all(np.diff(b1) < 0)
        assert np.all(np.abs(b1 - want) <= T * 4 * EPS * want), np.max(np.abs(b1 - want) / np.maximum(want, 1e-300)) / EPS
        np.testing.assert_array_equal(S1, ay.initial_S(b) + (lag / (float(k) + lag)) / time * (A[:-1] - A[1:]))
    assert moved >= 25


def test_the_guard_leaves_a_ladder_that_would_cross_unchanged(kmc):
    from kissmcmc_jl_amd.tempering import adapt_ladder
    b = np.array([1.0, 0.5, 0.11, 0.1])
    S = ay.initial_S(b)
    b1, S1, skipped = adapt_ladder(b, S, np.array([1.0, 1.0, 0.0]), 0, lag=1.0, time=0.01)        # kappa = 100: beta'_2 ~ e^-100
    assert skipped == 1
    np.testing.assert_array_equal(b1, b)
    np.testing.assert_array_equal(S1, S)
    assert ptemcee_betas(b, np.array([1.0, 1.0, 0.0]), 0, 1.0, 0.01)[2] < 0.1                      # ptemcee's own formula crosses here
    # a non-finite candidate is refused too: S' = +inf gives tau = inf, beta' = 0, not above a last rung of 0
    b0 = np.array([1.0, 0.5, 0.0])
    b1, S1, skipped = adapt_ladder(b0, np.array([np.inf]), np.array([0.5, 0.5]), 3, 10.0, 10.0)
    assert skipped == 1 and np.array_equal(b1, b0) and S1[0] == np.inf
    # with the last rung at 0 a finite update is never refused
    assert adapt_ladder(b0, ay.initial_S(b0), np.array([1.0, 0.0]), 0, 1.0, 0.01)[2] == 0


def test_the_operation_order_is_pinned_on_a_hand_computed_case(kmc):
    """Four rungs 1, 0.6, 0.3, 0.1; 40 walkers of which 13, 29 and 7 were exchanged; round 8, lag 10, time 7.  Step by step in Python
    floats, each operation rounded on its own: kappa = (10 / (8 + 10)) / 7, S'_j = S_j + kappa * (A_{j-1} - A_j).  The case was chosen
    so that each other order -- lag / ((k + lag) * time), a fused multiply-add, kappa A_{j-1} - kappa A_j -- changes a bit of S'."""
    from kissmcmc_jl_amd.tempering import adapt_ladder
    b = np.array([1.0, 0.6, 0.3, 0.1])
    S = ay.initial_S(b)
    assert [float(s).hex() for s in S] == ["-0x1.9f323ecbf984ap-2", "0x1.058aefa811452p-1"]       # log(1 / 0.6 - 1), log(1 / 0.3 - 1 / 0.6)
    A = np.array([13, 29, 7], dtype=np.float64) / 40.0
    k, lag, time = 8, 10.0, 7.0
    kappa = (lag / (float(k) + lag)) / time
    assert kappa.hex() == "0x1.4514514514515p-4"
    want = [S[j] + kappa * (A[j] - A[j + 1]) for j in range(2)]
    assert [w.hex() for w in want] == ["-0x1.bfb446ec7b8ccp-2", "0x1.1be4553e6aaacp-1"]
    b1, S1, skipped = adapt_ladder(b, S, A, k, lag, time)
    assert skipped == 0 and [float(s).hex() for s in S1] == [w.hex() for w in want]
    alt = lag / ((float(k) + lag) * time)
    assert [S[j] + alt * (A[j] - A[j + 1]) for j in range(2)] != want
    assert [float(fma(kappa, A[j] - A[j + 1], S[j])) for j in range(2)] != want
    assert [S[j] + (kappa * A[j] - kappa * A[j + 1]) for j in range(2)] != want
    tau1 = 1.0 + math.exp(want[0])
    tau2 = tau1 + math.exp(want[1])
    np.testing.assert_allclose(b1, [1.0, 1.0 / tau1, 1.0 / tau2, 0.1], rtol=4 * EPS)               # (exp: to rounding)


def _same(a, b, keys):
    for key in keys:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


@pytest.mark.parametrize("mv", ["stretch", "mix"])
def test_with_adaptation_off_the_yardstick_is_the_tempering_yardstick(kmc, oracle, mv):
    move = None if mv == "stretch" else [(sy.DE(), 0.8), (sy.Snooker(), 0.2)]
    betas = [1.0, 0.6, 0.35, 0.2, 0.1]
    th = np.random.default_rng(2).standard_normal((40, 3))
    f = lambda X: oracle.logpdf_batch(0, [0.0, 1.0], X)
    keys = ("pos", "logp", "nacc", "nswap", "logp_sum", "chain", "chain_logp", "generation")
    for adapt in (None, False):
        got = ay.emcee_tempered(f, th, betas, 24, 10, 2, seed=5, move=move, swap_every=3, adapt=adapt)
        _same(got, ty.emcee_tempered(f, th, betas, 24, 10, 2, seed=5, move=move, swap_every=3), keys)
        np.testing.assert_array_equal(got["betas"], betas)
        assert got["skipped"] == 0 and not got["round_acc"].any() and not got["history"]
    on = ay.emcee_tempered(f, th, betas, 24, 10, 2, seed=5, move=move, swap_every=1, adapt=dict(time=2.0))
    assert not np.array_equal(on["betas"], betas) and on["betas"][0] == 1.0 and on["betas"][-1] == 0.1
    # a checkpoint after an odd number of sweeps (a half-finished round) continues to the same bits
    cut = ay.emcee_tempered(f, th, betas, 7, 10, 2, seed=5, move=move, swap_every=1, adapt=dict(time=2.0))
    assert cut["round_acc"].any()
    rest = ay.emcee_tempered(f, None, betas, 24, 10, 2, seed=5, move=move, swap_every=1, adapt=dict(time=2.0), start=cut)
    _same(rest, on, ("pos", "logp", "nacc", "nswap", "betas", "S", "round_acc"))


def test_with_adaptation_off_the_data_yardstick_is_the_data_tempering_yardstick(kmc):
    m = small_evidence_model()
    f = dy.data_logpdf(m.term_fn, m.prior_fn)
    betas = [1.0, 0.4, 0.1, 0.0]
    th = m.theta0[:32]
    got = ay.emcee_data_tempered(f, th, betas, 16, 6, 1, seed=3, swap_every=1)
    want = dy.emcee_data_tempered(f, th, betas, 16, 6, 1, seed=3, swap_every=1)
    _same(got, want, ("pos", "logp", "loglike", "logprior", "nacc", "nswap", "logp_sum", "loglike_sum", "chain", "chain_logp"))
    on = ay.emcee_data_tempered(f, th, betas, 16, 6, 1, seed=3, swap_every=1, adapt=dict(time=2.0))
    assert not np.array_equal(on["betas"], betas) and on["betas"][-1] == 0.0 and np.all(np.diff(on["betas"]) < 0)


def small_evidence_model():
    """data_tempering_yardstick's conjugate regression at 60 observations."""
    class Model(dy.EvidenceModel):
        n = 60
    return Model()


# ---- what the rule is for -------------------------------------------------------------------------------------------------
# A d-dimensional unit Gaussian tempered as a whole: swap acceptance between rungs t and t + 1 depends on beta_t / beta_{t+1} alone, so
# equal acceptance on every pair means a geometric ladder.  6 rungs started LINEAR from 1 to 0.05 (log-spacings max / min = 7.44),
# 256 walkers x 4 dimensions, the stretch move, swap_every = 1, time = 5, lag = 1000, 800 generations of burn-in (400 rounds); start
# default_rng(seed).standard_normal((256, 4)), sampler seed = seed.  The yardstick, seeds 0 .. 9, ended with max / min of the interior
# log-spacings log(beta_t / beta_{t+1}) at
#     1.0489 1.0362 1.0563 1.0653 1.0758 1.0386 1.0710 1.0614 1.0268 1.0663        (no round skipped in any run)
# Bound: the worst seed's ratio plus half its distance from 1: 1.0758 + 0.0379.
CONV = dict(T=6, nw=256, nd=4, G=800, lag=1000.0, time=5.0)
CONV_BOUND = 1.1137


def conv_start(seed):
    return np.linspace(1.0, 0.05, CONV["T"]), np.random.default_rng(seed).standard_normal((CONV["nw"], CONV["nd"]))


@functools.lru_cache(maxsize=None)
def conv_yardstick(seed):
    """The yardstick's run of the convergence case (computed once; the GPU test of the same case compares against it)."""
    import oracle
    oracle.build()
    betas, th = conv_start(seed)
    return ay.emcee_tempered(lambda X: oracle.logpdf_batch(0, [0.0, 1.0], X), th, betas, CONV["G"], nburnin=CONV["G"], seed=seed,
                             adapt=dict(lag=CONV["lag"], time=CONV["time"]))


def spacing_ratio(betas):
    ls = np.log(betas[:-1] / betas[1:])
    return ls.max() / ls.min()


def test_a_linear_ladder_over_a_gaussian_becomes_geometric(kmc):
    """See the comment above CONV: bound 1.1137 from the ten seeds' 1.0489 1.0362 1.0563 1.0653 1.0758 1.0386 1.0710 1.0614 1.0268
    1.0663; the linear start's 7.44 is far outside it."""
    betas0, _ = conv_start(0)
    assert spacing_ratio(betas0) > 3.6 > CONV_BOUND                       # (7.44 over all five spacings)
    r = conv_yardstick(0)
    ratio = spacing_ratio(r["betas"])
    print("interior log-spacings max / min:", ratio, "betas", r["betas"], "skipped", r["skipped"])
    assert r["betas"][0] == 1.0 and r["betas"][-1] == 0.05 and np.all(np.diff(r["betas"]) < 0)
    assert ratio < CONV_BOUND, ratio
    assert len(r["history"]) == CONV["G"] // 2 and r["skipped"] == 0


# ---- the library's side that needs no device ------------------------------------------------------------------------------
def _cfg(_lib, betas, **kw):
    c = _lib.Config()
    c.dtype, c.density = _lib.F64, _lib.GAUSSIAN_ISO
    c.params[0], c.params[1] = 0.0, 1.0
    c.nwalkers, c.ndim, c.ngenerations, c.nburnin, c.nthin = 10, 2, 20, 10, 1
    c.a_scale, c.seed = 2.0, 1
    if betas is not None:
        c.betas, c.ntemps, c.swap_every = betas.ctypes.data_as(C.c_void_p), betas.size, 1
    c.adapt, c.adapt_lag, c.adapt_time = 1, 10000.0, 100.0
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_validation_refuses_by_status_and_names_the_adaptive_ladder(kmc):
    from kissmcmc_jl_amd import _lib
    L = _lib.lib()
    b4, b2 = np.array([1.0, 0.5, 0.2, 0.1]), np.array([1.0, 0.5])

    def v(betas=b4, **kw):
        st = L.kmc_validate(C.byref(_cfg(_lib, betas, **kw)))
        return st, L.kmc_last_error().decode()

    assert v()[0] == _lib.OK and v(adapt_until=10)[0] == _lib.OK and v(adapt_until=3)[0] == _lib.OK
    assert v(adapt=0, adapt_lag=0.0, adapt_time=0.0)[0] == _lib.OK                         # zeroed: off
    for kw in (dict(betas=None), dict(betas=b2), dict(swap_every=0), dict(adapt_until=-1), dict(adapt_until=11), dict(adapt_lag=0.0),
               dict(adapt_lag=-1.0), dict(adapt_lag=float("inf")), dict(adapt_lag=float("nan")), dict(adapt_time=0.0),
               dict(adapt_time=-2.0), dict(adapt_time=float("inf")), dict(adapt_time=float("nan")), dict(adapt=2)):
        st, msg = v(**kw)
        assert st == _lib.ERR_BAD_ARG and msg.startswith("adaptive ladder:"), (kw, st, msg)
    # what tempering refuses stays refused, in tempering's name
    st, msg = v(dtype=_lib.F32)
    assert st == _lib.ERR_UNSUPPORTED and msg.startswith("parallel tempering") and "KMC_F32" in msg
    st, msg = v(betas=np.array([1.0, 0.5, 0.5, 0.1]))
    assert st == _lib.ERR_BAD_ARG and "strictly decreasing" in msg and msg.startswith("parallel tempering")


def test_the_python_argument(kmc):
    from kissmcmc_jl_amd import _lib
    from kissmcmc_jl_amd.tempering import apply_adapt
    c = _lib.Config()
    assert apply_adapt(c, None) is None and apply_adapt(c, False) is None and c.adapt == 0 and c.adapt_lag == 0.0
    assert apply_adapt(c, True) == dict(lag=10000.0, time=100.0, until=None) and (c.adapt, c.adapt_until, c.adapt_lag, c.adapt_time) == (1, 0, 10000.0, 100.0)
    assert apply_adapt(c, dict(time=5, until=30))["until"] == 30 and (c.adapt_until, c.adapt_lag, c.adapt_time) == (30, 10000.0, 5.0)
    assert apply_adapt(c, dict(until=0))["until"] is None and (c.adapt, c.adapt_until) == (1, 0)      # 0 is nburnin, as in the C header
    for bad in (1, "yes", dict(rate=3)):
        with pytest.raises(ValueError, match="adapt"):
            apply_adapt(c, bad)
    if _lib.lib().kmc_device_count() == 0:                                                  # (creation validates before it looks for a device)
        with pytest.raises(kmc.KmcError, match="adaptive ladder: ntemps must be >= 3"):
            kmc.Sampler(kmc.GaussianIso(), 10, 2, 20, 10, betas=[1.0, 0.5], adapt=True)
