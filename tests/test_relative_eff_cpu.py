"""No GPU: what PSIS-LOO's per-observation relative efficiency decides from the arguments alone (the refusals of kmc_*_relative_eff,
kmc_*_pointwise_weights, kmc_*_psis_loo_reff and kmc_*_psis_tail_reff come before the device is touched and name the value), the
Python forms of ``r_eff``, and the facts about the inputs of tests/test_gpu_relative_eff.py that its comparisons rest on, measured on
the yardsticks (tests/relative_eff_cases.py)."""
import ctypes as C
import inspect

import numpy as np
import pytest

import psis_cases as pc
import psis_yardstick as Y
import relative_eff_cases as rc


def test_calls_are_public(kmc):
    for name in ("relative_eff", "pointwise_weights", "loo", "psis_tail"):
        assert name in kmc.__all__ and callable(getattr(kmc, name))
    for name in ("relative_eff", "pointwise_weights"):
        assert callable(getattr(kmc.Sampler, name))
    for f in (kmc.loo, kmc.Sampler.loo, kmc.psis_tail, kmc.Sampler.psis_tail, kmc.relative_eff, kmc.Sampler.relative_eff):
        assert {"split", "max_lag"} <= set(inspect.signature(f).parameters)
    for f in (kmc.loo, kmc.Sampler.loo, kmc.psis_tail, kmc.Sampler.psis_tail):
        assert inspect.signature(f).parameters["r_eff_j"].default is None
    assert inspect.signature(kmc.loo).parameters["r_eff"].default == 1.0


def test_argument_checks_need_no_device(kmc):
    from kissmcmc_jl_amd import _lib
    L = _lib.lib()
    dp = C.POINTER(C.c_double)
    p = lambda a: a.ctypes.data_as(dp)
    dd = kmc.DataDensity(pc.TERM, np.arange(10.0)[:, None])
    other = kmc.ExprDensity("-0.5*x*x")
    par, chain = np.zeros(6), np.zeros(40 * 3 * 2)
    stats, lp, ru, r10 = np.zeros(4 * 10), np.zeros(10), np.zeros(10), np.ones(10)
    tl, nn, n = np.zeros(10, dtype=np.int64), C.c_int64(-1), C.c_int64(-1)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    err = lambda: L.kmc_last_error()

    def loo(h=dd.user_handle, ns=40, nw=3, thin=1, r=r10, split=1, max_lag=0, first=0, count=10):
        return L.kmc_chain_psis_loo_reff(h, p(par), p(chain), ns, nw, 2, 0, None, thin, None if r is None else p(r), split, max_lag, first, count, 0, 0,
                                         p(stats), p(lp), p(ru), ip(tl), C.byref(nn), C.byref(n), None)

    def reff(h=dd.user_handle, ns=40, nw=3, thin=1, split=1, max_lag=0, first=0, count=10, out=p(ru)):
        return L.kmc_chain_relative_eff(h, p(par), p(chain), ns, nw, 2, 0, None, thin, first, count, split, max_lag, 0, 0, out, None, None, None,
                                        None, None, C.byref(n), None)

    bad = r10.copy()
    bad[4] = 0.0
    assert loo(r=bad) == _lib.ERR_BAD_ARG and b"r_eff_j[4] = 0" in err()
    bad[4] = np.inf
    assert loo(r=bad) == _lib.ERR_BAD_ARG and b"r_eff_j[4] = inf" in err()
    bad[4], bad[2] = 1.0, np.nan
    assert loo(r=bad) == _lib.ERR_BAD_ARG and b"r_eff_j[2] = nan" in err()
    assert loo(h=other.user_handle) == _lib.ERR_BAD_ARG and b"data density" in err()
    assert loo(ns=2, nw=2) == _lib.ERR_BAD_ARG and b"n = 4" in err()
    assert loo(count=0) == _lib.ERR_BAD_ARG and b"obs_count = 0" in err()
    assert loo(first=3, count=8) == _lib.ERR_BAD_ARG and b"[0, 10)" in err()
    # a supplied entry that asks for more than a workgroup sorts: the observation is named (0.2 n = 6000 here)
    big = np.zeros(30000 * 2)
    small = r10.copy()
    small[6] = 0.001
    assert L.kmc_chain_psis_loo_reff(dd.user_handle, p(par), p(big), 10000, 3, 2, 0, None, 1, p(small), 1, 0, 0, 10, 0, 0, p(stats), p(lp), p(ru), ip(tl),
                                     C.byref(nn), C.byref(n), None) == _lib.ERR_UNSUPPORTED
    assert b"observation 6:" in err() and b"M = 6000" in err() and b"r_eff_j = 0.001" in err() and b"thin the chain" in err()
    # the chains of the weight series: the convergence contract's refusals, in its words
    for call in (loo, reff):
        kw = dict(r=None) if call is loo else {}
        assert call(ns=7, **kw) == _lib.ERR_BAD_ARG and b"at least 4 samples (h = 3)" in err()
        assert call(nw=1, split=0, **kw) == _lib.ERR_BAD_ARG and b"at least 2 chains" in err()
        assert call(max_lag=2, **kw) == _lib.ERR_BAD_ARG and b"max_lag must lie in [3, h - 1] (h = 20)" in err()
        assert call(max_lag=20, **kw) == _lib.ERR_BAD_ARG and b"max_lag" in err()
        assert call(thin=2, max_lag=10, **kw) == _lib.ERR_BAD_ARG and b"(h = 10)" in err()      # thinning shortens the chains
        assert call(thin=0, **kw) == _lib.ERR_BAD_ARG and b"thin = 0" in err()
    assert reff(out=None) == _lib.ERR_BAD_ARG
    assert reff(first=8, count=3) == _lib.ERR_BAD_ARG and b"[0, 10)" in err()
    assert L.kmc_sampler_relative_eff(None, 0, None, 1, 0, 1, 1, 0, 0, p(ru), None, None, None, None, None, None, None) == _lib.ERR_BAD_ARG
    v = np.zeros(120 * 10)
    assert L.kmc_chain_pointwise_weights(dd.user_handle, p(par), p(chain), 40, 3, 2, 0, None, 1, None, 0, 0, 0, 11, 0, p(v), None, None) == _lib.ERR_BAD_ARG
    assert b"[0, 10)" in err()
    assert L.kmc_sampler_pointwise_weights(None, 0, None, 1, None, 0, 0, 0, 1, p(v), None, None) == _lib.ERR_BAD_ARG
    assert n.value == -1 and nn.value == -1 and not stats.any() and not ru.any() and not tl.any() and not v.any()


def test_python_forms_of_r_eff(kmc):
    dd = kmc.DataDensity(pc.TERM, np.arange(10.0)[:, None])
    th = np.zeros((3, 40, 2))
    for wrong in (np.ones(9), np.ones(11), np.ones((10, 1)), np.ones(0)):
        with pytest.raises(ValueError, match="one entry per observation"):
            kmc.loo(dd, th, r_eff_j=wrong)
        with pytest.raises(ValueError, match="one entry per observation"):
            kmc.psis_tail(dd, th, r_eff_j=wrong)
    with pytest.raises(ValueError, match="one entry per observation asked for \\(4\\)"):
        kmc.loo(dd, th, r_eff_j=np.ones(10), obs=(2, 4))
    with pytest.raises(ValueError, match='"chain"'):
        kmc.loo(dd, th, r_eff="auto")
    with pytest.raises(ValueError, match="r_eff_j="):                             # (an array in r_eff itself stays refused, and says where it goes)
        kmc.psis_tail(dd, th, r_eff=np.ones(10))
    with pytest.raises(kmc.KmcError, match=r"r_eff_j\[3\] = -1"):
        kmc.loo(dd, th, r_eff_j=np.where(np.arange(10) == 3, -1.0, 1.0))
    with pytest.raises(kmc.KmcError, match="at least 4 samples"):
        kmc.loo(dd, th[:, :6], r_eff="chain")
    with pytest.raises(kmc.KmcError, match="at least 4 samples"):
        kmc.relative_eff(dd, th[:, :6])
    with pytest.raises(kmc.KmcError, match="max_lag"):
        kmc.relative_eff(dd, th, max_lag=0)                                        # (an explicit 0 is not the default)
    with pytest.raises(TypeError):
        kmc.relative_eff(kmc.GaussianIso(), th)


def test_the_inputs_of_the_gpu_tests(kmc):
    """What tests/test_gpu_relative_eff.py relies on, on the yardsticks: no pair sum of the truncation rule and no 3 sqrt(n / r_eff_j)
    near enough to its threshold for a rounding to flip it; input C's tail lengths really differ; the over-long input is over."""
    for name, (nw, ns, J, phi) in rc.INPUTS.items():
        l = rc.case(name)[2]
        n = l.shape[0]
        r, want, raw = rc.yardstick_reff(rc.weights(l), nw)
        assert np.isfinite(r).all() and (r > 0).all()
        assert rc.smallest_margin(want, raw) > 6e-5 and rc.integer_distance(n, r) > 9e-4, name
        M = rc.tail_lengths(n, r)
        assert all(M[j] == kmc.psis_plan(n, J, float(r[j]))["tail_len"] for j in range(0, J, 7))
        if name == "C":
            assert (r.min(), r.max()) == pytest.approx((0.097, 0.270), abs=1e-3) and np.unique(M).size == 61
            assert (M.min(), M.max()) == (258, 400) and Y.tail_length(n) == 135
    for J in rc.SPREAD_JS:
        assert np.unique(rc.tail_lengths(457, rc.spread(J))).size > 10
    l = rc.over_case()[2]
    r = rc.yardstick_reff(rc.weights(l), rc.OVER[0])[0]
    assert (r < 0.0134).all() and (rc.tail_lengths(l.shape[0], r) == 5000).all()
