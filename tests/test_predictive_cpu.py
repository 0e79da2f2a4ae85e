"""No GPU: the host stage of WAIC (kmc_waic_stats) and the plan of the pointwise passes (kmc_pointwise_plan) against their restatements
in tests/predictive_yardstick.py, bit for bit; compare_waic against its formula; and the refusals of the host-chain calls that follow
from the sizes, which answer before any device is touched and name the offending value."""
import ctypes as C
import math

import numpy as np
import pytest

import predictive_yardstick as py


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """Equal bits, or NaN on both sides (the sign and payload of a NaN are not part of the contract)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def assert_same(got, want):
    for k in ("lppd", "p_waic", "elpd_waic", "se", "waic", "lppd_j", "p_waic_j", "elpd_j"):
        assert same(got[k], want[k]), (k, got[k], want[k])
    for k in ("n_high", "n_nan", "n"):
        assert got[k] == want[k], k


def test_predictive_calls_are_public(kmc):
    for name in ("waic", "pointwise_loglike", "pointwise_stats", "compare_waic", "waic_stats", "pointwise_plan"):
        assert name in kmc.__all__ and callable(getattr(kmc, name))
    assert callable(kmc.Sampler.waic) and callable(kmc.Sampler.pointwise_loglike)


def random_stats(rng, J):
    M = -np.abs(rng.standard_normal(J)) * np.exp(rng.uniform(-3, 6, J))
    S1 = M * rng.uniform(1.0, 50.0, J)
    E = rng.uniform(1.0, 40.0, J)
    V = rng.uniform(0.0, 30.0, J) * np.exp(rng.uniform(-8, 3, J))
    return np.stack([M, S1, E, V])


@pytest.mark.parametrize("J", [1, 2, 3, 7, 64, 201, 1000])
def test_host_stage_matches_its_restatement_bit_for_bit(kmc, J):
    rng = np.random.default_rng(J)
    for n in (2, 37, 6400):
        st = random_stats(rng, J)
        got = kmc.waic_stats(st, n)
        assert_same(got, py.host_stage(st, n))
        assert got["waic"] == -2.0 * got["elpd_waic"] and got["n_nan"] == 0
        assert math.isnan(got["se"]) == (J == 1)


def test_host_stage_special_columns(kmc):
    """E = 0 with M = -inf (an observation no row allows): lppd_j = -inf; NaN statistics stay in their own observation and count in
    n_nan; an infinite V gives an infinite p_waic_j; n_high counts p_waic_j > 0.4; the totals follow by the IEEE rules."""
    n = 50
    st = random_stats(np.random.default_rng(5), 9)
    st[:, 2] = [-np.inf, -np.inf, 0.0, np.nan]                 # all terms -inf
    st[:, 4] = [np.nan, np.nan, np.nan, np.nan]                # a NaN among the terms
    st[:, 6] = [-1.5, -np.inf, 3.0, np.nan]                    # a -inf among finite terms
    st[3, 7] = 0.41 * (n - 1)
    st[3, 8] = np.inf
    got = kmc.waic_stats(st, n)
    assert_same(got, py.host_stage(st, n))
    assert got["lppd_j"][2] == -np.inf and np.isnan(got["p_waic_j"][2])
    assert np.isnan(got["lppd_j"][4]) and np.isnan(got["p_waic_j"][4]) and np.isnan(got["elpd_j"][4]) and got["n_nan"] == 1
    assert np.isfinite(got["lppd_j"][6]) and np.isnan(got["p_waic_j"][6])
    assert got["p_waic_j"][8] == np.inf and got["elpd_j"][8] == -np.inf
    assert got["n_high"] >= 2 and got["p_waic_j"][7] > 0.4
    keep = [0, 1, 3, 5]
    clean = kmc.waic_stats(st[:, keep], n)
    assert (bits(clean["elpd_j"]) == bits(got["elpd_j"][keep])).all() and math.isfinite(clean["se"])
    with pytest.raises(ValueError):
        kmc.waic_stats(np.zeros((3, 4)), n)
    from kissmcmc_jl_amd import _lib
    z = np.zeros(16)
    p = z.ctypes.data_as(C.POINTER(C.c_double))
    for J, nn in ((0, 5), (3, 1)):
        assert _lib.lib().kmc_waic_stats(J, nn, p, p, p, p, p) == _lib.ERR_BAD_ARG
        assert str(min(J, nn)).encode() in _lib.lib().kmc_last_error()
    assert _lib.lib().kmc_waic_stats(2, 5, p, None, None, None, p) == _lib.OK      # the arrays may be NULL


def test_compare_waic_is_its_formula(kmc):
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal(200) - 1.0, rng.standard_normal(200) - 3.0
    d = kmc.compare_waic({"elpd_j": a}, {"elpd_j": b})
    diff = a - b
    assert d["J"] == 200 and d["elpd_diff"] == pytest.approx(diff.sum(), rel=1e-14)
    assert d["se"] == pytest.approx(math.sqrt(200 * np.sum((diff - diff.mean()) ** 2) / 199), rel=1e-13)
    r = kmc.compare_waic({"elpd_j": b}, {"elpd_j": a})
    assert r["elpd_diff"] == -d["elpd_diff"] and r["se"] == d["se"]
    assert math.isnan(kmc.compare_waic({"elpd_j": a[:1]}, {"elpd_j": b[:1]})["se"])
    with pytest.raises(ValueError):
        kmc.compare_waic({"elpd_j": a}, {"elpd_j": b[:10]})


def runs_of(p, n):
    """The rows every wave slot takes under a plan: wave w, slot q -> run w slots + q -> rows [run run_len, ...)."""
    rows = []
    for w in range(p["nwaves"]):
        for q in range(p["slots"]):
            r = w * p["slots"] + q
            if r < p["nruns"]:
                rows.extend(range(r * p["run_len"], min(n, (r + 1) * p["run_len"])))
    return rows


def test_plan_covers_every_row_once_and_depends_on_n_and_J_only(kmc):
    from kissmcmc_jl_amd import _lib
    for J in list(range(1, 66)) + [127, 128, 129, 1000, 100000, 2 ** 30]:
        for n in (2, 15, 16, 17, 33, 1000, 65537, 70001):
            p = kmc.pointwise_plan(n, J)
            assert p == py.plan(n, J) == kmc.pointwise_plan(n, J), (n, J)
            assert p["run_len"] >= 16 and (p["nruns"] - 1) * p["run_len"] < n <= p["nruns"] * p["run_len"]
            assert p["lanes_per_run"] * p["slots"] == 64 and (J >= 64 or J <= p["lanes_per_run"] < 2 * J)
            assert p["nruns"] <= max(1, 4096 // ((J + 63) // 64))
            if n <= 70001:
                assert runs_of(p, n) == list(range(n)), (n, J)
    big = kmc.pointwise_plan(2 ** 40 - 1, 100000)
    assert big == py.plan(2 ** 40 - 1, 100000) and big["nruns"] <= 4096
    for n, J, status, needle in ((1, 10, _lib.ERR_BAD_ARG, b"n = 1"), (2 ** 40, 10, _lib.ERR_UNSUPPORTED, str(2 ** 40).encode()),
                                 (5, 0, _lib.ERR_BAD_ARG, b"ndata = 0"), (5, 2 ** 30 + 1, _lib.ERR_BAD_ARG, str(2 ** 30 + 1).encode())):
        with pytest.raises(kmc.KmcError) as e:
            kmc.pointwise_plan(n, J)
        assert e.value.status == status and needle in str(e.value).encode()
    assert _lib.lib().kmc_pointwise_plan(40, 40, None, None, None, None, None) == _lib.OK       # pointers may be NULL


def test_argument_checks_need_no_device(kmc):
    """Every refusal that follows from the arguments alone comes before the device is touched: the statuses below are the same with and
    without a GPU (a call that got as far as the device would answer KMC_ERR_NO_DEVICE here, or run), and the message names the value."""
    from kissmcmc_jl_amd import _lib
    L = _lib.lib()
    dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    p = lambda a: a.ctypes.data_as(dp)
    D = np.arange(30.0).reshape(10, 3)
    dd = kmc.DataDensity(py.REG_TERM, D, params=[2.0])
    other = kmc.ExprDensity("-0.5*x*x")
    par, chain, out = np.array([2.0, 0, 0, 0, 0, 0]), np.zeros(4 * 3 * 40), np.zeros(4 * 1000)
    n = C.c_int64(-1)

    def stats(h=dd.user_handle, ch=p(chain), ns=4, nw=3, nd=2, first=0, mask=None, thin=1, data=None, nd2=0, nc2=0, res=p(out)):
        return L.kmc_chain_pointwise_stats(h, p(par), ch, ns, nw, nd, first, mask, thin, data, nd2, nc2, 0, res, C.byref(n), None)

    def matrix(first_obs, count, h=dd.user_handle, thin=1, data=None, nd2=0, nc2=0):
        return L.kmc_chain_pointwise_loglike(h, p(par), p(chain), 4, 3, 2, 0, None, thin, data, nd2, nc2, first_obs, count, 0, p(out), C.byref(n))

    err = lambda: L.kmc_last_error()
    assert stats(h=other.user_handle) == _lib.ERR_BAD_ARG and b"data density" in err()          # not a DataDensity
    assert stats(h=None) == _lib.ERR_BAD_ARG
    assert stats(nd=33) == _lib.ERR_BAD_ARG and b"ndim = 33" in err()
    assert stats(thin=0) == _lib.ERR_BAD_ARG and b"thin = 0" in err()
    assert stats(thin=-3) == _lib.ERR_BAD_ARG and b"thin = -3" in err()
    assert stats(ns=1, nw=1) == _lib.ERR_BAD_ARG and b"n = 1" in err()                           # n < 2
    assert stats(thin=4, nw=1) == _lib.ERR_BAD_ARG and b"n = 1" in err()                         # ... by the thinning
    one = np.array([0, 1, 0], dtype=np.uint8)
    assert stats(first=3, mask=one.ctypes.data_as(bp)) == _lib.ERR_BAD_ARG and b"n = 1" in err() # ... by the selection
    assert stats(mask=np.zeros(3, dtype=np.uint8).ctypes.data_as(bp)) == _lib.ERR_BAD_ARG        # an empty mask
    assert stats(first=5) == _lib.ERR_BAD_ARG and stats(first=-1) == _lib.ERR_BAD_ARG            # first_sample out of range
    assert stats(ch=None) == _lib.ERR_BAD_ARG and stats(res=None) == _lib.ERR_BAD_ARG            # null chain, null output
    held = np.zeros((5, 4))
    assert stats(data=p(held), nd2=5, nc2=4) == _lib.ERR_BAD_ARG and b"4 columns" in err() and b"have 3" in err()
    assert stats(data=p(held), nd2=0, nc2=3) == _lib.ERR_BAD_ARG and b"ndata = 0" in err()
    assert stats(data=p(held), nd2=2 ** 30 + 1, nc2=3) == _lib.ERR_BAD_ARG and str(2 ** 30 + 1).encode() in err()
    assert stats(ns=2 ** 30, nw=2 ** 10) == _lib.ERR_UNSUPPORTED and str(2 ** 40).encode() in err()   # n >= 2^40, from the sizes alone
    assert matrix(0, 0) == _lib.ERR_BAD_ARG and b"obs_count = 0" in err()
    assert matrix(-1, 2) == _lib.ERR_BAD_ARG and b"[-1, -1 + 2)" in err()
    assert matrix(9, 2) == _lib.ERR_BAD_ARG and b"[0, 10)" in err()                              # one past the end
    assert matrix(3, 2, data=p(held), nd2=4, nc2=3) == _lib.ERR_BAD_ARG and b"[0, 4)" in err()   # the held-out array's own range
    assert matrix(0, 5, thin=0) == _lib.ERR_BAD_ARG
    assert L.kmc_sampler_pointwise_stats(None, 0, None, 1, None, 0, 0, p(out), None, None) == _lib.ERR_BAD_ARG
    assert L.kmc_sampler_pointwise_loglike(None, 0, None, 1, None, 0, 0, 0, 1, p(out), None) == _lib.ERR_BAD_ARG
    assert n.value == -1 and not out.any()
    th = np.zeros((3, 4, 2))
    with pytest.raises(kmc.KmcError) as e:                                                       # ... and through the Python layer
        kmc.waic(dd, th, thin=0)
    assert e.value.status == _lib.ERR_BAD_ARG and "thin = 0" in str(e.value)
    with pytest.raises(kmc.KmcError, match="data density"):
        kmc.waic(other, th)
    with pytest.raises(TypeError):
        kmc.waic(kmc.GaussianIso(), th)
    with pytest.raises(kmc.KmcError, match=r"\[8, 8 \+ 3\)"):
        kmc.pointwise_loglike(dd, th, obs=(8, 11))
    with pytest.raises(kmc.KmcError, match="2 columns"):
        kmc.waic(dd, th, data=np.zeros((4, 2)))


def test_yardstick_statistics_are_exact():
    """The yardstick's own sums against rationals: S1 and V (about a given centre) are the correctly rounded exact sums."""
    from fractions import Fraction
    rng = np.random.default_rng(8)
    l = -np.abs(rng.standard_normal((37, 3))) * np.array([1e-3, 1.0, 1e4])
    c = l.mean(axis=0) * (1 + 1e-9)
    st = py.exact_stats(l, centre=c)
    for j in range(3):
        col = [Fraction(v) for v in l[:, j].tolist()]
        assert st[1, j] == float(sum(col))
        assert st[3, j] == float(sum((v - Fraction(c[j])) ** 2 for v in col))
        assert st[0, j] == l[:, j].max()
        assert st[2, j] == pytest.approx(np.exp(l[:, j] - l[:, j].max()).sum(), rel=1e-14)
    assert np.allclose(py.planned_sums(l, 37, 3), st[1], rtol=1e-14, atol=0)
