"""No GPU: the plan of a PSIS-LOO call (kmc_psis_plan) against its formula, the host stage (kmc_loo_stats) against its restatement in
tests/psis_yardstick.py bit for bit, the host form of fit and smoothing (kmc_psis_smooth_host) against the yardstick within the measured
tolerance, compare_loo, and the refusals that follow from the arguments alone.

The tolerance of kmc_psis_smooth_host, like the device's in tests/test_gpu_psis_loo.py: 8 times the distance of the float64 yardstick
from its longdouble mode on the same tail, per output and relative to max(1, |value|) -- the C library's exp / log / log1p / expm1 and
the fit's order of summation differ from numpy's, each a few ulp per operation over the same operation count -- with the floor
(nt + 4) 2^-53 on the same scale.  SMOOTH_DIST records what the measurement gave (the test measures again: it needs no device)."""
import ctypes as C
import math

import numpy as np
import pytest

import psis_yardstick as Y

# python -m pytest -s tests/test_psis_loo_cpu.py -k smooth_host   (prints one line per tail: k, then the yardstick's float64-to-longdouble
# distance and kmc_psis_smooth_host's error for k, sigma and s)
SMOOTH_DIST = {
    "gpd k=0.1 nt=256": dict(k=7.95e-16, sigma=1.53e-21, s=1.80e-16),     # host form's error: 1.92e-15, 3.39e-21, 3.33e-16
    "gpd k=0.5 nt=256": dict(k=2.92e-15, sigma=5.02e-21, s=1.03e-15),     #                    2.55e-15, 4.45e-21, 9.56e-16
    "gpd k=0.9 nt=256": dict(k=2.97e-15, sigma=6.89e-21, s=1.45e-15),     #                    1.11e-16, 4.24e-22, 1.88e-16
    "gpd k=0.5 nt=5": dict(k=2.12e-16, sigma=1.99e-22, s=5.24e-17),       #                    0, 1.06e-22, 0
    "equal nt=40": dict(k=6.77e-15, sigma=1.33e-15, s=6.21e-16),          #                    0, 0, 1.78e-16
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def test_loo_calls_are_public(kmc):
    for name in ("loo", "compare_loo", "psis_plan", "loo_stats", "psis_smooth", "psis_tail"):
        assert name in kmc.__all__ and callable(getattr(kmc, name))
    assert callable(kmc.Sampler.loo) and callable(kmc.Sampler.psis_tail)
    import inspect
    assert "data" not in inspect.signature(kmc.loo).parameters and "data" not in inspect.signature(kmc.Sampler.loo).parameters


@pytest.mark.parametrize("r_eff", [1.0, 0.01])
def test_plan_is_the_formula(kmc, r_eff):
    for n in (5, 20, 24, 25, 26, 30, 456, 7300):
        M = int(math.ceil(min(0.2 * n, 3.0 * math.sqrt(n / r_eff))))
        p = kmc.psis_plan(n, 1000, r_eff)
        assert p["tail_len"] == M == Y.tail_length(n, r_eff) and p["m_est"] == 30 + int(math.floor(math.sqrt(M))) and p["passes"] == 18
        nruns = kmc.pointwise_plan(n, 1000)["nruns"]
        per_obs = 8 * M + 72 * nruns + 72
        assert p["obs_per_block"] == max(64, (1 << 30) // per_obs // 64 * 64)
        assert kmc.psis_plan(n, 1000, r_eff, workspace=1 << 20)["obs_per_block"] == max(64, (1 << 20) // per_obs // 64 * 64)
        assert kmc.psis_plan(n, 1000, r_eff, workspace=1)["obs_per_block"] == 64


def test_plan_at_the_limit_of_the_tail(kmc):
    from kissmcmc_jl_amd import _lib
    assert kmc.psis_plan(20480, 10, 0.01)["tail_len"] == 4096 and kmc.psis_plan(20480, 10, 0.01)["m_est"] == 94        # 0.2 n = 4096
    with pytest.raises(kmc.KmcError, match=r"M = 4097 .*n / r_eff = 2048500") as e:
        kmc.psis_plan(20485, 10, 0.01)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    n = 1864135                                                                                     # 3 sqrt(n) = 4095.99...
    assert kmc.psis_plan(n, 10)["tail_len"] == 4096
    with pytest.raises(kmc.KmcError, match="M = 4097"):
        kmc.psis_plan(n + 500, 10)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(kmc.KmcError, match="r_eff") as e:
            kmc.psis_plan(100, 10, bad)
        assert e.value.status == _lib.ERR_BAD_ARG
    with pytest.raises(kmc.KmcError, match=r"n = 4\)"):
        kmc.psis_plan(4, 10)
    with pytest.raises(kmc.KmcError, match="ndata = 0"):
        kmc.psis_plan(100, 0)


def random_stats(rng, J):
    el = -np.abs(rng.standard_normal(J)) * np.exp(rng.uniform(-3, 4, J))
    k = rng.uniform(-0.3, 1.4, J)
    k[rng.random(J) < 0.1] = np.inf
    nt = rng.integers(0, 300, J).astype(np.float64)
    return np.stack([el, k, nt, rng.random(J)]), el + rng.random(J)


@pytest.mark.parametrize("J", [1, 2, 3, 7, 64, 201, 1000])
def test_host_stage_matches_its_restatement_bit_for_bit(kmc, J):
    rng = np.random.default_rng(J)
    st, lp = random_stats(rng, J)
    if J > 6:
        st[0, 3] = np.nan
        st[1, 3] = np.nan
        st[2, 3] = np.nan
        st[1, 5] = 0.5                                                                  # the edges of k_counts belong to the lower class
        st[1, 6] = 0.7
    got, want = kmc.loo_stats(st, lp, 50), Y.totals(st[0], lp, st[1])
    for key in ("elpd_loo", "se", "p_loo", "looic", "lppd", "p_loo_j"):
        assert same(got[key], want[key]), key
    assert got["n_nan"] == want["n_nan"] == (1 if J > 6 else 0) and got["k_counts"] == want["k_counts"] and got["n"] == 50
    assert sum(got["k_counts"]) == J - got["n_nan"] and math.isnan(got["se"]) == (J == 1 or J > 6)
    assert same(got["elpd_loo_j"], st[0]) and same(got["pareto_k"], st[1]) and same(got["lppd_j"], lp)
    assert (got["n_tail_j"] == np.where(np.isnan(st[2]), -1, st[2])).all()
    with pytest.raises(kmc.KmcError, match=r"n = 4\)"):
        kmc.loo_stats(st, lp, 4)
    with pytest.raises(ValueError):
        kmc.loo_stats(st[:3], lp, 50)


def gpd_tail(rng, k, nt, xc=-12.0):
    """The logarithms of exp(xc) (1 + r), r drawn from a generalised Pareto of shape k and scale 0.3: a tail above the cut-off xc."""
    u = rng.random(nt)
    r = 0.3 * np.expm1(-k * np.log1p(-u)) / k
    x = np.sort(xc + np.log1p(r))
    assert x[0] > xc and x[-1] <= 0.0
    return x, xc


def check_smooth(kmc, x, xc, label):
    h = kmc.psis_smooth(x, xc)
    d64, d80 = [], []
    k64, s64, sm64 = Y.smooth(x, xc, dropped=d64)
    k80, s80, sm80 = Y.smooth(x, xc, np.longdouble, dropped=d80)
    assert all((p == q).all() for p, q in zip(d64, d80))                                # the two modes drop the same weights
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a, dtype=np.longdouble) - b) / np.maximum(1.0, np.abs(b))))
    floor = (x.size + 4) * 2.0 ** -53
    line = f"{label}: k {h['k']:.6f}"
    for name, got, y64, y80 in (("k", h["k"], k64, k80), ("sigma", h["sigma"], s64, s80), ("s", h["s"], sm64, sm80)):
        dist, err = rel(y64, y80), rel(got, np.asarray(y64, dtype=np.longdouble))
        line += f"; {name}: yardstick {dist:.2e}, host {err:.2e}"
        assert err <= max(8.0 * SMOOTH_DIST[label][name], floor), (label, name, err, dist)
    print(line + f"; weights dropped: {bool(d64 and d64[0].any())}")
    with np.errstate(all="ignore"):
        assert abs(h["sums"][0] - float(np.exp(sm64).sum())) <= max(8.0 * rel(sm64, sm80), floor) * x.size
    return h


@pytest.mark.parametrize("k", [0.1, 0.5, 0.9])
def test_smooth_host_on_generalised_pareto_tails(kmc, k):
    rng = np.random.default_rng(int(10 * k))
    h = check_smooth(kmc, *gpd_tail(rng, k, 256), f"gpd k={k} nt=256")
    assert abs(h["k"] - k) < 0.35 and h["sigma"] > 0 and (np.diff(h["s"]) >= 0).all() and (h["s"] <= 0).all()
    again = kmc.psis_smooth(*gpd_tail(np.random.default_rng(int(10 * k)), k, 256))
    assert same(again["s"], h["s"]) and again["k"] == h["k"]


def test_smooth_host_small_and_degenerate_tails(kmc):
    rng = np.random.default_rng(3)
    check_smooth(kmc, *gpd_tail(rng, 0.5, 5), "gpd k=0.5 nt=5")                          # the smallest tail fitted
    x4 = np.array([-3.0, -2.0, -1.0, -0.5])
    h = kmc.psis_smooth(x4, -4.0)                                                       # not fitted: k = +inf, the tail as it is
    assert h["k"] == np.inf and math.isnan(h["sigma"]) and same(h["s"], x4) and h["sums"][1] == 4.0
    h0 = kmc.psis_smooth(np.zeros(0), -1.0)
    assert h0["k"] == np.inf and h0["s"].size == 0 and h0["sums"] == (0.0, 0.0)
    he = check_smooth(kmc, np.full(40, -2.5), -3.0, "equal nt=40")                      # all equal: a fit like any other, k about -4.7
    assert he["k"] < -4.0 and he["sigma"] > 0
    for bad, xc in ((np.array([-1.0, -2.0]), -3.0), (np.array([-2.0, 0.5]), -3.0), (np.array([-3.0, -1.0]), -3.0), (np.array([np.nan]), -3.0)):
        with pytest.raises(kmc.KmcError, match="ascending"):
            kmc.psis_smooth(bad, xc)


def test_compare_loo_is_compare_waic_on_elpd_loo_j(kmc):
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal(50), rng.standard_normal(50)
    d = kmc.compare_loo({"elpd_loo_j": a}, {"elpd_loo_j": b})
    assert d == kmc.compare_waic({"elpd_j": a}, {"elpd_j": b}) and d["J"] == 50
    assert d["elpd_diff"] == float((a - b).sum()) and d["se"] == float(np.sqrt(50 * (a - b).var(ddof=1)))
    with pytest.raises(ValueError):
        kmc.compare_loo({"elpd_loo_j": a}, {"elpd_loo_j": b[:49]})


def test_argument_checks_need_no_device(kmc):
    """Every refusal that follows from the arguments alone comes before the device is touched, and names the value."""
    from kissmcmc_jl_amd import _lib
    L = _lib.lib()
    dp = C.POINTER(C.c_double)
    p = lambda a: a.ctypes.data_as(dp)
    dd = kmc.DataDensity("double r = d[0] - x[0] * d[1] - x[1] * d[2]; return -0.5 * p[0] * r * r;", np.arange(30.0).reshape(10, 3), params=[2.0])
    other = kmc.ExprDensity("-0.5*x*x")
    par, chain, out, lp = np.array([2.0, 0, 0, 0, 0, 0]), np.zeros(4 * 3 * 2), np.zeros(4 * 10), np.zeros(10)
    n = C.c_int64(-1)

    def loo(h=dd.user_handle, ns=4, nw=3, thin=1, r_eff=1.0, first=0, count=10, work=0, res=p(out)):
        return L.kmc_chain_psis_loo(h, p(par), p(chain), ns, nw, 2, 0, None, thin, r_eff, first, count, work, 0, res, p(lp), C.byref(n), None)

    err = lambda: L.kmc_last_error()
    assert loo(h=other.user_handle) == _lib.ERR_BAD_ARG and b"data density" in err()
    assert loo(ns=2, nw=2) == _lib.ERR_BAD_ARG and b"n = 4" in err()
    assert loo(thin=4) == _lib.ERR_BAD_ARG and b"n = 3" in err()
    assert loo(thin=0) == _lib.ERR_BAD_ARG and b"thin = 0" in err()
    assert loo(r_eff=0.0) == _lib.ERR_BAD_ARG and b"r_eff = 0" in err()
    assert loo(r_eff=float("nan")) == _lib.ERR_BAD_ARG and b"r_eff = nan" in err()
    assert loo(count=0) == _lib.ERR_BAD_ARG and b"obs_count = 0" in err()
    assert loo(first=3, count=8) == _lib.ERR_BAD_ARG and b"[0, 10)" in err()
    assert loo(res=None) == _lib.ERR_BAD_ARG
    assert L.kmc_sampler_psis_loo(None, 0, None, 1, 1.0, 0, 1, 0, p(out), p(lp), None, None) == _lib.ERR_BAD_ARG
    assert n.value == -1 and not out.any() and not lp.any()
    th = np.zeros((3, 4, 2))
    with pytest.raises(kmc.KmcError, match="r_eff = -1"):
        kmc.loo(dd, th, r_eff=-1.0)
    with pytest.raises(ValueError, match="per-observation"):
        kmc.loo(dd, th, r_eff=np.ones(10))
    with pytest.raises(kmc.KmcError, match=r"M = 6000 .*n / r_eff = 4000000"):
        kmc.loo(dd, np.zeros((3, 10000, 2)), r_eff=0.0075)
    with pytest.raises(kmc.KmcError, match="data density"):
        kmc.psis_tail(other, th)
    with pytest.raises(TypeError):
        kmc.loo(kmc.GaussianIso(), th)
    with pytest.raises(TypeError):
        kmc.loo(dd, th, data=np.zeros((4, 3)))


def test_fit_header_under_host_sanitizers(tmp_path):
    """The shared fit header (csrc/kmc_psis_fit.hpp) in a stand-alone program of its own (tests/sanitize/psis_fit_main.cpp), built with the
    host's address and undefined-behaviour sanitizers and run: tails from empty to the 4 096 limit, where the grid scratch is full.  Nothing
    of it is loaded into Python."""
    import os
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "psis_fit_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(root, "kissmcmc.jl_amd", "csrc"), os.path.join(root, "tests", "sanitize", "psis_fit_main.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 30 and lines[2].startswith("shape 0 nt 4 k inf") and lines[9].startswith("shape 0 nt 4096 k 0.")
