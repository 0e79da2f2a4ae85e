"""No GPU: the yardstick of the highest-density interval (tests/hdi_yardstick.py) on arrays whose answer is visible by inspection,
kmc.hdi_span against numpy, every refusal of kmc.hdi / kmc.hdi_span that is raised before the device is touched, and the new exports.
(Header, SYMBOLS and the Julia ccalls are compared by tests/test_c_abi.py.)"""
import os
import re

import numpy as np
import pytest

import hdi_yardstick as hy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


# ---- the yardstick itself ----

@pytest.mark.parametrize("x, p, k, start, lo, hi", [
    ([1.0, 2.0, 3.0, 4.0], 0.5, 2, 0, 1.0, 3.0),                      # two windows of width 2: the smallest i
    ([-INF, 0.0, 1.0, INF], 0.5, 2, 0, -INF, 1.0),                    # both widths inf
    ([INF, INF, INF, INF], 0.5, 2, 0, INF, INF),                      # every width NaN
    ([3.0, 1.0], 0.94, 1, 0, 1.0, 3.0),
    ([4.0, 1.0, 3.5, 2.0, 3.0], 0.5, 2, 2, 3.0, 4.0),                 # sorted 1 2 3 3.5 4: widths 2, 1.5, 1
    ([0.0, -0.0, 5.0], 0.5, 1, 0, 0.0, 0.0),                          # the zeros tie
    ([-INF, -INF, 1.0, 2.0, INF, INF], 0.2, 1, 2, 1.0, 2.0),          # NaN widths at both ends lose to the number between them
])
def test_yardstick_on_arrays_read_by_eye(x, p, k, start, lo, hi):
    got = hy.column(np.array(x), p)
    assert got[3] == k and got[2] == start
    np.testing.assert_array_equal([got[0], got[1]], [lo, hi])
    assert not np.signbit(got[0]) or got[0] != 0.0                    # a zero is reported as +0.0


def test_yardstick_nan_column():
    lo, hi, start, k = hy.column(np.array([1.0, np.nan, 3.0, 4.0]), 0.5)
    assert np.isnan(lo) and np.isnan(hi) and start == -1 and k == 2


def test_yardstick_standard_normal():
    x = np.random.default_rng(20261020).standard_normal(100_000)
    lo, hi, start, k = hy.column(x, 0.94)
    xs = np.sort(x)
    assert k == 94_000 and xs[start] == lo and xs[start + k] == hi
    w = xs[k:] - xs[:-k]
    assert hi - lo == w.min() and start == int(np.argmax(w == w.min()))
    assert abs(lo + 1.88) < 0.05 and abs(hi - 1.88) < 0.05           # Phi^-1(0.97) = 1.8808


def test_yardstick_two_clusters_picks_the_denser_one():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(0.0, 1.0, 300), rng.uniform(10.0, 10.2, 700)])        # 70 % of the draws in a fifth of the width
    lo, hi, start, k = hy.column(rng.permutation(x), 0.5)
    assert k == 500 and 10.0 <= lo < hi <= 10.2 and start >= 300


def test_yardstick_columns_and_chain_layout():
    rng = np.random.default_rng(6)
    th = rng.standard_normal((5, 40, 3))                              # [walker][sample][dim]
    lp = rng.standard_normal((5, 40))
    lo, hi, start, k = hy.of_chain(th, [0.5, 0.9], logdensities=lp, first_sample=10, walkers=[0, 2, 3])
    assert lo.shape == hi.shape == start.shape == (2, 4) and k.tolist() == [45, 81]
    sel = th[[0, 2, 3], 10:]
    for c in range(3):
        assert (lo[1, c], hi[1, c], start[1, c]) == hy.column(sel[:, :, c].ravel(), 0.9)[:3]
    assert (lo[0, 3], hi[0, 3], start[0, 3]) == hy.column(lp[[0, 2, 3], 10:].ravel(), 0.5)[:3]


# ---- the host helper ----

def test_hdi_span_equals_numpy_floor(kmc):
    ns = [2, 3, 5, 7, 10, 64, 100, 999, 1000, 4096, 4097, 12301, 50_000, 10 ** 6, 2 ** 31 - 1]
    ps = [0.5, 0.94, 0.89, 0.95, 0.99, 0.1, 0.3, 1.0 / 3.0, 0.07, 2.0 / 3.0, 0.999, 0.29, 0.57, 0.7]
    seen = 0
    for n in ns:
        for p in ps:
            k = int(np.floor(p * n))
            if k < 1:
                with pytest.raises(kmc.KmcError):
                    kmc.hdi_span(n, p)
                continue
            assert kmc.hdi_span(n, p) == (k, n - k), (n, p)
            assert hy.span(n, p) == k
            seen += 1
    assert seen > 150
    for n, k in [(4096, 1), (4096, 4095), (4097, 1), (4097, 4096), (12301, 12300)]:
        assert kmc.hdi_span(n, hy.prob_for(n, k)) == (k, n - k)


@pytest.mark.parametrize("n, p, status, needle", [
    (100, float("nan"), "ERR_BAD_ARG", "nan"),
    (100, INF, "ERR_BAD_ARG", "inf"),
    (100, 0.0, "ERR_BAD_ARG", "prob = 0"),
    (100, 1.0, "ERR_BAD_ARG", "prob = 1"),
    (100, -0.25, "ERR_BAD_ARG", "-0.25"),
    (100, 1.5, "ERR_BAD_ARG", "1.5"),
    (100, 0.005, "ERR_BAD_ARG", "N = 100"),                           # k = 0
    (1, 0.5, "ERR_BAD_ARG", "N = 1"),
    (0, 0.5, "ERR_BAD_ARG", "N = 0"),
    (2 ** 31, 0.5, "ERR_UNSUPPORTED", str(2 ** 31)),
])
def test_hdi_span_refusals_name_the_value(kmc, n, p, status, needle):
    with pytest.raises(kmc.KmcError) as e:
        kmc.hdi_span(n, p)
    assert e.value.status == getattr(kmc._lib, status) and needle in str(e.value)


# ---- the refusals of the chain call that need no device (none is visible here: anything that got past them would say so) ----

def _chain(nw=4, ns=25, nd=2):
    return np.random.default_rng(1).standard_normal((nw, ns, nd))


@pytest.mark.parametrize("kw, status, needle", [
    (dict(prob=float("nan")), "ERR_BAD_ARG", "probs[0] = nan"),
    (dict(prob=[0.5, 1.0]), "ERR_BAD_ARG", "probs[1] = 1"),
    (dict(prob=[0.5, 0.0, 0.7]), "ERR_BAD_ARG", "probs[1] = 0"),
    (dict(prob=-0.5), "ERR_BAD_ARG", "-0.5"),
    (dict(prob=INF), "ERR_BAD_ARG", "inf"),
    (dict(prob=0.001), "ERR_BAD_ARG", "N = 100"),                     # p N < 1
    (dict(prob=list(np.linspace(0.1, 0.9, 17))), "ERR_BAD_ARG", "nprob = 17"),
    (dict(prob=[]), "ERR_BAD_ARG", "nprob = 0"),
    (dict(first_sample=25), "ERR_BAD_ARG", "empty"),
    (dict(walkers=np.zeros(4, dtype=bool)), "ERR_BAD_ARG", "empty"),
    (dict(first_sample=26), "ERR_BAD_ARG", "first_sample"),
    (dict(first_sample=24, walkers=[2]), "ERR_BAD_ARG", "N = 1"),
])
def test_chain_hdi_refusals_before_the_device(kmc, kw, status, needle):
    with pytest.raises(kmc.KmcError) as e:
        kmc.hdi(_chain(), **kw)
    assert e.value.status == getattr(kmc._lib, status) and needle in str(e.value), str(e.value)


def test_chain_hdi_refuses_more_columns_than_the_sort_takes(kmc):
    with pytest.raises(kmc.KmcError) as e:
        kmc.hdi(np.zeros((1, 2, 65536)), 0.5)
    assert e.value.status == kmc._lib.ERR_UNSUPPORTED and "65535" in str(e.value)


def test_python_argument_errors(kmc):
    with pytest.raises(ValueError):
        kmc.hdi(_chain(), [[0.5, 0.6]])
    with pytest.raises(ValueError):
        kmc.hdi(_chain(), 0.5, logdensities=np.zeros((4, 24)))
    with pytest.raises(ValueError):
        kmc.hdi(np.zeros(5), 0.5)
    with pytest.raises(IndexError):
        kmc.hdi(_chain(), 0.5, walkers=[4])


# ---- the exports ----

def test_exports(kmc):
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "kissmcmc_hip.h")).read(), flags=re.S)
    L = kmc._lib.lib()
    for name in ("kmc_sampler_hdi", "kmc_chain_hdi", "kmc_hdi_span"):
        assert re.search(r"kmc_status\s+%s\s*\(" % name, hdr), name
        assert name in kmc._lib.SYMBOLS and hasattr(L, name)
    assert {"hdi", "hdi_span"} <= set(kmc.__all__) and callable(kmc.Sampler.hdi)
    jl = open(os.path.join(ROOT, "kissmcmc.jl_amd", "julia", "src", "KissMCMCHIP.jl")).read()
    assert "ccall((:kmc_chain_hdi, LIB)" in jl and "ccall((:kmc_hdi_span, LIB)" in jl
    assert "hdi" in re.search(r"^export (.*)$", jl, re.M).group(1).replace(",", " ").split()
    assert "hdi(" in open(os.path.join(ROOT, "kissmcmc.jl_amd", "julia", "test", "runtests.jl")).read()


def test_summary_columns_without_the_keyword_are_what_they_were(kmc):
    from kissmcmc_jl_amd.summary import summary_columns
    m = np.arange(3.0)
    base = summary_columns(None, m, m, m)
    assert list(base) == ["var", "median", "mean", "mode", "std"]
    with_hdi = summary_columns(None, m, m, m, hdi={"lo": m - 1.0, "hi": m + 1.0})
    assert list(with_hdi) == list(base) + ["hdi_lo", "hdi_hi"]
    np.testing.assert_array_equal(with_hdi["hdi_lo"], m - 1.0)
    np.testing.assert_array_equal(with_hdi["hdi_hi"], m + 1.0)
