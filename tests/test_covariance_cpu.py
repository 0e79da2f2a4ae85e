"""No GPU: the host stage of the posterior covariance (kmc_cov_correlation) and the plan of its product kernel (kmc_cov_plan) against
their restatements in tests/covariance_yardstick.py, bit for bit; the argument refusals of kmc_chain_covariance, which answer before
any device is touched; and the yardstick's own error-free product against rationals."""
import ctypes as C

import numpy as np
import pytest

import covariance_yardstick as cy


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_covariance_is_public(kmc):
    for name in ("covariance", "correlation", "cov_plan"):
        assert name in kmc.__all__ and callable(getattr(kmc, name))
    assert callable(kmc.Sampler.covariance)


def test_correlation_matches_its_restatement_bit_for_bit(kmc):
    rng = np.random.default_rng(11)
    for ncols in (1, 2, 7, 33):
        a = rng.standard_normal((ncols + 5, ncols)) * np.exp(rng.uniform(-20, 20, ncols))
        cov = np.cov(a, rowvar=False).reshape(ncols, ncols)
        corr, std = kmc.correlation(cov)
        wc, ws = cy.correlation(cov)
        assert (bits(corr) == bits(wc)).all() and (bits(std) == bits(ws)).all()
        assert (np.diag(corr) == 1.0).all() and (bits(corr) == bits(corr.T)).all()
        off = corr[~np.eye(ncols, dtype=bool)]
        assert np.all(np.abs(off) <= 1.0 + 1e-12)


def test_correlation_of_constant_infinite_and_nan_columns(kmc):
    """A constant column (variance 0) gives NaN in its row and column, the diagonal included, without an error; so does an infinite
    variance (inf / (inf * inf)) and a NaN one; the other entries are untouched and the other diagonals are exactly 1.0."""
    cov = np.array([[4.0, 0.0, 1.0, 0.5, 0.25],
                    [0.0, 0.0, 0.0, 0.0, 0.0],
                    [1.0, 0.0, np.inf, 2.0, 0.125],
                    [0.5, 0.0, 2.0, np.nan, 0.75],
                    [0.25, 0.0, 0.125, 0.75, 1e-300]])
    corr, std = kmc.correlation(cov)
    wc, ws = cy.correlation(cov)
    assert (bits(corr) == bits(wc)).all() and (bits(std) == bits(ws)).all()
    assert np.isnan(corr[1]).all() and np.isnan(corr[:, 1]).all()
    assert np.isnan(corr[2, 2]) and np.isnan(corr[3]).all()
    assert corr[0, 2] == 0.0 and corr[2, 4] == 0.0                                 # finite / inf
    assert corr[0, 0] == 1.0 and corr[4, 4] == 1.0
    assert corr[0, 4] == 0.25 / (2.0 * np.sqrt(1e-300))
    assert std[1] == 0.0 and std[2] == np.inf and np.isnan(std[3])
    with pytest.raises(ValueError):
        kmc.correlation(np.zeros((2, 3)))


def test_plan_matches_its_restatement(kmc):
    from kissmcmc_jl_amd import _lib
    st = cy.STRIP_TILES
    for ncols in (1, 15, 16, 17, 32, 33, 16 * st, 16 * st + 1, 1024):
        assert kmc.cov_plan(ncols) == cy.plan(ncols), ncols
    assert kmc.cov_plan(32)["nstrips"] == 1 and kmc.cov_plan(33)["nstrips"] == 3 and kmc.cov_plan(16 * st + 1)["nstrips"] == st + 2
    for ncols, status in ((0, _lib.ERR_BAD_ARG), (1025, _lib.ERR_UNSUPPORTED)):
        with pytest.raises(kmc.KmcError) as e:
            kmc.cov_plan(ncols)
        assert e.value.status == status
    assert _lib.lib().kmc_cov_plan(40, None, None, None, None) == _lib.OK          # pointers may be NULL


def test_argument_checks_need_no_device(kmc):
    """Every refusal that follows from the arguments alone comes before the device is touched: the statuses below are the same with
    and without a GPU (a call that got as far as the device would answer KMC_ERR_NO_DEVICE here, or run)."""
    from kissmcmc_jl_amd import _lib
    L = _lib.lib()
    dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    p = lambda a: a.ctypes.data_as(dp)
    chain = np.zeros(2 * 3 * 1025)
    mean, cov = np.zeros(1025), np.zeros(1025 * 1025)
    n = C.c_int64(-1)
    call = lambda ch, ns, nw, nd, first, mask: L.kmc_chain_covariance(ch, None, ns, nw, nd, first, mask, 0, p(mean), p(cov), C.byref(n), None)
    assert call(p(chain), 2, 3, 1025, 0, None) == _lib.ERR_UNSUPPORTED             # C = 1025
    assert b"1024" in L.kmc_last_error()
    assert L.kmc_chain_covariance(p(chain), p(chain), 2, 3, 1024, 0, None, 0, p(mean), p(cov), C.byref(n), None) == _lib.ERR_UNSUPPORTED   # ... with the log-densities
    assert call(p(chain), 1, 1, 2, 0, None) == _lib.ERR_BAD_ARG                    # n = 1
    one = np.array([0, 1, 0], dtype=np.uint8)
    assert call(p(chain), 2, 3, 2, 1, one.ctypes.data_as(bp)) == _lib.ERR_BAD_ARG  # n = 1 by the selection
    none = np.zeros(3, dtype=np.uint8)
    assert call(p(chain), 2, 3, 2, 0, none.ctypes.data_as(bp)) == _lib.ERR_BAD_ARG         # an empty mask
    assert call(None, 2, 3, 2, 0, None) == _lib.ERR_BAD_ARG                        # a null chain
    assert call(p(chain), 2, 3, 2, 3, None) == _lib.ERR_BAD_ARG                    # first_sample out of range
    assert call(p(chain), 2, 3, 2, -1, None) == _lib.ERR_BAD_ARG
    assert call(p(chain), 2, 3, 2, 2, None) == _lib.ERR_BAD_ARG                    # no sample at or after first_sample
    assert L.kmc_chain_covariance(p(chain), None, 2, 3, 2, 0, None, 0, None, p(cov), None, None) == _lib.ERR_BAD_ARG      # null outputs
    assert L.kmc_sampler_covariance(None, 0, None, 0, p(mean), p(cov), None, None) == _lib.ERR_BAD_ARG
    assert n.value == -1
    assert L.kmc_cov_correlation(0, p(cov), p(cov), None) == _lib.ERR_BAD_ARG
    assert L.kmc_cov_correlation(2, None, p(cov), None) == _lib.ERR_BAD_ARG
    with pytest.raises(kmc.KmcError) as e:                                         # ... and through the Python layer
        kmc.covariance(np.zeros((1, 1, 2)))
    assert e.value.status == _lib.ERR_BAD_ARG


def test_yardstick_products_are_exact():
    """The error-free product behind the yardstick's sums: p + e == a b in rationals, and the sums equal those taken in rationals."""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(200) * 1e3, rng.standard_normal(200) * 1e-3
    p, e = cy.two_product(a, b)
    assert all(Fraction(x) * Fraction(y) == Fraction(q) + Fraction(r) for x, y, q, r in zip(a.tolist(), b.tolist(), p.tolist(), e.tolist()))
    x = rng.standard_normal((37, 5)) * np.array([1e-3, 1.0, 1e3, 7.0, 0.1]) + np.array([5.0, -2.0, 1e4, 0.0, 0.3])
    s = cy.sums(x)
    assert (bits(s["cross"]) == bits(cy.sums_fraction(x, s["mean"]))).all()
    assert np.allclose(s["cross"] / 36, np.cov(x, rowvar=False), rtol=1e-9, atol=0)
