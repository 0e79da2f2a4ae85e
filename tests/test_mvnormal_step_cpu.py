"""The host side of the covariance-shaped Metropolis proposal (kmc.MVNormalStep, kmc.TunedStep, kmc.cholesky_lower,
kmc_metropolis_validate) against tests/mvnormal_step_yardstick.py.  No device here.

The last test runs the tuning rule itself in numpy (numpy's own generator) over ten seeds and shows that the bounds of the
statistical GPU test (tests/test_gpu_mvnormal_step.py) hold for the rule: a failure there is then the kernels', not the rule's."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import mvnormal_step_yardstick as my


def _spd(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, n + 3))
    return a @ a.T / (n + 3) + 0.05 * np.eye(n)


def _hilbert(n):
    i = np.arange(n)
    return 1.0 / (i[:, None] + i[None, :] + 1.0)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 32, 128])
def test_cholesky_lower_equals_the_yardstick_bit_for_bit(kmc, n):
    a = _spd(n, 100 + n)
    want, bad = my.cholesky_lower(a)
    assert bad == -1
    got = kmc.cholesky_lower(a)
    np.testing.assert_array_equal(got, want)
    assert (np.triu(got, 1) == 0.0).all() and (np.diag(got) > 0).all()


def test_cholesky_lower_on_an_ill_conditioned_matrix_and_with_a_garbage_upper_triangle(kmc):
    h = _hilbert(8)                                              # condition number about 1.5e10, still positive definite in double
    assert np.linalg.cond(h) > 1e9
    want, bad = my.cholesky_lower(h)
    assert bad == -1
    np.testing.assert_array_equal(kmc.cholesky_lower(h), want)
    a = _spd(7, 3)
    g = a.copy()
    g[np.triu_indices(7, 1)] = [np.nan, np.inf, -1e300] * 7      # only the lower triangle is read
    np.testing.assert_array_equal(kmc.cholesky_lower(g), my.cholesky_lower(a)[0])
    np.testing.assert_array_equal(kmc.cholesky_lower(g), kmc.cholesky_lower(a))


@pytest.mark.parametrize("name", ["spd1", "spd2", "spd3", "spd5", "spd32", "hilbert8"])
def test_cholesky_residual_is_within_highams_bound(kmc, name):
    """|A - L L^T| <= gamma_{n+1} |L| |L^T| entry by entry, gamma_k = k u / (1 - k u), u = 2^-53 (Higham, Accuracy and Stability of
    Numerical Algorithms, theorem 10.3); the product L L^T is taken exactly, in rationals."""
    a = _hilbert(8) if name == "hilbert8" else _spd(int(name[3:]), 7)
    n = a.shape[0]
    L = kmc.cholesky_lower(a)
    u = Fraction(1, 2 ** 53)
    gamma = (n + 1) * u / (1 - (n + 1) * u)
    Lf = [[Fraction(float(v)) for v in row] for row in L]
    for i in range(n):
        for j in range(i + 1):
            prod = sum(Lf[i][k] * Lf[j][k] for k in range(j + 1))
            absprod = sum(abs(Lf[i][k]) * abs(Lf[j][k]) for k in range(j + 1))
            assert abs(Fraction(float(a[i, j])) - prod) <= gamma * absprod, (i, j)


def test_cholesky_lower_reports_the_failing_pivot(kmc):
    from kissmcmc_jl_amd import _lib
    lib = _lib.lib()
    nan3 = _spd(3, 1)
    nan3[2, 1] = np.nan
    cases = [(np.array([[1.0, 1.0], [1.0, 1.0]]), 1),                                  # semidefinite: the second pivot is exactly 0
             (np.array([[4.0, 2.0, 2.0], [2.0, 1.0, 1.0], [2.0, 1.0, 3.0]]), 1),       # semidefinite, rank 2
             (np.array([[1.0, 2.0], [2.0, 1.0]]), 1),                                  # indefinite
             (np.diag([1.0, 2.0, -3.0, 4.0]), 2),                                      # indefinite
             (nan3, 2),                                                                # a NaN below the diagonal
             (np.array([[np.nan]]), 0)]
    for a, pivot in cases:
        assert my.cholesky_lower(a)[1] == pivot
        a = np.ascontiguousarray(a)
        L, bad = np.zeros_like(a), C.c_int(-7)
        st = lib.kmc_cholesky_lower(a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[0], L.ctypes.data_as(C.POINTER(C.c_double)), C.byref(bad))
        assert st == _lib.ERR_BAD_ARG and bad.value == pivot
        assert f"pivot {pivot}" in lib.kmc_last_error().decode()
        with pytest.raises(ValueError, match=f"pivot {pivot}"):
            kmc.cholesky_lower(a)
    good, bad = np.eye(2), C.c_int(5)
    assert lib.kmc_cholesky_lower(good.ctypes.data_as(C.POINTER(C.c_double)), 2, good.copy().ctypes.data_as(C.POINTER(C.c_double)), C.byref(bad)) == _lib.OK
    assert bad.value == -1


def test_metropolis_validate_refuses_and_accepts(kmc):
    from kissmcmc_jl_amd import _lib
    lib = _lib.lib()
    dp = C.POINTER(C.c_double)
    keep = []

    def arr(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        keep.append(a)
        return a.ctypes.data_as(dp)

    def cfg(ndim=3, **kw):
        c = _lib.MetropolisConfig()
        c.dtype, c.density = _lib.F64, _lib.GAUSSIAN_ISO
        c.params[0], c.params[1] = 0.0, 1.0
        c.nchains, c.ndim, c.niter, c.nburnin, c.nthin = 16, ndim, 40, 20, 1
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def refused(c, status, *words):
        assert lib.kmc_metropolis_validate(C.byref(c)) == status
        msg = lib.kmc_last_error().decode()
        for w in words:
            assert str(w) in msg, (w, msg)

    Lgood = np.tril(0.3 * np.ones((3, 3))) + np.eye(3)
    step = np.full(3, 0.5)
    # the good configurations
    assert lib.kmc_metropolis_validate(C.byref(cfg(chol=arr(Lgood)))) == _lib.OK
    assert lib.kmc_metropolis_validate(C.byref(cfg(step=arr(step)))) == _lib.OK
    assert lib.kmc_metropolis_validate(C.byref(cfg(chol=arr(Lgood), tune_rounds=4, tune_scale=0.7))) == _lib.OK
    assert lib.kmc_metropolis_validate(C.byref(cfg(step=arr(step), tune_rounds=19))) == _lib.OK              # nburnin == rounds + 1
    assert lib.kmc_metropolis_validate(C.byref(cfg(ndim=128, nchains=129, chol=arr(np.eye(128)), tune_rounds=1))) == _lib.OK
    g = Lgood.copy()
    g[np.triu_indices(3, 1)] = np.nan                                                                        # the upper triangle is not read
    assert lib.kmc_metropolis_validate(C.byref(cfg(chol=arr(g)))) == _lib.OK
    cb = _lib.HOST_LOGPDF_FN(lambda rows, n, nd, out, user: 0)
    assert lib.kmc_metropolis_validate(C.byref(cfg(density=_lib.HOST_DENSITY, host_logpdf=C.cast(cb, C.c_void_p), chol=arr(Lgood), tune_rounds=2))) == _lib.OK
    # ndim > 128 with chol or tuning
    refused(cfg(ndim=129, nchains=200, chol=arr(np.eye(129))), _lib.ERR_UNSUPPORTED, "129", "128")
    refused(cfg(ndim=129, nchains=200, step=arr(np.ones(129)), tune_rounds=1), _lib.ERR_UNSUPPORTED, "129", "128")
    assert lib.kmc_metropolis_validate(C.byref(cfg(ndim=129, step=arr(np.ones(129))))) == _lib.OK            # the isotropic path has no such limit
    # entries of L
    for bad_val in (np.nan, np.inf):
        b = Lgood.copy()
        b[2, 1] = bad_val
        refused(cfg(chol=arr(b)), _lib.ERR_BAD_ARG, "chol[2][1]", "finite")
    for bad_val in (0.0, -1.5):
        b = Lgood.copy()
        b[1, 1] = bad_val
        refused(cfg(chol=arr(b)), _lib.ERR_BAD_ARG, "chol[1][1]", "> 0")
    # both or neither
    refused(cfg(chol=arr(Lgood), step=arr(step)), _lib.ERR_BAD_ARG, "both step and chol")
    refused(cfg(), _lib.ERR_BAD_ARG, "neither step nor chol")
    # tuning
    refused(cfg(step=arr(step), tune_rounds=-1), _lib.ERR_BAD_ARG, "tune_rounds = -1")
    refused(cfg(step=arr(step), tune_rounds=2, nchains=3), _lib.ERR_BAD_ARG, "nchains = 3", "ndim = 3", "singular")
    refused(cfg(step=arr(step), tune_rounds=20), _lib.ERR_BAD_ARG, "tune_rounds = 20", "nburnin >= 21")
    pb = _lib.HOST_PROPOSE_FN(lambda rows, n, nd, out, user: 0)
    refused(cfg(host_propose=C.cast(pb, C.c_void_p), tune_rounds=2), _lib.ERR_BAD_ARG, "host_propose")
    refused(cfg(host_propose=C.cast(pb, C.c_void_p), chol=arr(Lgood)), _lib.ERR_BAD_ARG, "host_propose")
    refused(cfg(step=arr(step), tune_scale=-0.5), _lib.ERR_BAD_ARG, "tune_scale = -0.5")
    refused(cfg(step=arr(step), tune_scale=np.nan), _lib.ERR_BAD_ARG, "tune_scale")
    refused(cfg(step=arr(step), tune_scale=np.inf), _lib.ERR_BAD_ARG, "tune_scale")
    refused(cfg(step=arr([0.5, 0.0, 0.5]), tune_rounds=2), _lib.ERR_BAD_ARG, "step[1]")
    # what Metropolis refused before stays refused
    refused(cfg(chol=arr(Lgood), nthin=0), _lib.ERR_BAD_ARG)
    refused(cfg(chol=arr(Lgood), dtype=_lib.F32), _lib.ERR_UNSUPPORTED)
    refused(cfg(chol=arr(Lgood), density=_lib.DATA_DENSITY), _lib.ERR_UNSUPPORTED)
    refused(cfg(ndim=1, chol=arr(np.eye(1)), density=_lib.ROSENBROCK), _lib.ERR_BAD_ARG)


def test_step_objects_produce_the_factor_the_yardstick_predicts(kmc):
    cov = _spd(5, 11)
    sc = my.default_scale(5)
    want, _ = my.cholesky_lower((sc * sc) * cov)
    np.testing.assert_array_equal(kmc.MVNormalStep(cov=cov).factor(5), want)
    np.testing.assert_array_equal(kmc.MVNormalStep.from_covariance({"cov": cov, "mean": np.zeros(5)}).factor(5), want)
    np.testing.assert_array_equal(kmc.MVNormalStep(cov=cov, scale=0.5).factor(5), my.cholesky_lower((0.5 * 0.5) * cov)[0])
    L = np.tril(np.random.default_rng(0).standard_normal((4, 4))) + 3 * np.eye(4)
    dense = L + np.triu(np.ones((4, 4)), 1)                                  # the upper triangle of chol is dropped
    np.testing.assert_array_equal(kmc.MVNormalStep(chol=dense).factor(4), L)
    np.testing.assert_array_equal(kmc.MVNormalStep(chol=L, scale=2.0).factor(4), 2.0 * L)
    with pytest.raises(ValueError, match="exactly one"):
        kmc.MVNormalStep()
    with pytest.raises(ValueError, match="exactly one"):
        kmc.MVNormalStep(cov=cov, chol=L)
    with pytest.raises(ValueError, match="pivot 1"):
        kmc.MVNormalStep(cov=np.ones((2, 2)))
    with pytest.raises(ValueError, match="4 x 4"):
        kmc.MVNormalStep(chol=L).factor(5)
    t = kmc.TunedStep(kmc.GaussianStep(0.1))
    assert t.rounds == 4 and t.scale is None
    with pytest.raises(TypeError, match="initial"):
        kmc.TunedStep(lambda x: x)
    with pytest.raises(ValueError, match="rounds"):
        kmc.TunedStep(kmc.GaussianStep(0.1), rounds=0)


def test_tuning_boundaries(kmc):
    from kissmcmc_jl_amd.metropolis import tune_boundaries
    for nburnin, rounds, want in [(40, 3, [10, 20, 30]), (2000, 4, [400, 800, 1200, 1600]), (7, 3, [1, 3, 5]), (4, 3, [1, 2, 3]),
                                  (5, 4, [1, 2, 3, 4]), (9, 7, [1, 2, 3, 4, 5, 6, 7]), (10, 1, [5]),
                                  (3, 2, [1, 2]), (100, 200, None)]:
        got = tune_boundaries(nburnin, rounds)
        assert got == my.tune_boundaries(nburnin, rounds)
        if want is not None:
            assert got == want
        assert all(b < nburnin for b in got) and got == sorted(set(got))
    assert my.tune_boundaries(100, 200)[:3] == [0, 1, 2] and len(my.tune_boundaries(100, 200)) == 100     # equal boundaries collapse


# ---- the statistical GPU test's bounds (mvnormal_step_yardstick.STAT, stat_bounds), for the rule itself ----
def test_the_tuning_rule_meets_the_statistical_bounds_over_ten_seeds():
    cov = np.array([[1.0, my.STAT["rho"]], [my.STAT["rho"], 1.0]])
    mean = np.array([0.5, -0.25])
    worst = np.zeros(3)
    accs = []
    for seed in range(10):
        x, L, acc = my.simulate_tuned(np.random.default_rng(seed), mean, cov, my.STAT["nchains"], my.STAT["step0"], my.STAT["rounds"],
                                      my.STAT["nburnin"], my.STAT["niter"])
        r = my.stat_bounds(x, L, mean, cov, my.default_scale(2))
        worst = np.maximum(worst, r)
        accs.append(acc)
    print("largest |error| / se over ten seeds: mean %.2f, covariance %.2f, L L^T %.2f; acceptance %.3f .. %.3f" % (*worst, min(accs), max(accs)))
    assert (worst < 5.0).all()
    assert min(accs) > 0.2            # 2.38 / sqrt(2) on a Gaussian: about 0.35
