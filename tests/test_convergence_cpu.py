"""CPU: the host stage of the convergence diagnostics (kmc_convergence_stats) against its restatement
(tests/convergence_yardstick.py: stats) bit for bit, the argument checks that need no device, the degenerate inputs, and the statistical
sanity of the definition itself (include/kissmcmc_hip.h) on AR(1) chains, whose effective sample size is known:
ess = m h (1 - phi) / (1 + phi).  No device anywhere: the three input arrays are the yardstick's exact ones."""
import ctypes as C
import math

import numpy as np
import pytest

import convergence_yardstick as cy

KEYS = ("mean", "W", "B", "var_plus", "rhat", "ess", "mcse", "T", "flags")
PHIS = (0.0, 0.5, 0.9)
NW, NS, MAX_LAG = 16, 2001, 256


@pytest.fixture(scope="module")
def ar1_raw():
    """{(phi, seed): (chain, raw arrays with every lag up to MAX_LAG)} for ten seeds: 30 chains of 16 walkers x 2 001 samples."""
    out = {}
    for phi in PHIS:
        for seed in range(10):
            x = cy.ar1(np.random.default_rng(seed), phi, NS, NW, 1)
            out[phi, seed] = (x, cy.raw(x, lag0=1, nlags=MAX_LAG))
    return out


def same_bits(got, want, keys=KEYS):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, k
        assert g.tobytes() == w.tobytes() or (np.array_equal(g, w, equal_nan=True) and not np.any(np.signbit(g) != np.signbit(w))), \
            f"{k}: {g} != {w}"


@pytest.mark.parametrize("phi", PHIS)
def test_host_stage_equals_the_yardstick_bit_for_bit(kmc, ar1_raw, phi):
    _, r = ar1_raw[phi, 0]
    m, h = r["m"], r["h"]
    assert (m, h) == (2 * NW, NS // 2)
    want = cy.stats(m, h, r["chain_mean"], r["chain_var"], r["lagsum"], MAX_LAG)
    got = kmc.convergence_stats(m, h, r["chain_mean"], r["chain_var"], r["lagsum"], MAX_LAG)
    same_bits(got, want)
    assert want["flags"][0] == 0 and want["T"][0] % 2 == 1 and 1.0 < want["ess"][0] <= 1.2 * m * h
    # the lags in pieces: too few first (bit 0 says so, ess is provisional), then more, until the rule fires; every step bit for bit
    T = int(want["T"][0])
    seen_need = False
    for nlags in sorted({0, 1, 2, 3, 4, T, T + 1, T + 2, T + 3, MAX_LAG}):
        piece = r["lagsum"][:, :nlags]
        w = cy.stats(m, h, r["chain_mean"], r["chain_var"], piece, MAX_LAG)
        same_bits(kmc.convergence_stats(m, h, r["chain_mean"], r["chain_var"], piece, MAX_LAG), w)
        need = bool(w["flags"][0] & cy.NEED_LAGS)
        assert need == (nlags < T + 2)
        seen_need = seen_need or need
        if not need:
            same_bits(w, want)                                                     # the lags beyond T + 2 are never read
    assert seen_need
    # max_lag = 3: one test of the rule, rho_2 + rho_3; where it does not fire, T = 3 and the walk is truncated there
    w3 = cy.stats(m, h, r["chain_mean"], r["chain_var"], r["lagsum"][:, :3], 3)
    same_bits(kmc.convergence_stats(m, h, r["chain_mean"], r["chain_var"], r["lagsum"][:, :3], 3), w3)
    assert w3["T"][0] == min(T, 3) and w3["flags"][0] == (cy.TRUNCATED if T > 1 else 0)
    # several columns at once, unsplit chains
    x = cy.ar1(np.random.default_rng(3), phi, 301, 5, 3)
    r3 = cy.raw(x, logp=x[:, :, 0] * x[:, :, 1], split=False, lag0=1, nlags=100)
    assert (r3["m"], r3["h"]) == (5, 301) and r3["lagsum"].shape == (4, 100)
    same_bits(kmc.convergence_stats(5, 301, r3["chain_mean"], r3["chain_var"], r3["lagsum"], 100),
              cy.stats(5, 301, r3["chain_mean"], r3["chain_var"], r3["lagsum"], 100))


def test_exact_row_sums_of_the_yardstick_are_math_fsum():
    """The yardstick adds long rows with numpy in slices that carry no rounding error and lets math.fsum add the slice sums; that is
    math.fsum over the elements, which this checks on rows it would take math.fsum itself a blink to add."""
    rng = np.random.default_rng(0)
    for trial in range(24):
        n, k = int(rng.integers(64, 5000)), int(rng.integers(1, 5))
        a = rng.standard_normal((k, n)) * np.exp(rng.uniform(-40, 40, (k, n))) if trial % 2 else rng.standard_normal((k, n)) ** 2
        if trial == 5:
            a[:] = 1e-320
        if trial == 7:
            a *= 1e280
        if trial == 9:
            a *= 1e-300
        if trial == 11:
            a[0, 3] = 0.1 * 2.0 ** 60
        np.testing.assert_array_equal(cy.fsum_rows(a), [math.fsum(row) for row in a.tolist()])
    a = rng.standard_normal((3, 500))
    a[0, 5], a[1, 6] = np.nan, np.inf
    got = cy.fsum_rows(a)
    assert np.isnan(got[0]) and got[1] == np.inf and got[2] == math.fsum(a[2].tolist())


def test_argument_checks_need_no_device(kmc):
    from kissmcmc_jl_amd import _lib
    L = _lib.lib()
    dp, ip, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    m, h, nlags = 4, 10, 9
    cm, cv, lag = np.zeros((1, m)), np.ones((1, m)), np.ones((1, nlags))
    outs = [np.zeros(1) for _ in range(7)]
    T, flags = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32)

    def call(m=m, h=h, ncols=1, nlags=nlags, max_lag=9, null=None):
        ptrs = [a.ctypes.data_as(dp) for a in (cm, cv, lag)] + [a.ctypes.data_as(dp) for a in outs] + [T.ctypes.data_as(ip), flags.ctypes.data_as(i32p)]
        if null is not None:
            ptrs[null] = None
        return L.kmc_convergence_stats(m, h, ncols, ptrs[0], ptrs[1], ptrs[2], nlags, max_lag, *ptrs[3:])

    assert call() == _lib.OK
    assert call(h=3, max_lag=2, nlags=2) == _lib.ERR_BAD_ARG                       # h < 4
    assert call(m=1) == _lib.ERR_BAD_ARG                                           # m < 2
    assert call(max_lag=2) == _lib.ERR_BAD_ARG and call(max_lag=10) == _lib.ERR_BAD_ARG and call(max_lag=0) == _lib.ERR_BAD_ARG
    assert call(max_lag=3) == _lib.OK and call(max_lag=h - 1) == _lib.OK
    assert call(nlags=-1) == _lib.ERR_BAD_ARG and call(nlags=h) == _lib.ERR_BAD_ARG and call(ncols=0) == _lib.ERR_BAD_ARG
    for k in range(12):
        assert call(null=k) == _lib.ERR_BAD_ARG, k
    assert call(nlags=0, null=2) == _lib.OK                                        # no lags given: no array needed
    # the host-chain calls check the whole request before they look for a device (none here: a request that passed would not say BAD_ARG)
    th = np.zeros((3, 9, 2))                                                       # [walker][sample][dim]: n = 9, h = 4 split
    for bad in (dict(first_sample=2),                                              # h = 3
                dict(walkers=[1], split=False),                                    # m = 1
                dict(max_lag=4), dict(max_lag=2), dict(max_lag=0),                 # h - 1 = 3
                dict(first_sample=9), dict(walkers=np.zeros(3, dtype=bool))):      # an empty selection
        with pytest.raises(kmc.KmcError) as e:
            kmc.convergence(th, **bad)
        assert e.value.status == _lib.ERR_BAD_ARG, bad
    for bad in (dict(lag0=0, nlags=1), dict(lag0=1, nlags=4), dict(lag0=4, nlags=1), dict(lag0=1, nlags=-1), dict(first_sample=2)):
        with pytest.raises(kmc.KmcError) as e:
            kmc.lag_sums(th, **bad)
        assert e.value.status == _lib.ERR_BAD_ARG, bad
    from kissmcmc_jl_amd import chain_convergence
    plan = chain_convergence.lag_plan()
    assert plan["lag_block"] >= 8 and plan["lds_bytes"] <= 64 * 1024 and plan["lanes"] == 64


def test_degenerate_inputs(kmc):
    m, h, nlags = 6, 50, 49
    rng = np.random.default_rng(1)
    # a constant chain: W == 0 -> NaN, no error; next to an ordinary column
    x = cy.ar1(rng, 0.5, 100, 3, 2)
    x[:, :, 0] = 2.5
    r = cy.raw(x, lag0=1, nlags=nlags)
    want = cy.stats(m, h, r["chain_mean"], r["chain_var"], r["lagsum"], nlags)
    got = kmc.convergence_stats(m, h, r["chain_mean"], r["chain_var"], r["lagsum"], nlags)
    same_bits(got, want)
    assert got["W"][0] == 0.0 and got["mean"][0] == 2.5 and got["T"][0] == 0 and got["flags"][0] == 0
    assert np.isnan(got["rhat"][0]) and np.isnan(got["ess"][0]) and np.isnan(got["mcse"][0])
    assert np.isfinite([got[k][1] for k in ("rhat", "ess", "mcse")]).all()
    # every chain constant at its own value: W == 0 still, B > 0
    cm = np.arange(6.0)[None, :]
    got = kmc.convergence_stats(m, h, cm, np.zeros((1, 6)), np.zeros((1, nlags)), nlags)
    assert got["B"][0] > 0 and np.isnan(got["rhat"][0]) and np.isnan(got["ess"][0])
    # a NaN in the chain propagates: mean, variance and every lag sum are NaN (sample 0 is in a pair at every lag)
    x = cy.ar1(rng, 0.5, 100, 3, 2)
    x[0, 1, 1] = np.nan
    r = cy.raw(x, lag0=1, nlags=nlags)
    assert np.isnan(r["lagsum"][1]).all() and np.isfinite(r["lagsum"][0]).all()
    got = kmc.convergence_stats(m, h, r["chain_mean"], r["chain_var"], r["lagsum"], nlags)
    same_bits(got, cy.stats(m, h, r["chain_mean"], r["chain_var"], r["lagsum"], nlags))
    assert all(np.isnan(got[k][1]) for k in ("mean", "W", "var_plus", "rhat", "ess", "mcse")) and got["flags"][1] == cy.TRUNCATED
    assert all(np.isfinite(got[k][0]) for k in ("mean", "W", "var_plus", "rhat", "ess", "mcse"))
    # an infinity likewise (inf - inf in the centred squares)
    x[0, 1, 1] = np.inf
    r = cy.raw(x, lag0=1, nlags=nlags)
    got = kmc.convergence_stats(m, h, r["chain_mean"], r["chain_var"], r["lagsum"], nlags)
    assert got["mean"][1] == np.inf and np.isnan(got["rhat"][1]) and np.isnan(got["ess"][1])
    # negative correlations large enough to take the denominator to zero or below: ess is NaN, not negative
    lag = np.array([[4.0 * (h - 1) / h * 2 * (h - t) for t in (1, 2, 3)]])         # V_t = 4 var+, so rho_t = -1 and 1 + 2 rho_1 = -1
    got = kmc.convergence_stats(2, h, np.zeros((1, 2)), np.ones((1, 2)), lag, 3)
    assert got["T"][0] == 1 and np.isnan(got["ess"][0]) and np.isnan(got["mcse"][0]) and np.isfinite(got["rhat"][0])


def test_statistical_sanity_of_the_definition(kmc, ar1_raw):
    """AR(1) chains of unit variance, 16 walkers x 2 001 samples split into m = 32 chains of h = 1 000, max_lag = 256, seeds 0 .. 9 and
    phi in {0, 0.5, 0.9}.  Measured with the yardstick (numpy + math.fsum), over the 30 runs:
        ess (1 + phi) / ((1 - phi) m h)    0.8361 ... 1.0870   (phi = 0: 0.972 ... 1.006; 0.5: 0.940 ... 1.029; 0.9: 0.836 ... 1.087)
        rhat                               0.99983 ... 1.01241
        T                                  1 ... 99, never truncated
    The bounds asserted are those ranges widened by half their width either way: 0.7107 ... 1.2125 and rhat <= 1.0187 (>= 0.9935).
    One walker of eight shifted by 3 sigma: 2 of the 16 split chains have mean 3, so B / h = (14 * 0.375^2 + 2 * 2.625^2) / 15 = 1.05,
    var+ = 2.05 W and rhat = 1.43 (measured 1.433 ... 1.440 over the three phi); asserted within 0.05.
    A step of 1 000 between the halves of every walker: split, B / h = 1000^2 / 4 * 32 / 31 against W = 1, rhat = 508 (measured
    507.9); unsplit, the step is inside every chain, W = 250 000 and rhat = sqrt((h - 1) / h + B / (h W)) = 0.99975 (measured)."""
    lo, hi, rlo, rhi = 0.8361 - 0.5 * (1.0870 - 0.8361), 1.0870 + 0.5 * (1.0870 - 0.8361), 0.99983 - 0.5 * (1.01241 - 0.99983), 1.01241 + 0.5 * (1.01241 - 0.99983)
    ratios, rhats = [], []
    for (phi, seed), (x, r) in ar1_raw.items():
        got = kmc.convergence_stats(r["m"], r["h"], r["chain_mean"], r["chain_var"], r["lagsum"], MAX_LAG)
        assert got["flags"][0] == 0, (phi, seed)                                  # no truncation
        ratios.append(got["ess"][0] * (1 + phi) / (1 - phi) / (r["m"] * r["h"]))
        rhats.append(got["rhat"][0])
        assert abs(got["mcse"][0] - math.sqrt(got["var_plus"][0] / got["ess"][0])) <= 1e-15
    print("ess ratio", min(ratios), max(ratios), "rhat", min(rhats), max(rhats))
    assert lo <= min(ratios) and max(ratios) <= hi
    assert rlo <= min(rhats) and max(rhats) <= rhi
    for phi in PHIS:
        x = cy.ar1(np.random.default_rng(0), phi, NS, 8, 1)
        x[:, 3, :] += 3.0
        r = cy.raw(x, lag0=1, nlags=MAX_LAG)
        got = kmc.convergence_stats(r["m"], r["h"], r["chain_mean"], r["chain_var"], r["lagsum"], MAX_LAG)
        print("shifted", phi, got["rhat"][0])
        assert abs(got["rhat"][0] - 1.43) < 0.05
    x = ar1_raw[0.5, 0][0].copy()
    x[NS // 2 + 1:] += 1000.0
    r = cy.raw(x, lag0=1, nlags=MAX_LAG)
    got = kmc.convergence_stats(r["m"], r["h"], r["chain_mean"], r["chain_var"], r["lagsum"], MAX_LAG)
    r1 = cy.raw(x, split=False, lag0=1, nlags=MAX_LAG)
    got1 = kmc.convergence_stats(r1["m"], r1["h"], r1["chain_mean"], r1["chain_var"], r1["lagsum"], MAX_LAG)
    print("step", got["rhat"][0], got1["rhat"][0])
    assert got["rhat"][0] > 100 and got1["rhat"][0] < 1.01 and (r1["m"], r1["h"]) == (NW, NS)


def test_python_surface_without_a_device(kmc):
    """What the Python layer does on its own: the column dict, the argument plumbing of evaluate_convergence and samples_vs_tau's
    prefixes -- the device calls themselves are in tests/test_gpu_convergence.py."""
    from kissmcmc_jl_amd import chain_convergence as conv
    raw = {"mean": np.zeros(2), "var_plus": np.array([4.0, np.nan]), "rhat": np.ones(2), "ess": np.ones(2), "mcse": np.ones(2),
           "T": np.array([3, 5]), "flags": np.array([0, 2], dtype=np.int32), "m": 4, "h": 10}
    cols = conv.columns(raw)
    assert list(cols) == list(conv.COLUMNS) and cols["std"][0] == 2.0 and np.isnan(cols["std"][1])
    assert cols["truncated"].tolist() == [False, True] and cols["lag"].tolist() == [3, 5]
    base = kmc.summary.summary_columns(None, np.zeros(2), np.zeros(2), np.ones(2))
    more = kmc.summary.summary_columns(None, np.zeros(2), np.zeros(2), np.ones(2), convergence=cols)
    assert list(more) == list(base) + ["rhat", "ess", "mcse"] and all(np.array_equal(more[k], base[k]) for k in base if k != "mode")
    with pytest.raises(ValueError):
        kmc.evaluate_convergence()
    with pytest.raises(ValueError):
        kmc.evaluate_convergence(np.zeros((2, 10, 1)), np.zeros((2, 11, 1)))
