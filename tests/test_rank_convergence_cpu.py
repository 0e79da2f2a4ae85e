"""The parts of the rank-normalised convergence diagnostics that need no device: the normal score (kmc_rank_normal_scores) against
statistics.NormalDist().inv_cdf and the yardstick's vectorised restatement of it (tests/rank_yardstick.py), the ranks of the yardstick
against scipy's, the plan, and the refusals of the host-chain calls, which must come before the device is looked for.

The tail bound.  In the central branch (|p - 0.5| <= 0.425) the score is +, -, *, / on the same inputs in the same order: the same bits.
In the tails both sides form t = sqrt(-log(r)) from the same r; the two logarithms are within 1 ulp each of the true one, the two sqrt
and the two subtractions move t - 1.6 (or t - 5) by at most 6 * 2^-53 t; |dz/dt| < 1.5 and t <= 1.12 |z| there; each side then commits
29 roundings in Horner sums whose coefficients and argument are all positive, so nothing cancels: (10 + 58) 2^-53 |z|, asserted with 96
for slack."""
import ctypes as C

import numpy as np
import pytest

import rank_yardstick as ry

U = 2.0 ** -53
TAIL = 96 * U


def same_values(a, b):
    """Bit for bit, compared by value: the sign of a zero does not count."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a == b))


def test_restatement_equals_the_standard_library_bit_for_bit():
    S = 1000
    r2 = np.arange(2, 2 * S + 1, dtype=np.int64)
    assert same_values(ry.scores(r2, S), ry.scores_scalar(r2, S))
    p = ry.p_of(r2, S)
    assert 0.80 < ry.central(p).mean() < 0.90 and p.min() > 0.0 and p.max() < 1.0
    S = 2 ** 31
    r2 = np.array([2, 3, S, S + 1, 2 * S], dtype=np.int64)
    z = ry.scores(r2, S)
    assert same_values(z, ry.scores_scalar(r2, S))
    assert z[0] < -6.0 and z[4] > 6.0 and abs(z[3]) < 1e-9                      # (the far tail branch, r > 5, on both sides)


def test_library_host_scores(kmc):
    for S in (40, 1000, 2 ** 31):
        r2 = np.arange(2, 2 * S + 1, dtype=np.int64) if S <= 1000 else np.array([2, 3, 5, S, S + 1, 2 * S - 1, 2 * S], dtype=np.int64)
        got, want = kmc.normal_scores(r2, S), ry.scores(r2, S)
        mid = ry.central(ry.p_of(r2, S))
        assert same_values(got[mid], want[mid])
        err = np.abs(got[~mid] - want[~mid]) / np.abs(want[~mid])
        print(f"S={S}: tails, largest error / bound {err.max() / TAIL:.3f}")
        assert np.all(err <= TAIL)
    assert kmc.normal_scores(np.array([[2, 3], [4, 5]]), 4).shape == (2, 2)


def test_library_host_scores_refusals(kmc):
    from kissmcmc_jl_amd import _lib
    for r2, S in (([2], 0), ([1], 4), ([9], 4), ([2, 3, 0], 4)):
        with pytest.raises(kmc.KmcError) as e:
            kmc.normal_scores(r2, S)
        assert e.value.status == _lib.ERR_BAD_ARG


def test_ranks_are_scipys_average_ranks():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(0)
    for x in (rng.standard_normal(1001), np.round(rng.standard_normal(1000), 1), np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 0.0, 1.0]),
              np.full(17, 2.5)):
        np.testing.assert_array_equal(ry.rank2_of(x) / 2, stats.rankdata(x, "average"))


def test_scores_against_ndtri():
    special = pytest.importorskip("scipy.special")
    S = 1000
    r2 = np.arange(2, 2 * S + 1, dtype=np.int64)
    z, ref = ry.scores(r2, S), special.ndtri(ry.p_of(r2, S))
    nz = ref != 0.0
    rel = np.abs(z[nz] - ref[nz]) / np.abs(ref[nz])
    print(f"largest relative difference from scipy.special.ndtri: {rel.max():.3e}")
    assert rel.max() < 1e-14 and np.all(z[~nz] == 0.0)


def test_plan(kmc):
    p = kmc.rank_plan()
    assert list(p) == ["tile_keys", "digit_bits", "passes", "lds_bytes"]
    assert p["digit_bits"] * p["passes"] == 64 and p["tile_keys"] % 256 == 0 and 256 <= p["tile_keys"] <= 65536
    assert 8 * p["tile_keys"] <= p["lds_bytes"] <= 64 * 1024


def test_yardstick_transforms():
    """The yardstick on a case small enough to check by hand: ties, the fold, the indicators and a NaN column."""
    chain = np.zeros((4, 2, 2))
    chain[:, :, 0] = [[1.0, 3.0], [2.0, 2.0], [5.0, -0.0], [0.0, 4.0]]
    chain[:, :, 1] = 1.0
    chain[2, 1, 1] = np.nan
    t = ry.transforms(chain, split=False)
    assert (t["m"], t["h"], t["S"]) == (2, 4, 8)
    np.testing.assert_array_equal(t["rank2"][0], [[6, 9, 16, 3], [12, 9, 3, 14]])
    assert t["median"][0] == 2.0 and t["nan_count"].tolist() == [0, 1] and t["nan_count_folded"].tolist() == [0, 8]
    np.testing.assert_array_equal(t["rank2_folded"][0], [[7, 3, 16, 12], [7, 3, 12, 12]])
    assert np.isnan(t["z"][1]).all() and (t["rank2"][1] == 0).all() and np.isnan(t["q05"][1])
    assert t["i95"][0].sum() == 7 and t["i05"][0].sum() == 2


def test_host_chain_refusals_come_before_the_device(kmc):
    from kissmcmc_jl_amd import _lib
    expect = {_lib.ERR_BAD_ARG}                                                # never ERR_NO_DEVICE: the checks come first
    th = np.random.default_rng(0).standard_normal((4, 20, 2))

    def status(fn):
        with pytest.raises(kmc.KmcError) as e:
            fn()
        return e.value.status

    for fn in (kmc.rank_convergence, kmc.rank_scores):
        assert status(lambda: fn(th[:, :7])) in expect                          # h = 3
        assert status(lambda: fn(th[:1], split=False)) in expect                # one chain
        assert status(lambda: fn(th, first_sample=21)) in expect
        assert status(lambda: fn(th, first_sample=14)) in expect                # h = 3
        assert status(lambda: fn(th, walkers=np.zeros(4, dtype=bool))) in expect
    assert status(lambda: kmc.rank_convergence(th, max_lag=10)) in expect       # max_lag >= h
    assert status(lambda: kmc.rank_convergence(th, max_lag=2)) in expect
    assert status(lambda: kmc.convergence(th, max_lag=2, rank=True)) in expect
    L = _lib.lib()
    dp = C.POINTER(C.c_double)
    x = np.zeros(64)
    assert L.kmc_chain_rank_convergence(x.ctypes.data_as(dp), None, 16, 2, 2, 0, None, 1, 0, 0, *([None] * 12), None, None, None) == _lib.ERR_BAD_ARG
    assert L.kmc_chain_rank_scores(None, None, 16, 2, 2, 0, None, 1, 0, 0, None, None, None, None, None, None) == _lib.ERR_BAD_ARG
    assert L.kmc_sampler_rank_scores(None, 0, None, 1, 0, 0, None, None, None, None, None, None) == _lib.ERR_BAD_ARG
    assert L.kmc_sampler_rank_convergence(None, 0, None, 1, 0, 0, *([None] * 12), None, None, None) == _lib.ERR_BAD_ARG


def test_every_host_chain_call_refuses_from_its_sizes_before_the_device(kmc):
    """All seven kmc_chain_* read-outs go describe -> arguments -> sizes out -> open -> device work, so a fault in
    the chain, the selection or the call's own arguments is ERR_BAD_ARG on a machine with no device, never ERR_NO_DEVICE."""
    from kissmcmc_jl_amd import _lib
    L = _lib.lib()
    dp, ip, bp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    NS, NW, ND = 16, 4, 2
    chain, logp = np.zeros(NS * NW * ND), np.zeros(NS * NW)
    d, i8 = np.zeros(4096), np.zeros(4096, dtype=np.int64)                     # room for every output of every call
    i4, ranks = np.zeros(64, dtype=np.int32), np.zeros(17, dtype=np.int64)
    edges = np.tile(np.linspace(-1.0, 1.0, 9), ND + 1)
    D, I, I4 = d.ctypes.data_as(dp), i8.ctypes.data_as(ip), i4.ctypes.data_as(i32p)

    def source(c):                                                              # the arguments every call leads with
        mask = None if c["mask"] is None else c["mask"].ctypes.data_as(bp)
        return (None if c["chain"] is None else c["chain"].ctypes.data_as(dp), None if c["logp"] is None else c["logp"].ctypes.data_as(dp),
                c["nsamples"], NW, ND, c["first"], mask)

    def order_stats(c):
        return L.kmc_chain_order_stats(*source(c), c["ranks"].ctypes.data_as(ip), c["nranks"], 0, D, c["logp_out"], I)

    calls = {
        "order_stats": order_stats,
        "argmax": lambda c: L.kmc_chain_argmax(*source(c), 0, I, I, D, D),
        "histograms": lambda c: L.kmc_chain_histograms(*source(c), None, 0, edges.ctypes.data_as(dp), 8, 0, I, I, I, I),
        "lag_sums": lambda c: L.kmc_chain_lag_sums(*source(c), 1, 1, 5, 0, D, D, D, I, I),
        "convergence": lambda c: L.kmc_chain_convergence(*source(c), 1, 0, 0, *([D] * 7), I, I4, I, I, I),
        "rank_scores": lambda c: L.kmc_chain_rank_scores(*source(c), 1, 1, 0, I, D, D, I, I, I),
        "rank_convergence": lambda c: L.kmc_chain_rank_convergence(*source(c), 1, 0, 0, *([D] * 10), I, I4, I, I, I),
    }
    good = dict(chain=chain, logp=logp, nsamples=NS, first=0, mask=None, ranks=ranks, nranks=1, logp_out=None)
    faults = {"null chain": dict(chain=None), "nsamples = 0": dict(nsamples=0), "an all-zero walker mask": dict(mask=np.zeros(NW, dtype=np.uint8)),
              "first_sample > nsamples": dict(first=NS + 1)}
    own = {"order_stats": {"a rank equal to N": dict(ranks=np.full(1, NS * NW, dtype=np.int64)), "17 ranks": dict(nranks=17),
                           "logp_out without logp_host": dict(logp=None, logp_out=D)},
           "argmax": {"null logp_host": dict(logp=None)}}
    for name, call in calls.items():
        assert call(good) in (_lib.OK, _lib.ERR_NO_DEVICE), name                  # the table's own call is sound: it gets as far as the device
        for what, change in {**faults, **own.get(name, {})}.items():
            assert call({**good, **change}) == _lib.ERR_BAD_ARG, (name, what)
