"""Posterior summaries without a device: quantile_ranks against hand values, summarize_run's column logic on a fake provider of order
statistics, and the numpy yardstick's radix select (tests/summary_yardstick.py -- what the GPU tests compare the kernels with) against
np.sort on the adversarial arrays.  (Header, SYMBOLS and the Julia ccalls are compared by tests/test_c_abi.py.)"""
import numpy as np
import pytest

import summary_yardstick as sy


def test_quantile_ranks_hand_values(kmc):
    lo, hi, frac = kmc.quantile_ranks([0.0, 0.5, 1.0, 0.25], 5)              # h = 0, 2, 4, 1: every frac is 0
    assert lo.tolist() == [0, 2, 4, 1] and hi.tolist() == [1, 3, 4, 2] and frac.tolist() == [0.0, 0.0, 0.0, 0.0]
    lo, hi, frac = kmc.quantile_ranks([0.5, 0.16], 4)                         # h = 1.5, 0.48
    assert lo.tolist() == [1, 0] and hi.tolist() == [2, 1] and frac.tolist() == [0.5, 0.16 * 3]
    lo, hi, frac = kmc.quantile_ranks([0.0, 0.3, 1.0], 1)                     # one value: every quantile is that value
    assert lo.tolist() == [0, 0, 0] and hi.tolist() == [0, 0, 0] and frac.tolist() == [0.0, 0.0, 0.0]
    lo, hi, frac = kmc.quantile_ranks(0.84, 1001)                             # a scalar q
    assert lo.tolist() == [840] and hi.tolist() == [841] and frac[0] == 0.84 * 1000 - 840
    for bad in ([-0.1], [1.5], [float("nan")]):
        with pytest.raises(ValueError):
            kmc.quantile_ranks(bad, 10)
    with pytest.raises(ValueError):
        kmc.quantile_ranks([0.5], 0)


def test_interpolation_is_exactly_x_lo_when_frac_is_zero(kmc):
    from kissmcmc_jl_amd.summary import interpolate
    out = interpolate(np.array([[-np.inf, 1.0], [1.0, 2.0]]), np.array([[-np.inf, 3.0], [np.inf, 4.0]]), [0.0, 0.25])
    np.testing.assert_array_equal(out, [[-np.inf, 1.0], [np.inf, 2.5]])


class FakeProvider:
    """Order statistics and arg-max from numpy, counting what summarize_run asks for."""

    def __init__(self, thetas, logp=None):
        self.chain = np.asarray(thetas).transpose(1, 0, 2)
        self.logp = None if logp is None else np.asarray(logp).T
        self.n, self.ndim = self.chain.shape[0] * self.chain.shape[1], self.chain.shape[2]
        self.rank_calls, self.argmax_calls = [], 0

    def order_stats(self, ranks, logp=False):
        self.rank_calls.append(list(ranks))
        th, lp, _ = sy.order_stats(self.chain, ranks, self.logp if logp else None)
        return th, lp

    def argmax(self):
        self.argmax_calls += 1
        return sy.argmax(self.chain, self.logp)


def test_summarize_run_columns_on_a_fake_provider(kmc):
    rng = np.random.default_rng(0)
    th = rng.standard_normal((6, 7, 3)) * [1.0, 2.0, 0.5] + [0.0, 5.0, -1.0]       # [walker][sample][dim], 42 values per dimension
    lp = rng.standard_normal((6, 7))
    flat = th.reshape(-1, 3)
    p = FakeProvider(th)
    out = kmc.summarize_run(th, provider=p)
    assert list(out) == ["var", "median", "mean", "mode", "std"]                   # analysis.jl:30
    assert out["var"] == ["1", "2", "3"] and out["mode"] is None
    assert p.rank_calls == [[20, 21]] and p.argmax_calls == 0                      # h = 0.5 * 41: the two middle order statistics
    s = np.sort(flat, axis=0)
    np.testing.assert_array_equal(out["median"], s[20] + 0.5 * (s[21] - s[20]))
    np.testing.assert_allclose(out["median"], np.median(flat, axis=0), rtol=1e-15)
    np.testing.assert_array_equal(out["mean"], flat.mean(axis=0))
    np.testing.assert_array_equal(out["std"], flat.std(axis=0, ddof=1))
    p = FakeProvider(th, lp)
    truth = np.array([0.1, 5.0, -1.2])
    out = kmc.summarize_run(th, lp, theta_true=truth, names=["a", "b", "c"], eff_samples=[10, 20, 30], provider=p)
    assert list(out) == ["var", "err", "median", "mean", "mode", "std", "eff_samples"]   # :15
    assert out["var"] == ["a", "b", "c"] and out["eff_samples"].tolist() == [10, 20, 30]
    np.testing.assert_array_equal(out["err"], np.abs(truth - out["median"]))       # :21
    w, k = np.unravel_index(np.argmax(lp), lp.shape)
    np.testing.assert_array_equal(out["mode"], th[w, k])
    assert p.argmax_calls == 1
    with pytest.raises(ValueError):
        kmc.summarize_run(th, provider=FakeProvider(th), names=["a"])
    with pytest.raises(ValueError):
        kmc.summarize_run(th, provider=FakeProvider(th), theta_true=[1.0])
    # an odd count: one order statistic, no interpolation
    p = FakeProvider(th[:5, :5])
    out = kmc.summarize_run(th[:5, :5], provider=p)
    assert p.rank_calls == [[12, 13]]                                              # h = 0.5 * 24 = 12, frac = 0: exactly x[12]
    np.testing.assert_array_equal(out["median"], np.sort(th[:5, :5].reshape(-1, 3), axis=0)[12])


def test_walker_mask_forms(kmc):
    from kissmcmc_jl_amd.summary import walker_mask
    assert walker_mask(None, 4) is None
    assert walker_mask([True, False, True, False], 4).tolist() == [1, 0, 1, 0]
    assert walker_mask([3, 0, 3], 4).tolist() == [1, 0, 0, 1]
    with pytest.raises(IndexError):
        walker_mask([4], 4)
    with pytest.raises(ValueError):
        walker_mask([True, False], 4)


def test_key_transform_orders_like_the_values():
    x = np.array([-np.inf, -1.7e308, -1.0, -2.2e-308, -5e-324, -0.0, 0.0, 5e-324, 2.2e-308, 1.0, 1.7e308, np.inf])
    k = sy.keys(x)
    assert np.all(k[1:] > k[:-1])                                                  # strictly: -0.0 below +0.0
    np.testing.assert_array_equal(sy.unkeys(k).view(np.uint64), x.view(np.uint64))
    nan_pos, nan_neg = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64), np.array([0xFFF8000000000000], dtype=np.uint64).view(np.float64)
    assert sy.keys(nan_pos)[0] > k[-1] and sy.keys(nan_neg)[0] < k[0]              # NaN policy: by bit pattern, beyond the infinities


@pytest.mark.parametrize("name", sorted(sy.adversarial()))
def test_yardstick_radix_select_equals_sort(name):
    x = sy.adversarial()[name]
    s = sy.sort_by_key(x)
    np.testing.assert_array_equal(s, np.sort(x))                                   # (as values; the key order also fixes -0.0 < +0.0)
    n = x.size
    for r in sorted({0, 1, n // 10, n // 2 - 1, n // 2, n // 2 + 1, n - n // 10, n - 2, n - 1}):
        got = sy.radix_select(x, r)
        assert np.float64(got).view(np.uint64) == s[r].view(np.uint64), (name, r)
