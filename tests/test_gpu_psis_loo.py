"""GPU: PSIS-LOO of a DataDensity over a stored chain (kmc.loo, kmc.psis_tail, Sampler.loo, Sampler.psis_tail) against
tests/psis_yardstick.py, the numpy restatement of the definition in include/kissmcmc_hip.h.

* The exact parts -- the shift m_j, the cut-off xc_j, the tail's size and its sorted entries -- equal numpy on the matrix the device
  itself returns (pointwise_loglike), bit for bit.
* The invariants: equal calls, a selection against the rows copied out, the sampler's route against the host route, a range of
  observations against the slice of the whole call, several blocks of observations against one -- all bit for bit.
* The values.  The tolerance is measured, not chosen: DIST holds, per row count and output, the distance of the float64 yardstick from its
  longdouble mode on these very inputs (the device's matrix of psis_cases.TERM equals numpy's bit for bit, which is asserted), relative
  to max(1, |value|); the device gets 8 times that -- its exp / log / log1p / expm1 and its order of summation differ from numpy's, each
  a few ulp per operation over the same operation count -- with the floor (M + 4) 2^-53 on the same scale, M the tail length.
* The statistics, on the conjugate normal-mean model, against ten seeds of the numpy route and the closed form.
"""
import functools
import math

import numpy as np
import pytest

import psis_cases as pc
import psis_yardstick as Y

pytestmark = pytest.mark.gpu

# python tests/psis_cases.py        (float64 yardstick against its longdouble mode, the largest over J in psis_cases.JS; no device)
DIST = {
    5: dict(pareto_k=0.00e+00, elpd_loo_j=2.66e-16, p_loo_j=5.13e-16, elpd_loo=5.55e-17, se=0.00e+00, p_loo=1.01e-15),    # same weights dropped: True; any dropped: False
    24: dict(pareto_k=1.01e-13, elpd_loo_j=1.92e-15, p_loo_j=2.47e-15, elpd_loo=8.88e-16, se=1.60e-16, p_loo=1.10e-15),    # same weights dropped: True; any dropped: False
    25: dict(pareto_k=4.26e-14, elpd_loo_j=1.07e-15, p_loo_j=9.69e-16, elpd_loo=1.61e-16, se=2.06e-16, p_loo=8.69e-16),    # same weights dropped: True; any dropped: False
    30: dict(pareto_k=4.64e-15, elpd_loo_j=3.17e-16, p_loo_j=6.62e-16, elpd_loo=1.58e-16, se=0.00e+00, p_loo=5.22e-16),    # same weights dropped: True; any dropped: False
    457: dict(pareto_k=2.26e-15, elpd_loo_j=4.01e-16, p_loo_j=1.03e-15, elpd_loo=1.94e-16, se=2.78e-16, p_loo=1.74e-15),    # same weights dropped: True; any dropped: True
    7300: dict(pareto_k=6.51e-15, elpd_loo_j=1.55e-15, p_loo_j=2.86e-15, elpd_loo=2.22e-16, se=4.68e-16, p_loo=1.01e-15),    # same weights dropped: True; any dropped: True
}
ARRAYS = ("elpd_loo_j", "p_loo_j", "pareto_k", "n_tail_j", "lppd_j")
SCALARS = ("elpd_loo", "se", "p_loo", "looic", "lppd", "n", "tail_len", "n_nan", "k_counts")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def same_result(a, b, keys=ARRAYS + SCALARS):
    return all(same(a[k], b[k]) for k in keys)


@functools.lru_cache(maxsize=None)
def density(J, n):
    import kissmcmc_jl_amd as kmc
    return kmc.DataDensity(pc.TERM, pc.case(J, n)[1])


@functools.lru_cache(maxsize=None)
def device_results(J, n):
    """One shape's matrix, tails and LOO from the device; computed once."""
    import kissmcmc_jl_amd as kmc
    th, _, _ = pc.case(J, n)
    pdf = density(J, n)
    return kmc.pointwise_loglike(pdf, th), kmc.psis_tail(pdf, th), kmc.loo(pdf, th)


def check_exact(l, t, r_eff=1.0):
    """m_j, xc_j, n_tail_j and the sorted tail of psis_tail against numpy on the matrix ``l``."""
    n, J = l.shape
    M = Y.tail_length(n, r_eff)
    assert t["tail_len"] == M and t["n"] == n and t["tail"].shape == (J, M)
    for j in range(J):
        st = Y.shift_and_tail(l[:, j], M)
        if st is None:
            assert t["n_tail_j"][j] == -1 and np.isnan(t["m_j"][j]) and np.isnan(t["xc_j"][j]) and np.isnan(t["tail"][j]).all(), j
            continue
        m, xc, x, mask = st
        tail = np.sort(x[mask])
        assert t["n_tail_j"][j] == tail.size <= M, j
        assert same(t["m_j"][j], m) and same(t["xc_j"][j], xc), j
        assert same(t["tail"][j, :tail.size], tail) and np.isnan(t["tail"][j, tail.size:]).all(), j


@pytest.mark.parametrize("n", pc.NS)
@pytest.mark.parametrize("J", pc.JS)
def test_exact_parts_equal_numpy_bit_for_bit(kmc, J, n):
    """No fit (n = 5: M = 1), the first fits (24, 25, 30: M = 5, 5, 7), a tail wider than a wave (457: M = 65) and wider than a
    workgroup (7300: M = 257); the packed form (J < 64) and the plain one with a ragged last wave; from n = 24 up more than one run,
    the last one short."""
    l, t, w = device_results(J, n)
    assert (bits(l) == bits(pc.case(J, n)[2])).all()                  # (so DIST was measured on this very matrix)
    plan = kmc.pointwise_plan(n, J)
    assert n < 24 or (plan["nruns"] > 1 and n % plan["run_len"] != 0)
    check_exact(l, t)
    assert (w["n_tail_j"] == t["n_tail_j"]).all() and w["tail_len"] == t["tail_len"] == kmc.psis_plan(n, J)["tail_len"]


def test_a_tail_of_four_thousand(kmc):
    """r_eff = 0.01 at n = 20 000: M = min(4000, 4242.6) = 4000, the sort's 4096 slots nearly full."""
    th, _, l_np = pc.case(3, 20000)
    pdf = density(3, 20000)
    l = kmc.pointwise_loglike(pdf, th)
    assert (bits(l) == bits(l_np)).all()
    t = kmc.psis_tail(pdf, th, r_eff=0.01)
    assert t["tail_len"] == 4000
    check_exact(l, t, 0.01)
    w = kmc.loo(pdf, th, r_eff=0.01)
    assert w["tail_len"] == 4000 and (w["n_tail_j"] == t["n_tail_j"]).all() and np.isfinite(w["elpd_loo_j"]).all()


def tolerance(n, key, value, M):
    return max(8.0 * DIST[n][key], (M + 4) * 2.0 ** -53) * np.maximum(1.0, np.abs(np.asarray(value, dtype=np.float64)))


@pytest.mark.parametrize("n", pc.NS)
@pytest.mark.parametrize("J", pc.JS)
def test_values_against_the_yardstick(kmc, J, n):
    l, _, w = device_results(J, n)
    d64, d80 = [], []
    y = Y.loo(l, dropped=d64)
    Y.loo(l, longdouble=True, dropped=d80)
    assert len(d64) == len(d80) and all((p == q).all() for p, q in zip(d64, d80))          # the two modes drop the same weights
    M = y["tail_len"]
    assert w["n"] == n and w["n_nan"] == 0 and w["tail_len"] == M
    for key in ("pareto_k", "elpd_loo_j", "p_loo_j"):
        inf = np.isinf(y[key])
        assert (np.isinf(w[key]) == inf).all() and (w[key][inf] == y[key][inf]).all(), key
        err, tol = np.abs(w[key][~inf] - y[key][~inf]), tolerance(n, key, y[key][~inf], M)
        print(f"J {J} n {n} {key}: largest error / tolerance {np.max(err / tol) if err.size else 0.0:.3f}")
        assert (err <= tol).all(), (key, float(np.max(err / tol)))
    for key in ("elpd_loo", "p_loo") + (("se",) if J > 1 else ()):
        tol = tolerance(n, key, y[key], M)
        print(f"J {J} n {n} {key}: error {abs(w[key] - y[key]):.3e}, tolerance {float(tol):.3e}")
        assert abs(w[key] - y[key]) <= tol, key
    assert w["looic"] == -2.0 * w["elpd_loo"]
    assert w["k_counts"] == Y.totals(w["elpd_loo_j"], w["lppd_j"], w["pareto_k"])["k_counts"] and sum(w["k_counts"]) == J
    again = kmc.loo(density(J, n), pc.case(J, n)[0])
    assert same_result(w, again)


def injected(kmc, cols):
    """kmc.loo / kmc.psis_tail / the matrix of an arbitrary [n][len(cols)] matrix, through INJECT_TERM."""
    l = np.column_stack(cols)
    n, J = l.shape
    pdf = kmc.DataDensity(pc.INJECT_TERM, np.arange(J, dtype=np.float64)[:, None])
    th = l.reshape(n // 4, 4, J).transpose(1, 0, 2)                                     # [walker][sample][dim]: row = sample * 4 + walker
    got = kmc.pointwise_loglike(pdf, th)
    assert same(got, l)
    return got, kmc.psis_tail(pdf, th), kmc.loo(pdf, th)


def test_special_columns(kmc):
    """n = 40, M = 8.  Ties straddling the cut-off, a constant column, +inf entries; a NaN and a -inf minimum make their own observation
    NaN and leave the neighbours' bits alone."""
    rng = np.random.default_rng(11)
    n = 40
    clean = [rng.standard_normal(n) * 2.0 for _ in range(8)]
    ties = rng.permutation(np.concatenate([np.arange(6.0), np.full(5, 6.0), 10.0 + np.arange(n - 11)]))
    plus = clean[3].copy()
    plus[[2, 9, 30]] = np.inf
    with_nan, no_min = clean[4].copy(), clean[5].copy()
    with_nan[7] = np.nan
    no_min[13] = -np.inf
    cols = [clean[0], ties, np.full(n, -1.25), plus, with_nan, no_min, clean[6], clean[7]]
    l, t, w = injected(kmc, cols)
    check_exact(l, t)
    assert t["tail_len"] == 8 and t["n_tail_j"][1] == 6 and t["xc_j"][1] == -6.0                   # the five entries at the cut-off stay out
    assert t["n_tail_j"][2] == 0 and w["elpd_loo_j"][2] == -1.25 and w["pareto_k"][2] == np.inf    # constant: elpd_loo_j = m_j
    assert np.isfinite(w["elpd_loo_j"][3]) and t["n_tail_j"][3] == 8
    for j in (4, 5):
        assert all(np.isnan(w[k][j]) for k in ("elpd_loo_j", "p_loo_j", "pareto_k")) and w["n_tail_j"][j] == -1
    assert w["n_nan"] == 2 and np.isnan(w["elpd_loo"]) and sum(w["k_counts"]) == 6
    good = [0, 1, 2, 3, 6, 7]
    y = Y.loo(l[:, good])
    dist, same_dropped, _ = pc.yardstick_distance(l[:, good])                             # the yardstick's own error on this matrix
    assert same_dropped
    for key in ("pareto_k", "elpd_loo_j"):
        a, b = w[key][good], y[key]
        fin = np.isfinite(b)
        tol = max(8.0 * dist[key], (8 + 4) * 2.0 ** -53) * np.maximum(1.0, np.abs(b[fin]))
        assert (a[~fin] == b[~fin]).all() and np.all(np.abs(a[fin] - b[fin]) <= tol), (key, np.abs(a[fin] - b[fin]) / tol)
    cols[4], cols[5] = clean[4], clean[5]
    _, t2, w2 = injected(kmc, cols)
    for key in ("elpd_loo_j", "pareto_k", "n_tail_j", "lppd_j", "p_loo_j"):
        assert same(w[key][good], w2[key][good]), key
    assert same(t["tail"][good], t2["tail"][good]) and w2["n_nan"] == 0


def run_sampler(kmc, pdf, th, G, nburn):
    nw, nd = th.shape[-2:]
    s = kmc.Sampler(pdf, nw, nd, G, nburn, 1, 2.0, 5, store_chain=True, store_logp=True)
    s.set_positions(th)
    s.run(G)
    s.sync()
    return s


def normal_data(outlier):
    rng = np.random.default_rng(5)
    y = 0.5 + 0.5 * rng.standard_normal(200)
    if outlier:
        y[17] = 0.5 + 0.5 * 20.0
    return y[:, None]


NORM = 0.5 * math.log(4.0 / (2.0 * math.pi))
MEAN_TERM = "double r = d[0] - x[0]; return -0.5 * p[0] * r * r + p[1];"


def test_invariants(kmc):
    """A real Sampler over a DataDensity (100 walkers x 2, 200 observations, 60 stored samples)."""
    rng = np.random.default_rng(0)
    t = rng.uniform(-1.0, 1.0, 200)
    D = np.column_stack([t, 0.5 + 2.0 * t + 0.5 * rng.standard_normal(200)])
    pdf = kmc.DataDensity("double r = d[1] - (x[0] + x[1] * d[0]); return -0.5 * p[0] * r * r;", D, params=[4.0])
    th = np.array([0.5, 2.0]) + 0.1 * np.random.default_rng(3).standard_normal((100, 2))
    s = run_sampler(kmc, pdf, th, 70, 10)
    try:
        chain = s.chain()
        w, wh = s.loo(), kmc.loo(pdf, chain)
        assert w["n"] == 6000 and w["n_nan"] == 0 and w["elpd_loo_j"].shape == (200,)
        assert same_result(w, wh) and same_result(w, s.loo())
        ts, th_ = s.psis_tail(), kmc.psis_tail(pdf, chain)
        assert all(same(ts[k], th_[k]) for k in ("tail", "m_j", "xc_j", "n_tail_j"))
        check_exact(s.pointwise_loglike(), ts)
        # a selection: the bits of the call on the rows copied out
        mask = np.arange(100) % 3 == 0
        ws = s.loo(first_sample=7, thin=5, walkers=mask)
        rows = np.ascontiguousarray(chain[0][7::5][:, mask])                                # [11][34][2]
        wc = kmc.loo(pdf, rows.transpose(1, 0, 2))
        assert ws["n"] == wc["n"] == 11 * 34 and same_result(ws, wc)
        assert same_result(ws, kmc.loo(pdf, chain, first_sample=7, thin=5, walkers=mask))
        # a range of observations: the slice of the whole call, with totals over the range
        part = s.loo(obs=(17, 40))
        for key in ARRAYS:
            assert part[key].shape == (40,) and same(part[key], w[key][17:57]), key
        st = np.stack([w["elpd_loo_j"], w["pareto_k"], w["n_tail_j"].astype(np.float64), np.zeros(200)])[:, 17:57]
        only = kmc.loo_stats(st, w["lppd_j"][17:57], 6000)
        assert all(same(part[k], only[k]) for k in ("elpd_loo", "se", "p_loo", "looic", "lppd", "k_counts"))
        # several blocks of observations: 64 at a time
        small = s.loo(workspace=1, with_info=True)
        assert small["info"]["blocks"] == 4 and small["info"]["obs_per_block"] == 64 and s.loo(with_info=True)["info"]["blocks"] == 1
        assert same_result(w, small)
        assert all(same(s.psis_tail(workspace=1)[k], ts[k]) for k in ("tail", "m_j", "xc_j", "n_tail_j"))
        assert "elpd_loo" not in s.summary()
    finally:
        s.close()


def test_loo_of_a_normal_mean_means_something(kmc):
    """200 observations y ~ N(mu, 1/4), precision known, flat prior: the leave-one-out predictive density of y_j is normal about the
    mean of the others with variance (1/4) 200/199, so elpd_loo is closed form: -138.6223.  Independent draws from the exact posterior
    through tests/psis_yardstick.py give elpd_loo -138.6774 .. -138.5601 over ten seeds at 640 draws (-138.6427 .. -138.5768 at 6 400)
    and pareto_k at most 0.30, computed on the CPU; the sampled chain, with more than 640 effective draws, must land inside the 640-draw
    range widened by half its width each side.  With observation 17 moved 20 standard deviations out, its pareto_k is the largest
    (numpy route: observation 17 in ten of ten seeds, k 0.21 .. 0.74)."""
    rng = np.random.default_rng(12)
    results = []
    for outlier in (False, True):
        y = normal_data(outlier)
        pdf = kmc.DataDensity(MEAN_TERM, y, params=[4.0, NORM])
        s = run_sampler(kmc, pdf, y.mean() + 0.05 * rng.standard_normal((64, 1)), 1200, 200)
        try:
            ess = s.convergence()["ess"]
            assert np.all(ess > 640), ess
            results.append((s.loo(), s.waic()))
        finally:
            s.close()
    (w, wa), (wo, _) = results
    y = normal_data(False)[:, 0]
    others = (y.sum() - y) / 199.0
    var = 0.25 * 200.0 / 199.0
    exact = float(np.sum(-0.5 * (y - others) ** 2 / var - 0.5 * np.log(2.0 * np.pi * var)))
    print(f"elpd_loo {w['elpd_loo']:.4f} (exact {exact:.4f}), se {w['se']:.3f}, p_loo {w['p_loo']:.4f}, largest k {w['pareto_k'].max():.3f}, "
          f"elpd_waic {wa['elpd_waic']:.4f}; with the outlier: k_17 {wo['pareto_k'][17]:.3f}, k_counts {wo['k_counts']}")
    assert w["n"] == 64 * 1000 and w["n_nan"] == 0 and w["tail_len"] == 759
    assert -138.6774 - 0.0587 <= w["elpd_loo"] <= -138.5601 + 0.0587
    assert abs(w["elpd_loo"] - exact) <= 0.1173
    assert np.all(w["pareto_k"] < 0.5) and w["k_counts"] == (200, 0, 0, 0)
    assert abs(w["elpd_loo"] - wa["elpd_waic"]) < min(w["se"], wa["se"])
    assert int(np.argmax(wo["pareto_k"])) == 17
    k = wo["pareto_k"]
    assert wo["k_counts"] == (int((k <= 0.5).sum()), int(((k > 0.5) & (k <= 0.7)).sum()), int(((k > 0.7) & (k <= 1.0)).sum()), int((k > 1.0).sum()))
    d = kmc.compare_loo(w, w)
    assert d["elpd_diff"] == 0.0 and d["J"] == 200


def test_refusals(kmc):
    from kissmcmc_jl_amd import _lib
    th, _, _ = pc.case(31, 24)
    pdf = density(31, 24)
    with pytest.raises(kmc.KmcError, match="data density"):
        kmc.loo(kmc.CDensity("return -0.5 * x[0] * x[0];"), th)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(kmc.KmcError, match="r_eff") as e:
            kmc.loo(pdf, th, r_eff=bad)
        assert e.value.status == _lib.ERR_BAD_ARG
    with pytest.raises(ValueError, match="per-observation"):
        kmc.loo(pdf, th, r_eff=np.ones(31))
    with pytest.raises(kmc.KmcError, match=r"n = 4\)"):
        kmc.loo(pdf, th[:, :1])
    with pytest.raises(kmc.KmcError, match=r"M = 6000 .*n / r_eff = 4000000") as e:
        kmc.loo(pdf, np.zeros((4, 10000, 2)), r_eff=0.01)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(kmc.KmcError, match="outside"):
        kmc.loo(pdf, th, obs=(20, 12))
    with pytest.raises(TypeError):
        kmc.loo(pdf, th, data=np.zeros((3, 1)))
    with kmc.Sampler(kmc.GaussianIso(), 16, 2, 10, 0, 1, 2.0, 1, store_chain=True) as s:
        s.set_positions(np.random.default_rng(1).standard_normal((16, 2)))
        s.run(10)
        with pytest.raises(kmc.KmcError, match="data density"):
            s.loo()
    with kmc.Sampler(pdf, 16, 2, 10, 0, 1, 2.0, 1) as s:                                  # a streamed chain: nothing stored
        s.set_positions(np.random.default_rng(1).standard_normal((16, 2)))
        s.run(10)
        with pytest.raises(kmc.KmcError, match="KMC_STORE_CHAIN"):
            s.loo()
        with pytest.raises(kmc.KmcError, match="KMC_STORE_CHAIN"):
            s.psis_tail()
