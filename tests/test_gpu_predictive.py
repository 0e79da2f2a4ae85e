"""GPU: the pointwise log-likelihoods of a DataDensity over a stored chain and WAIC (kmc.waic, kmc.pointwise_loglike, Sampler.waic,
Sampler.pointwise_loglike) against tests/predictive_yardstick.py.

What is asserted, and why the bounds are what they are (u = 2^-53, n rows, all per observation j):

* The matrix l[r][j] of an arithmetic-only term equals numpy bit for bit (the term is compiled with contraction off).
* M_j is exact.
* S1_j: the device adds the n terms run by run and then the runs, a chain of at most n + 1 additions on any path, so
  |S1 - fsum| <= (n + 1) u sum|l| to first order; asserted with the contract's (n + 4) u sum|l|.  S1 is also restated in the plan's
  order and compared bit for bit.
* V_j about the device's own centre c = S1 / n: a term fl(fl(l - c)^2) is within 3 u of the exact (l - c)^2 (one subtraction, squared,
  one product), the summation adds (n + 1) u: |V - V_exact| <= (n + 4) u V_exact, V_exact carried error-free by the yardstick.
* E_j: the arguments l - M have the same bits on both sides; the device's exp and math.exp are each taken to be within one ulp
  (2 u relative) of the true value, so a term differs by at most 4 u and |E - E_exact| <= (n + 1 + 4) u E; the issue's bound is
  (n + 8) u E and the assertion uses (n + 16) u E for slack.
* The host stage is restated bit for bit from the device's statistics (tests/test_predictive_cpu.py does the same on random ones).
  Against the exact statistics: lppd_j = M + (log E - log n) moves by at most dE / E <= (n + 16) u from E, plus the roundings of
  log, the subtraction and the addition on either side, each at most 2 u of |M| + |log E| + log n: bound
  (n + 16) u + 8 u (|M| + |log E| + log n).  p_waic_j = V / (n - 1) is within (n + 4) u + 2 u relative: (n + 6) u p_waic_j.  A total is
  the tree sum of J such numbers: the bounds add, plus (ceil(log2 J) + 1) u sum_j |x_j| for the tree on either side.
"""
import functools
import math

import numpy as np
import pytest

import predictive_yardstick as py

pytestmark = pytest.mark.gpu

U = py.U
JS = [1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 130, 1000]
P0 = 1.75


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def shape_of(n):
    """(walkers, samples) with walkers * samples == n, more than one walker where n allows."""
    for nw in (4, 3, 2):
        if n % nw == 0:
            return nw, n // nw
    return 1, n


@functools.lru_cache(maxsize=None)
def case(ndim, J, n):
    """Hand-built chain, data and the yardstick's matrix for one shape; computed once, never written to."""
    rng = np.random.default_rng(1000 * ndim + 7 * J + n)
    nw, ns = shape_of(n)
    th = rng.standard_normal((nw, ns, ndim)) * 0.3 + np.linspace(0.5, -0.5, ndim)
    D = np.column_stack([rng.standard_normal((J, ndim - 1)), rng.standard_normal(J) * 0.7])
    l = py.reg_matrix(py.rows_of(th), D, P0)
    for a in (th, D, l):
        a.setflags(write=False)
    return th, D, l


def row_counts(kmc, J):
    """n at the plan's run length - 1, at it, + 1 and at two runs + 1."""
    L = kmc.pointwise_plan(16, J)["run_len"]
    ns = [L - 1, L, L + 1, 2 * L + 1]
    for n in ns:
        assert kmc.pointwise_plan(n, J)["run_len"] == L
    return ns


@functools.lru_cache(maxsize=None)
def density(ndim, J, n):
    import kissmcmc_jl_amd as kmc
    return kmc.DataDensity(py.REG_TERM, case(ndim, J, n)[1], params=[P0])


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("J", JS)
def test_matrix_equals_numpy_bit_for_bit(kmc, ndim, J):
    for n in row_counts(kmc, J):
        th, D, l = case(ndim, J, n)
        pdf = density(ndim, J, n)
        assert (bits(kmc.pointwise_loglike(pdf, th)) == bits(l)).all(), n
        k = min(J, 3)
        assert (bits(kmc.pointwise_loglike(pdf, th, obs=(0, k))) == bits(l[:, :k])).all()
        assert (bits(kmc.pointwise_loglike(pdf, th, obs=(J - k, J))) == bits(l[:, J - k:])).all()
        assert (bits(kmc.pointwise_loglike(pdf, th, obs=(J - 1, J))) == bits(l[:, J - 1:])).all()


def check_statistics(kmc, pdf, th, l, J):
    n = l.shape[0]
    raw = kmc.pointwise_stats(pdf, th)
    st = raw["stats"]
    assert raw["n"] == n and st.shape == (4, J)
    plan = kmc.pointwise_plan(n, J)
    assert list(raw["info"][:4]) == [n, plan["nruns"], 2 * n * J, plan["run_len"]] and raw["info"][4] > 0 and raw["info"][5] > 0
    centre = st[1] / n
    ex = py.exact_stats(l, centre=centre)
    absum = np.array([math.fsum(np.abs(l[:, j]).tolist()) for j in range(J)])
    print(f"J {J} n {n}: S1 {np.max(np.abs(st[1] - ex[1]) / (U * absum)):.2f}  V {np.max(np.abs(st[3] - ex[3]) / (U * ex[3])):.2f}  "
          f"E {np.max(np.abs(st[2] - ex[2]) / (U * ex[2])):.2f}  (units of u x scale; bounds {n + 4}, {n + 4}, {n + 16})")
    assert (bits(st[0]) == bits(ex[0])).all()                                                   # M exact
    assert np.all(np.abs(st[1] - ex[1]) <= (n + 4) * U * absum)
    assert (bits(st[1]) == bits(py.planned_sums(l, n, J))).all()                                # ... and in the plan's order
    assert np.all(np.abs(st[3] - ex[3]) <= (n + 4) * U * ex[3])
    assert (bits(st[3]) == bits(py.planned_sums((l - centre) * (l - centre), n, J))).all()
    assert np.all(np.abs(st[2] - ex[2]) <= (n + 16) * U * ex[2])
    # the host stage: bit for bit from the device's statistics, and within the propagated bounds of the exact ones
    w = kmc.waic(pdf, th)
    hs = py.host_stage(st, n)
    for k in ("lppd", "p_waic", "elpd_waic", "se", "waic", "lppd_j", "p_waic_j", "elpd_j"):
        assert same(w[k], hs[k]), k
    assert w["n"] == n and w["n_nan"] == 0 and w["n_high"] == hs["n_high"]
    we = py.host_stage(ex, n)
    b_lppd = (n + 16) * U + 8 * U * (np.abs(ex[0]) + np.abs(np.log(ex[2])) + math.log(n))
    b_pw = (n + 6) * U * we["p_waic_j"]
    assert np.all(np.abs(w["lppd_j"] - we["lppd_j"]) <= b_lppd)
    assert np.all(np.abs(w["p_waic_j"] - we["p_waic_j"]) <= b_pw)
    tree = (math.ceil(math.log2(J)) + 1 if J > 1 else 0) * U
    assert abs(w["lppd"] - we["lppd"]) <= b_lppd.sum() + 2 * tree * np.abs(we["lppd_j"]).sum()
    assert abs(w["p_waic"] - we["p_waic"]) <= b_pw.sum() + 2 * tree * we["p_waic_j"].sum()
    assert abs(w["elpd_waic"] - we["elpd_waic"]) <= (b_lppd + b_pw).sum() + 2 * tree * np.abs(we["elpd_j"]).sum() + 2 * U * np.abs(we["elpd_j"]).sum()


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("J", JS)
def test_statistics_within_their_bounds(kmc, ndim, J):
    for n in row_counts(kmc, J):
        th, D, l = case(ndim, J, n)
        check_statistics(kmc, density(ndim, J, n), th, l, J)


@pytest.mark.parametrize("J,n", [(1000, 4200), (5, 70000), (64, 66000)])
def test_statistics_with_longer_runs(kmc, J, n):
    """Run lengths above the minimum: many runs of 17 rows over 16 groups of observations, the packed form with thousands of run
    slots, and one group of 64 with the full number of runs."""
    assert kmc.pointwise_plan(n, J)["run_len"] > 16 and kmc.pointwise_plan(n, J)["nruns"] > 200
    th, D, l = case(2, J, n)
    check_statistics(kmc, density(2, J, n), th, l, J)
    k = min(J, 2)
    assert (bits(kmc.pointwise_loglike(density(2, J, n), th, obs=(J - k, J))) == bits(l[:, J - k:])).all()


@pytest.mark.parametrize("J", [5, 33, 130])
def test_selection_equals_the_sliced_chain(kmc, J):
    """first_sample, thin and a walker mask give the bits of the same call on the rows copied out: the cut follows from (n, J) alone.
    A NaN in a row outside the selection changes nothing."""
    rng = np.random.default_rng(J)
    nw, ns, first = 6, 51, 3
    th = rng.standard_normal((nw, ns, 2)) * 0.3
    D = rng.standard_normal((J, 2))
    pdf = kmc.DataDensity(py.REG_TERM, D, params=[P0])
    mask = np.array([1, 0, 1, 1, 0, 1], dtype=bool)
    for thin in (1, 2, 7):
        sliced = np.ascontiguousarray(th[mask][:, first::thin])
        want = kmc.pointwise_stats(pdf, sliced)
        got = kmc.pointwise_stats(pdf, th, first_sample=first, thin=thin, walkers=mask)
        assert got["n"] == want["n"] == sliced.shape[0] * sliced.shape[1]
        assert (bits(got["stats"]) == bits(want["stats"])).all() and (got["info"][:4] == want["info"][:4]).all(), thin
        assert (bits(kmc.pointwise_stats(pdf, th, first_sample=first, thin=thin, walkers=np.flatnonzero(mask))["stats"]) == bits(want["stats"])).all()
        ll = kmc.pointwise_loglike(pdf, th, first_sample=first, thin=thin, walkers=mask)
        assert (bits(ll) == bits(py.reg_matrix(py.rows_of(th, first, thin, mask), D, P0))).all()
        dirty = th.copy()
        keep = np.zeros((nw, ns), dtype=bool)
        keep[np.ix_(mask, np.arange(first, ns, thin))] = True
        dirty[~keep] = np.nan
        assert (bits(kmc.pointwise_stats(pdf, dirty, first_sample=first, thin=thin, walkers=mask)["stats"]) == bits(want["stats"])).all()
        assert same(kmc.pointwise_loglike(pdf, dirty, first_sample=first, thin=thin, walkers=mask), ll)
        wa, wb = kmc.waic(pdf, th, first_sample=first, thin=thin, walkers=mask), kmc.waic(pdf, sliced)
        assert same(wa["elpd_j"], wb["elpd_j"]) and same(wa["se"], wb["se"]) and wa["n"] == wb["n"]


def test_special_values(kmc):
    """CUT_TERM is -inf where x[0] < d[0].  Observation 1 forbids every row (all -inf: lppd_j = -inf), observation 3 some rows (a -inf
    among finite terms: lppd_j finite, p_waic_j not), observation 5 carries a NaN (every term NaN: every output NaN, n_nan = 1); the
    other observations have the bits of the same call without observation 5."""
    rng = np.random.default_rng(4)
    th = np.stack([rng.uniform(0.0, 1.0, (4, 20)), rng.standard_normal((4, 20))], axis=2)
    D = np.column_stack([np.full(8, -1.0), rng.standard_normal(8)])
    D[1, 0], D[3, 0], D[5, 1] = 2.0, 0.5, np.nan
    pdf = kmc.DataDensity(py.CUT_TERM, D, params=[P0])
    l = py.cut_matrix(py.rows_of(th), D, P0)
    assert np.isinf(l[:, 1]).all() and 0 < np.isinf(l[:, 3]).sum() < 80 and np.isnan(l[:, 5]).all()
    assert same(kmc.pointwise_loglike(pdf, th), l)
    w = kmc.waic(pdf, th)
    st = kmc.pointwise_stats(pdf, th)["stats"]
    assert st[0, 1] == -np.inf and st[2, 1] == 0.0 and w["lppd_j"][1] == -np.inf
    assert np.isfinite(w["lppd_j"][3]) and not np.isfinite(w["p_waic_j"][3])
    assert st[0, 3] == l[:, 3].max() and st[1, 3] == -np.inf
    assert w["n_nan"] == 1 and all(np.isnan(w[k][5]) for k in ("lppd_j", "p_waic_j", "elpd_j")) and np.isnan(st[:, 5]).all()
    rest = [0, 1, 2, 3, 4, 6, 7]
    clean = kmc.waic(pdf, th, data=D[rest])
    assert clean["n_nan"] == 0
    for k in ("lppd_j", "p_waic_j", "elpd_j"):
        assert same(w[k][rest], clean[k]), k
    good = [0, 2, 4, 6, 7]
    ex = py.exact_stats(l[:, good], centre=st[1, good] / 80)
    assert (bits(st[0, good]) == bits(ex[0])).all() and np.all(np.abs(st[2, good] - ex[2]) <= (80 + 16) * U * ex[2])
    # a NaN in one ROW (not in an observation) reaches every observation that row has a finite term for
    th2 = th.copy()
    th2[2, 7] = [0.9, np.nan]
    w2 = kmc.waic(pdf, th2)
    assert w2["n_nan"] == 7 and w2["lppd_j"][1] == -np.inf


def run_sampler(kmc, pdf, th, G, nburn, **kw):
    nw, nd = th.shape[-2:]
    s = kmc.Sampler(pdf, nw, nd, G, nburn, 1, 2.0, 5, store_chain=True, store_logp=True, **kw)
    s.set_positions(th)
    s.run(G)
    s.sync()
    return s


def line_data():
    rng = np.random.default_rng(0)
    t = rng.uniform(-1.0, 1.0, 200)
    y = 0.5 + 2.0 * t + 0.5 * rng.standard_normal(200)
    return np.column_stack([t, y])


NORM = 0.5 * math.log(4.0 / (2.0 * math.pi))
LINE_TERM = "double r = d[1] - (x[0] + x[1] * d[0]); return -0.5 * p[0] * r * r + p[1];"
MEAN_TERM = "double r = d[1] - x[0]; return -0.5 * p[0] * r * r + p[1];"


@pytest.mark.parametrize("tempered", [False, True])
def test_sampler_route_equals_host_route(kmc, tempered):
    """A real Sampler over a DataDensity (100 walkers x 2, 200 observations, 60 stored samples): the read-outs on the chain where it lies
    equal those on the downloaded chain bit for bit, also for a likelihood-tempered sampler of three rungs (the chain is rung 0's),
    with a selection, and twice in a row; held-out observations give the entries of their own observations."""
    D = line_data()
    pdf = kmc.DataDensity(py.REG_TERM, D, params=[4.0])
    th = np.array([0.5, 2.0]) + 0.1 * np.random.default_rng(3).standard_normal((100, 2))
    kw = dict(betas=[1.0, 0.5, 0.25], temper="likelihood") if tempered else {}
    if tempered:
        th = np.stack([th, th, th])
    s = run_sampler(kmc, pdf, th, 70, 10, **kw)
    try:
        assert s.samples_done == 60
        chain = s.chain()
        assert chain[0].shape == (60, 100, 2)
        w, wh = s.waic(), kmc.waic(pdf, chain)
        for k in ("lppd", "p_waic", "elpd_waic", "se", "waic", "lppd_j", "p_waic_j", "elpd_j"):
            assert same(w[k], wh[k]), k
        assert w["n"] == wh["n"] == 6000 and w["n_nan"] == 0
        again = s.waic()
        assert all(same(w[k], again[k]) for k in ("elpd_waic", "se", "lppd_j", "p_waic_j", "elpd_j"))
        ll = s.pointwise_loglike(first_sample=50, thin=3, obs=(190, 200))
        assert ll.shape == (400, 10)
        assert (bits(ll) == bits(kmc.pointwise_loglike(pdf, chain, first_sample=50, thin=3, obs=(190, 200)))).all()
        assert (bits(ll) == bits(py.reg_matrix(chain[0][50::3].reshape(-1, 2), D[190:], 4.0))).all()
        assert (bits(s.pointwise_loglike(thin=20)) == bits(kmc.pointwise_loglike(pdf, chain, thin=20))).all()
        mask = np.arange(100) % 3 == 0
        ws, wm = s.waic(first_sample=7, thin=5, walkers=mask), kmc.waic(pdf, chain, first_sample=7, thin=5, walkers=mask)
        assert ws["n"] == 11 * 34 and same(ws["elpd_j"], wm["elpd_j"]) and same(ws["se"], wm["se"])
        # held-out observations
        part = s.waic(data=D[:50])
        assert part["lppd_j"].shape == (50,) and (bits(part["lppd_j"]) == bits(w["lppd_j"][:50])).all()
        assert (bits(part["p_waic_j"]) == bits(w["p_waic_j"][:50])).all()
        only = kmc.waic_stats(kmc.pointwise_stats(pdf, chain)["stats"][:, :50], 6000)
        assert all(same(part[k], only[k]) for k in ("lppd", "p_waic", "elpd_waic", "se", "waic"))
        assert (bits(s.pointwise_loglike(thin=20, data=D[40:50])) == bits(s.pointwise_loglike(thin=20, obs=(40, 50)))).all()
        summary = s.summary()
        assert "waic" not in summary and "elpd_waic" not in summary
    finally:
        s.close()


def test_refusals_on_the_device(kmc):
    """What only a sampler can refuse: a density without a per-observation term, a sampler without a stored chain."""
    from kissmcmc_jl_amd import _lib
    th = np.random.default_rng(1).standard_normal((16, 2))
    with kmc.Sampler(kmc.GaussianIso(), 16, 2, 10, 0, 1, 2.0, 1, store_chain=True) as s:
        s.set_positions(th)
        s.run(10)
        with pytest.raises(kmc.KmcError, match="data density") as e:
            s.waic()
        assert e.value.status == _lib.ERR_BAD_ARG
    pdf = kmc.DataDensity(py.REG_TERM, line_data(), params=[4.0])
    with kmc.Sampler(pdf, 16, 2, 10, 0, 1, 2.0, 1) as s:
        s.set_positions(th)
        s.run(10)
        with pytest.raises(kmc.KmcError, match="KMC_STORE_CHAIN"):
            s.waic()
        with pytest.raises(kmc.KmcError, match="KMC_STORE_CHAIN"):
            s.pointwise_loglike()


def test_waic_of_a_line_fit_means_something(kmc):
    """200 observations y = 0.5 + 2 t + 0.5 eps, precision p[0] = 4 known, flat prior, the term with its normalising constant.
    Independent draws from the exact posterior give p_waic 1.76 .. 2.03 and elpd_waic -151.46 .. -151.18 over ten seeds at 640 draws
    (1.88 .. 1.95 and -151.38 .. -151.31 at 6 400), computed on the CPU; the sampled chain, with more than 640 effective draws per
    parameter, must land inside the 640-draw ranges widened by half their width each side.  Against the intercept-only model the line
    wins by more than five standard errors (exact posterior: 547 +- 45)."""
    D = line_data()
    full = kmc.DataDensity(LINE_TERM, D, params=[4.0, NORM])
    flat = kmc.DataDensity(MEAN_TERM, D, params=[4.0, NORM])
    rng = np.random.default_rng(12)
    s = run_sampler(kmc, full, np.array([0.46, 1.94]) + 0.05 * rng.standard_normal((64, 2)), 1200, 200)
    try:
        ess = s.convergence()["ess"]
        assert np.all(ess > 640), ess
        w = s.waic()
        print(f"ess {ess}, p_waic {w['p_waic']:.4f}, elpd_waic {w['elpd_waic']:.4f}, se {w['se']:.3f}, n_high {w['n_high']}")
        assert w["n"] == 64 * 1000 and w["n_nan"] == 0 and w["n_high"] == 0
        assert 1.76 - 0.135 <= w["p_waic"] <= 2.03 + 0.135
        assert -151.46 - 0.14 <= w["elpd_waic"] <= -151.18 + 0.14
        assert w["waic"] == -2.0 * w["elpd_waic"] and w["lppd"] > w["elpd_waic"]
    finally:
        s.close()
    s = run_sampler(kmc, flat, 0.5 + 0.05 * rng.standard_normal((64, 1)), 1200, 200)
    try:
        w0 = s.waic()
    finally:
        s.close()
    d = kmc.compare_waic(w, w0)
    print(f"elpd difference {d['elpd_diff']:.1f} +- {d['se']:.1f}")
    assert d["elpd_diff"] > 5.0 * d["se"] > 0.0 and d["J"] == 200
