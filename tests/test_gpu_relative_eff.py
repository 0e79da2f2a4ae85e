"""GPU: PSIS-LOO's relative efficiency per observation, computed from the chain (kmc.relative_eff, kmc.pointwise_weights,
kmc.loo / kmc.psis_tail with r_eff="chain" or the array r_eff_j=, and the Sampler's methods), against the definition in include/kissmcmc_hip.h.

* The weight series v = exp(l - M_j): M_j exact, 1.0 at the arg-max rows, IEEE's special values, elsewhere within DEVICE_EXP_ULP of
  exp in longdouble.
* The defining identity, bit for bit: relative_eff's ess, lag and truncated are kmc.convergence's on the device's own v of each
  aligned group of 64 observations.
* Against numpy: the same three against tests/convergence_yardstick.py on the device's v, with the tolerance formula of
  tests/test_gpu_convergence.py::check_end_to_end, restated here.
* Independence (a range, a small work space), composition (the computed r_eff_j given back; an array of equal entries against the
  number) and the sampler's route against the host's: bit for bit.
* A tail length per observation against tests/psis_yardstick.py: the exact parts bit for bit, the values within
  max(8 DIST, (M_j + 4) 2^-53), DIST the yardstick's own float64-to-longdouble distance (tests/relative_eff_cases.py prints it).
"""
import functools

import numpy as np
import pytest

import convergence_yardstick as cy
import psis_cases as pc
import psis_yardstick as Y
import relative_eff_cases as rc

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
# HIP's math API documents the double-precision exp of the device library at a maximum error of 1 ULP (ROCm documentation, "HIP math
# API", double-precision floating-point functions).  The reference below is exp in longdouble rounded to double: half an ulp more.
DEVICE_EXP_ULP = 1.0
# The pair sums of the truncation rule and 3 sqrt(n / r_eff_j) on the yardstick: measured 6.6e-5 and 9.3e-4 at the least on these inputs
# (python tests/relative_eff_cases.py).  The device's ess differs from the yardstick's by ESS_TOL (below), under 1e-10 relative here,
# which moves a pair sum by as much and 3 sqrt(n / r) <= 400 by under 400 * 1e-10 / 2: nothing within these bounds can flip.
MARGIN_MIN = 1e-9
INTEGER_MIN = 1e-6
# python tests/relative_eff_cases.py   (float64 yardstick against its longdouble mode with a tail length per observation; no device)
DIST = {
    ("spread", 65): dict(pareto_k=1.13e-15, elpd_loo_j=2.79e-16),    # same weights dropped: True
    ("spread", 130): dict(pareto_k=1.57e-15, elpd_loo_j=3.39e-16),    # same weights dropped: True
    ("chain", "C"): dict(pareto_k=5.34e-15, elpd_loo_j=7.32e-16),    # same weights dropped: True
}
LOO_ARRAYS = ("elpd_loo_j", "p_loo_j", "pareto_k", "n_tail_j", "lppd_j", "r_eff_j", "tail_len_j")
LOO_SCALARS = ("elpd_loo", "se", "p_loo", "looic", "lppd", "n", "tail_len", "n_nan", "n_reff_nan", "k_counts")
B_MASK = np.array([True, False, True])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def same_result(a, b, keys=LOO_ARRAYS + LOO_SCALARS):
    return all(same(a[k], b[k]) for k in keys)


@functools.lru_cache(maxsize=None)
def density(name):
    import kissmcmc_jl_amd as kmc
    return kmc.DataDensity(pc.TERM, rc.case(name)[1])


@functools.lru_cache(maxsize=None)
def device(name, masked=False):
    """One input's series, relative efficiency and the yardstick on the device's own series; computed once."""
    import kissmcmc_jl_amd as kmc
    th = rc.case(name)[0]
    sel = dict(walkers=B_MASK, thin=2) if masked else {}
    v, M = kmc.pointwise_weights(density(name), th, **sel)
    re = kmc.relative_eff(density(name), th, **sel)
    nsel = int(B_MASK.sum()) if masked else th.shape[0]
    want, raw = cy.convergence(v.reshape(v.shape[0] // nsel, nsel, v.shape[1]))
    return v, M, re, want, raw, nsel


@functools.lru_cache(maxsize=None)
def chain_loo(name):
    import kissmcmc_jl_amd as kmc
    return kmc.loo(density(name), rc.case(name)[0], r_eff="chain", with_info=True)


CASES = [("A", False), ("B", False), ("C", False), ("B", True)]


@pytest.mark.parametrize("name,masked", CASES)
def test_weights(kmc, name, masked):
    th, _, l_all = rc.case(name)
    v, M, _, _, _, nsel = device(name, masked)
    l = kmc.pointwise_loglike(density(name), th, **(dict(walkers=B_MASK, thin=2) if masked else {}))
    if not masked:
        assert (bits(l) == bits(l_all)).all()                                      # the device's terms are numpy's
    else:
        nw, ns = th.shape[:2]
        assert (bits(l) == bits(l_all.reshape(ns, nw, -1)[::2][:, B_MASK].reshape(-1, l_all.shape[1]))).all()
    assert v.shape == l.shape and (bits(M) == bits(l.max(axis=0))).all()
    top = l == M
    assert (v[top] == 1.0).all() and top.any(axis=0).all()
    ref = np.exp((l - M).astype(np.longdouble))
    err = np.abs(v.astype(np.longdouble) - ref) / np.spacing(ref.astype(np.float64))
    print(f"{name}: exp error at most {float(err.max()):.3f} ulp")
    assert float(err.max()) <= DEVICE_EXP_ULP + 0.5


def special_columns():
    """n = 160 rows (4 walkers x 40), 31 columns: one partial group.  Clean columns, entries of -inf, a NaN, a column of -inf, a constant."""
    rng = np.random.default_rng(23)
    n = 160
    cols = [rng.standard_normal(n) * 1.5 for _ in range(31)]
    cols[3] = cols[3].copy(); cols[3][[5, 77, 159]] = -np.inf
    cols[9] = cols[9].copy(); cols[9][40] = np.nan
    cols[17] = np.full(n, -np.inf)
    cols[30] = np.full(n, -2.5)
    l = np.column_stack(cols)
    th = l.reshape(n // 4, 4, 31).transpose(1, 0, 2)                                # [walker][sample][dim]: row = sample * 4 + walker
    return l, th


def test_special_values_and_fallback(kmc):
    """Input D.  The IEEE rules of the series; a constant column has no r_eff, counts in n_reff_nan and gets the tail length of r = 1."""
    l, th = special_columns()
    pdf = kmc.DataDensity(pc.INJECT_TERM, np.arange(31, dtype=np.float64)[:, None])
    assert same(kmc.pointwise_loglike(pdf, th), l)
    v, M = kmc.pointwise_weights(pdf, th)
    assert same(M, np.array([np.nan if np.isnan(c).any() else c.max() for c in l.T]))
    assert (v[[5, 77, 159], 3] == 0.0).all() and np.isfinite(v[:, 3]).all()
    assert np.isnan(v[:, 9]).all() and np.isnan(v[:, 17]).all() and (v[:, 30] == 1.0).all()
    clean = [j for j in range(31) if j not in (9, 17)]
    assert np.isfinite(v[:, clean]).all()
    re = kmc.relative_eff(pdf, th)
    assert np.isnan(re["r_eff_j"][[9, 17, 30]]).all() and np.isfinite(np.delete(re["r_eff_j"], [9, 17, 30])).all()
    assert (re["m"], re["h"], re["n"]) == (8, 20, 160)
    w = kmc.loo(pdf, th, r_eff="chain")
    assert w["n_reff_nan"] == 3 and same(w["r_eff_j"], re["r_eff_j"])
    assert (w["tail_len_j"][[9, 17, 30]] == Y.tail_length(160, 1.0)).all()
    assert (w["tail_len_j"] == rc.tail_lengths(160, re["r_eff_j"])).all() and w["tail_len"] == w["tail_len_j"].max()
    assert w["n_nan"] == 3 and w["elpd_loo_j"][30] == -2.5                       # (3, 17: no finite minimum; 9: a NaN)
    # the neighbours of the special columns keep the bits they have without them
    sub = [0, 1, 2, 4, 5]
    pdf2 = kmc.DataDensity(pc.INJECT_TERM, np.array(sub, dtype=np.float64)[:, None])
    assert same(kmc.relative_eff(pdf2, th)["r_eff_j"], re["r_eff_j"][sub])


@pytest.mark.parametrize("name,masked", CASES)
def test_defining_identity_bit_for_bit(kmc, name, masked):
    """relative_eff is kmc.convergence on the device's own series, group of 64 observations by group, padded to 64 columns."""
    v, _, re, _, _, nsel = device(name, masked)
    n, J = v.shape
    for g in range((J + 63) // 64):
        live = min(64, J - 64 * g)
        block = np.zeros((n, 64))
        block[:, :live] = v[:, 64 * g:64 * g + live]
        c = kmc.convergence(np.ascontiguousarray(block.reshape(n // nsel, nsel, 64).transpose(1, 0, 2)))
        assert (c["m"], c["h"]) == (re["m"], re["h"])
        sl = slice(64 * g, 64 * g + live)
        assert same(c["ess"][:live], re["ess_j"][sl]) and (c["lag"][:live] == re["lag"][sl]).all(), (name, g)
        assert (c["truncated"][:live] == re["truncated"][sl]).all(), (name, g)
    assert same(re["r_eff_j"], re["ess_j"] / (re["m"] * re["h"])) and re["n"] == n


@pytest.mark.parametrize("name,masked", CASES)
def test_against_numpy(kmc, name, masked):
    """ess, lag and truncated against the yardstick on the device's series; the tolerance of test_gpu_convergence.check_end_to_end."""
    v, _, re, want, raw, nsel = device(name, masked)
    m, h = raw["m"], raw["h"]
    n = v.shape[0]
    assert (re["m"], re["h"]) == (m, h) and h == (n // nsel) // 2
    assert rc.smallest_margin(want, raw) > MARGIN_MIN                              # the truncation condition, on the yardstick
    r_want = want["ess"] / (m * h)
    assert rc.integer_distance(n, r_want) > INTEGER_MIN
    T = want["T"]
    np.testing.assert_array_equal(re["lag"], T)
    np.testing.assert_array_equal(re["truncated"], (want["flags"] & cy.TRUNCATED) != 0)
    rel = 4 * (h + m + 8) * U
    den = m * h / want["ess"]
    ESS_TOL = 4 * T * (m * h + 4) * U / den + rel
    err = np.abs(re["ess_j"] - want["ess"]) / want["ess"]
    print(f"{name} masked={masked} m={m} h={h}: T {T.min()}..{T.max()}, truncated {int(re['truncated'].sum())}, ess err/tol {np.max(err / ESS_TOL):.3f}, "
          f"r_eff {re['r_eff_j'].min():.3f}..{re['r_eff_j'].max():.3f}")
    assert np.all(err <= ESS_TOL) and float(ESS_TOL.max()) < 1e-10
    if name == "A":
        assert (n // nsel) % 2 == 1 and re["truncated"].any() and not re["truncated"].all()
    if name == "B":
        assert T.max() + 2 > 32 or masked                                          # more than one lag block
    if name == "C":
        M = rc.tail_lengths(n, re["r_eff_j"])
        assert np.unique(M).size > 40 and M.min() > Y.tail_length(n) and (M == rc.tail_lengths(n, r_want)).all()


def test_independence(kmc):
    """Input B: a range of observations and a work space of one group and 64 observations at a time return the bits of the whole call."""
    th = rc.case("B")[0]
    pdf = density("B")
    w = chain_loo("B")
    assert w["info"]["groups"] == 3 and w["info"]["blocks"] == 1
    part = kmc.loo(pdf, th, r_eff="chain", obs=(37, 70))
    for key in LOO_ARRAYS:
        assert part[key].shape == (70,) and same(part[key], w[key][37:107]), key
    small = kmc.loo(pdf, th, r_eff="chain", workspace=1, with_info=True)
    assert small["info"]["blocks"] == 3 and small["info"]["obs_per_block"] == 64
    assert same_result(w, small)
    assert same_result(w, kmc.loo(pdf, th, r_eff="chain"))
    re = device("B")[2]
    assert same(w["r_eff_j"], re["r_eff_j"])
    assert same(kmc.relative_eff(pdf, th, obs=(37, 70), workspace=1)["r_eff_j"], re["r_eff_j"][37:107])
    tp, tw = kmc.psis_tail(pdf, th, r_eff="chain", obs=(37, 70)), kmc.psis_tail(pdf, th, r_eff="chain")
    assert all(same(tp[k], tw[k][37:107]) for k in ("m_j", "xc_j", "n_tail_j", "r_eff_j", "tail_len_j"))
    # a selection: the bits of the call on the rows copied out
    ws = kmc.loo(pdf, th, r_eff="chain", walkers=B_MASK, thin=2)
    wc = kmc.loo(pdf, np.ascontiguousarray(th[B_MASK][:, ::2]), r_eff="chain")
    assert ws["n"] == 150 and same_result(ws, wc) and same(ws["r_eff_j"], device("B", True)[2]["r_eff_j"])


def test_sampler_route_equals_host_route(kmc):
    rng = np.random.default_rng(4)
    D = rng.standard_normal((70, 1))
    pdf = kmc.DataDensity(pc.TERM, D)
    th0 = np.array([0.0, 1.0]) + 0.1 * rng.standard_normal((16, 2))
    with kmc.Sampler(pdf, 16, 2, 60, 10, 1, 2.0, 5, store_chain=True, store_logp=True) as s:
        s.set_positions(th0)
        s.run(60)
        s.sync()
        chain = s.chain()
        w, wh = s.loo(r_eff="chain"), kmc.loo(pdf, chain, r_eff="chain")
        assert w["n"] == 800 and same_result(w, wh)
        rs, rh = s.relative_eff(), kmc.relative_eff(pdf, chain)
        assert all(same(rs[k], rh[k]) for k in ("r_eff_j", "ess_j", "lag", "truncated")) and same(w["r_eff_j"], rs["r_eff_j"])
        vs, vh = s.pointwise_weights(), kmc.pointwise_weights(pdf, chain)
        assert same(vs[0], vh[0]) and same(vs[1], vh[1])
        ts, tt = s.psis_tail(r_eff="chain"), kmc.psis_tail(pdf, chain, r_eff="chain")
        assert all(same(ts[k], tt[k]) for k in ("tail", "m_j", "xc_j", "n_tail_j", "tail_len_j"))
        mask = np.arange(16) % 3 != 0
        assert same_result(s.loo(r_eff="chain", first_sample=3, thin=2, walkers=mask), kmc.loo(pdf, chain, r_eff="chain", first_sample=3, thin=2, walkers=mask))


def test_composition(kmc):
    th = rc.case("B")[0]
    pdf = density("B")
    w = chain_loo("B")
    r = w["r_eff_j"]
    ok = np.isfinite(r) & (r > 0)
    keys = tuple(k for k in LOO_ARRAYS + LOO_SCALARS if k not in ("r_eff_j", "n_reff_nan"))
    assert same_result(w, kmc.loo(pdf, th, r_eff_j=np.where(ok, r, 1.0)), keys)
    for c in (1.0, 0.37):
        a, b = kmc.loo(pdf, th, r_eff_j=np.full(130, c)), kmc.loo(pdf, th, r_eff=c)
        assert same_result(a, b) and (a["tail_len_j"] == Y.tail_length(450, c)).all() and a["n_reff_nan"] == 0
        ta, tb = kmc.psis_tail(pdf, th, r_eff_j=np.full(130, c)), kmc.psis_tail(pdf, th, r_eff=c)
        assert all(same(ta[k], tb[k]) for k in ("tail", "m_j", "xc_j", "n_tail_j", "tail_len"))


def check_per_observation(kmc, pdf, th, l, how, r_j, dist):
    """psis_tail and loo with a tail length per observation against tests/psis_yardstick.py, column by column."""
    n, J = l.shape
    Mj = rc.tail_lengths(n, r_j)
    t, w = kmc.psis_tail(pdf, th, **how), kmc.loo(pdf, th, **how)
    assert (t["tail_len_j"] == Mj).all() and (w["tail_len_j"] == Mj).all() and t["tail_len"] == w["tail_len"] == Mj.max()
    assert t["tail"].shape == (J, Mj.max())
    d64, d80 = [], []
    y = rc.loo_per_observation(l, Mj, dropped=d64)
    rc.loo_per_observation(l, Mj, True, dropped=d80)
    assert len(d64) == len(d80) and all((p == q).all() for p, q in zip(d64, d80))
    worst = dict(pareto_k=0.0, elpd_loo_j=0.0)
    for j in range(J):
        m, xc, x, mask = Y.shift_and_tail(l[:, j], int(Mj[j]))
        tail = np.sort(x[mask])
        assert t["n_tail_j"][j] == w["n_tail_j"][j] == tail.size <= Mj[j], j
        assert same(t["m_j"][j], m) and same(t["xc_j"][j], xc), j
        assert same(t["tail"][j, :tail.size], tail) and np.isnan(t["tail"][j, tail.size:]).all(), j
        for key in ("pareto_k", "elpd_loo_j"):
            want = float(y[key][j])
            tol = max(8.0 * dist[key], (Mj[j] + 4) * U) * max(1.0, abs(want))
            worst[key] = max(worst[key], abs(w[key][j] - want) / tol)
    print(f"n {n} J {J}: tail lengths {Mj.min()}..{Mj.max()}, largest error / tolerance " + ", ".join(f"{k} {e:.3f}" for k, e in worst.items()))
    assert all(e <= 1.0 for e in worst.values()), worst
    tot = Y.totals(w["elpd_loo_j"], w["lppd_j"], w["pareto_k"])
    assert all(same(w[k], tot[k]) for k in ("elpd_loo", "se", "p_loo", "looic", "lppd", "k_counts", "n_nan", "p_loo_j"))
    return w


@pytest.mark.parametrize("J", rc.SPREAD_JS)
def test_supplied_tail_lengths_against_the_yardstick(kmc, J):
    th, D, l = pc.case(J, 457)
    pdf = kmc.DataDensity(pc.TERM, D)
    r = rc.spread(J)
    assert np.unique(rc.tail_lengths(457, r)).size > 10
    w = check_per_observation(kmc, pdf, th, l, dict(r_eff_j=r), r, DIST[("spread", J)])
    assert same(w["r_eff_j"], r) and w["n_reff_nan"] == 0


def test_computed_tail_lengths_against_the_yardstick(kmc):
    th, _, l = rc.case("C")
    re = device("C")[2]
    check_per_observation(kmc, density("C"), th, l, dict(r_eff="chain"), re["r_eff_j"], DIST[("chain", "C")])


def test_refusals(kmc):
    from kissmcmc_jl_amd import _lib
    th = rc.case("A")[0]
    pdf = density("A")
    # by the yardstick r_eff_j is 0.0024 .. 0.0029 here (python tests/relative_eff_cases.py): 3 sqrt(n / r) > 8800, 0.2 n = 5000
    big, D, _ = rc.over_case()
    with pytest.raises(kmc.KmcError, match=r"observation \d+: a tail of M = 5000 .*r_eff_j = 0\.00.*thin the chain") as e:
        kmc.loo(kmc.DataDensity(pc.TERM, D), big, r_eff="chain")
    assert e.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(kmc.KmcError, match=r"r_eff_j\[7\] = nan") as e:
        kmc.loo(pdf, th, r_eff_j=np.where(np.arange(65) == 7, np.nan, 1.0))
    assert e.value.status == _lib.ERR_BAD_ARG
    with pytest.raises(ValueError, match="one entry per observation"):
        kmc.loo(pdf, th, r_eff_j=np.ones(64))
    with pytest.raises(ValueError, match="chain"):
        kmc.loo(pdf, th, r_eff="arviz")
    with pytest.raises(kmc.KmcError, match="at least 4 samples"):
        kmc.loo(pdf, th[:, :7], r_eff="chain")
    with pytest.raises(kmc.KmcError, match=r"max_lag must lie in \[3, h - 1\]"):
        kmc.relative_eff(pdf, th, max_lag=12)
    with pytest.raises(kmc.KmcError, match="at least 2 chains"):
        kmc.relative_eff(pdf, th, walkers=np.arange(4) == 0, split=False)
    with kmc.Sampler(kmc.GaussianIso(), 16, 2, 10, 0, 1, 2.0, 1, store_chain=True) as s:
        s.set_positions(np.random.default_rng(1).standard_normal((16, 2)))
        s.run(10)
        with pytest.raises(kmc.KmcError, match="data density"):
            s.relative_eff()
        with pytest.raises(kmc.KmcError, match="data density"):
            s.pointwise_weights()
