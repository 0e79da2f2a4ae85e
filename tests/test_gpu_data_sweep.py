"""GPU: the data-density kernels (kmc_data.hpp) and their planner (kmc_data.hip: data_plan) at every edge of the tree, bit for bit
against the numpy restatement of the value contract.  The matrix, the restated planner and the reference are tests/data_sweep.py
(checked without a device by tests/test_data_sweep_cpu.py; `python tests/data_sweep.py` prints the table).

  1. the sweep: one stateless evaluation (DataDensity._eval_rows: kmc_logpdf_eval_host) per case and mapping; the regime each case
     claims is asserted from the restated planner, and the restated planner from Sampler.describe()
  2. samplers whose half-step and whole-ensemble plans fall on different sides of the 512-proposal mapping boundary
  3. the largest (ndim 32, ncols 16) and the smallest (1, 1) kernels
  4. non-finite terms and priors, by the contract
  5. kmc_logpdf_eval itself, on the caller's device memory and stream

Measured on an MI355X: the two cases at 4096 rounds per wave take 3 ms (1025 x 524 289, observation per lane) and 6 ms (65 600 x
131 073, proposal per lane) per evaluation, copies included, and under 0.1 s per test with the numpy reference; the module 6 s.

Five runtime-compiled kernel sets in all (term, prior, ncols, ndim): REG_TERM 2/2 (1, 2, 5), REG_TERM + GAUSS_PRIOR 3/3 (2), BIG_TERM
16/32 (3), ONE_TERM 1/1 (3), FLAG_TERM + FLAG_PRIOR 3/2 (4)."""
import ctypes as C
import time

import numpy as np
import pytest

import data_sweep as ds
import data_tempering_yardstick as dy
from test_data_density_cpu import REG_TERM
from test_gpu_data_density import assert_same, host_yardstick, run
from test_gpu_data_tempering import GAUSS_PRIOR, assert_matches, gauss_prior
from test_gpu_data_tempering import run as run_tempered

pytestmark = pytest.mark.gpu


def set_mapping(kmc_debug, mapping):
    if mapping is None:
        kmc_debug.unset("data-map")
    else:
        kmc_debug.set("data-map", mapping)


def eval_in_both_mappings(kmc_debug, dd, X):
    out = {}
    for m in ("lane", "obs"):
        set_mapping(kmc_debug, m)
        out[m] = dd._eval_rows(X)
    set_mapping(kmc_debug, None)
    return out


# ---- 1. the sweep ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ds.CASES, ids=ds.case_id)
def test_sweep_is_bit_identical_to_the_reference(kmc, kmc_debug, c):
    p, last = ds.plan(*c), ds.last_block(*c)
    assert p.mapping == (c.force or ("obs" if c.nprop < 512 else "lane"))
    assert 1 <= p.rounds <= 4096 and 1 <= p.nblocks <= 2048 and (p.nblocks == 1 or p.groups * p.nblocks <= 2048 or p.rounds == 4096)
    D, X = ds.inputs(c)
    rows = ds.check_rows(c.nprop, c.ndata)
    want = ds.reg_reference(X[rows], D)
    dd = kmc.DataDensity(REG_TERM, D, params=[ds.P0])
    set_mapping(kmc_debug, c.force)
    if 2 * c.nprop >= ds.ND + 2:                       # a legal half-ensemble: the library's own plan for these proposals
        with kmc.Sampler(dd, 2 * c.nprop, ds.ND, 2) as s:
            desc = s.describe()
        for words in ds.describe_words(*c):
            assert words in desc, (words, desc)
        assert "%d observations of %d doubles" % (c.ndata, ds.ND) in desc
    t0 = time.perf_counter()
    got = dd._eval_rows(X)
    t1 = time.perf_counter()
    set_mapping(kmc_debug, ds.other_mapping(c))
    other = dd._eval_rows(X)
    set_mapping(kmc_debug, None)
    print("%s: %s, %d rounds, %d blocks, last block %s; evaluation %.2f ms (copies included), %d of %d rows differ from the reference, %d from the other mapping"
          % (ds.case_id(c), p.mapping, p.rounds, p.nblocks, tuple(last), 1e3 * (t1 - t0), int(np.sum(got[rows] != want)), rows.size, int(np.sum(got != other))))
    np.testing.assert_array_equal(got[rows], want)
    np.testing.assert_array_equal(other, got)


# ---- 2. plans either side of the mapping boundary -------------------------------------------------------------------------
@pytest.mark.parametrize("nw,half", [(600, "obs"), (1022, "obs"), (1024, "lane")])
def test_half_step_and_whole_ensemble_plans_either_side_of_512(kmc, nw, half):
    """set_positions evaluates nwalkers rows (proposal per lane from 512), a half-step nwalkers / 2 (observation per lane below 512): the
    accept test subtracts the one kernel's value from the other's.  Against the host route, as
    test_regression_is_bit_identical_to_the_host_route; 333 observations: a ragged last block in both mappings."""
    nd, ndata, p0, G = ds.ND, 333, ds.P0, 20
    assert ds.plan(nw, ndata).mapping == "lane" and ds.plan(nw // 2, ndata).mapping == half
    assert ds.last_block(nw, ndata)[:4] == (1, 13, 1, 13) and ds.last_block(511, ndata)[:4] == (2, 13, 1, 13)
    D, beta = ds.reg_data(ndata, nd, nw)
    dd = kmc.DataDensity(REG_TERM, D, params=[p0])
    host = host_yardstick(kmc, lambda X: ds.reg_terms(X, D, p0))
    th = beta + 0.05 * np.random.default_rng(nw).standard_normal((nw, nd))
    got, want = run(kmc, dd, th, G, 4, 2), run(kmc, host, th, G, 4, 2)
    for words in ds.describe_words(nw // 2, ndata):
        assert words in got["desc"], got["desc"]
    assert_same(got, want)
    assert 0 < got["nacc"].sum() < nw * (G - 4)
    np.testing.assert_array_equal(dd._eval_rows(got["pos"]), got["logp"])


@pytest.mark.parametrize("T,nw,half,whole", [(8, 132, "lane", "lane"), (4, 200, "obs", "lane")], ids=["8x132", "4x200"])
def test_a_likelihood_tempered_ladder_across_the_mapping_boundary(kmc, T, nw, half, whole):
    """A ladder's plans are made for ntemps x h and ntemps x nwalkers rows: 8 x 66 = 528 proposals take the proposal-per-lane kernel
    although 66 alone would not; 4 x 100 = 400 stay below 512 while the 800 rows of set_positions do not."""
    nd, ndata, p0, G = 3, 333, ds.P0, 12
    h = nw // 2
    assert h < 512 and ds.plan(T * h, ndata).mapping == half and ds.plan(T * nw, ndata).mapping == whole
    betas = [1.0, 0.5, 0.2, 0.05] if T == 4 else [*(1e-3 ** (np.arange(7) / 6.0)), 0.0]
    D, beta = ds.reg_data(ndata, nd, nw)
    dd = kmc.DataDensity(REG_TERM, D, prior=GAUSS_PRIOR, params=[p0])
    th = beta + 0.05 * np.random.default_rng(T).standard_normal((nw, nd))
    got = run_tempered(kmc, dd, th, betas, G, 3, 2, seed=7)
    for words in ds.describe_words(T * h, ndata, tempered=True):
        assert words in got["desc"], got["desc"]
    want = dy.emcee_data_tempered(dy.data_logpdf(lambda X: ds.reg_terms(X, D, p0), gauss_prior), th, betas, G, 3, 2, seed=7)
    assert_matches(got, want)
    assert 0 < got["nacc"].sum() < T * nw * (G - 3) and got["nswap"].sum() > 0


# ---- 3. the largest and the smallest kernels ------------------------------------------------------------------------------
BIG_TERM = ("double a = 0.0; for (int k = 0; k < 16; ++k) a += x[k] * d[k]; double b = 0.0; for (int k = 16; k < 32; ++k) b += x[k] * d[k - 16]; "
            "double r = a - p[0] * b; return -0.5 * r * r;")
ONE_TERM = "double r = d[0] - x[0]; return -0.5 * p[0] * r * r;"


def big_terms(X, D, p0=0.75):
    a = np.zeros((X.shape[0], D.shape[0]))
    b = np.zeros((X.shape[0], D.shape[0]))
    for k in range(16):
        a = a + X[:, k:k + 1] * D[None, :, k]
    for k in range(16, 32):
        b = b + X[:, k:k + 1] * D[None, :, k - 16]
    r = a - p0 * b
    return -0.5 * r * r


def one_terms(X, D, p0=0.75):
    r = D[None, :, 0] - X[:, 0:1]
    return -0.5 * p0 * r * r


@pytest.mark.parametrize("nd,ncols,term,terms", [(32, 16, BIG_TERM, big_terms), (1, 1, ONE_TERM, one_terms)], ids=["32x16", "1x1"])
@pytest.mark.parametrize("nprop,ndata", [(70, 1229), (4100, 2100), (1, 1)])
def test_largest_and_smallest_kernels_are_exact_in_both_mappings(kmc, kmc_debug, nd, ncols, term, terms, nprop, ndata):
    """ndim 32 keeps 32 doubles of the row in registers next to the stack, ncols 16 is the widest observation row (one s_load_dwordx16
    a term in the lane mapping, 128-byte strides in the other); 1 and 1 are the other end.  70 x 1229: ragged last blocks (13 rows), one
    round; 4100 x 2100: 2 rounds (lane) and 16 (obs), four proposals in the last wave of lanes."""
    assert [ds.plan(nprop, ndata, m).rounds for m in ("lane", "obs")] == {70: [1, 1], 4100: [2, 16], 1: [1, 1]}[nprop]
    rng = np.random.default_rng(100 * nd + nprop)
    D = rng.standard_normal((ndata, ncols))
    X = 0.3 * rng.standard_normal((nprop, nd))
    dd = kmc.DataDensity(term, D, params=[0.75])
    rows = ds.check_rows(nprop, ndata * (nd + 1))                      # (the reference's temporaries are per term, its work per column)
    want = ds.reference(lambda X_, D_: terms(X_, D_), None, X[rows], D)
    got = eval_in_both_mappings(kmc_debug, dd, X)
    assert np.all(np.isfinite(want)) and (ndata < 17 or np.any(want != ds.sequential(terms(X[rows], D))))
    np.testing.assert_array_equal(got["lane"][rows], want)
    np.testing.assert_array_equal(got["obs"], got["lane"])


# ---- 4. non-finite values -------------------------------------------------------------------------------------------------
# observations [flag, z, y]: flag 1 -> -inf, 2 -> NaN, 3 -> +inf, 4 -> -0.0, else the regression term; -inf outside the likelihood's
# own support x[1] <= p[1].  The prior is -inf where x[0] > p[2].
FLAG_TERM = ("if (d[0] == 1.0) return -INFINITY; if (d[0] == 2.0) return __builtin_nan(\"\"); if (d[0] == 3.0) return INFINITY; if (d[0] == 4.0) return -0.0; "
             "if (x[1] > p[1]) return -INFINITY; double mu = x[0] + x[1] * d[1]; double r = d[2] - mu; return -0.5 * p[0] * r * r;")
FLAG_PRIOR = "return x[0] > p[2] ? -INFINITY : 0.25 * x[0];"
NEVER = 1e300


def flag_terms(X, D, p):
    with np.errstate(all="ignore"):
        mu = X[:, 0:1] + X[:, 1:2] * D[None, :, 1]
        r = D[None, :, 2] - mu
        t = -0.5 * p[0] * r * r
        t = np.where(X[:, 1:2] > p[1], -np.inf, t)
        for flag, v in ((4.0, -0.0), (3.0, np.inf), (2.0, np.nan), (1.0, -np.inf)):
            t = np.where(D[None, :, 0] == flag, v, t)
    return t


def flag_prior(X, p):
    return np.where(X[:, 0] > p[2], -np.inf, 0.25 * X[:, 0])


def flag_inputs(nprop, ndata, flags):
    D2, beta = ds.reg_data(ndata, 2, ndata)
    D = np.column_stack([np.zeros(ndata), D2])
    for j, f in flags.items():
        D[j, 0] = f
    X = beta + 0.05 * np.random.default_rng(nprop).standard_normal((nprop, 2))
    return D, X, beta


# (nprop, ndata): where the LAST observation sits in each mapping.  lane / obs:
FLAG_SHAPES = [(64, 33),        # alone in the third wave / the 33rd row of the only round
               (4096, 4977),    # alone in a padded chunk after three whole ones, 4 rounds / the 49th row of the 14th round of 32
               (5, 129),        # alone in a padded chunk of the first wave of the third block / alone in the third wave
               (700, 3457)]     # alone in the first wave of the 55th block / alone in the 7th round of the third wave, 8 rounds


@pytest.mark.parametrize("nprop,ndata", FLAG_SHAPES)
def test_non_finite_terms_follow_ieee_and_a_minus_inf_prior_wins(kmc, kmc_debug, nprop, ndata):
    if (nprop, ndata) == (4096, 4977):
        assert ds.last_block(nprop, ndata, "lane")[:4] == (2, 49, 4, 1) and ds.plan(nprop, ndata, "lane").rounds == 4
    if (nprop, ndata) == (700, 3457):
        assert ds.last_block(nprop, ndata, "obs")[:4] == (3, 385, 7, 1) and ds.plan(nprop, ndata, "obs").rounds == 8
    if ndata in (33, 129):
        assert ds.last_block(nprop, ndata, "lane" if ndata == 33 else "obs")[:2] == (3, 1)
    last, mid = ndata - 1, ndata // 2
    inf, nan = np.inf, np.nan
    settings = [("no flag", {}, None), ("-inf first", {0: 1.0}, -inf), ("-inf last", {last: 1.0}, -inf), ("NaN first", {0: 2.0}, nan), ("NaN last", {last: 2.0}, nan),
                ("+inf last", {last: 3.0}, inf), ("+inf first, -inf last", {0: 3.0, last: 1.0}, nan), ("-inf in the middle, +inf last", {mid: 1.0, last: 3.0}, nan),
                ("NaN first, -inf last", {0: 2.0, last: 1.0}, nan)]
    rows = ds.check_rows(nprop, 4 * ndata)
    for name, flags, kind in settings:
        D, X, beta = flag_inputs(nprop, ndata, flags)
        p = [ds.P0, NEVER, beta[0]]                                      # about half the rows have a -inf prior
        out_of_prior = X[:, 0] > p[2]
        assert 0.2 < out_of_prior.mean() < 0.8
        dd = kmc.DataDensity(FLAG_TERM, D, prior=FLAG_PRIOR, params=p)
        got = eval_in_both_mappings(kmc_debug, dd, X)
        want = ds.reference(lambda X_, D_: flag_terms(X_, D_, p), lambda X_: flag_prior(X_, p), X[rows], D)
        for m in ("lane", "obs"):
            np.testing.assert_array_equal(got[m][rows], want, err_msg="%s, %s" % (name, m))
            assert np.all(got[m][out_of_prior] == -inf), (name, m)       # exactly -inf, whatever the tree sum is
            inside = got[m][~out_of_prior]
            if kind is None:
                assert np.all(np.isfinite(inside)), (name, m)
            elif np.isnan(kind):
                assert np.all(np.isnan(inside)), (name, m)
            else:
                assert np.all(inside == kind), (name, m)
        np.testing.assert_array_equal(got["obs"], got["lane"], err_msg=name)


def test_minus_zero_terms_sum_to_a_zero(kmc, kmc_debug):
    """17 terms of -0.0: the static tree pads its tail with +0.0, so S is a zero of either sign (the contract's one exception); the
    log-pdf is then the prior's value exactly.  The sign itself shows in S read alone (likelihood tempering)."""
    D, X, beta = flag_inputs(70, 17, {j: 4.0 for j in range(17)})
    p = [ds.P0, NEVER, NEVER]
    dd = kmc.DataDensity(FLAG_TERM, D, prior=FLAG_PRIOR, params=p)
    got = eval_in_both_mappings(kmc_debug, dd, X)
    for m in ("lane", "obs"):
        np.testing.assert_array_equal(got[m], 0.25 * X[:, 0])
    with kmc.Sampler(dd, 70, 2, 2, betas=[1.0, 0.0], temper="likelihood") as s:
        s.set_positions(X)
        assert np.all(s.rung_loglike() == 0.0)                           # +0.0 or -0.0
        np.testing.assert_array_equal(s.rung_logprior()[0], 0.25 * X[:, 0])


@pytest.mark.parametrize("nw", [64, 1100])
def test_proposals_that_leave_the_likelihood_s_support_are_refused(kmc, nw):
    """A term that is -inf for x[1] > p[1], with the walkers started just inside: the sum is -inf for such a proposal in whichever kernel
    evaluates it, it is never accepted, and every counter equals the host route's."""
    ndata, G = 333, 24
    D, X, beta = flag_inputs(nw, ndata, {})
    X[:, 1] = beta[1] - np.abs(X[:, 1] - beta[1])
    p = [ds.P0, beta[1], NEVER]
    outside = []

    def terms(X_):
        t = flag_terms(X_, D, p)
        outside.append(int(np.sum(X_[:, 1] > p[1])))
        return t

    dd = kmc.DataDensity(FLAG_TERM, D, prior=FLAG_PRIOR, params=p)
    host = host_yardstick(kmc, terms, lambda X_: flag_prior(X_, p))
    got, want = run(kmc, dd, X, G, 4, 1), run(kmc, host, X, G, 4, 1)
    assert np.all(X[:, 1] <= p[1]) and sum(outside) > nw                    # the start is inside; many proposals were not
    assert_same(got, want)
    assert np.all(np.isfinite(got["chain_logp"])) and np.all(np.isfinite(got["logp"])) and np.all(got["chain"][:, :, 1] <= p[1])
    assert 0 < got["nacc"].sum() < nw * (G - 4)


# ---- 5. kmc_logpdf_eval on the caller's device memory and stream ----------------------------------------------------------
GUARD = -12345.678


def eval_on_device(kmc, pdf, X, nrows=None):
    """kmc_logpdf_eval on torch tensors and a torch stream that is not the default one; returns the output buffer, 8 guard values long
    past its last row."""
    import torch
    from kissmcmc_jl_amd import _lib
    n, nd = X.shape
    nrows = n if nrows is None else nrows
    cfg = _lib.Config()
    cfg.dtype, cfg.density, cfg.user_density = _lib.F64, pdf.density_id, pdf.user_handle
    for i, v in enumerate(pdf.params()):
        cfg.params[i] = v
    cfg.nwalkers, cfg.ndim, cfg.nthin, cfg.a_scale = max(2, n + (n & 1)), nd, 1, 2.0
    pos = torch.from_numpy(np.ascontiguousarray(X)).to("cuda")
    out = torch.full((n + 8,), GUARD, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.default_stream().cuda_stream
    _lib.check(_lib.lib().kmc_logpdf_eval(C.byref(cfg), C.c_void_p(pos.data_ptr()), C.c_void_p(out.data_ptr()), nrows, C.c_void_p(side.cuda_stream)))
    side.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("c", [ds.Case(300, 3000, None), ds.Case(3000, 3001, None)], ids=ds.case_id)
def test_logpdf_eval_of_a_data_density_on_device_pointers(kmc, c):
    assert ds.plan(*c).mapping == ("obs" if c.nprop == 300 else "lane")
    D, X = ds.inputs(c)
    dd = kmc.DataDensity(REG_TERM, D, params=[ds.P0])
    rows = ds.check_rows(c.nprop, c.ndata)
    out = eval_on_device(kmc, dd, X)
    np.testing.assert_array_equal(out[:c.nprop][rows], ds.reg_reference(X[rows], D))
    np.testing.assert_array_equal(out[:c.nprop], dd._eval_rows(X))
    np.testing.assert_array_equal(out[c.nprop:], GUARD)
    np.testing.assert_array_equal(eval_on_device(kmc, dd, X, nrows=0), GUARD)          # OK, and nothing written
    part = eval_on_device(kmc, dd, X, nrows=65)
    np.testing.assert_array_equal(part[:65], out[:65])
    np.testing.assert_array_equal(part[65:], GUARD)


def test_logpdf_eval_of_a_menu_density_on_device_pointers(kmc, oracle):
    pdf = kmc.Rosenbrock()
    X = 1.0 + 0.5 * np.random.default_rng(5).standard_normal((300, 5))
    out = eval_on_device(kmc, pdf, X)
    np.testing.assert_array_equal(out[:300], oracle.logpdf_batch(oracle.ROSENBROCK, pdf.params(), X))
    np.testing.assert_array_equal(out[300:], GUARD)
    np.testing.assert_array_equal(eval_on_device(kmc, pdf, X, nrows=0), GUARD)
    part = eval_on_device(kmc, pdf, X, nrows=257)
    np.testing.assert_array_equal(part[:257], out[:257])
    np.testing.assert_array_equal(part[257:], GUARD)
