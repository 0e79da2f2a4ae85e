"""GPU: the move and tempered kernels at every walkers-per-group count (ITER > 1) that kmc_tables.hpp builds for them.

make_plan picks ITER >= 2 only from n_active * L / 64 >= 3072 waves on, so the sibling modules (which never set KMC_PLAN, or set it
once) compare the DE, snooker, mixture and tempered kernels with their yardsticks at ITER = 1 almost only -- while every large
ensemble runs ITER > 1.  What ITER > 1 adds to half_step_vec_body is the scalar-to-row routing (lane gbase + it carries walker slot
it), the clamped walkers of a last wave, the partner loads split round the first logarithm, the workgroup moment fold (ITER >= 4 at
L = 8 and 32) and the moment ring's room check (L = 64).

1. forced geometries (KMC_PLAN) against snooker_yardstick.emcee_moves / tempering_yardstick.emcee_tempered, bit for bit under
   DESIGN.md section 6's bar, at active halves that are the smallest legal one, one walker past a wave, and whole workgroups
   (tests/move_geometries.py holds the matrix; `python tests/move_geometries.py` shows that no case is vacuous);
2. the planner's own choice at 65 536 walkers (ITER = 2) against the same sampler forced to ITER = 1;
3. runtime-compiled densities, compiled for exactly one geometry;
4. ragged rows of the plain stretch move at ITER > 1, against the oracle.

Every case first asserts on describe() that it ran the geometry and the kernel it asked for: a forced plan without an instantiation
falls back to the one-walker-per-lane kernel, the planner caps ITER for snooker and mixtures, and small plain stretch ensembles
leave for the resident kernel -- all without a word."""
import numpy as np
import pytest

import kmcenv
import move_geometries as mg
import snooker_yardstick as sy
from test_gpu_de_move import GENERAL_BODY, general_body_host
from test_gpu_de_move import assert_matches as assert_matches_plain
from test_gpu_parity import _compare as assert_matches_oracle
from test_gpu_tempering import assert_matches as assert_matches_ladder

pytestmark = pytest.mark.gpu

GAUSS_EXPR = "-0.5*((x-p[0])*p[1])*((x-p[0])*p[1])"
gauss_expr_host = lambda X: np.array([sum(-0.5 * ((x - 0.25) * (1.0 / 1.5)) * ((x - 0.25) * (1.0 / 1.5)) for x in row) for row in X])


def library_move(kmc, name):
    return {"stretch": None, "de": kmc.DEMove(), "snooker": kmc.DESnookerMove(),
            "mix": [(kmc.DEMove(), mg.MIX[0]), (kmc.DESnookerMove(), mg.MIX[1])]}[name]


def run(kmc, pdf, th, G, nburn, nthin, seed, move=None, betas=None, chain=True):
    """The job in two run() calls; every read-out the assert_matches of the sibling modules compare (a ladder: every rung's)."""
    nw, nd = th.shape
    kw = dict(betas=betas, swap_every=1) if betas is not None else {}
    with kmc.Sampler(pdf, nw, nd, G, nburn, nthin, 2.0, seed, store_chain=chain, store_logp=chain, moments=True, move=move, **kw) as s:
        desc = s.describe()
        s.set_positions(th)
        s.run(G // 2)
        s.run(G - G // 2)
        s.sync()
        m = s.moments()
        out = dict(desc=desc, sum=m[0], sumsq=m[1], n=m[2])
        if chain:
            out["chain"], out["chain_logp"] = s.chain()
        if betas is None:
            out.update(pos=s.positions(), logp=s.logp(), nacc=s.naccept())
        else:
            out.update(pos=s.rung_positions(), logp=s.rung_logp(), nacc=s.rung_naccept(), nswap=s.nswap().astype(np.int64),
                       logp_sum=s.rung_logp_sum(), pos0=s.positions(), logp0=s.logp(), nacc0=s.naccept())
        return out


def assert_ran(got, words):
    for w in words:
        assert w in got["desc"], (w, got["desc"])


def assert_moments_are_the_chains(got):
    """The streaming moments (sojourn-weighted credits, rung 0's under tempering) against the sums over the device's own chain."""
    ch = got["chain"]
    assert got["n"] == ch.shape[0] * ch.shape[1]
    np.testing.assert_allclose(got["sum"], ch.sum(axis=(0, 1)), rtol=1e-11, atol=1e-9)
    np.testing.assert_allclose(got["sumsq"], (ch * ch).sum(axis=(0, 1)), rtol=1e-11, atol=1e-9)


def assert_not_vacuous(c, nacc, nswap=None):
    problems = mg.cap_problems(c, nacc, nswap)
    assert not problems, problems


def check_case(kmc, monkeypatch, c, pdf, logpdf, th, also=()):
    """Section 1 and 3: the device under KMC_PLAN against the yardstick of the case."""
    lib_move = library_move(kmc, c.move)
    betas = mg.BETAS if c.tempered else None
    monkeypatch.setenv("KMC_PLAN", mg.plan_of(c))
    got = run(kmc, pdf, th, mg.G, mg.NBURN, mg.NTHIN, mg.SEED, move=lib_move, betas=betas)
    every = run(kmc, pdf, th, mg.G, mg.NBURN, 1, mg.SEED, move=lib_move, betas=betas) if c.tempered else None
    monkeypatch.delenv("KMC_PLAN")
    assert_ran(got, mg.describe_words(c) + list(also))
    want = mg.yardstick(c, logpdf, th)
    if c.tempered:
        assert_matches_ladder(got, want)
        assert_moments_are_the_chains(got)
        assert_ran(every, mg.describe_words(c))
        assert_moments_are_the_chains(every)                            # (every counted generation sampled: nthin = 1)
        np.testing.assert_array_equal(every["pos"], got["pos"])
        assert_not_vacuous(c, got["nacc"], got["nswap"])
    else:
        assert_matches_plain(got, want)
        assert_not_vacuous(c, got["nacc"])


# ---- 1. forced geometries against the yardsticks ------------------------------------------------------------------------------
@pytest.mark.parametrize("c", mg.cases(), ids=mg.case_id)
def test_forced_geometry_matches_the_yardstick(kmc, oracle, monkeypatch, c):
    pdf = kmc.GaussianIso(*mg.PARAMS[mg.GAUSS]) if c.dens == mg.GAUSS else kmc.Rosenbrock(*mg.PARAMS[mg.ROSEN])
    check_case(kmc, monkeypatch, c, pdf, lambda X: oracle.logpdf_batch(c.dens, mg.PARAMS[c.dens], X), mg.start(c))


# ---- 2. the planner's own choice at a size that gets ITER > 1 ------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_start():
    return np.random.default_rng(0).standard_normal((65536, 32))


@pytest.mark.parametrize("nd", [32, 29], ids=["exact32", "ragged29"])
@pytest.mark.parametrize("move,betas", [("de", None), ("mix", None), ("stretch", [1.0, 0.5])], ids=["de", "mix", "stretch-tempered"])
def test_the_planners_iter_2_equals_iter_1(kmc, monkeypatch, big_start, move, betas, nd):
    """No yardstick at this size: the result is a function of (seed, inputs) alone, so the geometry the planner picks for 65 536
    walkers -- ITER = 2, what users run -- gives what the same sampler gives one walker per group.  Positions, counters and log-pdfs
    (the same reduction order per row) identical; the moment sums, whose order does depend on the geometry, to the moments' bar."""
    th = np.ascontiguousarray(big_start[:, :nd])
    G, nburn, seed = 6, 1, 23
    c = mg.Case(8, 2, 2, nd, nd != 32, "planned", 32768, move, betas is not None, mg.GAUSS)
    monkeypatch.delenv("KMC_PLAN", raising=False)
    planned = run(kmc, kmc.GaussianIso(), th, G, nburn, 1, seed, move=library_move(kmc, move), betas=betas, chain=False)
    assert_ran(planned, mg.describe_words(c))
    monkeypatch.setenv("KMC_PLAN", "8,2,1")
    single = run(kmc, kmc.GaussianIso(), th, G, nburn, 1, seed, move=library_move(kmc, move), betas=betas, chain=False)
    monkeypatch.delenv("KMC_PLAN")
    assert_ran(single, mg.describe_words(c._replace(ITER=1)))
    for k in ("pos", "nacc", "logp") + (("nswap",) if betas else ()):
        np.testing.assert_array_equal(planned[k], single[k], err_msg=k)
    assert planned["n"] == single["n"] == (G - nburn) * 65536
    np.testing.assert_allclose(planned["sum"], single["sum"], rtol=1e-11, atol=1e-9)
    np.testing.assert_allclose(planned["sumsq"], single["sumsq"], rtol=1e-11, atol=1e-9)
    nacc = np.atleast_2d(planned["nacc"])
    assert 0 < nacc[0].sum() < (G - nburn) * 65536 and 0 < nacc.sum() < nacc.shape[0] * (G - nburn) * 65536
    if move == "mix":
        _, cum = sy.mix_weights(list(mg.MIX))
        assert set(sy.mix_choices(seed, np.arange(2 * G), cum).tolist()) == {0, 1}


# ---- 3. runtime-compiled densities: compiled for exactly one geometry --------------------------------------------------------------
@pytest.mark.parametrize("kind,plan,nd,move,tempered", [("expr", (16, 2, 4), 61, "de", False), ("expr", (8, 2, 2), 29, "mix", True),
                                                        ("body", (8, 2, 2), 29, "de", False)],
                         ids=["expr-16,2,4-nd61-de", "expr-8,2,2-nd29-mix-tempered", "body-8,2,2-nd29-de"])
def test_runtime_compiled_density_matches_the_yardstick(kmc, monkeypatch, kind, plan, nd, move, tempered):
    """An ExprDensity (lane-striped) and a function body evaluated per walker through the wave's LDS tile (row js G + g of it), one
    walker past a wave."""
    L, K, ITER = plan
    c = mg.Case(L, K, ITER, nd, True, "tail", mg.sizes(L, ITER, nd)["tail"], move, tempered, mg.GAUSS)
    th = np.random.default_rng(nd).standard_normal((2 * c.nhalf, nd))
    if kind == "expr":
        pdf, f = kmc.ExprDensity(GAUSS_EXPR, params=[0.25, 1.0 / 1.5]), gauss_expr_host
    else:
        pdf, f = kmc.CDensity(GENERAL_BODY, params=[4.0]), lambda X: general_body_host(X, 4.0)
    check_case(kmc, monkeypatch, c, pdf, f, th, also=["runtime-compiled"])


# ---- 4. ragged rows of the plain stretch move at ITER > 1 --------------------------------------------------------------------------
@pytest.mark.parametrize("name,plan,nd", [("gauss", (4, 2, 2), 13), ("gauss", (8, 2, 4), 29), ("rosen", (8, 2, 4), 29), ("gauss", (16, 2, 4), 61),
                                          ("rosen", (16, 2, 4), 61), ("gauss", (64, 2, 4), 200), ("gauss", (64, 4, 2), 400)],
                         ids=lambda v: "%d,%d,%d" % v if isinstance(v, tuple) else str(v))
def test_ragged_stretch_rows_match_the_oracle(kmc, oracle, monkeypatch, name, plan, nd):
    """Plain stretch, one walker past a wave, against the oracle as tests/test_gpu_parity.py compares (ensembles this small would
    leave for the LDS-resident kernel whatever KMC_PLAN says: kept in the multi-launch kernels)."""
    from test_gpu_parity import _densities, _theta0
    L, K, ITER = plan
    c = mg.Case(L, K, ITER, nd, True, "tail", mg.sizes(L, ITER, nd)["tail"], "stretch", False, mg.GAUSS)
    nw, seed = 2 * c.nhalf, 1234 + nd
    pdf, did, params = _densities(kmc, oracle)[name]
    th = _theta0(name, nw, nd, seed)
    ref = oracle.emcee(oracle.make_config(did, params, nw, nd, mg.G, mg.NBURN, mg.NTHIN, 2.0, seed), th)
    monkeypatch.setenv("KMC_PLAN", mg.plan_of(c))
    kmcenv.no_resident(monkeypatch)
    with kmc.Sampler(pdf, nw, nd, mg.G, mg.NBURN, mg.NTHIN, 2.0, seed, store_chain=True, store_logp=True, moments=True) as s:
        desc = s.describe()
        s.set_positions(th)
        s.run(mg.G // 2)
        s.run(mg.G - mg.G // 2)
        s.sync()
        got = dict(final_pos=s.positions(), final_logp=s.logp(), naccept=s.naccept(), accept_ratio=s.accept_ratio())
        got["chain"], got["chain_logp"] = s.chain()
        got["sum"], got["sumsq"], got["nmoment"] = s.moments()
    monkeypatch.delenv("KMC_PLAN")
    assert_ran(dict(desc=desc), mg.describe_words(c))
    assert_matches_oracle(ref, got)
    assert_not_vacuous(c, got["naccept"])
    assert 0 < ref["naccept"].sum() < nw * (mg.G - mg.NBURN)
