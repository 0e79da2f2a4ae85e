"""GPU: the path by which a sampler's state goes in and comes out (kmc_state.hip), pinned from outside.  Three tables of small
samplers: one per accumulator layout that kmc_sampler_get_moments decodes, one per way in (set_positions, init_ball, set_state,
set_rung_state, set_walker_ids), one per refusal of those entry points that no other test pins.  A row of the first two creates its
sampler, asserts that describe() (under KMC_DEBUG=geometry) names the route the row claims -- so that a row cannot silently test
another route --, runs 16 burn-in generations plus 16 sampled and compares a sha256 over the raw bytes of everything it reads out
with a recorded value.  The values were recorded from the library before the setters, resets and the moment read-out were given
one path each, and hold unchanged after it: a row that differs means some bit of what goes in or comes out has changed.

Every row was run in two separate processes first; all of them gave the same bytes in both.  The one tempered row with moments
(test_tempered_moments_are_reset_and_read_out) still keeps a digest over its state alone: its sums include the exchange sweeps' atomic
adds in double, whose order two agreeing runs do not guarantee, and are compared with the stored chain the way
tests/test_gpu_tempering.py compares them."""
import ctypes as C
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G, NBURN, SEED = 32, 16, 5
LADDER3 = [1.0, 0.5, 0.25]

# a coupling through the mean: no sum over elements, evaluated per walker as written
BODY = ("double m = 0.0; for (int i = 0; i < n; ++i) m += x[i]; m = m / n; double s = 0.0; "
        "for (int i = 0; i < n; ++i) { double t = x[i] - m; s += t * t; } return -0.5 * s - 0.5 * p[0] * m * m;")
BLOB_BODY = "double s = 0.0; for (int i = 0; i < n; ++i) s += x[i] * x[i]; blob[0] = x[0]; blob[1] = s; return -0.5 * s;"
REG_TERM = "double mu = x[0]; for (int k = 1; k < n; ++k) mu += x[k] * d[k - 1]; double r = d[n - 1] - mu; return -0.5 * p[0] * r * r;"
GAUSS_PRIOR = "double s = 0.0; for (int k = 0; k < n; ++k) s += x[k] * x[k]; return -0.5 * s;"

_made = {}


def density(kmc, name, nd):
    """One density object per name (per ndim for the data density): a runtime-compiled one is compiled once per geometry."""
    key = (name, nd if name == "data" else 0)
    if key not in _made:
        if name == "gauss":
            d = kmc.GaussianIso()
        elif name == "expo":
            d = kmc.Exponential()
        elif name == "term":
            d = kmc.ExprDensity("-0.5*x*x")
        elif name == "body":
            d = kmc.CDensity(BODY, params=[4.0])
            assert not d.separable
        elif name == "blobbody":
            d = kmc.CDensity(BLOB_BODY, nblob=2)
        elif name == "host":
            d = kmc.HostLogPdf(lambda X: -0.5 * (X * X).sum(axis=1), vectorized=True)
        elif name == "data":
            d = kmc.DataDensity(REG_TERM, np.random.default_rng(1).standard_normal((50, nd)), prior=GAUSS_PRIOR, params=[1.0])
        else:
            raise KeyError(name)
        _made[key] = d
    return _made[key]


def theta0(nw, nd, ntemps=None):
    th = 0.5 + 0.1 * np.abs(np.random.default_rng(0).standard_normal((nw, nd) if ntemps is None else (ntemps, nw, nd)))
    return th


def make(kmc, kmc_debug, monkeypatch, dens, nw, nd, kw, opts, words):
    """The row's sampler, after describe() has named every word of the route the row claims."""
    kmc_debug.set("geometry")
    plan = None
    for k, v in opts.items():
        if k == "plan":
            plan = v
        else:
            kmc_debug.set(k, v)
    if plan is None:
        monkeypatch.delenv("KMC_PLAN", raising=False)
    else:
        monkeypatch.setenv("KMC_PLAN", plan)
    s = kmc.Sampler(density(kmc, dens, nd), nw, nd, G, NBURN, 1, 2.0, SEED, **kw)
    how = s.describe()
    for w in words:
        assert w in how, (w, how)
    return s


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def has_moments(s):
    from kissmcmc_jl_amd import _lib
    return bool(s.cfg.flags & _lib.MOMENTS)


def read_all(s, moments=True):
    s.sync()
    out = []
    if s.betas0 is not None:
        out += [s.rung_positions(), s.rung_logp(), s.rung_naccept(), s.nswap(), s.rung_logp_sum()]
        if s.temper == "likelihood":
            out += [s.rung_loglike(), s.rung_logprior(), s.rung_loglike_sum()]
        if s.adapt:
            b, S, ra, sk = s._ladder()
            out += [b, S, ra, np.array([sk], dtype=np.int64)]
    out += [s.positions(), s.logp(), s.naccept()]
    if s.cfg.deal_count > 0:
        out.append(s.walker_ids())
    if s.nblob:
        out.append(s.current_blobs())
    if moments and has_moments(s):
        msum, msq, n = s.moments()
        out += [msum, msq, np.array([n], dtype=np.int64)]
    return out


# ---- 1. one row per accumulator layout of kmc_sampler_get_moments ---------------------------------------------------------------
NORES = {"no-resident": None}
TWO = {"no-resident": None, "fused": "0"}
STAGED = {"no-resident": None, "fused": "0", "no-body-vec": None}
# (id, density, nwalkers, ndim, Sampler keywords, KMC_DEBUG options (and `plan`: KMC_PLAN), words of describe(), generations stepped by halves at the end)
MOMENT_ROWS = [
    # one launch per generation, rows lane-striped, accumulators per wave in the transposed layout: the decode differs per L
    ("gen_fold_L8_64x32", "gauss", 64, 32, {}, NORES, ["one launch per generation", "plan=vec/8/2/", "fused=1 fused_L=8 ", "fused_fold=1"], 0),
    ("gen_fold_L16_66x64", "gauss", 66, 64, {}, {}, ["one launch per generation", "plan=vec/16/2/", "fused=1 fused_L=16 ", "fused_fold=1"], 0),
    ("gen_fold_L32_130x128", "gauss", 130, 128, {}, {}, ["one launch per generation", "plan=vec/32/2/", "fused=1 fused_L=32 ", "fused_fold=1"], 0),
    ("gen_fold_odd_66x31", "gauss", 66, 31, {}, NORES, ["one launch per generation", "plan=vec/8/2/1/ragged", "fused=1 fused_L=8 ", "fused_fold=1"], 0),
    # ... accumulators per walker
    ("gen_striped_64x16", "gauss", 64, 16, {}, NORES, ["one launch per generation", "fused=1 fused_L=4 ", "fused_fold=0"], 0),
    ("gen_lane_64x4", "gauss", 64, 4, {}, NORES, ["one launch per generation", "one walker per lane", "fused=1 fused_L=0 ", "fused_fold=0"], 0),
    ("gen_lane_odd_66x3", "gauss", 66, 3, {}, NORES, ["one launch per generation", "one walker per lane", "fused=1 fused_L=0 "], 0),
    # one launch per generation, then stepped by halves: what was credited until then is carried on the host
    ("gen_fold_then_halves_64x32", "gauss", 64, 32, {}, NORES, ["one launch per generation", "fused=1 fused_L=8 ", "fused_fold=1"], 8),
    ("gen_lane_then_halves_64x4", "gauss", 64, 4, {}, NORES, ["one launch per generation", "fused=1 fused_L=0 "], 8),
    # islands and resident mode: sums per island
    ("islands_256x8", "gauss", 256, 8, dict(island_gens=16, island_size=64), {}, ["islands=1", "resident=0"], 0),
    ("resident_lane_64x4", "gauss", 64, 4, {}, {}, ["resident mode", "resident=1", "resident_lane=1"], 0),
    ("resident_pair_64x16", "gauss", 64, 16, {}, {}, ["resident mode", "resident=1", "resident_lane=0"], 0),
    # two launches per generation, the vector kernel: transposed (K = 2, L = 8 / 16 / 32) ...
    ("two_fold_L8_64x32", "gauss", 64, 32, {}, TWO, ["multi-launch", "half_step_vec L=8 K=2", "fused=0"], 0),
    ("two_fold_L16_66x64", "gauss", 66, 64, {}, TWO, ["multi-launch", "half_step_vec L=16 K=2", "fused=0"], 0),
    ("two_fold_L32_130x128", "gauss", 130, 128, {}, TWO, ["multi-launch", "half_step_vec L=32 K=2", "fused=0"], 0),
    ("two_fold_f32_64x32", "gauss", 64, 32, dict(dtype="f32"), {}, ["multi-launch", "half_step_vec L=8 K=2", "KMC_F32", "fused=0"], 0),
    # ... and plain
    ("two_plain_K1_64x4", "gauss", 64, 4, {}, TWO, ["multi-launch", "half_step_vec L=2 K=1", "fused=0"], 0),
    ("two_plain_L4K2_66x15", "gauss", 66, 15, {}, TWO, ["multi-launch", "half_step_vec L=4 K=2", "ragged", "fused=0"], 0),
    ("two_plain_L64_ring_258x256", "gauss", 258, 256, {}, TWO, ["multi-launch", "half_step_vec L=64 K=2", "fused=0", "d_mring=1"], 0),
    # a function body, one walker per lane: rows staged through LDS (accumulator rows per wave, or columns per lane), and the generic kernel
    # (describe() does not say which of the two: kmc_kernels.hpp staged_tile_moments(ndim) = 64 % (tile / 2) == 0 with tile = min(ld, 32) doubles does --
    #  ndim 4: tile 4, 64 % 2 == 0, rows per wave; ndim 6: tile 6, 64 % 3 != 0, columns per lane.  A change of staged_tile_doubles has to keep one row of each.)
    ("staged_tile_64x4", "body", 64, 4, {}, STAGED, ["half_step_staged", "fused=0"], 0),
    ("staged_columns_64x6", "body", 64, 6, {}, STAGED, ["half_step_staged", "fused=0"], 0),
    ("generic_64x4", "gauss", 64, 4, {}, {"no-resident": None, "plan": "generic"}, ["half_step_generic", "fused=0"], 0),
]


@pytest.mark.parametrize("row", MOMENT_ROWS, ids=[r[0] for r in MOMENT_ROWS])
def test_moments_of_every_accumulator_layout(kmc, kmc_debug, monkeypatch, row):
    rid, dens, nw, nd, kw, opts, words, halves = row
    with make(kmc, kmc_debug, monkeypatch, dens, nw, nd, dict(kw, moments=True), opts, words) as s:
        s.set_positions(theta0(nw, nd))
        s.run(G - halves)
        for _ in range(halves):
            s.half_step(0)
            s.half_step(1)
        if halves:
            assert "multi-launch" in s.describe()
        out = read_all(s)
        assert out[-1][0] == (G - NBURN) * nw
    got = digest(out)
    print(f"\nDIGEST {rid} {got}")
    assert got == EXPECTED[rid]


# ---- 2. every way in, followed by the same short run -----------------------------------------------------------------------------
def enter_positions(kmc, s, twin):
    s.set_positions(theta0(s.nwalkers, s.ndim))
    return G


def enter_rung_positions(kmc, s, twin):
    s.set_positions(theta0(s.nwalkers, s.ndim, s.ntemps))       # [ntemps, nwalkers, ndim]: kmc_sampler_set_rung_state at generation 0
    return G


def enter_ball(kmc, s, twin):
    s.init_ball(0.7 if s.pdf.density_id == 1 else 0.0, 0.3, seed=11)
    return G


def checkpoint(twin, at):
    """The state of a sampler like the row's after `at` generations (one per row: the row's second entry restores the same one)."""
    if "state" not in twin:
        t = twin["make"]()
        with t:
            t.set_positions(theta0(t.nwalkers, t.ndim))
            t.run(at)
            twin["state"] = t.state()
            twin["ids"] = t.walker_ids()
    return twin["state"]


def enter_state(kmc, s, twin, at=24, naccept=True, ids=False):
    st = checkpoint(twin, at)
    if naccept:
        s.restore(st)
    else:
        from kissmcmc_jl_amd import _lib
        pos, lp = np.ascontiguousarray(st["positions"]), np.ascontiguousarray(st["logp"])
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        _lib.check(s._L.kmc_sampler_set_state(s._h, dp(pos), dp(lp), None, int(st["generation"])))
    if ids:
        s.set_walker_ids(twin["ids"][::-1])                     # (any assignment will do: the slots' walkers, reversed)
    return G - at


def enter_state_no_naccept(kmc, s, twin):
    return enter_state(kmc, s, twin, naccept=False)


def enter_state_ids(kmc, s, twin):
    return enter_state(kmc, s, twin, ids=True)


def enter_state_early(kmc, s, twin):
    return enter_state(kmc, s, twin, at=8)                      # (an adaptive ladder: in the middle of its adaptation)


LIKE = dict(betas=[1.0, 0.3, 0.0], temper="likelihood")
# (id, the way in, density, nwalkers, ndim, Sampler keywords, words of describe())
ENTRY_ROWS = [
    ("set_positions", enter_positions, "gauss", 64, 4, dict(moments=True), ["resident=1"]),
    ("set_positions_two_launch_66x15", enter_positions, "gauss", 66, 15, dict(moments=True, use_graph=False), ["multi-launch", "eager launches"]),
    ("init_ball_menu", enter_ball, "gauss", 64, 4, dict(moments=True), ["resident=1"]),
    ("init_ball_user", enter_ball, "term", 64, 4, dict(moments=True), ["resident=1"]),
    ("init_ball_f32", enter_ball, "expo", 100, 1, dict(moments=True, dtype="f32"), ["resident=1", "KMC_F32"]),
    ("init_ball_dealt", enter_ball, "gauss", 64, 4, dict(moments=True, deal_rank=1, deal_count=2), ["d_ids=1"]),
    ("set_state", enter_state, "gauss", 64, 4, {}, ["resident=1"]),
    ("set_state_no_naccept", enter_state_no_naccept, "gauss", 64, 4, {}, ["resident=1"]),
    ("set_state_blobs", enter_state, "blobbody", 64, 2, {}, ["d_blob=1"]),
    ("set_state_moments", enter_state, "gauss", 64, 4, dict(moments=True), ["resident=1", "d_msum=1"]),
    ("set_state_moments_two_launch", enter_state, "gauss", 66, 15, dict(moments=True, use_graph=False), ["multi-launch", "d_msum=1"]),
    ("set_walker_ids_dealt", enter_state_ids, "gauss", 64, 4, dict(moments=True, deal_rank=1, deal_count=2), ["d_ids=1"]),
    ("rung_positions_whole", enter_rung_positions, "gauss", 64, 4, dict(betas=LADDER3), ["d_betas=1"]),
    ("rung_positions_likelihood", enter_rung_positions, "data", 64, 3, LIKE, ["d_betas=1", "d_like=1"]),
    ("rung_positions_adapt", enter_rung_positions, "gauss", 64, 4, dict(betas=LADDER3, adapt=True), ["d_betas=1", "adapt"]),
    ("rung_checkpoint_whole", enter_state, "gauss", 64, 4, dict(betas=LADDER3), ["d_betas=1"]),
    ("rung_checkpoint_likelihood", enter_state, "data", 64, 3, LIKE, ["d_betas=1", "d_like=1"]),
    ("rung_checkpoint_adapt", enter_state_early, "gauss", 64, 4, dict(betas=LADDER3, adapt=True), ["d_betas=1", "adapt"]),
    ("rung_replicated_whole", enter_positions, "gauss", 64, 4, dict(betas=LADDER3), ["d_betas=1"]),
    ("rung_replicated_likelihood", enter_positions, "data", 64, 3, LIKE, ["d_betas=1", "d_like=1"]),
]


@pytest.mark.parametrize("row", ENTRY_ROWS, ids=[r[0] for r in ENTRY_ROWS])
def test_every_way_in(kmc, kmc_debug, monkeypatch, row):
    rid, enter, dens, nw, nd, kw, words = row
    twin = {"make": lambda: make(kmc, kmc_debug, monkeypatch, dens, nw, nd, kw, {}, words)}
    with twin["make"]() as s:
        togo = enter(kmc, s, twin)
        s.run(togo)
        first = digest(read_all(s))
        if has_moments(s):                       # the entry point again on the same sampler: the reset really resets
            assert enter(kmc, s, twin) == togo
            s.run(togo)
            assert digest(read_all(s)) == first
    print(f"\nDIGEST {rid} {first}")
    assert first == EXPECTED[rid]


def test_tempered_moments_are_reset_and_read_out(kmc, kmc_debug, monkeypatch):
    """The moments of a tempered sampler: rung 0's sums, plus what the exchange sweeps credited when a walker left rung 0 (atomic adds
    in double: compared with the stored chain, as tests/test_gpu_tempering.py compares them); its state bit for bit."""
    nw, nd = 64, 4
    with make(kmc, kmc_debug, monkeypatch, "gauss", nw, nd, dict(betas=LADDER3, moments=True, store_chain=True), {}, ["d_betas=1", "d_msum=1"]) as s:
        for _ in range(2):
            s.set_positions(theta0(nw, nd))
            s.run(G)
            out = read_all(s, moments=False)
            msum, msq, n = s.moments()
            ch, _ = s.chain(logp=False)
            assert n == (G - NBURN) * nw
            np.testing.assert_allclose(msum, ch.sum(axis=(0, 1)), rtol=1e-11, atol=1e-9)
            np.testing.assert_allclose(msq, (ch * ch).sum(axis=(0, 1)), rtol=1e-11, atol=1e-9)
            got = digest(out)
            print(f"\nDIGEST tempered_moments {got}")
            assert got == EXPECTED["tempered_moments"]


# ---- 3. the refusals of these entry points that no other test pins ---------------------------------------------------------------
def refused(kmc, status, text, call):
    from kissmcmc_jl_amd import _lib
    with pytest.raises((_lib.KmcError, RuntimeError)) as e:
        call()
    err = e.value.__cause__ if not isinstance(e.value, _lib.KmcError) else e.value
    assert err.status == getattr(_lib, status), str(err)
    assert str(err) == text


def test_set_state_refuses_chain_storage_and_tempering(kmc):
    st = dict(positions=theta0(64, 4), logp=np.zeros(64), naccept=np.zeros(64, dtype=np.int64), generation=4)
    with kmc.Sampler(kmc.GaussianIso(), 64, 4, G, NBURN, 1, 2.0, SEED, store_chain=True) as s:
        refused(kmc, "ERR_UNSUPPORTED", "kmc_sampler_set_state: not with chain / blob storage (download the chain before checkpointing)", lambda: s.restore(st))
    with kmc.Sampler(kmc.GaussianIso(), 64, 4, G, NBURN, 1, 2.0, SEED, betas=LADDER3) as s:
        from kissmcmc_jl_amd import _lib
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        pos, lp = np.ascontiguousarray(st["positions"]), st["logp"]
        refused(kmc, "ERR_UNSUPPORTED", "kmc_sampler_set_state restores one ensemble: a sampler with parallel tempering takes every rung through kmc_sampler_set_rung_state",
                lambda: _lib.check(s._L.kmc_sampler_set_state(s._h, dp(pos), dp(lp), None, 4)))


BALL_REFUSALS = [
    ("data", 3, {}, "kmc_sampler_init_ball: not with KMC_DATA_DENSITY (build the initial ensemble on the host, e.g. make_theta0s)"),
    ("host", 3, {}, "kmc_sampler_init_ball evaluates the density on the device; with KMC_HOST_DENSITY build the ball on the host"),
    ("gauss", 4, dict(betas=LADDER3), "kmc_sampler_init_ball: not with parallel tempering (build the initial ensemble on the host, e.g. make_theta0s; "
                                      "kmc_sampler_set_positions copies it to every rung)"),
]


@pytest.mark.parametrize("case", BALL_REFUSALS, ids=["data", "host", "tempered"])
def test_init_ball_refuses_what_it_cannot_fill(kmc, case):
    dens, nd, kw, text = case
    with kmc.Sampler(density(kmc, dens, nd), 64, nd, G, NBURN, 1, 2.0, SEED, **kw) as s:
        refused(kmc, "ERR_UNSUPPORTED", text, lambda: s.init_ball(0.0, 0.3, seed=1))


def test_set_ladder_refuses_a_ladder_that_does_not_decrease(kmc):
    with kmc.Sampler(kmc.GaussianIso(), 64, 4, G, NBURN, 1, 2.0, SEED, betas=[1.0, 0.5, 0.3, 0.25], adapt=True) as s:
        s.set_positions(theta0(64, 4))
        st = s.state()
        st["betas"] = np.array([1.0, 0.4, 0.4, 0.25])
        refused(kmc, "ERR_BAD_ARG", "adaptive ladder: kmc_sampler_set_ladder: betas must be finite and strictly decreasing", lambda: s.restore(st))


def test_a_non_finite_initial_log_pdf_names_its_walker_and_rung(kmc):
    """... and leaves the sampler without positions: the next run is refused."""
    not_set = "kmc_sampler_set_positions has not succeeded yet"
    with kmc.Sampler(kmc.Exponential(), 64, 2, G, NBURN, 1, 2.0, SEED) as s:
        th = theta0(64, 2)
        s.set_positions(th)
        th[5, 1] = -1.0
        refused(kmc, "ERR_NONFINITE_LOGP", "walker 5 has a non-finite initial log-pdf", lambda: s.set_positions(th))
        refused(kmc, "ERR_BAD_ARG", not_set, lambda: s.run(1))
    with kmc.Sampler(kmc.Exponential(), 64, 2, G, NBURN, 1, 2.0, SEED, betas=LADDER3) as s:
        th = theta0(64, 2, 3)
        s.set_positions(th)
        th[1, 7, 0] = -1.0
        refused(kmc, "ERR_NONFINITE_LOGP", "walker 7 of rung 1 has a non-finite initial log-pdf", lambda: s.set_positions(th))
        refused(kmc, "ERR_BAD_ARG", not_set, lambda: s.run(1))
        th[1, 7, 0], th[0, 9, 0] = 1.0, -1.0
        refused(kmc, "ERR_NONFINITE_LOGP", "walker 9 has a non-finite initial log-pdf", lambda: s.set_positions(th))
        refused(kmc, "ERR_BAD_ARG", not_set, lambda: s.run(1))


# id -> sha256 of the row's read-out, recorded before kmc_state.hip was reordered
EXPECTED = {
    "gen_fold_L8_64x32": "85d14d07dc5a46431c6036e98a8f511459a5738f18ca51586c5d0677665e035d",
    "gen_fold_L16_66x64": "038c6058230572ae4fa9508336ab6f38d6638424e657ac01461d4fab03f77172",
    "gen_fold_L32_130x128": "39a244e24454a2fc55cec40f368de4396d62f903ce527d10b01d69600c96b1a8",
    "gen_fold_odd_66x31": "f5311f29d082f188126340213cdd2195a09b304134508d66df760f7e58887b47",
    "gen_striped_64x16": "f1aba91e1d2a2dc18d3bc0f0177a85506e9d8db9483b5c11017a45677465bf62",
    "gen_lane_64x4": "d956cef90d459100005011f43827d49b6304d077eef92b2216b9a8a3aaa63f50",
    "gen_lane_odd_66x3": "adf3aabc763bc436362802afd55314a935838940d4c89c79c1afa0edc4caf5a0",
    "gen_fold_then_halves_64x32": "d9dbb746c0e738be8dd4afecc5a244ca32e169579634115bb48858cf27244303",
    "gen_lane_then_halves_64x4": "79b7a658b3108c3d7675214ffd9f1733a5443602b10805b2f0abd0ba898e5c56",
    "islands_256x8": "63975aa3030cd0391b7137f3547532cb86f45e85e3e73527627ed675646500ae",
    "resident_lane_64x4": "d956cef90d459100005011f43827d49b6304d077eef92b2216b9a8a3aaa63f50",
    "resident_pair_64x16": "7cb77626a23d8b7f0a26ebbac0c697f858e492c25de26fb4a2813c20d7cd03d1",
    "two_fold_L8_64x32": "ace3fd06a1d59624fb54e5db09e995cc554b81b113395a09ec4f03da8d0e0bc8",
    "two_fold_L16_66x64": "176f90f99501c527eb575261bc4b0f49ea93ae769d16329fe85e4581d3ca6c21",
    "two_fold_L32_130x128": "60ff58b65c895d96024bbba082ed2a432beddcf8f7a971fb83d9d468434b6eac",
    "two_fold_f32_64x32": "a751b46e9d6229fef1420b7301612e8de67642c67d488a6465918c6816e33c02",
    "two_plain_K1_64x4": "e7cfa14559e91f097b55bb678e1c6e386ea0c94d4d48b0e2025fd41a5b154f1a",
    "two_plain_L4K2_66x15": "cc15e2ebc2bd843ac7d514d36072d44a5d97cd080ec5f07eddc8bfb5c4244917",
    "two_plain_L64_ring_258x256": "fe7dcdb3add3ff4d18180e329c04ad520bf8c30afaf1c22001816a2c68518ba3",
    "staged_tile_64x4": "20372beb874622954d4bbfc58becb332b02132ff327f4786a022f9ea958ba520",
    "staged_columns_64x6": "6c71c26771057c75f557af650836fd081e4628306d022a66192630022af0dbb8",
    "generic_64x4": "0bad4b4e4af41a1794e1165d1a09bda756d7c6c05781f7db0997596e0cd81547",
    "set_positions": "d956cef90d459100005011f43827d49b6304d077eef92b2216b9a8a3aaa63f50",
    "set_positions_two_launch_66x15": "cc15e2ebc2bd843ac7d514d36072d44a5d97cd080ec5f07eddc8bfb5c4244917",
    "init_ball_menu": "0360e475c08ca7fcc3c28b28f5cff1500197b483d857132c9798f880a86da161",
    "init_ball_user": "0360e475c08ca7fcc3c28b28f5cff1500197b483d857132c9798f880a86da161",
    "init_ball_f32": "078a3195a15c87497adfbf16f6fc13361891efa690c315e5940d121b2533eaf8",
    "init_ball_dealt": "5997f8d69ec20cc0c5610a1622af12b9cca44ad8656e6aa2979cd78684fdeb41",
    "set_state": "967e184daf7a3a6bec2b3df157e75a6cb9b81c3f0e962f8d4a8ef4d90a55ef59",
    "set_state_no_naccept": "6bc11360955cce7e157e9daf4e0f3209707e0ca8d3a428e95344b9d2e729e2c5",
    "set_state_blobs": "5614cb9f1ce46751feedf381b88e7c5cb60e638ff3f4204a660dc8e7bdb29892",
    "set_state_moments": "8547cf941996fa4df5ed70eaa939217a74c68ced7dfe1134e1a7dd4013b9c359",
    "set_state_moments_two_launch": "2394d056b084252caa29c28eabc8af3e3ebfaec3ca6dca22a9e7136b98ac08c6",
    "set_walker_ids_dealt": "a703cd7b628641d91e89a981ce97a82769ec5bef60ca676850c619720bd917f6",
    "rung_positions_whole": "cf92c1c03d89e999fa0d0e70b780fa2dc0045e62278bc617b1578bfb7530ad0f",
    "rung_positions_likelihood": "3e04151fea2794fcdebdf30b40c7474c7eb6ae878ce0d982d72f61b6c3e8256a",
    "rung_positions_adapt": "2fc1eff8d6c7f8e2c6d551625a71909a91d13785e227a4af3bfc7e0bf8fe10de",
    "rung_checkpoint_whole": "f462a8bec0b81eafdf19020467a8459436a05bd16cb66f19f687e57c13b56e56",
    "rung_checkpoint_likelihood": "7224c43f51a0e5a8140592085b33e0fa56f42e85329a6f54bc93cf0ee8fa8f5f",
    "rung_checkpoint_adapt": "c344dd1e72a4941ffa6a96d20e614f2971bd5e7770ef1f5a93264123103c3619",
    "rung_replicated_whole": "f462a8bec0b81eafdf19020467a8459436a05bd16cb66f19f687e57c13b56e56",
    "rung_replicated_likelihood": "7224c43f51a0e5a8140592085b33e0fa56f42e85329a6f54bc93cf0ee8fa8f5f",
    "tempered_moments": "f462a8bec0b81eafdf19020467a8459436a05bd16cb66f19f687e57c13b56e56",
}
