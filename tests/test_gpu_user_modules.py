"""GPU: the program text of every runtime-compiled module, pinned from outside.  A module's code object is cached on disk under a
hash of its text, its headers and its options, so equal text means the same kernels, the same results and the same speed -- and a
slip where the samplers meet the run-time compiler (a wrong kernel, a stale module) shows as another text or as a text that is
missing.  Under KMC_DEBUG=rtc-text=<dir> the library writes every text that asks for a compile into <dir>.  Each row of the table
below makes a FRESH density (a code object the density already holds never reaches the compiler), creates one small sampler at the
smallest shape on one side of a decision, checks that describe() names the route the row claims, runs 8 generations and compares a
sha256 over the dumped texts, sorted by content, with the recorded one.  The digests were recorded from the library while
compile_user still took fifteen positional arguments, in two processes that agreed, and hold unchanged after it takes a
UserModuleSpec: a row that differs means some caller now asks for another program.  A fresh density per row cannot see the
in-memory key merge two programs, so a second table (REUSE_ROWS) runs ONE density at two row lengths and compares the second run
with a fresh density's."""
import hashlib
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G, NBURN, NRUN, SEED = 16, 8, 8, 5

TERM = ("-0.5*x*x",)
ROSEN_TERM = ("d < n-1 ? -((p[0]-x)*(p[0]-x))/p[2] : 0.0", "-(p[1]*((y-x*x)*(y-x*x)))/p[2]", [1.0, 100.0, 20.0])
# a coupling through the mean: no sum over elements, evaluated per walker as written
BODY = ("double m = 0.0; for (int i = 0; i < n; ++i) m += x[i]; m = m / n; double s = 0.0; "
        "for (int i = 0; i < n; ++i) { double t = x[i] - m; s += t * t; } return -0.5 * s - 0.5 * p[0] * m * m;")
SUM_BODY = "double s = 0.0; for (int i = 0; i < n; ++i) { double t = (x[i] - p[0]) * p[1]; s += t * t; } return -0.5 * s;"
TWO_SUMS_BODY = "double s = 0.0, t = 0.0; for (int i = 0; i < n; ++i) { s += x[i] * x[i]; t += x[i]; } return -0.5 * (s + p[0] * t * t);"
BLOB_BODY = "double s = 0.0; for (int i = 0; i < n; ++i) s += x[i] * x[i]; blob[0] = x[0]; blob[1] = s; return -0.5 * s;"
REG_TERM = "double mu = x[0]; for (int k = 1; k < n; ++k) mu += x[k] * d[k - 1]; double r = d[n - 1] - mu; return -0.5 * p[0] * r * r;"
GAUSS_PRIOR = "double s = 0.0; for (int k = 0; k < n; ++k) s += x[k] * x[k]; return -0.5 * s;"
LADDER3 = [1.0, 0.5, 0.25]


def fresh_density(kmc, name, nd):
    if name == "term":
        return kmc.ExprDensity(*TERM)
    if name == "termpair":
        return kmc.ExprDensity(*ROSEN_TERM)
    if name == "body":
        d = kmc.CDensity(BODY, params=[4.0])
        assert not d.separable
        return d
    if name in ("sumbody", "twosums"):
        d = kmc.CDensity(SUM_BODY, params=[0.0, 1.0]) if name == "sumbody" else kmc.CDensity(TWO_SUMS_BODY, params=[0.3])
        assert d.separable
        return d
    if name == "blobbody":
        return kmc.CDensity(BLOB_BODY, nblob=2)
    if name == "data":
        return kmc.DataDensity(REG_TERM, np.random.default_rng(1).standard_normal((50, nd)), prior=GAUSS_PRIOR, params=[1.0])
    raise KeyError(name)


def moves(kmc, name):
    return {"de": lambda: kmc.DEMove(), "snooker": lambda: kmc.DESnookerMove(),
            "mix": lambda: [(kmc.DEMove(), 0.5), (kmc.DESnookerMove(), 0.5)]}[name]()


GENERIC = {"KMC_PLAN": "generic"}       # (an option in capitals is an environment variable of its own, the others go into KMC_DEBUG)
TWO = {"fused": "0"}                    # the two-launch kernels where one launch per generation would be chosen

# (id, density, nwalkers, ndim, Sampler keywords, options, what describe() must say)
ROWS = [
    # a term density: resident
    ("term_lane_64x4", "term", 64, 4, {}, {}, ["resident mode", "one walker per thread"]),
    ("term_lane_f32_100x1", "term", 100, 1, dict(dtype="f32"), {}, ["resident mode", "one walker per thread", "KMC_F32"]),
    ("term_lane2_1026x4", "term", 1026, 4, {}, {}, ["resident mode", "two walkers per thread"]),
    ("term_pair_ragged_64x12", "term", 64, 12, {}, {}, ["resident mode", "rows 2 lanes x 4 chunks"]),
    ("term_pair_64x16", "term", 64, 16, {}, {}, ["resident mode", "rows 2 lanes x 4 chunks"]),
    ("termpair_islands_256x4", "termpair", 256, 4, dict(island_gens=32, island_size=128), {}, ["island mode: 2 islands of 128", "rows 2 lanes x 1 chunks"]),
    ("termpair_islands_ragged_512x5", "termpair", 512, 5, dict(island_gens=32, island_size=256), {}, ["island mode: 2 islands of 256", "rows 2 lanes x 2 chunks"]),
    # ... one launch per generation
    ("term_gen_lane_4096x2", "term", 4096, 2, {}, {}, ["generation_lane ND=2"]),
    ("term_gen_quad_4096x6", "term", 4096, 6, {}, {}, ["generation_group L=4 K=1"]),
    ("term_gen_striped_4096x16", "term", 4096, 16, {}, {}, ["generation_group L=4 K=2"]),
    # ... two launches
    ("term_vec_4096x16", "term", 4096, 16, {}, TWO, ["half_step_vec L=4 K=2 ITER=1 exact-size"]),
    ("term_vec_ragged_4096x13", "term", 4096, 13, {}, TWO, ["half_step_vec L=4 K=2 ITER=1 ragged"]),
    ("term_vec_f32_64x16", "term", 64, 16, dict(dtype="f32"), {}, ["half_step_vec L=4 K=2", "KMC_F32"]),
    ("term_generic_64x4", "term", 64, 4, {}, {"no-resident": None, **GENERIC}, ["half_step_generic"]),
    ("term_p2p_vec_4096x16", "term", 4096, 16, dict(p2p=True), {}, ["half_step_vec L=4 K=2", "P2P shard 0/1"]),
    ("term_p2p_generic_64x4", "term", 64, 4, dict(p2p=True), GENERIC, ["half_step_generic", "P2P shard 0/1"]),
    # a body density
    ("body_lane_200x4", "body", 200, 4, {}, {}, ["resident mode", "(256 threads)", "one walker per thread"]),
    ("body_lane_400x4", "body", 400, 4, {}, {}, ["resident mode", "(448 threads)", "one walker per thread"]),
    ("body_lane_1000x4", "body", 1000, 4, {}, {}, ["resident mode", "(1024 threads)", "one walker per thread"]),
    ("body_lane_f32_64x4", "body", 64, 4, dict(dtype="f32"), {}, ["resident mode", "one walker per thread", "KMC_F32"]),
    ("body_lane2_1500x4", "body", 1500, 4, {}, {}, ["resident mode", "two walkers per thread"]),
    ("body_gen_lane_4096x4", "body", 4096, 4, {}, {}, ["generation_lane ND=4", "function body, evaluated as written"]),
    ("body_staged_4096x4", "body", 4096, 4, {}, {"fused": "0", "no-body-vec": None}, ["half_step_staged"]),
    ("body_generic_4096x4", "body", 4096, 4, {}, {"no-body-vec": None, **GENERIC}, ["half_step_generic"]),
    ("body_vec_4096x16", "body", 4096, 16, {}, {}, ["half_step_vec L=4 K=2", "the body evaluated per walker on the whole proposal"]),
    ("blobbody_64x2", "blobbody", 64, 2, {}, {}, ["resident mode", "one walker per thread", "with a blob of 2 doubles"]),
    # ... recognised as a sum over elements
    ("sumbody_gen_4096x16", "sumbody", 4096, 16, {}, {}, ["generation_group L=4 K=2", "recognised as a sum over elements"]),
    ("sumbody_vec_4096x16", "sumbody", 4096, 16, {}, TWO, ["half_step_vec L=4 K=2", "recognised as a sum over elements"]),
    ("twosums_vec_4096x16", "twosums", 4096, 16, {}, TWO, ["half_step_vec L=4 K=2", "recognised as a sum over elements"]),
    # the other moves, rows lane-striped and one walker per lane
    ("de_vec_64x4", "term", 64, 4, dict(move="de"), {}, ["half_step_vec L=2 K=1", "kernel half_step_de_vec"]),
    ("de_generic_64x4", "term", 64, 4, dict(move="de"), GENERIC, ["half_step_generic", "kernel half_step_de_generic"]),
    ("snooker_vec_64x4", "term", 64, 4, dict(move="snooker"), {}, ["half_step_vec L=2 K=1", "kernel half_step_snooker_vec"]),
    ("snooker_generic_64x4", "term", 64, 4, dict(move="snooker"), GENERIC, ["half_step_generic", "kernel half_step_snooker_generic"]),
    ("mix_vec_64x4", "term", 64, 4, dict(move="mix"), {}, ["half_step_vec L=2 K=1", "kernel half_step_mix_vec"]),
    ("mix_generic_64x4", "term", 64, 4, dict(move="mix"), GENERIC, ["half_step_generic", "kernel half_step_mix_generic"]),
    # tempered ladders
    ("temper_vec_64x4", "term", 64, 4, dict(betas=LADDER3), {}, ["half_step_vec L=2 K=1", "kernel half_step_temper_vec"]),
    ("temper_generic_64x4", "term", 64, 4, dict(betas=LADDER3), GENERIC, ["half_step_generic", "kernel half_step_temper_generic"]),
    ("temper_de_vec_64x4", "term", 64, 4, dict(betas=LADDER3, move="de"), {}, ["kernel half_step_de_vec", "kernel half_step_temper_vec"]),
    ("temper_de_generic_64x4", "term", 64, 4, dict(betas=LADDER3, move="de"), GENERIC, ["kernel half_step_de_generic", "kernel half_step_temper_generic"]),
    ("temper_mix_vec_64x4", "term", 64, 4, dict(betas=LADDER3, move="mix"), {}, ["kernel half_step_mix_vec", "kernel half_step_temper_vec"]),
    ("temper_mix_generic_64x4", "term", 64, 4, dict(betas=LADDER3, move="mix"), GENERIC, ["kernel half_step_mix_generic", "kernel half_step_temper_generic"]),
    ("temper_vec_ragged_64x13", "term", 64, 13, dict(betas=LADDER3), {}, ["half_step_vec L=4 K=2 ITER=1 ragged", "kernel half_step_temper_vec"]),
]

# (id, density, nchains, ndim, options, the kernel the module must hold)
METROPOLIS_ROWS = [
    ("metropolis_register_512x2", "term", 512, 2, {"metro-table": "0"}, "kmc::metropolis_chains_body<UD, 2>"),
    ("metropolis_memory_512x2", "body", 512, 2, {"metro-table": "0"}, "kmc::metropolis_chains_any_body<UD>"),
    ("metropolis_tabled_64x3", "term", 64, 3, {}, "kmc::metropolis_chains_tabled_body<UD, 4>"),
]

# every kmc::<name>_body the emitters of kmc_rtc.hip and kmc_metropolis_api.hip can name: the rows above reach them all
BODIES = {
    "half_step_generic", "half_step_mix_generic", "logpdf_rows", "init_ball", "half_step_staged", "half_step_vec", "half_step_mix_vec",
    "resident_lane", "resident_lane2", "resident", "island_epoch", "generation_lane", "generation_group",
    "metropolis_chains", "metropolis_chains_any", "metropolis_chains_tabled",
}
_bodies = {}        # row id -> the kmc::<name>_body names in the texts it dumped


def set_options(kmc_debug, monkeypatch, dump, opts):
    if not hasattr(kmc_debug, "base"):
        kmc_debug.base = dict(kmc_debug.opts)                # (options the whole run was started with stay)
    kmc_debug.opts = dict(kmc_debug.base)
    monkeypatch.delenv("KMC_DEBUG", raising=False)           # (the fixture keeps a `no-resident` it finds there: an earlier row's, in the last test)
    monkeypatch.delenv("KMC_PLAN", raising=False)
    kmc_debug.set("geometry")
    kmc_debug.set("rtc-text", str(dump))
    for k, v in opts.items():
        if k.isupper():
            monkeypatch.setenv(k, v)
        else:
            kmc_debug.set(k, v)


def dumped(dump, row_id):
    """(sha256 over the texts in `dump`, sorted by content; the texts)"""
    texts = sorted(open(os.path.join(dump, f), "rb").read() for f in os.listdir(dump))
    _bodies[row_id] = {name for t in texts for name in re.findall(r"kmc::(\w+)_body<", t.decode())}
    return hashlib.sha256(b"\0".join(texts)).hexdigest(), texts


def sampler_row(kmc, kmc_debug, monkeypatch, dump, row):
    name, dens, nw, nd, kw, opts, says = row
    set_options(kmc_debug, monkeypatch, dump, opts)
    kw = dict(kw)
    if "move" in kw:
        kw["move"] = moves(kmc, kw["move"])
    th = 0.5 + 0.1 * np.abs(np.random.default_rng(0).standard_normal((nw, nd)))
    with kmc.Sampler(fresh_density(kmc, dens, nd), nw, nd, G, NBURN, 1, 2.0, SEED, **kw) as s:
        how = s.describe()
        s.set_positions(th)
        s.run(NRUN)
        s.sync()
    for words in says:
        assert words in how
    return {name: dumped(dump, name)[0]}


def data_row(kmc, kmc_debug, monkeypatch, dump):
    """The sampler's module, then the pointwise module that one `waic` and one `loo` call share."""
    nw, nd = 64, 3
    set_options(kmc_debug, monkeypatch, dump, {})
    th = 0.1 * np.random.default_rng(0).standard_normal((nw, nd))
    got = {}
    with kmc.Sampler(fresh_density(kmc, "data", nd), nw, nd, G, NBURN, 1, 2.0, SEED, store_chain=True, store_logp=True) as s:
        assert "data density (exact)" in s.describe() and "data_partial_obs" in s.describe()
        s.set_positions(th)
        s.run(G)
        s.sync()
        got["data_64x3"], texts = dumped(dump, "data_64x3")
        assert not any(b"kmc_pw::" in t for t in texts)
        s.waic()
        got["data_64x3_waic"], texts = dumped(dump, "data_64x3")
        assert any(b"kmc_pw::pw_partials<UserData, 3, 3, 1, false>" in t for t in texts)
        assert s.loo()["n"] == 8 * nw
        got["data_64x3_loo"], _ = dumped(dump, "data_64x3")
    return got


def logpdf_row(kmc, kmc_debug, monkeypatch, dump):
    """The stateless evaluation of rows: the log-pdf module at the rows' ndim (a body's is compiled for its ndim), and its blob form."""
    set_options(kmc_debug, monkeypatch, dump, {})
    body, blob = fresh_density(kmc, "body", 5), fresh_density(kmc, "blobbody", 3)
    assert np.isfinite(body(np.full(5, 0.25)))
    lp, bl = blob.eval_with_blobs(np.full((3, 3), 0.5))
    assert lp.shape == (3,) and (bl[:, 0] == 0.5).all()
    got, texts = dumped(dump, "logpdf_rows")
    assert any(b"kmc::BodyDensity<UserB, 5>" in t for t in texts) and any(b"kmc::BodyBlobDensity<UserB, 3, 2>" in t for t in texts)
    return {"logpdf_rows": got}


def metropolis_row(kmc, kmc_debug, monkeypatch, dump, row):
    from kissmcmc_jl_amd.metropolis import run_chains
    name, dens, nc, nd, opts, kernel = row
    set_options(kmc_debug, monkeypatch, dump, opts)
    th = 0.1 * np.random.default_rng(2).standard_normal((nc, nd))
    r = run_chains(fresh_density(kmc, dens, nd), kmc.GaussianStep(0.5), th, 16, 8, 1, 11)
    assert r["nsamples"] == 8 and r["naccept"].sum() > 0
    got, texts = dumped(dump, name)
    assert any(kernel.encode() in t for t in texts)
    assert any(b"metropolis_chains_tabled_body" in t for t in texts) == ("tabled" in name)
    return {name: got}


# id -> sha256 over the texts the row has sent to the compiler, sorted by content
EXPECTED = {
    'term_lane_64x4': '495b629f0cac0351a980b732dd4db10f9e7be8a359fba86ad67ddf2abfb9e9b2',
    'term_lane_f32_100x1': '471093cdf869e32205e72a342d30e716d35a7dd3a30e7323768ff5c3c12de014',
    'term_lane2_1026x4': 'cbbcd45413dddf4335380eb8476e5ac42f00ae29fc65847f38a42758a263238e',
    'term_pair_ragged_64x12': '2691b5134d3370dede8cb8c1c944e116972be2246d85c57f206db7a8536bafdb',
    'term_pair_64x16': '84937aaeb544e3b16761827e7d73a9c268b3271fc90e9b99923db46b10abf8c4',
    'termpair_islands_256x4': '58ed890ab5a82b8369cd12b4eb78bb6280500d3e43fbc3fd64735ad4a6bda209',
    'termpair_islands_ragged_512x5': '80dc58a780c36ca2af3f32e645eeb39b74e0731b60fd1e2248abcc7b052fa547',
    'term_gen_lane_4096x2': '543cca50a21ab70fd73e4468f241327c1ede9b76b1a15acf7d8c2a8822d5937b',
    'term_gen_quad_4096x6': 'b371ff3a72a90da1a308a084e79e1290b6c46a3472cfb09694018cc5eb8c5d3e',
    'term_gen_striped_4096x16': '6d8574172f598f8b2f4de5fb0f56dcb4858dfa8cc4b2977f362cf50199ef89db',
    'term_vec_4096x16': '9d07635a7abe067e2feab3ceeda7edfaf7a9ed5d5ae1ca253b6dd1ae2a18d111',
    'term_vec_ragged_4096x13': 'b5017a1c6f16e9d1211a169a9649672f014256cc4ee09abfb94a96a673bd4960',
    'term_vec_f32_64x16': 'f748ee3abc63c5dd4efae955226e9b503cc3295ace8c677f1f93e6d08c2b485f',
    'term_generic_64x4': '978c9cc4201998bfcefc1c3bb40bbf5a1b393503f6ff83ca55f71d19472ea755',
    'term_p2p_vec_4096x16': '3607b182693eed4b2a7b88b9c83dd9403505dc0666985886e3758d24840137c8',
    'term_p2p_generic_64x4': '8dcfc18b838c6843bab4c44cee3212dcfcb90494fdb7f91138cf60279d92a992',
    'body_lane_200x4': '03a01b365789f8a718071eb4fb768f2dabe4d0c49c0f6131c36b71fa9de5a123',
    'body_lane_400x4': '66f493bdf38aa37196d6969cd6a6532af8ad4497bcb15d649dc12d58ea1dc46c',
    'body_lane_1000x4': '4ee3b3a5cb9e81b7821ba6473e744d8e60919f6f7beac9037d25b2b51e0d68f7',
    'body_lane_f32_64x4': 'c996751df85db1e2a1abcc23770bcda3c2ebc543d20aa0e03e69a0b12bf1d249',
    'body_lane2_1500x4': '3bd3abd1f3f4173845728669f550a03d0dc7e451517b1a5f158bcb4f65e833f5',
    'body_gen_lane_4096x4': '4de4db6b196cae36aaee39590920d34745142adffa918023d2ccf830159009f0',
    'body_staged_4096x4': '74671be79ad68870697f4fea5b7a20c6cd68356d29cc3724fbbd40bcbc9535d0',
    'body_generic_4096x4': 'ecfe1d48bcdbf3bde95b6f2852e3c997ba72615d61d95a555abb1bc027c3bc17',
    'body_vec_4096x16': 'e2e08a90dea949d9a7e0ef1801059d62643195b28e9fd3e9967d012cb86632d8',
    'blobbody_64x2': '029a535bfdab8cffa4fe9ac0957f75fcb0f5fd2e6494aa53470b0d5b1f38350c',
    'sumbody_gen_4096x16': 'd470cc049a8407e0f3d1403abb0a51d57944ce6c4218c4aeb74d994d6c7e1a95',
    'sumbody_vec_4096x16': '7cb07d7ac073069af19e37a91a80acf592f1f5a8a904b011b0e194ad99c5f866',
    'twosums_vec_4096x16': '1202ad8b8cb0a896372e601bf73df755e81dddce1142d5dae5fe1928c68cc4fc',
    'de_vec_64x4': 'eb15077e90c79daf75b075c35539889c19afcbef453e85ae03c7de0ed2714781',
    'de_generic_64x4': 'ef858c53da21132603fbc3bbcf9a6b9b81fd33d1b2e4446cf9802473ed05a3b3',
    'snooker_vec_64x4': 'f788a3e9ae238f5c554448e20b6bbcdcaad0ae159b88dde31f7ebb6c053089a7',
    'snooker_generic_64x4': '62a4b1ca31ae454685f6424f57d7ba65ff82959af9b62880d2a86257d6b5b962',
    'mix_vec_64x4': 'c9052e28a7c353eecdc01612f5fc7148784209f1d8d113f8f3843cd344ef9f35',
    'mix_generic_64x4': 'a52b426dd511ed8d7d142d482f7334e5e1dc64900b44c7e7541ab5896f9d967b',
    'temper_vec_64x4': 'ed6ec29cd8415744182383a730f5abf47fb7ca4afc2b70621c63c45f8a0b7e94',
    'temper_generic_64x4': 'dcf4be6be3e36bc9b2ddf6f6d1c244af0270b40f2d65ff303ab73c2b5dbd9428',
    'temper_de_vec_64x4': 'c4670751f8f1eb636554b4c9ade11eb076dad1794b1590b756f4c85001d12178',
    'temper_de_generic_64x4': 'a319db8221368f49af0d3c9b721c4cad6eb385c501b9f1e7ba572a11d89c53b9',
    'temper_mix_vec_64x4': '21bc219438ec834f4a816c5265990c1c2a7425ad4a7c42c229723775d7deb41a',
    'temper_mix_generic_64x4': '53c4d3eee4da93a9f828daa60166ec607b6fa2246c39b001c84fdc2c8108cc38',
    'temper_vec_ragged_64x13': 'c9afebda0767ff0f7fdea1cc3cbd314e703cc70c11cf8c4d7c1d34e0f4e5d5ed',
    'data_64x3': '6871cc2e804574040c175aca28571853bed4b546fdb2b6bcf66f836fe1665309',
    'data_64x3_waic': '803472da158cae0e9d7f79be925fbcc1fdb056c60b420c87a925a43cc256f06a',
    'data_64x3_loo': '803472da158cae0e9d7f79be925fbcc1fdb056c60b420c87a925a43cc256f06a',
    'logpdf_rows': '34174ef584d949c810d4f8e2206b09c43fae264a6a19f06ee6138d142024dc7f',
    'metropolis_register_512x2': 'c81115665d78a1cfa684dd9cc6d510f745e5b1a2b5006b5322803e6be5537b68',
    'metropolis_memory_512x2': '1eed664c5825ad3e886a14d26c4b09e7e811a4e72bf9a757e221e61bbe1e45d4',
    'metropolis_tabled_64x3': '676d8b9f411e7494a2f298ae26cedad4b97bb003ca3c8ffecc0c6f8463126c01',
}


def check(got):
    assert got == {k: EXPECTED.get(k) for k in got}, "".join(f"\n    '{k}': '{v}'," for k, v in got.items())


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_a_sampler_asks_for_the_program_it_asked_for(kmc, kmc_debug, monkeypatch, tmp_path, row):
    check(sampler_row(kmc, kmc_debug, monkeypatch, tmp_path, row))


def test_a_data_density_asks_for_the_programs_it_asked_for(kmc, kmc_debug, monkeypatch, tmp_path):
    check(data_row(kmc, kmc_debug, monkeypatch, tmp_path))


def test_logpdf_rows_ask_for_the_log_pdf_module(kmc, kmc_debug, monkeypatch, tmp_path):
    check(logpdf_row(kmc, kmc_debug, monkeypatch, tmp_path))


@pytest.mark.parametrize("row", METROPOLIS_ROWS, ids=[r[0] for r in METROPOLIS_ROWS])
def test_metropolis_asks_for_the_program_it_asked_for(kmc, kmc_debug, monkeypatch, tmp_path, row):
    check(metropolis_row(kmc, kmc_debug, monkeypatch, tmp_path, row))


# One density object over two shapes whose programs differ in the row length alone: the second sampler must not be handed the first
# one's code object.  (density, first shape, second shape, options, a kernel only the second shape's text holds, or None where the two
# shapes may rightly share a text)
REUSE_ROWS = [
    ("term_gen_lane_9000x5_x6", "term", (9000, 5), (9000, 6), {}, "kmc::generation_lane_body<UD, 6>"),      # beyond the quad's 8 192 walkers
    ("term_gen_forced_lane_4096x6_x7", "term", (4096, 6), (4096, 7), {"fused": "lane"}, "kmc::generation_lane_body<UD, 7>"),
    ("term_lane2_1026x3_x4", "term", (1026, 3), (1026, 4), {}, "kmc::resident_lane2_body<UD, 4>"),
    ("term_lane_64x4_x5", "term", (64, 4), (64, 5), {}, None),
    ("term_pair_64x12_x16", "term", (64, 12), (64, 16), {}, "kmc::resident_body<UD, 4, false>"),
    ("term_vec_4096x13_x16", "term", (4096, 13), (4096, 16), TWO, "kmc::half_step_vec_body<UDV, 4, 2, 1, false, false, double>"),
    ("body_lane_200x4_x5", "body", (200, 4), (200, 5), {}, "kmc::resident_lane_body<UD, 5, true, double>"),
    ("body_gen_lane_4096x4_x5", "body", (4096, 4), (4096, 5), {}, "kmc::generation_lane_body<UD, 5>"),
]


@pytest.mark.parametrize("row", REUSE_ROWS, ids=[r[0] for r in REUSE_ROWS])
def test_a_density_used_again_at_another_row_length_gets_its_own_program(kmc, kmc_debug, monkeypatch, tmp_path, row):
    """The in-memory key of a density's code objects must never merge two specs whose texts differ: the density that has run the first
    shape runs the second exactly as a fresh density does, and where the second shape's text differs it reaches the compiler."""
    _, dens, first, second, opts, kernel = row
    set_options(kmc_debug, monkeypatch, tmp_path, opts)

    def run(d, shape):
        nw, nd = shape
        th = 0.5 + 0.1 * np.abs(np.random.default_rng(0).standard_normal((nw, nd)))
        with kmc.Sampler(d, nw, nd, G, NBURN, 1, 2.0, SEED) as s:
            how = s.describe()
            s.set_positions(th)
            s.run(NRUN)
            s.sync()
            return how, s.positions(), s.logp(), s.naccept(), th

    shared = fresh_density(kmc, dens, first[1])
    run(shared, first)
    before = set(os.listdir(tmp_path))
    got = run(shared, second)
    new_texts = [open(os.path.join(tmp_path, f), "rb").read() for f in sorted(set(os.listdir(tmp_path)) - before)]
    if kernel is not None:
        assert any(kernel.encode() in t for t in new_texts)
    want = run(fresh_density(kmc, dens, second[1]), second)
    assert got[0] == want[0]
    assert (got[1] != got[4]).any(axis=0).all()                             # (every coordinate moves; the counters restart after burn-in)
    for g, w in zip(got[1:4], want[1:4]):
        np.testing.assert_array_equal(g, w)


def test_the_rows_reach_every_emitter_branch(kmc, kmc_debug, monkeypatch, tmp_path):
    """The union of the bodies named in every row's texts is the full list: a later emitter branch cannot go unpinned.  (Rows that have
    not run in this process yet -- this test alone, or in another order -- run here first.)"""
    def dump_of(name):
        os.mkdir(tmp_path / name)
        return tmp_path / name
    for row in ROWS:
        if row[0] not in _bodies:
            sampler_row(kmc, kmc_debug, monkeypatch, dump_of(row[0]), row)
    for row in METROPOLIS_ROWS:
        if row[0] not in _bodies:
            metropolis_row(kmc, kmc_debug, monkeypatch, dump_of(row[0]), row)
    if "data_64x3" not in _bodies:
        data_row(kmc, kmc_debug, monkeypatch, dump_of("data_64x3"))
    if "logpdf_rows" not in _bodies:
        logpdf_row(kmc, kmc_debug, monkeypatch, dump_of("logpdf_rows"))
    assert set().union(*_bodies.values()) == BODIES
