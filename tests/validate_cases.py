"""kmc_validate without a device: one `config` / `validate` pair for the CPU tests, and the fixed list of configurations whose
(status, message) tests/golden/validate_matrix.json records (tests/golden/make_validate_matrix.py writes it,
tests/test_validate_matrix_cpu.py compares).  kmc_validate touches no device, and neither does making the runtime-compiled handles
(their text is compiled for gfx950 when they are made; nothing is loaded before a sampler is created)."""
import ctypes as C
import itertools

import numpy as np

REG_TERM = "double r = d[0] - x[0] * d[1] - x[1] * d[2]; return -0.5 * p[0] * r * r;"
BODY = "double s = 0.0; for (int i = 0; i < n; ++i) { double t = (x[i] - p[0]) * p[1]; s += t * t; } return -0.5 * s;"
BLOB_BODY = "double s = 0.0; for (int i = 0; i < n; ++i) s += x[i] * x[i]; blob[0] = s; blob[1] = x[0]; return -0.5 * s;"


def config(**kw):
    """A kmc_config that kmc_validate accepts (a standard normal, 256 walkers x 3 dimensions, one shard), then `kw` field by field;
    betas=[...] sets betas and ntemps (ntemps=... after it overrides the count).  Returns (config, what it points to)."""
    from kissmcmc_jl_amd import _lib
    c = _lib.Config()
    c.dtype, c.density = _lib.F64, _lib.GAUSSIAN_ISO
    c.params[0], c.params[1] = 0.0, 1.0
    c.nwalkers, c.ndim, c.ngenerations, c.nburnin, c.nthin = 256, 3, 10, 0, 1
    c.a_scale, c.shard_count = 2.0, 1
    kw = dict(kw)
    keep = None
    betas = kw.pop("betas", None)
    if betas is not None:
        keep = (C.c_double * len(betas))(*betas)
        c.betas, c.ntemps = C.cast(keep, C.c_void_p), len(betas)
    params = kw.pop("params", None)
    if params is not None:
        for i, v in enumerate(params):
            c.params[i] = v
    for k, v in kw.items():
        setattr(c, k, v)
    return c, keep


def validate(**kw):
    """(status, kmc_last_error() when refused else "") of kmc_validate on config(**kw)."""
    from kissmcmc_jl_amd import _lib
    L = _lib.lib()
    c, keep = config(**kw)
    st = L.kmc_validate(C.byref(c))
    del keep
    return st, L.kmc_last_error().decode() if st else ""


def validate_null():
    from kissmcmc_jl_amd import _lib
    L = _lib.lib()
    st = L.kmc_validate(None)
    return st, L.kmc_last_error().decode() if st else ""


class Densities:
    """The handles the list points to, alive as long as this object."""

    def __init__(self, kmc):
        from kissmcmc_jl_amd import _lib
        self.data = kmc.DataDensity(REG_TERM, np.zeros((8, 3)), params=[1.0])
        self.body = kmc.CDensity(BODY, params=[0.0, 1.0])
        self.blob = kmc.CDensity(BLOB_BODY, nblob=2)
        self.callback = _lib.HOST_LOGPDF_FN(lambda rows, n, nd, out, user: 0)
        self.host_fn = C.cast(self.callback, C.c_void_p)

    def kinds(self):
        from kissmcmc_jl_amd import _lib
        return dict(menu=dict(),
                    data=dict(density=_lib.DATA_DENSITY, user_density=self.data.user_handle),
                    body=dict(density=_lib.USER_DENSITY, user_density=self.body.user_handle),
                    blob=dict(density=_lib.USER_DENSITY, user_density=self.blob.user_handle),
                    host=dict(density=_lib.HOST_DENSITY, host_logpdf=self.host_fn))


LADDER = [1.0, 0.5, 0.25]


def _moves(_lib):
    return dict(stretch=dict(), de=dict(move=_lib.MOVE_DE), snooker=dict(move=_lib.MOVE_SNOOKER),
                mix=dict(move=_lib.MOVE_MIX, mix_count=2, mix_move0=_lib.MOVE_DE, mix_move1=_lib.MOVE_SNOOKER, mix_weight0=1.0, mix_weight1=3.0))


def product_cases(dens):
    """Part (a): every combination of the features, each at a value its own checks accept -- what a change in the ORDER of the checks shows in."""
    from kissmcmc_jl_amd import _lib
    flags = {"0": dict(), "islands": dict(flags=_lib.ISLANDS, island_size=64), "p2p": dict(flags=_lib.P2P), "blobs": dict(flags=_lib.STORE_BLOBS),
             "stream": dict(flags=_lib.STREAM_CHAIN), "stream+chain": dict(flags=_lib.STREAM_CHAIN | _lib.STORE_CHAIN)}
    dtypes = dict(f64=dict(), f32=dict(dtype=_lib.F32))
    shards = dict(P1=dict(), P2=dict(shard_count=2))
    deals = dict(deal0=dict(), deal2=dict(deal_count=2))
    ladders = dict(flat=dict(), ladder=dict(betas=LADDER))
    modes = dict(whole=dict(), like=dict(temper_mode=_lib.TEMPER_LIKELIHOOD))
    out = []
    for combo in itertools.product(dens.kinds().items(), flags.items(), dtypes.items(), shards.items(), deals.items(), _moves(_lib).items(),
                                   ladders.items(), modes.items()):
        kw = {}
        for _, part in combo:
            kw.update(part)
        out.append(("x/" + "/".join(name for name, _ in combo), kw))
    # two flags at once, where a configuration breaks the rules of two features
    pair_flags = {"islands": _lib.ISLANDS, "p2p": _lib.P2P, "push": _lib.P2P_PUSH, "blobs": _lib.STORE_BLOBS, "stream": _lib.STREAM_CHAIN,
                  "chain": _lib.STORE_CHAIN, "logp": _lib.STORE_LOGP}
    for (kn, kind), (dn, dt), ((an, a), (bn, b)) in itertools.product(dens.kinds().items(), dtypes.items(), itertools.combinations(pair_flags.items(), 2)):
        for sn, sh in shards.items():
            out.append((f"xx/{kn}/{dn}/{an}+{bn}/{sn}", dict(kind, **dt, **sh, flags=a | b, island_size=64)))
    return out


def fault_cases(dens):
    """Part (b): one fault at a time from an accepted configuration -- every refusal over the VALUE of an argument."""
    from kissmcmc_jl_amd import _lib
    k = dens.kinds()
    nan, inf = float("nan"), float("inf")
    LIKE = _lib.TEMPER_LIKELIHOOD
    out = [("base", dict())]

    def add(name, **kw):
        out.append((name, kw))

    # sizes and scale
    for f, v in (("nwalkers", 0), ("nwalkers", -2), ("ndim", 0), ("nthin", 0), ("ngenerations", -1), ("nburnin", -1)):
        add(f"size/{f}={v}", **{f: v})
    add("size/ngenerations=0", ngenerations=0)
    for v in (1.0, 0.5, nan, inf):
        add(f"size/a_scale={v}", a_scale=v)
    add("size/odd", nwalkers=255)
    add("size/few", nwalkers=4)
    add("size/just_enough", nwalkers=6, ndim=4)
    add("size/nwalkers=2^31", nwalkers=1 << 31)
    add("size/nwalkers=2^31-2", nwalkers=(1 << 31) - 2)
    add("size/ndim=2^24", nwalkers=1 << 25, ndim=1 << 24)
    add("size/ngenerations=2^31", ngenerations=1 << 31)
    add("size/ngenerations=2^31-1", ngenerations=(1 << 31) - 1)
    # density handles
    add("density/user_null", density=_lib.USER_DENSITY)
    add("density/user_with_data_handle", density=_lib.USER_DENSITY, user_density=dens.data.user_handle)
    add("density/data_null", density=_lib.DATA_DENSITY)
    add("density/data_with_body_handle", density=_lib.DATA_DENSITY, user_density=dens.body.user_handle)
    add("density/data_ndim=33", nwalkers=256, ndim=33, **k["data"])
    add("density/data_ndim=32", nwalkers=256, ndim=32, **k["data"])
    add("density/host_null", density=_lib.HOST_DENSITY)
    add("density/host_accepted_ok", host_accepted=dens.host_fn, **k["host"])
    for kind in ("menu", "data", "body"):
        add(f"density/host_accepted_{kind}", host_accepted=dens.host_fn, **k[kind])
    for dt in (2, -1):
        add(f"dtype={dt}", dtype=dt)
        for kind in ("data", "body", "blob", "host"):
            add(f"dtype={dt}/{kind}", dtype=dt, **k[kind])
        add(f"dtype={dt}/islands", dtype=dt, flags=_lib.ISLANDS, island_size=64)
        add(f"dtype={dt}/dealt", dtype=dt, deal_count=2)
    # check_ndim and digest_params
    add("ndim/rosenbrock=1", density=_lib.ROSENBROCK, params=[1.0, 100.0, 20.0], ndim=1)
    add("ndim/rosenbrock=2", density=_lib.ROSENBROCK, params=[1.0, 100.0, 20.0], ndim=2)
    add("ndim/mvnormal2=3", density=_lib.MVNORMAL2, params=[0.0, 0.0, 1.0, 0.0, 1.0])
    add("ndim/mvnormal2=2", density=_lib.MVNORMAL2, params=[0.0, 0.0, 1.0, 0.0, 1.0], ndim=2)
    add("params/gaussian_sigma=0", params=[0.0, 0.0])
    add("params/gaussian_sigma=nan", params=[0.0, nan])
    add("params/exponential_rate=0", density=_lib.EXPONENTIAL, params=[0.0])
    add("params/exponential_ok", density=_lib.EXPONENTIAL, params=[1.0])
    add("params/rosenbrock_scale=0", density=_lib.ROSENBROCK, params=[1.0, 100.0, 0.0])
    add("params/lognormal_sigma=-1", density=_lib.LOGNORMAL, params=[0.0, -1.0])
    add("params/lognormal_ok", density=_lib.LOGNORMAL, params=[0.0, 1.0])
    for d in (5, 99, 103, -1):
        add(f"params/density={d}", density=d)
    # shards and the P2P flags
    for r, n in ((-1, 1), (1, 1), (1, 0), (0, 0), (0, -1), (2, 2), (1, 2), (0, 3), (0, 16)):
        add(f"shard/rank={r}/count={n}", shard_rank=r, shard_count=n)
    for n in (2, 8, 16, 3):
        add(f"shard/p2p/count={n}", flags=_lib.P2P, shard_count=n)
    add("shard/p2p_push/count=2", flags=_lib.P2P | _lib.P2P_PUSH, shard_count=2)
    add("shard/p2p_finegrained/count=2", flags=_lib.P2P | _lib.P2P_FINEGRAINED, shard_count=2)
    add("shard/push_without_p2p", flags=_lib.P2P_PUSH)
    for bit in (8, 10):
        add(f"shard/removed_flag_{bit}", flags=1 << bit)
        add(f"shard/removed_flag_{bit}/p2p", flags=(1 << bit) | _lib.P2P, shard_count=2)
        add(f"shard/removed_flag_{bit}/push_without_p2p", flags=(1 << bit) | _lib.P2P_PUSH)
    # islands
    for S in (0, 64, 128, 256, 100, 32, 512, -64):
        add(f"islands/size={S}", flags=_lib.ISLANDS, island_size=S)
    add("islands/size_not_dividing", flags=_lib.ISLANDS, island_size=128, nwalkers=320)
    add("islands/ndim=33", flags=_lib.ISLANDS, island_size=64, ndim=33)
    add("islands/ndim=32", flags=_lib.ISLANDS, island_size=64, ndim=32)
    add("islands/ndim=63", flags=_lib.ISLANDS, island_size=64, ndim=63)
    for g in (-1, 0, 7):
        add(f"islands/gens={g}", flags=_lib.ISLANDS, island_size=64, island_gens=g)
    add("islands/shard_count=0", flags=_lib.ISLANDS, island_size=64, shard_count=0)
    for name, extra in (("chain", _lib.STORE_CHAIN), ("logp", _lib.STORE_LOGP), ("moments", _lib.MOMENTS)):
        add(f"islands/{name}", flags=_lib.ISLANDS | extra, island_size=64)
    # (the 156 KiB bound of a user density: island_size 256 and ndim 32, the largest the line before it lets through, stay under it)
    for S, nd in ((256, 32), (256, 33), (128, 32), (64, 3)):
        add(f"islands/body/size={S}/ndim={nd}", flags=_lib.ISLANDS, island_size=S, ndim=nd, nwalkers=512, **k["body"])
    # streamed chain
    for name, extra in (("none", 0), ("chain", _lib.STORE_CHAIN), ("logp", _lib.STORE_LOGP), ("both", _lib.STORE_CHAIN | _lib.STORE_LOGP),
                        ("by_walker", _lib.STORE_CHAIN | _lib.CHAIN_BY_WALKER)):
        add(f"stream/{name}", flags=_lib.STREAM_CHAIN | extra)
        add(f"stream/{name}/shard_count=0", flags=_lib.STREAM_CHAIN | extra, shard_count=0)
    # moves
    for m in (2, 5, -1):
        add(f"move={m}", move=m)
    for g in (-0.1, inf, nan, 0.7):
        add(f"de/gamma0={g}", move=_lib.MOVE_DE, de_gamma0=g)
    for s in (-1e-6, 1.0, nan, inf, 0.5):
        add(f"de/sigma={s}", move=_lib.MOVE_DE, de_sigma=s)
    add("stretch/ignores_move_fields", de_gamma0=-5.0, de_sigma=3.0, snooker_gamma=-1.0, mix_count=9)
    for g in (-1.0, inf, nan, 2.0):
        add(f"snooker/gamma={g}", move=_lib.MOVE_SNOOKER, snooker_gamma=g)
    add("snooker/ndim=1", move=_lib.MOVE_SNOOKER, ndim=1)
    add("snooker/nwalkers=4", move=_lib.MOVE_SNOOKER, nwalkers=4, ndim=2)
    add("snooker/nwalkers=6", move=_lib.MOVE_SNOOKER, nwalkers=6, ndim=2)
    mix = _moves(_lib)["mix"]
    for n in (0, 1, 3, 5, -1):
        add(f"mix/count={n}", **dict(mix, mix_count=n))
    add("mix/four_members", **dict(mix, mix_count=4, mix_move2=_lib.MOVE_DE, mix_move3=_lib.MOVE_SNOOKER, mix_weight2=0.5, mix_weight3=0.5))
    for i in (0, 1):
        add(f"mix/member{i}=stretch", **dict(mix, **{f"mix_move{i}": _lib.MOVE_STRETCH}))
        for m in (2, _lib.MOVE_MIX, -1):
            add(f"mix/member{i}={m}", **dict(mix, **{f"mix_move{i}": m}))
        for w in (0.0, -1.0, nan, inf):
            add(f"mix/weight{i}={w}", **dict(mix, **{f"mix_weight{i}": w}))
    add("mix/weights_sum_overflows", **dict(mix, mix_weight0=1.5e308, mix_weight1=1.5e308))
    for g in (-0.1, inf, nan):
        add(f"mix/de_gamma0={g}", **dict(mix, mix_gamma0=g))
        add(f"mix/snooker_gamma={g}", **dict(mix, mix_gamma1=g))
    for s in (-1e-6, 1.0, nan):
        add(f"mix/de_sigma={s}", **dict(mix, mix_sigma0=s))
    add("mix/snooker_ignores_sigma", **dict(mix, mix_sigma1=7.0))
    add("mix/ndim=1", **dict(mix, ndim=1))
    add("mix/nwalkers=4", **dict(mix, nwalkers=4, ndim=2))
    add("mix/two_de/ndim=1", **dict(mix, mix_move1=_lib.MOVE_DE, ndim=1))
    add("mix/bad_member_after_bad_weight", **dict(mix, mix_weight0=0.0, mix_move1=2))
    # blobs
    add("blobs/stored", flags=_lib.STORE_BLOBS | _lib.STORE_CHAIN, **k["blob"])
    add("blobs/shard_count=0", shard_count=0, **k["blob"])
    add("blobs/flag_without_handle", flags=_lib.STORE_BLOBS, density=_lib.USER_DENSITY)
    # tempering, in both modes
    for mode_name, mode, base in (("whole", dict(), dict()), ("like", dict(temper_mode=LIKE), k["data"])):
        def t(name, **kw):
            add(f"temper/{mode_name}/{name}", **dict(base, **mode, **kw))
        t("ok", betas=LADDER, swap_every=2)
        t("two_rungs", betas=[1.0, 0.5])
        for n in (-1, 0, 1, 2, 3):
            t(f"ntemps={n}/no_betas", ntemps=n)
        t("ntemps=1/swap_every=5", ntemps=1, swap_every=5)
        for e in (-1, 0, 1):
            t(f"swap_every={e}", betas=LADDER, swap_every=e)
        t("swap_every=-1/no_ladder", swap_every=-1)
        t("ntemps=65", betas=[1.0] + [0.9 ** (i + 1) for i in range(64)])
        t("ntemps=64", betas=[1.0] + [0.9 ** (i + 1) for i in range(63)])
        for b0 in (0.9, 1.5, nan):
            t(f"betas0={b0}", betas=[b0, 0.5])
        for b in (0.0, -0.1, nan, inf, -inf):
            t(f"last={b}", betas=[1.0, 0.5, b])
            t(f"middle={b}", betas=[1.0, b, 0.1])
        t("middle=0/last=0", betas=[1.0, 0.0, 0.0])
        t("equal", betas=[1.0, 0.5, 0.5])
        t("rising", betas=[1.0, 0.25, 0.5])
        t("second=1", betas=[1.0, 1.0])
        t("ntemps*nwalkers=2^31", betas=[1.0, 0.5], nwalkers=1 << 30)
        t("ntemps*nwalkers<2^31", betas=LADDER, nwalkers=1 << 29)
        for name, kw in (("f32", dict(dtype=_lib.F32)), ("islands", dict(flags=_lib.ISLANDS, island_size=64)), ("p2p", dict(flags=_lib.P2P, shard_count=2)),
                         ("shards", dict(shard_count=2)), ("dealt", dict(deal_count=2)), ("blobs_flag", dict(flags=_lib.STORE_BLOBS)),
                         ("chain", dict(flags=_lib.STORE_CHAIN | _lib.STORE_LOGP | _lib.MOMENTS))):
            t(f"with/{name}", betas=[1.0, 0.5], **kw)
        for name, mv in _moves(_lib).items():
            t(f"move/{name}", betas=[1.0, 0.0], **mv)
            t(f"move/{name}/ok_ladder", betas=LADDER, **mv)
    for mode in (0, LIKE, 2, -1):
        add(f"temper/mode={mode}", temper_mode=mode)
        add(f"temper/mode={mode}/ladder", betas=LADDER, temper_mode=mode)
    for kind in ("menu", "body", "blob", "host"):
        add(f"temper/like/{kind}", betas=LADDER, temper_mode=LIKE, **k[kind])
    for kind in ("data", "body", "blob", "host"):
        add(f"temper/whole/{kind}", betas=LADDER, **k[kind])
    # adaptive ladder
    for mode_name, base in (("whole", dict()), ("like", dict(k["data"], temper_mode=LIKE))):
        good = dict(base, betas=LADDER, swap_every=1, adapt=1, adapt_lag=10.0, adapt_time=100.0, nburnin=5)

        def a(name, **kw):
            add(f"adapt/{mode_name}/{name}", **dict(good, **kw))
        a("ok")
        for v in (2, -1):
            a(f"adapt={v}", adapt=v)
        add(f"adapt/{mode_name}/no_ladder", **{f: v for f, v in good.items() if f != "betas"})
        a("no_ladder/whole", betas=None, temper_mode=0)
        a("ntemps=1", betas=[1.0], temper_mode=0)
        a("two_rungs", betas=[1.0, 0.5])
        a("swap_every=0", swap_every=0)
        for u in (-1, 0, 5, 6):
            a(f"until={u}", adapt_until=u)
        a("until=1/nburnin=0", adapt_until=1, nburnin=0)
        for f in ("adapt_lag", "adapt_time"):
            for v in (0.0, -1.0, nan, inf):
                a(f"{f}={v}", **{f: v})
        a("off_ignores_fields", adapt=0, adapt_until=-1, adapt_lag=nan, adapt_time=-1.0)
    # dealt sub-ensembles
    for r, n in ((0, -1), (-1, 2), (2, 2), (1, 2), (0, 1), (3, 4), (-1, 0), (5, 0)):
        add(f"deal/rank={r}/count={n}", deal_rank=r, deal_count=n)
    add("deal/count=3", deal_count=3)
    add("deal/2^32_walkers", nwalkers=1 << 30, deal_count=4)
    add("deal/2^31_walkers", nwalkers=1 << 30, deal_count=2)
    add("deal/shard_count=0", deal_count=2, shard_count=0)
    add("deal/chain", deal_count=2, flags=_lib.STORE_CHAIN | _lib.STORE_LOGP | _lib.MOMENTS)
    return out


def cases(dens):
    """[(case id, config keywords)]: fixed, in a fixed order; the ids are unique."""
    out = fault_cases(dens) + product_cases(dens)
    assert len({cid for cid, _ in out}) == len(out)
    return out


def run_cases(dens):
    """[(case id, status, message)] of the library as it is loaded, the null configuration first."""
    return [("null_config",) + validate_null()] + [(cid,) + validate(**kw) for cid, kw in cases(dens)]
