"""The pointwise / PSIS-LOO family without a device: the fixed list of calls whose (status, kmc_last_error()) -- and, for the accepted
calls of the plans and the host stages, whose outputs -- tests/golden/pointwise_refusals.json records
(tests/golden/make_pointwise_refusals.py writes it, tests/test_pointwise_refusals_cpu.py compares).  The seven kmc_chain_* calls with
arguments that are refused before the device is touched, one fault at a time and two or three at once (then the ORDER of the checks
decides which refusal is given); the kmc_sampler_* forms with a null sampler; kmc_pointwise_plan, kmc_psis_plan, kmc_waic_stats,
kmc_loo_stats and kmc_psis_smooth_host, refused and accepted.

Every chain case holds at least one fault that is refused from the arguments alone, so the list runs the same with and without a
device.  What is checked only after the device is open (the tail array's column count, a null tail_len, the second psis_check of one
r_eff) appears here only next to such a fault: alone it would reach the device.  A chain of floats exists only inside a sampler, so its
refusal cannot be reached without a device and is not in the list.

Every output array starts filled with a sentinel; a refused call must leave all of them as they were."""
import ctypes as C
import itertools

import numpy as np

REG_TERM = "double r = d[0] - x[0] * d[1] - x[1] * d[2]; return -0.5 * p[0] * r * r;"
SENTINEL = -7.0
J = 10                                   # observations of the density
dp, ip, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)


class Outs:
    """Output arrays by name, sentinel-filled; ptr(name) gives the pointer, untouched() says whether all still hold the sentinel."""

    def __init__(self):
        self.a, self.init = {}, {}

    def _new(self, name, size, value, dtype, ptr):
        self.a[name], self.init[name] = np.full(size, value, dtype=dtype), value
        return self.a[name].ctypes.data_as(ptr)

    def d(self, name, size):
        return self._new(name, size, SENTINEL, np.float64, dp)

    def i(self, name, size=1, value=-7):
        return self._new(name, size, value, np.int64, ip)

    def i32(self, name, size):
        return self._new(name, size, -7, np.int32, i32p)

    def untouched(self):
        return all((v == self.init[k]).all() for k, v in self.a.items())

    def record(self):
        return {k: [float(x).hex() for x in v] if v.dtype == np.float64 else [int(x) for x in v] for k, v in self.a.items()}


class World:
    """The handles and inputs the list points to, alive as long as this object."""

    def __init__(self, kmc):
        from kissmcmc_jl_amd import _lib
        self.L = _lib.lib()
        self.dd = kmc.DataDensity(REG_TERM, np.arange(3.0 * J).reshape(J, 3), params=[2.0])
        self.other = kmc.ExprDensity("-0.5*x*x")
        self.par = np.array([2.0, 0, 0, 0, 0, 0])
        self.zeros = np.zeros(10000 * 3 * 33)            # any chain of the list fits: at most 10000 x 3 x 2, or 40 x 3 x 33
        self.held = np.arange(12.0)                      # held-out observations [4][3]

    def p(self, a):
        return None if a is None else a.ctypes.data_as(dp)

    def call(self, fn, **kw):
        """(status, message, outputs untouched) of kmc_chain_<fn> on 40 samples x 3 walkers x 2 dimensions (n = 120), then `kw`."""
        k = dict(h=self.dd.user_handle, par=self.par, ns=40, nw=3, nd=2, first=0, mask=None, thin=1, data=None, nd2=0, nc2=0, obs=(0, J),
                 r_eff=1.0, r_j=np.ones(J), split=1, max_lag=0, work=0, null=(), tail_len=64)
        k.update(kw)
        o = Outs()
        n_rows, (of, oc) = 10000 * 3, k["obs"]
        mask = None if k["mask"] is None else np.asarray(k["mask"], dtype=np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
        lead = [k["h"], self.p(k["par"]), self.p(self.zeros), k["ns"], k["nw"], k["nd"], k["first"], mask, k["thin"]]
        held = [self.p(self.held if k["data"] else None), k["nd2"], k["nc2"]]
        out = lambda name, ptr: None if name in k["null"] else ptr
        r_j = None if k["r_j"] is None else self.p(np.ascontiguousarray(k["r_j"], dtype=np.float64))
        reff = [r_j, k["split"], k["max_lag"], of, oc, k["work"]]
        used = [out("r_eff_used", o.d("r_eff_used", J)), out("tail_len_j", o.i("tail_len_j", J)), out("n_reff_nan", o.i("n_reff_nan"))]
        n_out = o.i("n_out")
        if fn == "pointwise_stats":
            args = lead + held + [0, out("stats", o.d("stats", 4 * J)), n_out, o.i("info", 6)]
        elif fn == "pointwise_loglike":
            args = lead + held + [of, oc, 0, out("out", o.d("out", n_rows * J)), n_out]
        elif fn == "pointwise_weights":
            args = lead + held + [of, oc, 0, out("v", o.d("v", n_rows * J)), out("M_j", o.d("M_j", J)), n_out]
        elif fn == "relative_eff":
            args = lead + [of, oc, k["split"], k["max_lag"], k["work"], 0, out("r_eff_j", o.d("r_eff_j", J)), o.d("ess_j", J), o.i("T_j", J),
                           o.i32("flags_j", J), o.i("m_out"), o.i("h_out"), n_out, o.i("info", 6)]
        elif fn in ("psis_loo", "psis_loo_reff"):
            sel = [k["r_eff"], of, oc, k["work"]] if fn == "psis_loo" else reff
            args = lead + sel + [0, out("stats", o.d("stats", 4 * J)), out("lppd_j", o.d("lppd_j", J))] + (used if fn == "psis_loo_reff" else []) + \
                [n_out, o.i("info", 16)]
        else:
            sel = [k["r_eff"], of, oc, k["work"]] if fn == "psis_tail" else reff
            args = lead + sel + [0, out("tail", o.d("tail", J * 64)), o.d("m_j", J), o.d("xc_j", J), o.i32("n_tail_j", J),
                                 out("tail_len", o.i("tail_len", 1, k["tail_len"]))] + (used if fn == "psis_tail_reff" else []) + [n_out]
        st = getattr(self.L, "kmc_chain_" + fn)(*args)
        return st, self.L.kmc_last_error().decode() if st else "", o.untouched(), None


CHAIN_CALLS = ("pointwise_stats", "pointwise_loglike", "pointwise_weights", "relative_eff", "psis_loo", "psis_tail", "psis_loo_reff", "psis_tail_reff")
TAKES_DATA = ("pointwise_stats", "pointwise_loglike", "pointwise_weights")
TAKES_RANGE = CHAIN_CALLS[1:]
RESULT = dict(pointwise_stats="stats", pointwise_loglike="out", pointwise_weights="v", relative_eff="r_eff_j", psis_loo="stats", psis_tail="tail",
              psis_loo_reff="stats", psis_tail_reff="tail")


def bad_at(i, v):
    r = np.ones(J)
    r[i] = v
    return r


def faults(w, fn):
    """{name: keywords}: the single faults `fn` refuses before the device, each from the accepted call."""
    nan, inf = float("nan"), float("inf")
    f = {"non_data": dict(h=w.other.user_handle), "null_density": dict(h=None), "ndim=33": dict(nd=33), "thin=0": dict(thin=0), "thin=-2": dict(thin=-2),
         "no_samples": dict(first=40), "first=41": dict(first=41), "first=-1": dict(first=-1), "empty_mask": dict(mask=[0, 0, 0]),
         "n=1": dict(ns=1, nw=1), "null_result": dict(null=(RESULT[fn],)), "null_params": dict(par=None), "nwalkers=0": dict(nw=0), "ndim=0": dict(nd=0)}
    if fn in TAKES_DATA:
        f.update({"held_cols=2": dict(data=True, nd2=4, nc2=2), "held_ndata=0": dict(data=True, nd2=0, nc2=3), "held_ndata=-1": dict(data=True, nd2=-1, nc2=3)})
    if fn in TAKES_RANGE:
        f.update({"obs_count=0": dict(obs=(0, 0)), "obs_count=-1": dict(obs=(0, -1)), "obs_past_J": dict(obs=(3, 8)), "obs_first=-1": dict(obs=(-1, 4)),
                  "obs_first=J": dict(obs=(J, 1))})
    if fn == "pointwise_weights":
        f["obs_past_held"] = dict(data=True, nd2=4, nc2=3, obs=(0, 5))
    if "psis" in fn:
        f.update({"n=4": dict(ns=2, nw=2), "n=3_by_thin": dict(ns=4, nw=3, thin=4)})
        if fn in ("psis_loo", "psis_loo_reff"):
            f["null_lppd"] = dict(null=("lppd_j",))
    if fn in ("psis_loo", "psis_tail"):
        for v in (0.0, -1.0, nan, inf):
            f[f"r_eff={v}"] = dict(r_eff=v)
        f["tail=6000"] = dict(ns=10000, r_eff=0.0075)
    if fn in ("psis_loo_reff", "psis_tail_reff"):
        for v in (0.0, -1.0, nan, inf):
            f[f"r_eff_j[0]={v}"] = dict(r_j=bad_at(0, v))
            f[f"r_eff_j[9]={v}"] = dict(r_j=bad_at(J - 1, v))
        f["r_eff_j[2]=nan,[4]=0"] = dict(r_j=np.where(np.arange(J) == 2, nan, np.where(np.arange(J) == 4, 0.0, 1.0)))
        f["tail_j[6]=6000"] = dict(ns=10000, r_j=bad_at(6, 0.001))
        f["tail_j[0]=6000/range"] = dict(ns=10000, r_j=bad_at(0, 0.001), obs=(2, 5))
    if fn in ("relative_eff", "psis_loo_reff", "psis_tail_reff"):
        c = dict(r_j=None) if fn != "relative_eff" else {}
        f.update({"chain/h=3": dict(c, ns=7), "chain/one_chain": dict(c, nw=1, split=0), "chain/max_lag=2": dict(c, max_lag=2),
                  "chain/max_lag=20": dict(c, max_lag=20), "chain/thin=2/max_lag=10": dict(c, thin=2, max_lag=10), "chain/max_lag=-1": dict(c, max_lag=-1)})
    return f


def after_open(fn):
    """{name: keywords}: what `fn` checks only after the device is open; in the list only together with a fault of faults()."""
    a = {}
    if fn in ("psis_tail", "psis_tail_reff"):
        a.update({"null_tail_len": dict(null=("tail_len",)), "tail_len=1": dict(tail_len=1)})
    return a


def disjoint(*kws):
    """No keyword but `null` set twice: every fault of a combination stays as it is written."""
    keys = [k for kw in kws for k in kw if k != "null"]
    return len(keys) == len(set(keys))


def merged(*kws):
    out = {}
    for kw in kws:
        for k, v in kw.items():
            out[k] = tuple(out.get(k, ())) + tuple(v) if k == "null" else v
    return out


def chain_cases(w):
    """[(case id, function, keywords)]"""
    out = []
    for fn in CHAIN_CALLS:
        f = faults(w, fn)
        out += [(f"{fn}/{name}", fn, kw) for name, kw in f.items()]
        out += [(f"{fn}/{a}+{b}", fn, merged(f[a], f[b])) for a, b in itertools.combinations(f, 2) if disjoint(f[a], f[b])]
        out += [(f"{fn}/{a}+{b}", fn, merged(kw, f[b])) for a, kw in after_open(fn).items() for b in f if disjoint(kw, f[b])]
    for fn in ("pointwise_weights", "psis_loo", "psis_tail_reff"):               # three at once, every 29th triple
        f = faults(w, fn)
        out += [(f"{fn}/{a}+{b}+{c}", fn, merged(f[a], f[b], f[c])) for a, b, c in list(itertools.combinations(f, 3))[::29]
                if disjoint(f[a], f[b], f[c])]
    return out


def sampler_cases(w):
    """The kmc_sampler_* forms with a null sampler, all other arguments good; and the null lppd_j next to it."""
    L, o = w.L, Outs()
    d, i = o.d, o.i
    sel = [None, 0, None, 1]
    calls = {
        "pointwise_stats": lambda: L.kmc_sampler_pointwise_stats(*sel, None, 0, 0, d("stats", 40), i("n"), None),
        "pointwise_loglike": lambda: L.kmc_sampler_pointwise_loglike(*sel, None, 0, 0, 0, 1, d("out", 10), i("n")),
        "pointwise_weights": lambda: L.kmc_sampler_pointwise_weights(*sel, None, 0, 0, 0, 1, d("v", 10), None, i("n")),
        "relative_eff": lambda: L.kmc_sampler_relative_eff(*sel, 0, 1, 1, 0, 0, d("r", 10), None, None, None, None, None, i("n"), None),
        "psis_loo": lambda: L.kmc_sampler_psis_loo(*sel, 1.0, 0, 1, 0, d("stats", 40), d("lp", 10), i("n"), None),
        "psis_loo/null_lppd": lambda: L.kmc_sampler_psis_loo(*sel, 1.0, 0, 1, 0, d("stats", 40), None, i("n"), None),
        "psis_tail": lambda: L.kmc_sampler_psis_tail(*sel, 1.0, 0, 1, 0, d("tail", 64), d("m", 10), d("xc", 10), o.i32("nt", 10), i("tl", 1, 64), i("n")),
        "psis_loo_reff": lambda: L.kmc_sampler_psis_loo_reff(*sel, None, 1, 0, 0, 1, 0, d("stats", 40), d("lp", 10), d("ru", 10), i("tlj", 10), i("nn"), i("n"),
                                                             None),
        "psis_loo_reff/null_lppd": lambda: L.kmc_sampler_psis_loo_reff(*sel, None, 1, 0, 0, 1, 0, d("stats", 40), None, d("ru", 10), i("tlj", 10), i("nn"),
                                                                       i("n"), None),
        "psis_tail_reff": lambda: L.kmc_sampler_psis_tail_reff(*sel, None, 1, 0, 0, 1, 0, d("tail", 64), d("m", 10), d("xc", 10), o.i32("nt", 10),
                                                               i("tl", 1, 64), d("ru", 10), i("tlj", 10), i("nn"), i("n")),
    }
    rows = []
    for name, f in calls.items():
        st = f()
        rows.append((f"null_sampler/{name}", st, L.kmc_last_error().decode() if st else "", o.untouched(), None))
    return rows


def host_cases(w):
    """kmc_pointwise_plan, kmc_psis_plan, kmc_waic_stats, kmc_loo_stats, kmc_psis_smooth_host: refused, and accepted with their outputs."""
    L, nan = w.L, float("nan")
    rows = []

    def run(cid, f):
        o = Outs()
        st = f(o)
        rows.append((cid, st, L.kmc_last_error().decode() if st else "", o.untouched(), o.record() if st == 0 else None))

    for n, nd in ((1, 10), (2, 0), (2, (1 << 30) + 1), (1 << 40, 10), (1, 0), (2, 1), (189, 70), (189, 10), (100000, 1000)):
        run(f"pointwise_plan/n={n}/ndata={nd}",
            lambda o: L.kmc_pointwise_plan(n, nd, o.i("run_len"), o.i("nruns"), o.i32("lanes", 1), o.i32("slots", 1), o.i("nwaves")))
    for n, nd, r, ws in ((4, 10, 1.0, 0), (100, 0, 1.0, 0), (100, 10, 1.0, -1), (100, 10, 0.0, 0), (100, 10, nan, 0), (100, 10, float("inf"), 0),
                         (1 << 31, 10, 1.0, 0), (20485, 10, 0.01, 0), (4, 0, 0.0, -1), (4, 10, 0.0, 0), (100, 0, 1.0, -1), (100, 10, -1.0, -1),
                         (189, 70, 1.0, 0), (189, 70, 0.25, 1), (20480, 10, 0.01, 1 << 20)):
        run(f"psis_plan/n={n}/ndata={nd}/r_eff={r}/workspace={ws}",
            lambda o: L.kmc_psis_plan(n, nd, r, ws, o.i("tail_len"), o.i("m_est"), o.i("obs_per_block"), o.i("passes")))
    rng = np.random.default_rng(11)
    st7 = np.concatenate([-rng.random(7), -rng.random(7), rng.random(7) + 0.5, 0.5 * rng.random(7)])
    for Jn, n, null in ((0, 50, ()), (7, 1, ()), (0, 1, ()), (7, 50, ("stats",)), (7, 50, ("totals",)), (0, 50, ("stats",)), (7, 50, ()), (1, 2, ()),
                        (7, 50, ("lppd_j", "p_waic_j", "elpd_j"))):
        run(f"waic_stats/J={Jn}/n={n}/null={'+'.join(null)}",
            lambda o: L.kmc_waic_stats(Jn, n, None if "stats" in null else w.p(st7), None if "lppd_j" in null else o.d("lppd_j", 7),
                                       None if "p_waic_j" in null else o.d("p_waic_j", 7), None if "elpd_j" in null else o.d("elpd_j", 7),
                                       None if "totals" in null else o.d("totals", 7)))
    loo7, lp7 = np.concatenate([-rng.random(7), rng.uniform(-0.3, 1.4, 7), np.full(7, 20.0), rng.random(7)]), -rng.random(7)
    for Jn, n, null in ((0, 50, ()), (7, 4, ()), (0, 4, ()), (7, 50, ("stats",)), (7, 50, ("lppd_j",)), (7, 50, ("totals",)), (7, 4, ("stats",)), (7, 50, ()),
                        (1, 5, ()), (7, 50, ("p_loo_j",))):
        run(f"loo_stats/J={Jn}/n={n}/null={'+'.join(null)}",
            lambda o: L.kmc_loo_stats(Jn, n, None if "stats" in null else w.p(loo7), None if "lppd_j" in null else w.p(lp7),
                                      None if "p_loo_j" in null else o.d("p_loo_j", 7), None if "totals" in null else o.d("totals", 10)))
    x = np.sort(-12.0 + np.log1p(0.3 * np.expm1(-0.5 * np.log1p(-rng.random(40))) / 0.5))
    tails = {"fit40": (x, -12.0, ()), "four": (np.array([-3.0, -2.0, -1.0, -0.5]), -4.0, ()), "empty": (np.zeros(0), -1.0, ("x", "s")),
             "nt=-1": (None, -1.0, ()), "nt=4097": (np.full(4097, -1.0), -2.0, ()), "null_x": (x, -12.0, ("x",)), "null_s": (x, -12.0, ("s",)),
             "descending": (np.array([-1.0, -2.0]), -3.0, ()), "positive": (np.array([-2.0, 0.5]), -3.0, ()), "at_cut": (np.array([-3.0, -1.0]), -3.0, ()),
             "nan": (np.array([nan]), -3.0, ()), "nt=4097+null_x": (np.full(4097, -1.0), -2.0, ("x",)), "null_x+descending": (np.array([-1.0, -2.0]), -3.0, ("x",)),
             "fit40/no_outs": (x, -12.0, ("k", "sigma", "sums"))}
    for name, (t, xc, null) in tails.items():
        nt = -1 if t is None else t.size
        run(f"psis_smooth_host/{name}",
            lambda o: L.kmc_psis_smooth_host(nt, None if "x" in null or t is None else w.p(np.ascontiguousarray(t)), xc, None if "k" in null else o.d("k", 1),
                                             None if "sigma" in null else o.d("sigma", 1), None if "s" in null else o.d("s", max(nt, 1)),
                                             None if "sums" in null else o.d("sums", 2)))
    return rows


def run_cases(kmc):
    """[(case id, status, message, outputs untouched, recorded outputs or None)] of the library as it is loaded; the ids are unique."""
    w = World(kmc)
    rows = [(cid,) + w.call(fn, **kw) for cid, fn, kw in chain_cases(w)] + sampler_cases(w) + host_cases(w)
    assert len({r[0] for r in rows}) == len(rows)
    return rows
