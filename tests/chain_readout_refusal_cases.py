"""The convergence / rank / quantile / HDI read-outs of a stored chain without a device: the fixed list of calls whose status,
kmc_last_error() text and sizes out (what the call left in m_out, h_out, n_out) tests/golden/chain_readout_refusals.json records
(tests/golden/make_chain_readout_refusals.py writes it, tests/test_chain_readout_refusals_cpu.py compares).  The seven kmc_chain_* calls
-- lag_sums, convergence, rank_scores, rank_convergence, indicator_lags, quantile_mcse, hdi -- with arguments that are refused before
the device is touched, one fault at a time and two or three at once (then the ORDER of the checks decides which refusal is given); the
kmc_sampler_* forms with a null sampler; and the stages that touch no device, refused and accepted, the accepted outputs as bits:
kmc_convergence_stats, kmc_rank_normal_scores, kmc_hdi_span, kmc_beta_quantile, kmc_quantile_mcse_ranks, kmc_indicator_moments and the
three plans.

Every fault of the list is refused from the arguments alone, so the list runs the same with and without a device.  Every output starts
filled with a sentinel.  The sizes out are recorded, not asserted untouched: kmc_chain_hdi, for one, writes n_out before a later
refusal.  Every other output array must be left as it was by a refused call."""
import ctypes as C
import itertools

import numpy as np

from pointwise_refusal_cases import Outs, disjoint, merged

dp, ip, u64p = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
CHAIN_CALLS = ("lag_sums", "convergence", "rank_scores", "rank_convergence", "indicator_lags", "quantile_mcse", "hdi")
SIZES = ("m_out", "h_out", "n_out")
BIG = 4096                               # every output array: more than any case of the list could fill
OUTPUTS = dict(lag_sums=("chain_mean", "chain_var", "lagsum"),
               convergence=("mean", "W", "B", "var_plus", "rhat", "ess", "mcse", "T", "flags"),
               rank_scores=("rank2", "z", "centre", "nan_count"),
               rank_convergence=("rhat", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "ess_q05", "ess_q95", "median", "q05", "q95", "T", "flags"),
               indicator_lags=("ones", "lagcount"),
               quantile_mcse=("quantile", "ess", "mcse", "lower", "upper", "T", "flags"),
               hdi=("lo", "hi", "start"))
INT_OUTPUTS = ("T", "rank2", "nan_count", "ones", "lagcount", "start")
TAKES_MAX_LAG = ("convergence", "rank_convergence", "quantile_mcse")
TAKES_LAGS = ("lag_sums", "indicator_lags")
TAKES_PROBS = ("indicator_lags", "quantile_mcse", "hdi")


class Sized(Outs):
    """Outs whose sizes out (m_out, h_out, n_out) are recorded and do not count as touched."""

    def untouched(self):
        return all((v == self.init[k]).all() for k, v in self.a.items() if k not in SIZES)

    def sizes(self):
        return [int(self.a[k][0]) if k in self.a else None for k in SIZES]


class World:
    """The library and the chain the list points to."""

    def __init__(self, kmc):
        from kissmcmc_jl_amd import _lib
        self.L = _lib.lib()
        self.zeros = np.zeros(64 * 8 * 4)

    def outputs(self, fn, o, null):
        ptrs = []
        for name in OUTPUTS[fn]:
            p = o.i32(name, BIG) if name == "flags" else o.i(name, BIG) if name in INT_OUTPUTS else o.d(name, BIG)
            if name == "lagcount":
                p = C.cast(p, u64p)
            ptrs.append(None if name in null else p)
        return ptrs

    def call(self, fn, **kw):
        """(status, message, other outputs untouched, [m_out, h_out, n_out]) of kmc_chain_<fn> on 40 samples x 3 walkers x 2 dimensions,
        split, then `kw`."""
        k = dict(chain=True, logp=False, ns=40, nw=3, nd=2, first=0, mask=None, split=1, max_lag=0, lag0=1, nlags=5, nprobs=2, probs=(0.25, 0.9),
                 folded=1, null=())
        k.update(kw)
        o = Sized()
        dptr = lambda a: a.ctypes.data_as(dp)
        mask = None if k["mask"] is None else np.asarray(k["mask"], dtype=np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
        probs = np.zeros(32)
        probs[:len(k["probs"])] = k["probs"]
        lead = [dptr(self.zeros) if k["chain"] else None, dptr(self.zeros) if k["logp"] else None, k["ns"], k["nw"], k["nd"], k["first"], mask]
        pr = None if "probs" in k["null"] else dptr(probs)
        outs = self.outputs(fn, o, k["null"])
        mh = [] if fn == "hdi" else [o.i("m_out"), o.i("h_out")]
        if fn == "lag_sums":
            args = lead + [k["split"], k["lag0"], k["nlags"], 0] + outs + mh
        elif fn == "convergence":
            args = lead + [k["split"], k["max_lag"], 0] + outs + mh + [o.i("info", 8)]
        elif fn == "rank_scores":
            args = lead + [k["split"], k["folded"], 0] + outs + mh
        elif fn == "rank_convergence":
            args = lead + [k["split"], k["max_lag"], 0] + outs + mh + [o.i("info", 8)]
        elif fn == "indicator_lags":
            args = lead + [k["split"], k["nprobs"], pr, k["lag0"], k["nlags"], 0] + outs + mh
        elif fn == "quantile_mcse":
            args = lead + [k["split"], k["max_lag"], k["nprobs"], pr, 0] + outs + mh + [o.i("info", 8)]
        else:
            args = lead + [pr, k["nprobs"], 0] + outs + [o.i("n_out"), o.i("nan_count", BIG), o.i("info", 8)]
        st = getattr(self.L, "kmc_chain_" + fn)(*args)
        return st, self.L.kmc_last_error().decode() if st else "", o.untouched(), o.sizes()


def faults(fn):
    """{name: keywords}: the single faults `fn` refuses before the device, each from the accepted call."""
    nan = float("nan")
    f = {"null_chain": dict(chain=False), "nsamples=0": dict(ns=0), "nwalkers=0": dict(nw=0), "ndim=-1": dict(nd=-1), "first=-1": dict(first=-1),
         "first=41": dict(first=41), "no_samples": dict(first=40), "empty_mask": dict(mask=[0, 0, 0])}
    if fn != "hdi":
        f.update({"h=3": dict(ns=7), "m=1": dict(nw=1, split=0), "m=1_by_mask": dict(mask=[0, 1, 0], split=0)})
    if fn in TAKES_MAX_LAG:
        f.update({"max_lag=2": dict(max_lag=2), "max_lag=-1": dict(max_lag=-1), "max_lag=h": dict(max_lag=20)})
    if fn in TAKES_LAGS:
        f.update({"lag0=0": dict(lag0=0), "nlags=-1": dict(nlags=-1), "lags_past_h": dict(lag0=15, nlags=6), "lag0=h": dict(lag0=20, nlags=1)})
    if fn == "lag_sums":
        f.update({"mean_without_var": dict(null=("chain_var",)), "var_without_mean": dict(null=("chain_mean",)), "null_lagsum": dict(null=("lagsum",))})
    if fn in TAKES_PROBS:
        f.update({"nprobs=0": dict(nprobs=0), "nprobs=17": dict(nprobs=17, probs=(0.5,) * 17), "null_probs": dict(null=("probs",))})
    if fn in ("quantile_mcse", "hdi"):
        f.update({"prob=0": dict(probs=(0.0, 0.9)), "prob=1": dict(probs=(0.25, 1.0)), "prob=nan": dict(probs=(nan, 0.9))})
    if fn == "hdi":
        f.update({"prob*N<1": dict(probs=(0.25, 0.005)), "N=1": dict(ns=1, nw=1)})
    if fn not in ("lag_sums", "rank_scores"):                                    # (rank_scores: every output may be null)
        f.update({"null_" + name: dict(null=(name,)) for name in OUTPUTS[fn]})
    return f


def apart(*kws):
    """disjoint, and not both of chain_mean and chain_var null: together they are no fault"""
    return disjoint(*kws) and not {"chain_mean", "chain_var"} <= set(merged(*kws).get("null", ()))


def chain_cases():
    """[(case id, function, keywords)]: every fault alone, every pair, every 37th triple."""
    out = []
    for fn in CHAIN_CALLS:
        f = faults(fn)
        out += [(f"{fn}/{name}", fn, kw) for name, kw in f.items()]
        out += [(f"{fn}/{a}+{b}", fn, merged(f[a], f[b])) for a, b in itertools.combinations(f, 2) if apart(f[a], f[b])]
        out += [(f"{fn}/{a}+{b}+{c}", fn, merged(f[a], f[b], f[c])) for a, b, c in list(itertools.combinations(f, 3))[::37]
                if apart(f[a], f[b], f[c])]
    return out


def sampler_cases(w):
    """The kmc_sampler_* forms with a null sampler: all other arguments good, and next to a second fault."""
    L, rows = w.L, []
    for fn in CHAIN_CALLS:
        for second, null, first, max_lag, nprobs in (("", (), 0, 0, 2), ("+first=-1", (), -1, 0, 2), ("+max_lag=2+nprobs=0", (), 0, 2, 0),
                                                     ("+null_outputs", OUTPUTS[fn] + ("probs",), 0, 0, 2)):
            o = Sized()
            outs, pr = w.outputs(fn, o, null), None if "probs" in null else np.full(2, 0.5).ctypes.data_as(dp)
            mh = [o.i("n_out")] if fn == "hdi" else [o.i("m_out"), o.i("h_out")]
            args = {"lag_sums": [1, 0, 1, 5] + outs + mh, "convergence": [1, 0, max_lag] + outs + mh + [None],
                    "rank_scores": [1, 0, 1] + outs + mh, "rank_convergence": [1, 0, max_lag] + outs + mh + [None],
                    "indicator_lags": [1, 0, nprobs, pr, 1, 5] + outs + mh, "quantile_mcse": [1, 0, max_lag, nprobs, pr] + outs + mh + [None],
                    "hdi": [0, pr, nprobs] + outs + mh + [None, None]}[fn]
            st = getattr(L, "kmc_sampler_" + fn)(None, first, None, *args)
            rows.append((f"null_sampler/{fn}{second}", st, L.kmc_last_error().decode() if st else "", o.untouched(), o.sizes(), None))
    return rows


def host_cases(w):
    """The stages that touch no device: refused, and accepted with their outputs."""
    L, nan, inf = w.L, float("nan"), float("inf")
    rows = []

    def run(cid, f):
        o = Outs()
        st = f(o)
        rows.append((cid, st, L.kmc_last_error().decode() if st else "", o.untouched(), [None] * 3, o.record() if st == 0 else None))

    rng = np.random.default_rng(5)
    cm, cv, lag = rng.standard_normal(6), 0.5 + rng.random(6), (2.0 * rng.random(2 * 8) * 3 * 20)
    lag[8:] = np.linspace(1.0, 100.0, 8)                                      # column 1: the rule needs more lags than it is given
    p = lambda a: a.ctypes.data_as(dp)
    for m, h, nc, nl, ml, null in ((3, 20, 2, 8, 19, ()), (3, 20, 2, 8, 5, ()), (3, 20, 2, 0, 19, ("lagsum",)), (3, 20, 2, 8, 19, ("lagsum",)),
                                   (3, 20, 0, 8, 19, ()), (3, 3, 2, 2, 3, ()), (1, 20, 2, 8, 19, ()), (3, 20, 2, 8, 2, ()), (3, 20, 2, 8, 20, ()),
                                   (3, 20, 2, -1, 19, ()), (3, 20, 2, 20, 19, ()), (3, 20, 2, 8, 19, ("chain_var",)), (3, 20, 2, 8, 19, ("flags",)),
                                   (1, 3, 0, -1, 2, ("mean",)), (3, 20, 1, 8, 19, ("constant",))):
        run(f"convergence_stats/m={m}/h={h}/ncols={nc}/nlags={nl}/max_lag={ml}/{'+'.join(null)}",
            lambda o: L.kmc_convergence_stats(m, h, nc, p(cm), None if "chain_var" in null else p(np.zeros(6) if "constant" in null else cv),
                                              None if "lagsum" in null else p(lag), nl, ml, None if "mean" in null else o.d("mean", 2), o.d("W", 2),
                                              o.d("B", 2), o.d("var_plus", 2), o.d("rhat", 2), o.d("ess", 2), o.d("mcse", 2), o.i("T", 2),
                                              None if "flags" in null else o.i32("flags", 2)))
    for name, r2, n, S, null in (("ok", [2, 3, 7, 14], 4, 7, ()), ("n=0", [2], 0, 7, ("rank2", "z")), ("n=-1", [2], -1, 7, ()), ("null_z", [2], 1, 7, ("z",)),
                                 ("S=0", [2], 1, 0, ()), ("S=2^52", [2], 1, 1 << 52, ()), ("rank2=1", [2, 1], 2, 7, ()), ("rank2=15", [2, 15], 2, 7, ()),
                                 ("null_rank2+S=0", [2], 1, 0, ("rank2",))):
        run(f"rank_normal_scores/{name}",
            lambda o: L.kmc_rank_normal_scores(None if "rank2" in null else np.asarray(r2, dtype=np.int64).ctypes.data_as(ip), n, S,
                                               None if "z" in null else o.d("z", 4)))
    for n, pr in ((120, 0.9), (120, 0.005), (2, 0.75), (2, 0.25), (1, 0.5), (1 << 31, 0.5), (120, 0.0), (120, 1.0), (120, nan), (1, nan), (120, 0.999),
                  (7800, 0.05), (120, inf)):
        run(f"hdi_span/n={n}/p={pr}", lambda o: L.kmc_hdi_span(n, pr, o.i("k"), o.i("nwindows")))
    for pr, A, B, null in ((0.5, 2.0, 3.0, ()), (0.1587, 41.0, 361.0, ()), (0.8413, 1.0, 1.0, ()), (0.0, 2.0, 3.0, ()), (1.0, 2.0, 3.0, ()), (nan, 2.0, 3.0, ()),
                           (0.5, 0.5, 3.0, ()), (0.5, 2.0, inf, ()), (0.5, nan, 3.0, ()), (0.5, 2.0, 3.0, ("x",)), (0.0, 0.5, 3.0, ("x",))):
        run(f"beta_quantile/p={pr}/A={A}/B={B}/{'+'.join(null)}", lambda o: L.kmc_beta_quantile(pr, A, B, None if null else o.d("x", 1)))
    for S, pr, ess in ((7800, 0.05, 412.5), (120, 0.5, 30.0), (120, 0.5, nan), (120, 0.5, -1.0), (120, 0.5, inf), (0, 0.5, 30.0), (1 << 52, 0.5, 30.0),
                       (120, 0.0, 30.0), (120, 1.0, 30.0), (120, nan, 30.0), (0, nan, 30.0), (1, 0.5, 1.0)):
        run(f"quantile_mcse_ranks/S={S}/p={pr}/ess={ess}", lambda o: L.kmc_quantile_mcse_ranks(S, pr, ess, o.d("a", 1), o.d("b", 1), o.i("i1"), o.i("i2")))
    for h, kk in ((20, 7), (20, 0), (20, 20), (2, 1), (1, 0), (20, -1), (20, 21), (650, 33)):
        run(f"indicator_moments/h={h}/k={kk}", lambda o: L.kmc_indicator_moments(h, kk, o.d("mu", 1), o.d("s2", 1)))
    for plan in ("convergence", "rank", "indicator"):
        run(f"{plan}_plan", lambda o: getattr(L, f"kmc_{plan}_plan")(o.i32("a", 1), o.i32("b", 1), o.i32("c", 1), o.i32("d", 1)))
    return rows


def run_cases(kmc):
    """[(case id, status, message, other outputs untouched, [m_out, h_out, n_out], recorded outputs or None)] of the library as it is
    loaded; the ids are unique."""
    w = World(kmc)
    rows = [(cid,) + w.call(fn, **kw) + (None,) for cid, fn, kw in chain_cases()] + sampler_cases(w) + host_cases(w)
    assert len({r[0] for r in rows}) == len(rows)
    return rows
