#!/usr/bin/env python
"""The ess and MCSE of quantiles from bit-packed indicator chains: profiles/quantile_mcse.json.

Per shape (a menu Gaussian, chain stored on the device; the three shapes of scripts/posterior_summary_bench.py), in each of three child
processes, every call blocking and bracketed by HIP events after one untimed call:

  The indicator stage alone, 2 probabilities (q05, q95), the lags 1 .. min(32, h - 1):
    bits      Sampler.indicator_lags on the chain where it lies, with the lags and with nlags = 0 (the pack kernel alone); and
              kmc.indicator_lags on the downloaded chain (its upload included);
    doubles   kmc.lag_sums (kmc_chain_lag_sums, moments=False) of this same build over a host chain whose 2 ndim columns are those same
              indicators stored as 0.0 / 1.0 -- the existing way through an existing public call -- with the lags and with nlags = 0
              (the upload of the 2 ndim columns alone).  The D_t of the two routes are compared for equality.
    ratios    bits_over_doubles_device = the sampler route of the bits (a whole call: allocations, pack, the counts of the ones copied to
              the host, lag counts) over (doubles - its upload), a difference of two calls from which their fixed costs cancel;
              lag_kernels_bits_over_doubles = (bits - bits with nlags = 0) over (doubles - its upload): the two lag stages alone;
              bits_over_doubles_host = both host-chain calls whole, each with its own upload.
  The whole call, Sampler.quantile_mcse with 3 and with 16 probabilities, Sampler.rank_convergence next to it for scale, and a stage
  split pieced together from separate calls: sort = the gather and sort times of Sampler.hdi's info on the same draws, pack =
  indicator_lags with nlags = 0, lag counts = indicator_lags with the lags the whole call computed (its info) minus the pack, picks
  and host = the rest of the whole call.  The pieces are separate calls with their own allocations and copies: a split to a few tenths of a
  millisecond, not better.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from convergence_bench import CASES, bracket, spread                               # noqa: E402

PROBS3 = [0.16, 0.5, 0.84]
PROBS16 = [0.01, 0.025, 0.05, 0.1, 0.16, 0.25, 0.4, 0.5, 0.6, 0.75, 0.84, 0.9, 0.95, 0.975, 0.99, 0.999]


def timed(fn):
    fn()
    out, ev, _ = bracket(fn)
    return out, ev


def child(idx):
    import kissmcmc_jl_amd as kmc
    from kissmcmc_jl_amd.chain_convergence import sampler_quantile_mcse
    from kissmcmc_jl_amd.summary import _SamplerProvider, hdi_from
    name, nw, nd, ns = CASES[idx]
    nburn = 20
    th0 = np.random.default_rng(0).standard_normal((nw, nd))
    res = dict(case=name)
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, nburn + ns, nburn, 1, 2.0, 3, store_chain=True) as s:
        s.set_positions(th0)
        s.run(nburn + ns)
        s.sync()
        q3, res["whole3_ms"] = timed(lambda: sampler_quantile_mcse(s, PROBS3, raw=True))
        q16, res["whole16_ms"] = timed(lambda: sampler_quantile_mcse(s, PROBS16, raw=True))
        _, res["rank_convergence_ms"] = timed(lambda: s.rank_convergence())
        h = q3["h"]
        L = min(32, h - 1)
        thr = sampler_quantile_mcse(s, [0.05, 0.95])["quantile"]
        bits, res["bits_sampler_ms"] = timed(lambda: s.indicator_lags(thr, 1, L))
        _, res["bits_sampler_pack_ms"] = timed(lambda: s.indicator_lags(thr, 1, 0))
        for tag, q in (("3", q3), ("16", q16)):
            lags = int(q["info"][0])
            _, res[f"pack{tag}_ms"] = timed(lambda: s.indicator_lags(q["quantile"], 1, 0))
            _, both = timed(lambda: s.indicator_lags(q["quantile"], 1, lags))
            res[f"lagcounts{tag}_ms"] = both - res[f"pack{tag}_ms"]
            res[f"lags{tag}"] = lags
        info = hdi_from(_SamplerProvider(s), 0.94, with_info=True)["info"]
        res["sort_ms"] = (info[3] + info[4]) * 1e-6
        res["info3"], res["info16"] = [int(v) for v in q3["info"]], [int(v) for v in q16["info"]]
        chain = s.chain(logp=False)[0]                                             # [sample][walker][dim]
    th = chain.transpose(1, 0, 2)
    bits_host, res["bits_host_ms"] = timed(lambda: kmc.indicator_lags(th, thr, None, 1, L))
    ind = np.concatenate([(chain <= thr[p][None, None, :]).astype(np.float64) for p in range(2)], axis=2)          # [sample][walker][2 ndim]
    ith = ind.transpose(1, 0, 2)
    dbl, res["doubles_ms"] = timed(lambda: kmc.lag_sums(ith, None, 1, L, moments=False))
    _, res["doubles_upload_ms"] = timed(lambda: kmc.lag_sums(ith, None, 1, 0, moments=False))
    want = dbl["lagsum"].reshape(2, nd, L)
    res["same_counts"] = bool(np.array_equal(bits["lagcount"].astype(np.float64), want) and bits_host["lagcount"].tobytes() == bits["lagcount"].tobytes())
    res.update(m=int(q3["m"]), h=int(h), lags=int(L))
    print("RESULT " + json.dumps(res), flush=True)


def derive(row):
    med = lambda k: row[k]["median"]
    row["bits_over_doubles_device"] = med("bits_sampler_ms") / (med("doubles_ms") - med("doubles_upload_ms"))
    row["bits_over_doubles_host"] = med("bits_host_ms") / med("doubles_ms")
    row["bits_lagcounts_ms"] = med("bits_sampler_ms") - med("bits_sampler_pack_ms")
    row["doubles_lagsums_ms"] = med("doubles_ms") - med("doubles_upload_ms")
    row["lag_kernels_bits_over_doubles"] = row["bits_lagcounts_ms"] / row["doubles_lagsums_ms"]
    row["whole16_over_whole3"] = med("whole16_ms") / med("whole3_ms")
    for tag in ("3", "16"):
        rest = med(f"whole{tag}_ms") - med("sort_ms") - med(f"pack{tag}_ms") - med(f"lagcounts{tag}_ms")
        row[f"split{tag}_ms"] = dict(sort=med("sort_ms"), pack=med(f"pack{tag}_ms"), lag_counts=med(f"lagcounts{tag}_ms"), picks_and_host=rest)
    row["whole3_over_rank_convergence"] = med("whole3_ms") / med("rank_convergence_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantile_mcse.json"))
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default=",".join(str(i) for i in range(len(CASES))))
    ap.add_argument("--child-timeout", type=int, default=300)
    a = ap.parse_args()
    if a.child >= 0:
        return child(a.child)
    rec = dict(device="MI355X", density="GaussianIso(0, 1)",
               timing="HIP events around each blocking call, one untimed call first; median of %d child processes (min, max)" % a.repeats,
               stage="indicator_lags, 2 probabilities (q05, q95), lags 1 .. min(32, h - 1), against kmc_chain_lag_sums over the same indicators as doubles",
               whole="Sampler.quantile_mcse with 3 and 16 probabilities; the split is pieced together from separate calls (see the script)",
               probs3=PROBS3, probs16=PROBS16, cases=[])
    if os.path.exists(a.out) and len(a.cases.split(",")) < len(CASES):                # (one case per run: keep the others)
        with open(a.out) as f:
            rec["cases"] = [c for c in json.load(f).get("cases", []) if c["case"] not in [CASES[int(v)][0] for v in a.cases.split(",")]]
    for idx in (int(v) for v in a.cases.split(",")):
        name, nw, nd, ns = CASES[idx]
        runs = []
        for _ in range(a.repeats):
            p = subprocess.run(["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", str(idx)],
                               stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:                     # a fault or a time limit: nothing more is started on the device
                raise SystemExit(f"child for {name} ended with status {p.returncode}")
            runs.append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
            print(f"{name}: process {len(runs)} of {a.repeats} done", flush=True)
        r0 = runs[0]
        row = dict(case=name, nwalkers=nw, ndim=nd, nsamples=ns)
        for key in ("m", "h", "lags", "lags3", "lags16", "info3", "info16"):
            row[key] = r0[key]
        row["same_counts"] = all(r["same_counts"] for r in runs)
        for key in r0:
            if key.endswith("_ms"):
                row[key] = spread([r[key] for r in runs])
        derive(row)
        rec["cases"].append(row)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
