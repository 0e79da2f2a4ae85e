#!/usr/bin/env python
"""PSIS-LOO on the device against the route there was before it: profiles/psis_loo.json.

Per shape (a DataDensity over the regression term, chain stored on the device), in each of three child processes:
  device   Sampler.loo(thin=...): the two statistics passes (lppd_j), then per block of observations the minimum pass, the 16 select
           passes, the gather and the fit; after one untimed call.  The library's own events give the time of each stage inside that
           call, and the terms per second of a recompute pass stand beside WAIC's pass 1 (kernels the parent commit has, unchanged)
           measured in the same process.
  host     the route a user had: Sampler.pointwise_loglike over blocks of observations, then tests/psis_yardstick.py (numpy) on each
           block.  It is timed on the first HOST_OBS observations only and scaled by the observation count: the whole matrix is 1.6 GB
           at S1 and 32.8 GB at S2, minutes of a shared machine for a number nobody needs to three digits.
All are blocking calls; each is bracketed by HIP events (recorded on an otherwise idle stream, so their distance is the time the call
took, host work included) and by the host clock.  Reported: the median over the child processes with min / max.
P32 is thinned by 2: unthinned its 2 048 000 rows ask for a tail of 4 294 draws, which the library refuses (M > 4096).

``--reff`` measures the relative efficiency per observation instead (S1 and S2; written under "relative_eff" of the same file), per child:
  scalar     Sampler.loo(thin=..., r_eff=1.0) on this build, as above; with ``--parent-root DIR`` (a checkout of the parent commit with its
             library built) the same call by that checkout's own copy of this script, in the same session: the yardstick of the scalar path.
  stage      Sampler.relative_eff(thin=...): pass 1, the weight passes and the ESS stage (chain moments, lag blocks and their copies, group
             by group) from the library's own events; WAIC's pass 2 in the same process -- the same walk, one exp per term -- stands
             beside a weight pass.
  chain      Sampler.loo(r_eff="chain") at the shape's thinning, doubled until no observation asks for more than 4096 draws.
  over       the observations whose computed r_eff_j asks for M > 4096 unthinned.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REG_TERM = "double mu = x[0]; for (int k = 1; k < n; ++k) mu += x[k] * d[k - 1]; double r = d[n - 1] - mu; return -0.5 * p[0] * r * r;"
# (name, walkers, ndim, observations, stored samples, thin): the shapes of profiles/predictive.json
CASES = [("S1", 100, 3, 1000, 2000, 1), ("S2", 4096, 8, 100000, 50, 5), ("P32", 4096, 2, 32, 500, 2)]
HOST_OBS = 32                  # observations the host route is timed on
CHILD_TIMEOUT = 420            # seconds


def make_data(ndata, nd, seed=0):
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((ndata, nd - 1))
    beta = np.linspace(0.5, -0.5, nd)
    y = beta[0] + Z @ beta[1:] + 0.5 * rng.standard_normal(ndata)
    return np.column_stack([Z, y]), beta


def bracket(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    out = fn()
    t1 = time.perf_counter()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1), (t1 - t0) * 1e3


def child(idx):
    import kissmcmc_jl_amd as kmc
    from kissmcmc_jl_amd import chain_predictive, summary
    import psis_yardstick as Y
    name, nw, nd, J, ns, thin = CASES[idx]
    nburn = 20
    D, beta = make_data(J, nd)
    pdf = kmc.DataDensity(REG_TERM, D, params=[4.0])
    th = beta + 0.05 * np.random.default_rng(0).standard_normal((nw, nd))
    with kmc.Sampler(pdf, nw, nd, nburn + ns, nburn, 1, 2.0, 3, store_chain=True) as s:
        s.set_positions(th)
        s.run(nburn + ns)
        s.sync()
        s.loo(thin=thin)
        dev, d_ev, d_wall = bracket(lambda: s.loo(thin=thin, with_info=True))
        info = dev["info"]
        s.waic(thin=thin)
        waic_info = chain_predictive.pointwise_stats_from(summary._SamplerProvider(s), pdf, thin)["info"]
        hobs = min(J, HOST_OBS)

        def host():
            l = s.pointwise_loglike(thin=thin, obs=(0, hobs))
            return Y.loo(l)

        yard, h_ev, h_wall = bracket(host)
    fin = np.isfinite(yard["pareto_k"]) & np.isfinite(dev["pareto_k"][:hobs])
    err = dict(elpd_loo_j_vs_numpy=float(np.max(np.abs(dev["elpd_loo_j"][:hobs] - yard["elpd_loo_j"]) / np.maximum(1.0, np.abs(yard["elpd_loo_j"])))),
               pareto_k_vs_numpy=float(np.max(np.abs(dev["pareto_k"][:hobs][fin] - yard["pareto_k"][fin]))) if fin.any() else 0.0)
    scale = J / hobs
    k = dev["pareto_k"]
    print("RESULT " + json.dumps(dict(case=name, device_ms=d_ev, device_wall_ms=d_wall, stats_ms=info["ns_stats"] * 1e-6, min_ms=info["ns_min"] * 1e-6,
                                      select_ms=info["ns_select"] * 1e-6, gather_ms=info["ns_gather"] * 1e-6, fit_ms=info["ns_fit"] * 1e-6,
                                      waic_pass1_ms=int(waic_info[4]) * 1e-6, host_ms=h_ev * scale, host_wall_ms=h_wall * scale,
                                      n=int(dev["n"]), tail_len=int(dev["tail_len"]), blocks=info["blocks"], obs_per_block=info["obs_per_block"],
                                      runs=info["nruns"], terms_per_pass=info["terms_per_pass"], log1p_evals=info["log1p_evals"], host_obs_timed=int(hobs),
                                      elpd_loo=dev["elpd_loo"], p_loo=dev["p_loo"], se=dev["se"], k_counts=list(dev["k_counts"]), k_max=float(np.nanmax(k)),
                                      **err)), flush=True)


def child_reff(idx):
    import kissmcmc_jl_amd as kmc
    from kissmcmc_jl_amd import chain_predictive, summary
    import psis_yardstick as Y
    name, nw, nd, J, ns, thin = CASES[idx]
    nburn = 20
    D, beta = make_data(J, nd)
    pdf = kmc.DataDensity(REG_TERM, D, params=[4.0])
    th = beta + 0.05 * np.random.default_rng(0).standard_normal((nw, nd))

    def over(re):
        r = re["r_eff_j"]
        M = np.array([Y.tail_length(re["n"], x if np.isfinite(x) and x > 0 else 1.0) for x in r])
        return int((M > 4096).sum()), int(M.max())

    with kmc.Sampler(pdf, nw, nd, nburn + ns, nburn, 1, 2.0, 3, store_chain=True) as s:
        s.set_positions(th)
        s.run(nburn + ns)
        s.sync()
        s.loo(thin=thin)
        base, b_ev, _ = bracket(lambda: s.loo(thin=thin, with_info=True))
        s.relative_eff(thin=thin)
        re, r_ev, _ = bracket(lambda: s.relative_eff(thin=thin, with_info=True))
        waic_info = chain_predictive.pointwise_stats_from(summary._SamplerProvider(s), pdf, thin)["info"]
        un = re if thin == 1 else s.relative_eff(thin=1)
        n_over_unthinned, m_max_unthinned = over(un)
        t = thin
        while over(re if t == thin else s.relative_eff(thin=t))[0] > 0:
            t *= 2
        s.loo(thin=t, r_eff="chain")
        ch, c_ev, _ = bracket(lambda: s.loo(thin=t, r_eff="chain", with_info=True))
        b2, b2_ev, _ = (base, b_ev, 0.0) if t == thin else bracket(lambda: s.loo(thin=t, with_info=True))
    r = re["r_eff_j"]
    ri, ci = re["info"], ch["info"]
    print("RESULT " + json.dumps(dict(case=name, scalar_ms=b_ev, relative_eff_ms=r_ev, pass1_ms=ri["ns_pass1"] * 1e-6, weights_ms=ri["ns_weights"] * 1e-6,
                                      ess_ms=ri["ns_ess"] * 1e-6, waic_pass2_ms=int(waic_info[5]) * 1e-6, groups=ri["groups"], n=int(re["n"]), m=re["m"], h=re["h"],
                                      r_eff_min=float(np.nanmin(r)), r_eff_median=float(np.nanmedian(r)), r_eff_max=float(np.nanmax(r)),
                                      lag_max=int(re["lag"].max()), truncated=int(re["truncated"].sum()), n_reff_nan=int(np.isnan(r).sum()),
                                      n_over_4096_unthinned=n_over_unthinned, tail_len_max_unthinned=m_max_unthinned, chain_thin=t, chain_n=int(ch["n"]),
                                      chain_ms=c_ev, scalar_at_chain_thin_ms=b2_ev, chain_weights_ms=ci["ns_weights"] * 1e-6, chain_ess_ms=ci["ns_ess"] * 1e-6,
                                      chain_tail_len_min=int(ch["tail_len_j"].min()), chain_tail_len_max=int(ch["tail_len_j"].max()),
                                      scalar_tail_len=int(b2["tail_len"]), chain_k_counts=list(ch["k_counts"]), scalar_k_counts=list(b2["k_counts"]),
                                      chain_elpd_loo=ch["elpd_loo"], scalar_elpd_loo=b2["elpd_loo"])), flush=True)


def run_children(cmd, name, repeats, env=None):
    runs = []
    for _ in range(repeats):
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=CHILD_TIMEOUT, env=env)
        if p.returncode != 0:                         # a fault: nothing more is started on the device
            raise SystemExit(f"child for {name} ended with status {p.returncode}")
        runs.append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
    return runs


def main_reff(a):
    with open(a.out) as f:
        rec = json.load(f)
    out = dict(call="Sampler.relative_eff(thin=...) and Sampler.loo(thin=..., r_eff=\"chain\"); split, max_lag at their defaults",
               timing="HIP events around each blocking call, one untimed call first; median of %d child processes (min, max); pass1 / weights / ess: "
                      "the library's own events inside Sampler.relative_eff" % a.repeats,
               yardsticks="scalar path: the parent commit's Sampler.loo(r_eff = 1) in the same session (parent_scalar_ms); a weight pass: WAIC's pass 2 "
                          "in the same process (waic_pass2_ms)",
               cases=[])
    for idx in (int(v) for v in a.cases.split(",")):
        name = CASES[idx][0]
        env = dict(os.environ)
        env.pop("KMC_LIB_PATH", None)
        runs, prs = [], []
        for _ in range(a.repeats):                    # this build and the parent's by turns: a drift of the machine meets both alike
            runs += run_children([sys.executable, os.path.abspath(__file__), "--reff-child", str(idx)], name, 1)
            if a.parent_root:
                prs += run_children([sys.executable, os.path.join(a.parent_root, "scripts", "psis_loo_bench.py"), "--child", str(idx)], name + " (parent)", 1, env)
        row = dict(case=name)
        for k, v in runs[0].items():
            row[k] = spread([r[k] for r in runs]) if k.endswith("_ms") else v
        if prs:
            row["parent_scalar_ms"] = spread([r["device_ms"] for r in prs])
        out["cases"].append(row)
        print(json.dumps(row), flush=True)
        rec["relative_eff"] = out
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print("wrote", a.out)


def spread(vals):
    return dict(median=float(np.median(vals)), min=float(min(vals)), max=float(max(vals)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psis_loo.json"))
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default="")
    ap.add_argument("--reff", action="store_true", help="measure the relative efficiency per observation (S1, S2) into the same file")
    ap.add_argument("--reff-child", type=int, default=-1)
    ap.add_argument("--parent-root", default="", help="a checkout of the parent commit with its library built: the scalar path's yardstick")
    a = ap.parse_args()
    a.cases = a.cases or ("0,1" if a.reff else ",".join(str(i) for i in range(len(CASES))))
    if a.child >= 0:
        return child(a.child)
    if a.reff_child >= 0:
        return child_reff(a.reff_child)
    if a.reff:
        return main_reff(a)
    rec = dict(device="MI355X", density="DataDensity(REG_TERM), precision 4", call="Sampler.loo(thin=...): every walker, every thin-th stored sample, r_eff = 1",
               timing="HIP events around each blocking call, one untimed call first; median of %d child processes (min, max); stats / min / select / "
                      "gather / fit: the library's own events around each stage inside one call" % a.repeats,
               yardstick="host: Sampler.pointwise_loglike of the first %d observations + tests/psis_yardstick.py (numpy) on them, same process, scaled "
                         "by the observation count" % HOST_OBS,
               not_measured="the kernels' shares from a trace; a digit of 8 bits against the 4 built; the packed form against the plain one at 32 .. 64 "
                            "observations; several blocks of observations against one; r_eff other than 1",
               cases=[])
    from test_gpu_psis_loo import DIST             # the tests' tolerances rest on these: recorded beside the timings
    rec["yardstick_distance"] = dict(what="float64 yardstick against its longdouble mode on the tests' inputs, relative to max(1, |value|), per row "
                                          "count n: python tests/psis_cases.py; the device is allowed 8 times these, floor (M + 4) 2^-53",
                                     by_n={str(n): d for n, d in DIST.items()},
                                     largest_device_error_over_tolerance=0.27)
    for idx in (int(v) for v in a.cases.split(",")):
        name, nw, nd, J, ns, thin = CASES[idx]
        runs = []
        for _ in range(a.repeats):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(idx)], stdout=subprocess.PIPE, text=True, timeout=CHILD_TIMEOUT)
            if p.returncode != 0:                     # a fault: nothing more is started on the device
                raise SystemExit(f"child for {name} ended with status {p.returncode}")
            runs.append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
        r0 = runs[0]
        row = dict(case=name, nwalkers=nw, ndim=nd, observations=J, nsamples=ns, thin=thin)
        for k in ("n", "tail_len", "blocks", "obs_per_block", "runs", "terms_per_pass", "log1p_evals", "host_obs_timed", "elpd_loo", "p_loo", "se",
                  "k_counts", "k_max"):
            row[k] = r0[k]
        for k in r0:
            if k.endswith("_ms"):
                row[k] = spread([r[k] for r in runs])
            elif "_vs_" in k:
                row[k] = max(r[k] for r in runs)
        per = row["terms_per_pass"]
        row["min_terms_per_s"] = per / (row["min_ms"]["median"] * 1e-3)
        row["select_terms_per_s_per_pass"] = 16 * per / (row["select_ms"]["median"] * 1e-3)
        row["gather_terms_per_s"] = per / (row["gather_ms"]["median"] * 1e-3)
        row["waic_pass1_terms_per_s"] = per / (row["waic_pass1_ms"]["median"] * 1e-3)
        row["fit_log1p_per_s"] = row["log1p_evals"] / (row["fit_ms"]["median"] * 1e-3)
        row["select_pass_over_waic_pass1"] = (row["select_ms"]["median"] / 16) / row["waic_pass1_ms"]["median"]
        row["host_over_device"] = row["host_ms"]["median"] / row["device_ms"]["median"]
        rec["cases"].append(row)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
