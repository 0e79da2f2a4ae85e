#!/usr/bin/env python
"""Rank-normalised convergence diagnostics on the device against the routes there were before: profiles/rank_convergence.json.

Per shape (a menu Gaussian, chain stored on the device), in each of three child processes, every call blocking and bracketed by HIP
events after one untimed call:
  device   Sampler.rank_convergence(): gather, two segmented radix sorts (the draws, the folded draws), the scores, and the lag
           schedule of Sampler.convergence() over the four transformed column sets;
  scores   Sampler.rank_scores() and Sampler.rank_scores(folded=True): the ranking stages alone, with rank2 and z copied to the host;
  plain    Sampler.convergence(): what the rank form costs over the plain one;
  host     s.chain() followed by the same definitions in numpy on the host (np.sort + np.searchsorted per column for the ranks, the
           vectorised normal score, the fold and the indicators, then the lag schedule of scripts/convergence_bench.py's host route
           over the 4 ncols transformed columns) -- the route there was before;
  torch    torch.sort along the column axis of the same [ncols, S] double tensor on the device: a yardstick for the sort stage alone.
Reported: the median over the processes with min / max; the bytes the two sorts moved (counted by the library: 8 passes x (two reads and
one write of the keys) x 2 sorts) per second of the whole call, against the 6.29 TB/s copy rate -- a lower bound of the sort kernels'
own rate, since the stages are not bracketed one by one; the whole call over the plain one and over the numpy route.
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

COPY_RATE = 6.29e12


def scores_host(rank2, S):
    """The normal score on arrays (AS 241; the operation order of include/kissmcmc_hip.h, np.log for the tails)."""
    A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4, 1.3731693765509461125e+4,
         1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0)
    B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4, 5.3941960214247511077e+3,
         6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0)
    Cc = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0, 3.64784832476320460504e+0,
          5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0)
    D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1, 6.89767334985100004550e-1,
         1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0)
    E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2, 2.96560571828504891230e-1,
         1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0)
    F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4, 1.48753612908506148525e-2,
         1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0)

    def horner(co, r):
        acc = co[0] * r + co[1]
        for c in co[2:]:
            acc = acc * r + c
        return acc
    p = (rank2.astype(np.float64) * 0.5 - 0.375) / (S + 0.25)
    q = p - 0.5
    z = np.empty_like(p)
    mid = np.abs(q) <= 0.425
    r = 0.180625 - q[mid] * q[mid]
    z[mid] = horner(A, r) * q[mid] / horner(B, r)
    pt, qt = p[~mid], q[~mid]
    r = np.sqrt(-np.log(np.where(qt <= 0.0, pt, 1.0 - pt)))
    x = np.where(r <= 5.0, horner(Cc, r - 1.6) / horner(D, r - 1.6), horner(E, r - 5.0) / horner(F, r - 5.0))
    z[~mid] = np.where(qt < 0.0, -x, x)
    return z


def rank2_host(v):
    s = np.sort(v)
    return np.searchsorted(s, v, side="left") + np.searchsorted(s, v, side="right") + 1, s


def quantile_host(s, q):
    hq = q * (s.size - 1)
    lo = int(np.floor(hq))
    hi = min(lo + 1, s.size - 1)
    return s[lo] if hq == lo else s[lo] + (hq - lo) * (s[hi] - s[lo])


def host_route(kmc, chain):
    """Rank-normalised diagnostics from a chain [sample][walker][dim] in host memory, in numpy."""
    from convergence_bench import host_route as lag_route
    ns, nw, nd = chain.shape
    h = ns // 2
    x = np.concatenate([chain[:h], chain[ns - h:]], axis=1)                        # [h][m][nd]
    m, S = 2 * nw, 2 * nw * h
    t = np.empty((h, m, 4 * nd))
    for c in range(nd):
        v = x[:, :, c].ravel() + 0.0
        r2, s = rank2_host(v)
        med, q05, q95 = quantile_host(s, 0.5), quantile_host(s, 0.05), quantile_host(s, 0.95)
        t[:, :, c] = scores_host(r2, S).reshape(h, m)
        t[:, :, nd + c] = scores_host(rank2_host(np.abs(v - med) + 0.0)[0], S).reshape(h, m)
        t[:, :, 2 * nd + c] = (v <= q05).reshape(h, m)
        t[:, :, 3 * nd + c] = (v <= q95).reshape(h, m)
    # the lag schedule of the plain diagnostics over the transformed chain
    return lag_route(kmc, _unsplit(t))                                             # (its split cuts the halves apart again)


def _unsplit(t):
    """[h][2 nw][cols] with chain j = half * nw + k -> [2 h][nw][cols], which the split of convergence_bench.host_route cuts back."""
    h, m, cols = t.shape
    nw = m // 2
    return np.concatenate([t[:, :nw], t[:, nw:]], axis=0)


def child(idx, with_host=True):
    import torch

    import kissmcmc_jl_amd as kmc
    from kissmcmc_jl_amd import chain_convergence
    name, nw, nd, ns = CASES[idx]
    nburn = 20
    th = np.random.default_rng(0).standard_normal((nw, nd))
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, nburn + ns, nburn, 1, 2.0, 3, store_chain=True) as s:
        s.set_positions(th)
        s.run(nburn + ns)
        s.sync()
        s.rank_convergence()
        dev, d_ev, d_wall = bracket(lambda: s.rank_convergence())
        info = chain_convergence.sampler_rank_convergence_raw(s)["info"]
        sc, sc_ev, _ = bracket(lambda: (s.rank_scores(), s.rank_scores(folded=True)))
        s.convergence()
        _, p_ev, _ = bracket(lambda: s.convergence())
        chain = s.chain(logp=False)[0]
        if with_host:
            (st, host_lags), h_ev, h_wall = bracket(lambda: host_route(kmc, s.chain(logp=False)[0]))
    h = ns // 2
    cols = torch.from_numpy(np.ascontiguousarray(np.concatenate([chain[:h], chain[ns - h:]], axis=1).reshape(-1, nd).T)).cuda()
    torch.sort(cols, dim=1)
    torch.cuda.synchronize()
    _, t_ev, _ = bracket(lambda: (torch.sort(cols, dim=1), torch.cuda.synchronize()))
    if with_host:
        agree = bool(np.array_equal(dev["lag"][0], st["T"][:nd]) and np.allclose(dev["rhat_bulk"], st["rhat"][:nd], rtol=1e-9) and
                     np.allclose(dev["rhat_folded"], st["rhat"][nd:2 * nd], rtol=1e-9) and np.allclose(dev["ess_bulk"], st["ess"][:nd], rtol=1e-6))
    else:
        agree, host_lags, h_ev, h_wall = None, -1, None, None
    print("RESULT " + json.dumps(dict(case=name, device_ms=d_ev, device_wall_ms=d_wall, scores_ms=sc_ev, plain_ms=p_ev, host_ms=h_ev, host_wall_ms=h_wall,
                                      torch_sort_ms=t_ev, lags=int(info[0]), sort_bytes=int(info[1]), lag_bytes=int(info[2]),
                                      moment_bytes=int(info[3]), host_lags=int(host_lags), device_equals_host=agree, m=int(dev["m"]),
                                      h=int(dev["h"]), rhat_max=float(np.nanmax(dev["rhat"])), ess_bulk_min=float(np.nanmin(dev["ess_bulk"])),
                                      ess_tail_min=float(np.nanmin(dev["ess_tail"])))), flush=True)


def derive(row):
    """What follows from the measured columns.  The stages of the device call are not bracketed one by one: the sort rate is over the
    time of the WHOLE call (a lower bound of the sort kernels' own rate), and rank_scores' time includes copying rank2 and z to the host."""
    dev = row["device_ms"]["median"]
    row["sort_bytes_per_s_of_whole_call"] = row["sort_bytes"] / (dev * 1e-3)
    row["of_copy_rate"] = row["sort_bytes_per_s_of_whole_call"] / COPY_RATE
    row["host_over_device"] = None if row["host_ms"] is None else row["host_ms"]["median"] / dev
    row["device_over_plain"] = dev / row["plain_ms"]["median"]
    row["one_sort_upper_bound_ms"] = 0.5 * (dev - row["plain_ms"]["median"])     # two sorts, two gathers and two score passes share this
    row["torch_sort_over_that_bound"] = row["torch_sort_ms"]["median"] / row["one_sort_upper_bound_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_convergence.json"))
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default=",".join(str(i) for i in range(len(CASES))))
    ap.add_argument("--child-timeout", type=int, default=400)
    ap.add_argument("--skip-host", action="store_true", help="leave the numpy route out (minutes at the middle shape): its columns are then null")
    a = ap.parse_args()
    if a.child >= 0:
        return child(a.child, not a.skip_host)
    rec = dict(device="MI355X", density="GaussianIso(0, 1)",
               call="Sampler.rank_convergence(): split chains, every walker a chain, max_lag min(h - 1, 1024)",
               timing="HIP events around each blocking call, one untimed call first; median of %d child processes (min, max)" % a.repeats,
               yardsticks="host: s.chain() + numpy (np.sort, np.searchsorted, the lag schedule); torch: torch.sort(dim=1) of the [ncols, S] doubles; plain: Sampler.convergence()",
               cases=[])
    for idx in (int(v) for v in a.cases.split(",")):
        name, nw, nd, ns = CASES[idx]
        runs = []
        for _ in range(a.repeats):
            p = subprocess.run(["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", str(idx)] +
                               (["--skip-host"] if a.skip_host else []),
                               stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:                     # a fault or a time limit: nothing more is started on the device
                raise SystemExit(f"child for {name} ended with status {p.returncode}")
            runs.append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
            print(f"{name}: process {len(runs)} of {a.repeats} done", flush=True)
        r0 = runs[0]
        row = dict(case=name, nwalkers=nw, ndim=nd, nsamples=ns, pooled_draws=r0["m"] * r0["h"],
                   device_equals_host=None if a.skip_host else all(r["device_equals_host"] for r in runs))
        for k in ("m", "h", "lags", "sort_bytes", "lag_bytes", "moment_bytes", "host_lags", "rhat_max", "ess_bulk_min", "ess_tail_min"):
            row[k] = r0[k]
        for k in r0:
            if k.endswith("_ms"):
                row[k] = None if r0[k] is None else spread([r[k] for r in runs])
        derive(row)
        rec["cases"].append(row)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
