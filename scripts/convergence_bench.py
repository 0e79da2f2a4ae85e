#!/usr/bin/env python
"""Convergence diagnostics on the device against the route a user had before them: profiles/convergence.json.

Per shape (a menu Gaussian, chain stored on the device), in each of three child processes:
  device   Sampler.convergence(): the chain moments, lag blocks until every column's truncation rule has fired, the host stage;
           after one untimed call;
  host     s.chain() followed by the same formulas in plain numpy on the host (chain means and variances, then D_t for 32, 64, 128,
           ... lags until the rule has fired, one subtraction, one square and one np.sum per lag; the host stage is the library's
           own, which needs no device) -- the yardstick: what the same columns cost without these calls, timed in the same process.
Both are blocking calls; each is bracketed by HIP events (recorded on an otherwise idle stream, so their distance is the time the call
took, host work included) and by the host clock.  Reported: the median over the three processes with min / max; the lags computed, the
blocks of 32 lags run and the bytes of the chain the lag kernel and the moment kernels loaded (counted by the library from the shapes:
rows of every window that lie inside a half x selected walkers x columns x element size), that byte count per second of the whole call,
and the terms (x[i] - x[i - t])^2 summed.
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

# (name, walkers, ndim, stored samples)
CASES = [("65536x32x50", 65536, 32, 50), ("4096x8x2000", 4096, 8, 2000), ("100x3x10000", 100, 3, 10000)]


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


def host_route(kmc, chain):
    """The same columns from a chain [sample][walker][dim] in host memory, in plain numpy."""
    ns, nw, nd = chain.shape
    h = ns // 2
    x = np.concatenate([chain[:h], chain[ns - h:]], axis=1)                        # [h][m][nd], chain j = half * nw + walker
    m = 2 * nw
    cm = x.mean(axis=0)
    cv = ((x - cm) ** 2).sum(axis=0) / (h - 1)
    max_lag, have, lag = min(h - 1, 1024), 0, np.zeros((nd, 0))
    while True:
        want = min(max_lag, 32 if have == 0 else 2 * have)
        new = np.empty((nd, want - have))
        for t in range(have + 1, want + 1):
            d = x[t:] - x[:h - t]
            d *= d
            new[:, t - have - 1] = d.sum(axis=(0, 1))
        lag, have = np.concatenate([lag, new], axis=1), want
        st = kmc.convergence_stats(m, h, cm.T.copy(), cv.T.copy(), lag, max_lag)
        if not (st["flags"] & 1).any():
            return st, have


def child(idx):
    import kissmcmc_jl_amd as kmc
    from kissmcmc_jl_amd import chain_convergence
    name, nw, nd, ns = CASES[idx]
    nburn = 20
    th = np.random.default_rng(0).standard_normal((nw, nd))
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, nburn + ns, nburn, 1, 2.0, 3, store_chain=True) as s:
        s.set_positions(th)
        s.run(nburn + ns)
        s.sync()
        run_ms = s.last_run_ms()
        s.convergence()
        dev, d_ev, d_wall = bracket(lambda: s.convergence())
        info = chain_convergence.sampler_convergence_raw(s)["info"]
        (st, host_lags), h_ev, h_wall = bracket(lambda: host_route(kmc, s.chain(logp=False)[0]))
    agree = bool(np.array_equal(dev["lag"], st["T"]) and np.allclose(dev["ess"], st["ess"], rtol=1e-6) and np.allclose(dev["rhat"], st["rhat"], rtol=1e-9))
    print("RESULT " + json.dumps(dict(case=name, sampling_ms=run_ms, device_ms=d_ev, device_wall_ms=d_wall, host_ms=h_ev, host_wall_ms=h_wall,
                                      lags=int(info[0]), lag_blocks=int(info[1]), lag_bytes=int(info[2]), moment_bytes=int(info[3]),
                                      host_lags=int(host_lags), device_equals_host=agree, m=int(dev["m"]), h=int(dev["h"]),
                                      rhat_max=float(np.max(dev["rhat"])), ess_min=float(np.min(dev["ess"])), lag_max=int(np.max(dev["lag"])))), flush=True)


def spread(vals):
    return dict(median=float(np.median(vals)), min=float(min(vals)), max=float(max(vals)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convergence.json"))
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default=",".join(str(i) for i in range(len(CASES))))
    a = ap.parse_args()
    if a.child >= 0:
        return child(a.child)
    rec = dict(device="MI355X", density="GaussianIso(0, 1)", call="Sampler.convergence(): split chains, every walker a chain, max_lag min(h - 1, 1024)",
               timing="HIP events around each blocking call, one untimed call first; median of %d child processes (min, max)" % a.repeats,
               yardstick="s.chain() + the same formulas in plain numpy on the host, same process", cases=[])
    for idx in (int(v) for v in a.cases.split(",")):
        name, nw, nd, ns = CASES[idx]
        runs = []
        for _ in range(a.repeats):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(idx)], stdout=subprocess.PIPE, text=True, timeout=900)
            if p.returncode != 0:                     # a fault: nothing more is started on the device
                raise SystemExit(f"child for {name} ended with status {p.returncode}")
            runs.append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
        r0 = runs[0]
        row = dict(case=name, nwalkers=nw, ndim=nd, nsamples=ns, chain_bytes=ns * nw * (nd + nd % 2) * 8,
                   device_equals_host=all(r["device_equals_host"] for r in runs))
        for k in ("m", "h", "lags", "lag_blocks", "lag_bytes", "moment_bytes", "host_lags", "rhat_max", "ess_min", "lag_max"):
            row[k] = r0[k]
        row["terms"] = sum(r0["m"] * (r0["h"] - t) for t in range(1, r0["lags"] + 1)) * nd
        for k in r0:
            if k.endswith("_ms"):
                row[k] = spread([r[k] for r in runs])
        row["bytes_per_s"] = (row["lag_bytes"] + row["moment_bytes"]) / (row["device_ms"]["median"] * 1e-3)
        row["terms_per_s"] = row["terms"] / (row["device_ms"]["median"] * 1e-3)
        row["host_over_device"] = row["host_ms"]["median"] / row["device_ms"]["median"]
        rec["cases"].append(row)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
