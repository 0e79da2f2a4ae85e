#!/usr/bin/env python
"""Posterior summaries on the device against the route a user had before them: profiles/posterior_summary.json.

Per shape (a menu Gaussian, chain and log-densities stored on the device), in each of three child processes:
  device   Sampler.quantiles([0.16, 0.5, 0.84], logp=True) and Sampler.map_sample(), after one untimed call of each;
  host     s.chain() followed by np.quantile(..., axis=0) of the chain and of the log-densities / np.argmax -- the yardstick: what the
           same summary cost without these calls, timed in the same process.
Both are blocking calls; each is bracketed by HIP events (recorded on an otherwise idle stream, so their distance is the time the call
took, host work included) and by the host clock.  Reported: the median over the three processes with min / max, the bytes the select
reads (passes x selected chain bytes, log-densities included) and that byte count per second against the 6.29 TB/s a plain copy
reaches on this card (README "Measured").  The middle shape is run once more with every walker started at the same point: the chain is
then one value repeated, every lane of a wave hits one counter -- the contention case of the LDS histogram.
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

COPY_BPS = 6.29e12
Q = [0.16, 0.5, 0.84]
PASSES = 8
# (name, walkers, ndim, stored samples, all walkers at one point)
CASES = [("65536x32x50", 65536, 32, 50, False), ("4096x8x2000", 4096, 8, 2000, False), ("100x3x10000", 100, 3, 10000, False),
         ("4096x8x2000-all-equal", 4096, 8, 2000, True)]


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
    name, nw, nd, ns, equal = CASES[idx]
    nburn = 20
    th = np.zeros((nw, nd)) if equal else np.random.default_rng(0).standard_normal((nw, nd))
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, nburn + ns, nburn, 1, 2.0, 3, store_chain=True, store_logp=True) as s:
        s.set_positions(th)
        s.run(nburn + ns)
        s.sync()
        run_ms = s.last_run_ms()
        s.quantiles(Q, logp=True)
        s.map_sample()
        (qd, qlp), q_ev, q_wall = bracket(lambda: s.quantiles(Q, logp=True))
        md, m_ev, m_wall = bracket(lambda: s.map_sample())

        def host_quantiles():
            ch, lp = s.chain()
            return np.quantile(ch.reshape(-1, nd), Q, axis=0), np.quantile(lp.ravel(), Q), ch, lp

        (hq, hlp, ch, lp), hq_ev, hq_wall = bracket(host_quantiles)
        del ch, lp

        def host_map():
            ch, lp = s.chain()
            k, w = np.unravel_index(np.argmax(lp), lp.shape)
            return ch[k, w].copy(), lp[k, w], int(k), int(w)

        hm, hm_ev, hm_wall = bracket(host_map)
    agree = bool(np.all(np.abs(qd - hq) <= np.spacing(np.abs(hq))) and np.all(np.abs(qlp - hlp) <= np.spacing(np.abs(hlp))) and
                 md[2:] == hm[2:] and np.array_equal(md[0], hm[0]))
    print("RESULT " + json.dumps(dict(case=name, sampling_ms=run_ms, device_quantiles_ms=q_ev, device_quantiles_wall_ms=q_wall, device_map_ms=m_ev,
                                      device_map_wall_ms=m_wall, host_quantiles_ms=hq_ev, host_quantiles_wall_ms=hq_wall, host_map_ms=hm_ev,
                                      host_map_wall_ms=hm_wall, device_equals_host=agree)), flush=True)


def spread(vals):
    return dict(median=float(np.median(vals)), min=float(min(vals)), max=float(max(vals)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_summary.json"))
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default=",".join(str(i) for i in range(len(CASES))))
    a = ap.parse_args()
    if a.child >= 0:
        return child(a.child)
    rec = dict(device="MI355X", density="GaussianIso(0, 1)", q=Q, copy_bytes_per_s=COPY_BPS, select_passes=PASSES,
               timing="HIP events around each blocking call, one untimed call first; median of %d child processes (min, max)" % a.repeats,
               yardstick="s.chain() + np.quantile / np.argmax on the host, same process", cases=[])
    for idx in (int(v) for v in a.cases.split(",")):
        name, nw, nd, ns, equal = CASES[idx]
        runs = []
        for _ in range(a.repeats):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(idx)], stdout=subprocess.PIPE, text=True, timeout=600)
            if p.returncode != 0:                     # a fault: nothing more is started on the device
                raise SystemExit(f"child for {name} ended with status {p.returncode}")
            runs.append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
        chain_bytes = ns * nw * ((nd + nd % 2) * 8 + 8)                   # what a pass reads: padded rows and the log-densities
        row = dict(case=name, nwalkers=nw, ndim=nd, nsamples=ns, all_equal=equal, chain_bytes=chain_bytes, select_bytes=PASSES * chain_bytes,
                   device_equals_host=all(r["device_equals_host"] for r in runs))
        for k in runs[0]:
            if k.endswith("_ms"):
                row[k] = spread([r[k] for r in runs])
        row["select_bytes_per_s"] = row["select_bytes"] / (row["device_quantiles_ms"]["median"] * 1e-3)
        row["select_fraction_of_copy_rate"] = row["select_bytes_per_s"] / COPY_BPS
        row["host_over_device_quantiles"] = row["host_quantiles_ms"]["median"] / row["device_quantiles_ms"]["median"]
        row["host_over_device_map"] = row["host_map_ms"]["median"] / row["device_map_ms"]["median"]
        rec["cases"].append(row)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
