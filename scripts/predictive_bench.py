#!/usr/bin/env python
"""WAIC on the device against the routes there were before it: profiles/predictive.json.

Per shape (a DataDensity over the regression term, chain stored on the device), in each of three child processes:
  device   Sampler.waic(thin=...): both passes over rows x observations, the two folds, the host stage; after one untimed call.  The
           library's own events give the time of each pass (partial kernel + fold) inside that call.
  host     the route a user had: s.chain(), then numpy over blocks of the [rows, observations] matrix, two passes (max and sum; then
           sum exp and centred squares).  At the large shape it is timed on the first HOST_ROWS rows only and scaled by the row count:
           the whole thing would take minutes of a shared machine for a number nobody needs to three digits.
  torch    the same blocks with torch on the device (float64), the chain and the data uploaded beforehand and not timed; one untimed
           call first.
All are blocking calls; each is bracketed by HIP events (recorded on an otherwise idle stream, so their distance is the time the call
took, host work included) and by the host clock.  Reported: the median over the child processes with min / max; terms per second of
the whole call (2 rows x observations term evaluations) and of each pass, beside the one figure on record for this term: the sampler's
kmc_data_lane at S2, DATA_LANE_TERMS_PER_S (profiles/data_density.json).
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

REG_TERM = "double mu = x[0]; for (int k = 1; k < n; ++k) mu += x[k] * d[k - 1]; double r = d[n - 1] - mu; return -0.5 * p[0] * r * r;"
# (name, walkers, ndim, observations, stored samples, thin): the README's two data shapes and one below 64 observations (the packed form)
CASES = [("S1", 100, 3, 1000, 2000, 1), ("S2", 4096, 8, 100000, 50, 5), ("P32", 4096, 2, 32, 500, 1)]
DATA_LANE_TERMS_PER_S = 7.3e11
HOST_ROWS = 2048               # S2: rows the numpy route is timed on
BLOCK_TERMS = 1 << 24          # terms of one block of the matrix (128 MiB of doubles)
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


def blocked_waic(xp, X, D, p0, sync=lambda: None):
    """lppd_j and p_waic_j over blocks of rows, with numpy or torch as ``xp``: what a user writes."""
    n, nd = X.shape
    J = D.shape[0]
    step = max(1, BLOCK_TERMS // J)

    def block(i):
        x = X[i:i + step]
        mu = x[:, 0:1] + x[:, 1:] @ D[:, :nd - 1].T
        r = D[:, nd - 1][None, :] - mu
        return -0.5 * p0 * r * r

    M, S = None, None
    for i in range(0, n, step):
        l = block(i)
        m = l.max(0) if xp is np else l.max(0).values
        M = m if M is None else xp.maximum(M, m)
        S = l.sum(0) if S is None else S + l.sum(0)
    c = S / n
    E = V = 0.0
    for i in range(0, n, step):
        l = block(i)
        E = E + xp.exp(l - M).sum(0)
        V = V + ((l - c) ** 2).sum(0)
    lppd = M + xp.log(E) - np.log(n)
    pw = V / (n - 1)
    sync()
    return lppd, pw


def child(idx):
    import torch
    import kissmcmc_jl_amd as kmc
    from kissmcmc_jl_amd import chain_predictive, summary
    name, nw, nd, J, ns, thin = CASES[idx]
    nburn = 20
    D, beta = make_data(J, nd)
    pdf = kmc.DataDensity(REG_TERM, D, params=[4.0])
    th = beta + 0.05 * np.random.default_rng(0).standard_normal((nw, nd))
    with kmc.Sampler(pdf, nw, nd, nburn + ns, nburn, 1, 2.0, 3, store_chain=True) as s:
        s.set_positions(th)
        s.run(nburn + ns)
        s.sync()
        run_ms = s.last_run_ms()
        s.waic(thin=thin)
        dev, d_ev, d_wall = bracket(lambda: s.waic(thin=thin))
        raw = chain_predictive.pointwise_stats_from(summary._SamplerProvider(s), pdf, thin)
        info = raw["info"]
        ll, m_ev, m_wall = bracket(lambda: s.pointwise_loglike(thin=thin, obs=(0, min(J, 64))))
        n = int(dev["n"])
        host_rows = n if n * J <= (1 << 29) else HOST_ROWS

        def host():
            X = s.chain(logp=False)[0][::thin].reshape(-1, nd)
            return blocked_waic(np, X[:host_rows], D, 4.0)

        (h_lppd, h_pw), h_ev, h_wall = bracket(host)
        X = s.chain(logp=False)[0][::thin].reshape(-1, nd)
    Xd, Dd = torch.from_numpy(np.ascontiguousarray(X)).cuda(), torch.from_numpy(D).cuda()
    tw = lambda: blocked_waic(torch, Xd, Dd, 4.0, torch.cuda.synchronize)
    tw()
    (t_lppd, t_pw), t_ev, t_wall = bracket(tw)
    t_lppd, t_pw = t_lppd.cpu().numpy(), t_pw.cpu().numpy()
    err = dict(lppd_vs_torch=float(np.max(np.abs(dev["lppd_j"] - t_lppd) / np.abs(t_lppd))), p_waic_vs_torch=float(np.max(np.abs(dev["p_waic_j"] - t_pw) / t_pw)))
    if host_rows == n:
        err["lppd_vs_numpy"] = float(np.max(np.abs(dev["lppd_j"] - h_lppd) / np.abs(h_lppd)))
    scale = n / host_rows
    print("RESULT " + json.dumps(dict(case=name, sampling_ms=run_ms, device_ms=d_ev, device_wall_ms=d_wall, pass1_ms=info[4] * 1e-6, pass2_ms=info[5] * 1e-6,
                                      matrix64_ms=m_ev, host_ms=h_ev * scale, host_wall_ms=h_wall * scale, torch_ms=t_ev, torch_wall_ms=t_wall,
                                      n=n, runs=int(info[1]), run_len=int(info[3]), terms=int(info[2]), host_rows_timed=int(host_rows),
                                      elpd_waic=dev["elpd_waic"], p_waic=dev["p_waic"], se=dev["se"], **err)), flush=True)


def spread(vals):
    return dict(median=float(np.median(vals)), min=float(min(vals)), max=float(max(vals)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictive.json"))
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default=",".join(str(i) for i in range(len(CASES))))
    a = ap.parse_args()
    if a.child >= 0:
        return child(a.child)
    rec = dict(device="MI355X", density="DataDensity(REG_TERM), precision 4", call="Sampler.waic(thin=...): every walker, every thin-th stored sample",
               timing="HIP events around each blocking call, one untimed call first; median of %d child processes (min, max); pass1 / pass2: the "
                      "library's own events around each pass inside one call" % a.repeats,
               yardsticks="host: s.chain() + numpy over blocks of the matrix, same process (S2: timed on %d rows, scaled by the row count); "
                          "torch: the same blocks in float64 on the device, uploads not timed" % HOST_ROWS,
               data_lane_terms_per_s=DATA_LANE_TERMS_PER_S,
               not_measured="the kernels' shares from a trace; the packed form against the plain one at 32 .. 64 observations; held-out data",
               cases=[])
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
        for k in ("n", "runs", "run_len", "terms", "host_rows_timed", "elpd_waic", "p_waic", "se"):
            row[k] = r0[k]
        for k in r0:
            if k.endswith("_ms"):
                row[k] = spread([r[k] for r in runs])
            elif "_vs_" in k:
                row[k] = max(r[k] for r in runs)
        per_pass = row["terms"] / 2
        row["terms_per_s"] = row["terms"] / (row["device_ms"]["median"] * 1e-3)
        row["pass1_terms_per_s"] = per_pass / (row["pass1_ms"]["median"] * 1e-3)
        row["pass2_terms_per_s"] = per_pass / (row["pass2_ms"]["median"] * 1e-3)
        row["pass1_share_of_data_lane"] = row["pass1_terms_per_s"] / DATA_LANE_TERMS_PER_S
        row["pass2_share_of_data_lane"] = row["pass2_terms_per_s"] / DATA_LANE_TERMS_PER_S
        row["host_over_device"] = row["host_ms"]["median"] / row["device_ms"]["median"]
        row["torch_over_device"] = row["torch_ms"]["median"] / row["device_ms"]["median"]
        rec["cases"].append(row)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
