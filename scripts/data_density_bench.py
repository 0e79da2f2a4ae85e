"""Data densities (kmc.DataDensity, KMC_DATA_DENSITY) against the two routes a user has without them: the host route
(HostLogPdf with a vectorised numpy callable -- the same terms and pairwise tree) and a torch-on-GPU evaluation of the same
log-likelihood batch.  Gaussian linear regression, ncols = ndim (ndim - 1 covariates and y), precision in p[0].

    python scripts/data_density_bench.py --out profiles/data_density.json          # the record
    python scripts/data_density_bench.py --profile S2                              # one shape's data route only (for rocprofv3)
    python scripts/data_density_bench.py --merge-stats DIR --out profiles/data_density.json   # add a rocprofv3 --stats run's kernel times

FLOPs per term are counted by hand from the body (REG_TERM below): mu = x[0] + sum_{k<n} x[k] d[k-1] is 2 (n - 1); the residual 1; the
two products of -0.5 p[0] r r 2; the add of the tree 1 -- 2 n + 2 in all (-0.5 * p[0] is loop-invariant and not counted).  The
kernels are compiled with -ffp-contract=off (the value contract), so these are separate v_mul_f64 / v_add_f64, and the spec figure
they are compared with -- AMD's published MI355X FP64 vector peak, 78.6 TFLOPS, not measured here -- counts an FMA as two FLOPs.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REG_TERM = "double mu = x[0]; for (int k = 1; k < n; ++k) mu += x[k] * d[k - 1]; double r = d[n - 1] - mu; return -0.5 * p[0] * r * r;"
SHAPES = {"S1": (100, 3, 1000), "S2": (4096, 8, 100000), "S3": (65536, 4, 10000)}
PEAK_FP64_VECTOR_SPEC = 78.6e12      # AMD's published MI355X figure (FMA = 2 FLOPs); not measured on this project's machines
GENS = {"S1": 2000, "S2": 20, "S3": 10}
HOST_GENS = {"S1": 200, "S2": 2, "S3": 1}


def flops_per_term(nd):
    return 2 * nd + 2


def pairwise(T):
    while T.shape[1] > 1:
        n = T.shape[1]
        S = T[:, 0:n - 1:2] + T[:, 1:n:2]
        T = np.concatenate([S, T[:, -1:]], axis=1) if n % 2 else S
    return T[:, 0]


def make_data(ndata, nd, seed=0):
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((ndata, nd - 1))
    beta = np.linspace(0.5, -0.5, nd)
    y = beta[0] + Z @ beta[1:] + 0.5 * rng.standard_normal(ndata)
    return np.column_stack([Z, y]), beta


def host_fn(D, p0):
    def rows(X):
        n = X.shape[1]
        mu = np.repeat(X[:, 0:1], D.shape[0], axis=1)
        for k in range(1, n):
            mu = mu + X[:, k:k + 1] * D[None, :, k - 1]
        r = D[None, :, n - 1] - mu
        return pairwise(-0.5 * p0 * r * r)

    def f(X):                                      # (in pieces of rows: the [rows, ndata] temporaries stay near 100 MB)
        step = max(1, int(1.2e7 // D.shape[0]))
        return np.concatenate([rows(X[i:i + step]) for i in range(0, X.shape[0], step)])
    return f


def time_route(kmc, pdf, nw, nd, th, gens, warm=2):
    with kmc.Sampler(pdf, nw, nd, gens + warm, 0, 1, 2.0, 7) as s:
        s.set_positions(th)
        s.run(warm)                                # warm: code objects, caches
        s.sync()
        t0 = time.perf_counter()
        s.run(gens)
        s.sync()
        wall = time.perf_counter() - t0
        dev_ms = s.last_run_ms()
        desc = s.describe()
    return wall, dev_ms, desc


def torch_batch(D, nd, nprop, reps=10):
    import torch
    dev = torch.device("cuda:0")
    Dt = torch.as_tensor(D, device=dev)
    Z, y = Dt[:, :nd - 1], Dt[:, nd - 1]
    X = torch.randn(nprop, nd, dtype=torch.float64, device=dev) * 0.05
    chunk = max(1, int(2e8 // D.shape[0]))        # keep the [rows, ndata] intermediate near 1.6 GB

    def ll():
        out = []
        for i in range(0, nprop, chunk):
            Xi = X[i:i + chunk]
            r = y[None, :] - (Xi[:, 0:1] + Xi[:, 1:] @ Z.T)
            out.append((-0.5 * r * r).sum(dim=1))
        return torch.cat(out)

    ll()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ll()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(kmc, name):
    nw, nd, ndata = SHAPES[name]
    D, beta = make_data(ndata, nd)
    th = beta + 0.05 * np.random.default_rng(1).standard_normal((nw, nd))
    dd = kmc.DataDensity(REG_TERM, D, params=[4.0])
    G = GENS[name]
    wall, dev_ms, desc = time_route(kmc, dd, nw, nd, th, G)
    ws = nw * G / wall
    rec = dict(shape=dict(nwalkers=nw, ndim=nd, ndata=ndata, ncols=nd), describe=desc,
               data_route=dict(generations=G, wall_s=wall, device_ms=dev_ms, walker_steps_per_s=ws, terms_per_s=ws * ndata,
                               fp64_flops_per_s=ws * ndata * flops_per_term(nd),
                               fraction_of_fp64_vector_peak_spec=ws * ndata * flops_per_term(nd) / PEAK_FP64_VECTOR_SPEC),
               flops_per_term_hand_count=flops_per_term(nd))
    Gh = HOST_GENS[name]
    hwall, _, _ = time_route(kmc, kmc.HostLogPdf(host_fn(D, 4.0), vectorized=True), nw, nd, th, Gh, warm=1)
    hws = nw * Gh / hwall
    rec["host_route"] = dict(generations=Gh, wall_s=hwall, walker_steps_per_s=hws, terms_per_s=hws * ndata)
    rec["data_over_host"] = ws / hws
    try:
        tms = torch_batch(D, nd, nw // 2)
        rec["torch_gpu_batch"] = dict(rows=nw // 2, ms_per_batch=tms, terms_per_s=(nw // 2) * ndata / (tms / 1e3),
                                      note="log-likelihood of one half-step's proposals, eager torch ops (matmul + elementwise + sum); no sampler")
        rec["data_terms_over_torch"] = rec["data_route"]["terms_per_s"] / rec["torch_gpu_batch"]["terms_per_s"]
    except Exception as e:                          # (torch without a device: recorded, not fatal)
        rec["torch_gpu_batch"] = dict(error=repr(e))
    print(name, json.dumps({k: v for k, v in rec.items() if k != "describe"}), flush=True)
    return rec


def merge_stats(path, out):
    rec = json.load(open(out)) if os.path.exists(out) else {}
    rows = []
    for f in glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True):
        import csv
        for r in csv.DictReader(open(f)):
            if "kmc_data" in r.get("Name", "") or "half_step" in r.get("Name", ""):
                rows.append({k: r[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage") if k in r})
    rec["rocprofv3_kernel_stats_S2"] = rows
    json.dump(rec, open(out, "w"), indent=1)
    print(json.dumps(rows, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="S1,S2,S3")
    ap.add_argument("--profile", default=None, help="run one shape's data route only (under rocprofv3)")
    ap.add_argument("--merge-stats", default=None)
    a = ap.parse_args()
    if a.merge_stats:
        merge_stats(a.merge_stats, a.out)
        return
    import kissmcmc_jl_amd as kmc
    if a.profile:
        nw, nd, ndata = SHAPES[a.profile]
        D, beta = make_data(ndata, nd)
        th = beta + 0.05 * np.random.default_rng(1).standard_normal((nw, nd))
        print(time_route(kmc, kmc.DataDensity(REG_TERM, D, params=[4.0]), nw, nd, th, GENS[a.profile]))
        return
    rec = dict(peak_fp64_vector_spec_flops=PEAK_FP64_VECTOR_SPEC,
               peak_note="AMD's published MI355X FP64 vector figure (FMA counted as 2 FLOPs); a spec number, not measured here",
               shapes={n: measure(kmc, n) for n in a.shapes.split(",")})
    if a.out:
        old = json.load(open(a.out)) if os.path.exists(a.out) else {}
        old.update(rec)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(old, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
