import sys, os, time
sys.path.insert(0, '.')
import numpy as np
import kissmcmc_jl_amd as kmc
import torch
def rss():
    for l in open('/proc/self/status'):
        if l.startswith('VmRSS'): return int(l.split()[1]) / 1024
def create_destroy(n=300):
    """`leak_check.py create`: samplers created and destroyed in a loop, device memory free before and after (the allocation cache is
    warm by then) -- a menu sampler with moments, a tempered one and one that streams its chain."""
    kinds = (("menu", lambda: kmc.Sampler(kmc.GaussianIso(), 16384, 16, 16, moments=True)),
             ("tempered", lambda: kmc.Sampler(kmc.GaussianIso(), 256, 4, 16, betas=[1.0, 0.5, 0.25])),
             ("stream-chain", lambda: kmc.Sampler(kmc.GaussianIso(), 256, 4, 16, store_chain=True, store_logp=True, stream_chain=True)))
    for name, make in kinds:
        for _ in range(10):
            make().close()
        r0, f0 = rss(), torch.cuda.mem_get_info(0)[0]
        t0 = time.time()
        for _ in range(n):
            make().close()
        print(f"{name}: {n} samplers created and destroyed in {time.time() - t0:.1f} s; host RSS {r0:.0f} -> {rss():.0f} MiB; device free changed by {(f0 - torch.cuda.mem_get_info(0)[0]) / 2**20:.1f} MiB", flush=True)
if sys.argv[1:] == ["create"]:
    create_destroy()
    sys.exit(0)
pdf = kmc.Exponential(1.0)
th0 = kmc.make_theta0s(0.5, 0.1, pdf, 100, rng=3)
cd = kmc.CDensity("return x[0] >= 0 ? -x[0] : -INFINITY;")
for name, p in (("menu", pdf), ("cdensity", cd)):
    kmc.emcee(p, th0, niter=10 ** 5, seed=1, use_progress_meter=False)
    r0, f0 = rss(), torch.cuda.mem_get_info(0)[0]
    t0 = time.time()
    N = 3000
    for i in range(N):
        kmc.emcee(p, th0, niter=10 ** 5, seed=i, use_progress_meter=False)
    print(f"{name}: {N} README calls in {time.time() - t0:.1f} s; host RSS {r0:.0f} -> {rss():.0f} MiB; device free changed by {(f0 - torch.cuda.mem_get_info(0)[0]) / 2**20:.1f} MiB", flush=True)
from kissmcmc_jl_amd.metropolis import GaussianStep
r0 = rss(); t0 = time.time()
for i in range(500):
    kmc.metropolis(kmc.GaussianIso(-5.0, 3.0), GaussianStep(5.0), 0.0, niter=10 ** 4, seed=i, use_progress_meter=False)
print(f"metropolis: 500 calls in {time.time() - t0:.1f} s; host RSS {r0:.0f} -> {rss():.0f} MiB")
