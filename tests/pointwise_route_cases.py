"""The calls of tests/test_gpu_pointwise_routes.py: the seven pointwise / PSIS-LOO entry pairs (kmc_sampler_* on the chain a sampler
holds, kmc_chain_* on a chain in host memory) with one fixed set of arguments per pair, run through ctypes so that nothing but the
library lies between the arguments and the outputs.  tests/golden/make_pointwise_routes.py records the kmc_chain_* outputs of these
calls as tests/golden/pointwise/routes.npz.

The shape: a linear regression in 2 dimensions (d = (y, a, b), term -0.5 p0 (y - x0 a - x1 b)^2), 32 walkers, 24 stored samples;
first_sample = 4, thin = 3 and a mask that drops 5 walkers, so n = 7 * 27 = 189 rows and every element of the selection is non-default.
Case J70: 70 observations, the range [3, 68) (unpacked kernels; the range starts unaligned and crosses a group of 64).  Case J10: 10
observations, the range [1, 9) (packed kernels).  The calls that take held-out data also run with the other case's observations held
out.  workspace = 1 gives blocks and batches of one group of 64 observations, so J70 runs two of each."""
import ctypes as C
import hashlib

import numpy as np

REG_TERM = "double r = d[0] - x[0] * d[1] - x[1] * d[2]; return -0.5 * p[0] * r * r;"
NW, ND, NS, NBURN, SEED = 32, 2, 24, 4, 17
FIRST, THIN = 4, 3
MASK = np.array([w not in (0, 7, 13, 14, 31) for w in range(NW)], dtype=np.uint8)
N = 7 * 27
TAIL_COLS = 40                                   # >= ceil(0.2 n) = 38, the longest tail any r_eff gives
CASES = {"J70": (70, (3, 65)), "J10": (10, (1, 8))}
FAMILIES = ("pointwise_stats", "pointwise_loglike", "pointwise_weights", "relative_eff", "psis_loo", "psis_tail", "psis_loo_reff", "psis_tail_reff")
# info slots that are not times
INFO_KEPT = dict(pointwise_stats=[0, 1, 2, 3], relative_eff=[0, 1, 5], psis_loo=[0, 1, 2, 3, 8, 9, 11], psis_loo_reff=[0, 1, 2, 3, 8, 9, 11, 14, 15])
dp, ip, i32p, bp = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


def data(J):
    rng = np.random.default_rng(1000 + J)
    a, b = rng.standard_normal(J), rng.standard_normal(J)
    return np.ascontiguousarray(np.stack([1.0 * a + 0.5 * b + 0.7 * rng.standard_normal(J), a, b], axis=1))


def theta0():
    return np.array([1.0, 0.5]) + 0.1 * np.random.default_rng(SEED).standard_normal((NW, ND))


def supplied_r_eff(count):
    """Between 0.9 and 4.4: tail lengths from 20 to 38 (3 sqrt(n / r) against 0.2 n = 37.8)."""
    return np.ascontiguousarray(0.9 + 3.5 * np.random.default_rng(count).random(count))


def density(kmc, case):
    return kmc.DataDensity(REG_TERM, data(CASES[case][0]), params=[2.0])


def sample_chain(kmc, pdf):
    """A sampler of `pdf` with its 24 stored samples; the caller closes it."""
    s = kmc.Sampler(pdf, NW, ND, NBURN + NS, NBURN, 1, 2.0, SEED, store_chain=True)
    s.set_positions(theta0())
    s.run(NBURN + NS)
    s.sync()
    return s


class SamplerRoute:
    def __init__(self, s):
        self.s = s

    def __call__(self, name, mid, outs):
        return getattr(self.s._L, "kmc_sampler_" + name)(self.s._h, FIRST, MASK.ctypes.data_as(bp), THIN, *mid, *outs)


class ChainRoute:
    """chain: [sample][walker][dim] in host memory"""

    def __init__(self, kmc, pdf, chain):
        from kissmcmc_jl_amd import _lib
        self.L, self.pdf, self.chain = _lib.lib(), pdf, np.ascontiguousarray(chain, dtype=np.float64)
        assert self.chain.shape == (NS, NW, ND)
        self.params = np.zeros(6)
        self.params[:len(pdf.params())] = pdf.params()

    def __call__(self, name, mid, outs):
        return getattr(self.L, "kmc_chain_" + name)(self.pdf.user_handle, self.params.ctypes.data_as(dp), self.chain.ctypes.data_as(dp), NS, NW, ND, FIRST,
                                                    MASK.ctypes.data_as(bp), THIN, *mid, 0, *outs)


def run_family(route, case, family):
    """{call label: {output name: array}} of one entry pair's calls by `route`.  Every call must be accepted."""
    J, (of, oc) = CASES[case]
    other = [c for c in CASES if c != case][0]
    held, (hof, hoc) = data(CASES[other][0]), CASES[other][1]
    results = {}

    def call(label, name, mid, arrays, kept=None):
        ptr = {np.dtype(np.float64): dp, np.dtype(np.int64): ip, np.dtype(np.int32): i32p}
        st = route(name, mid, [a.ctypes.data_as(ptr[a.dtype]) for a in arrays.values()])
        assert st == 0, (label, st)
        if "info" in arrays:
            arrays["info"] = arrays["info"][kept]
        results[label] = arrays

    d = lambda *shape: np.full(shape, np.nan)
    i = lambda n=1, v=0: np.full(n, v, dtype=np.int64)
    own, out = [None, 0, 0], [held.ctypes.data_as(dp), held.shape[0], 3]
    if family == "pointwise_stats":
        call("own", family, own, dict(stats=d(4, J), n=i(), info=i(6)), INFO_KEPT[family])
        call("held", family, out, dict(stats=d(4, held.shape[0]), n=i(), info=i(6)), INFO_KEPT[family])
    elif family == "pointwise_loglike":
        call("own", family, own + [of, oc], dict(out=d(N, oc), n=i()))
        call("held", family, out + [hof, hoc], dict(out=d(N, hoc), n=i()))
    elif family == "pointwise_weights":
        call("own", family, own + [of, oc], dict(v=d(N, oc), M_j=d(oc), n=i()))
        call("held", family, out + [hof, hoc], dict(v=d(N, hoc), M_j=d(hoc), n=i()))
    elif family == "relative_eff":
        for label, max_lag, work in (("default", 0, 0), ("max_lag=5/workspace=1", 5, 1)):
            call(label, family, [of, oc, 0, max_lag, work],
                 dict(r_eff_j=d(oc), ess_j=d(oc), T_j=i(oc), flags_j=np.zeros(oc, dtype=np.int32), m=i(), h=i(), n=i(), info=i(6)), INFO_KEPT[family])
    else:
        r_j = supplied_r_eff(oc)
        if family in ("psis_loo", "psis_tail"):
            sels = [("r_eff=0.7", [0.7, of, oc, 0]), ("r_eff=0.7/workspace=1", [0.7, of, oc, 1])]
        else:
            sels = [("supplied", [r_j.ctypes.data_as(dp), 1, 0, of, oc, 0]), ("supplied/workspace=1", [r_j.ctypes.data_as(dp), 1, 0, of, oc, 1]),
                    ("computed/split=0", [None, 0, 0, of, oc, 0]), ("computed/split=0/max_lag=5/workspace=1", [None, 0, 5, of, oc, 1])]
        for label, sel in sels:
            used = dict(r_eff_used=d(oc), tail_len_j=i(oc), n_reff_nan=i(1, -1)) if family.endswith("_reff") else {}
            if family.startswith("psis_loo"):
                call(label, family, sel, dict(stats=d(4, oc), lppd_j=d(oc), **used, n=i(), info=i(16)), INFO_KEPT[family])
            else:
                call(label, family, sel, dict(tail=d(oc, TAIL_COLS), m_j=d(oc), xc_j=d(oc), n_tail_j=np.zeros(oc, dtype=np.int32), tail_len=i(1, TAIL_COLS), **used,
                                              n=i()))
    return results


def flatten(results, prefix):
    """{"prefix/label/name": array}"""
    return {f"{prefix}/{label}/{name}": a for label, arrays in results.items() for name, a in arrays.items()}


def digest(a):
    """What the fixture keeps of one output: the array itself up to 2 KiB, else the SHA-256 of its bytes (bit-for-bit all the same)."""
    a = np.ascontiguousarray(a)
    if a.nbytes <= 2048:
        return a
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
