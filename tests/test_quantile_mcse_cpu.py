"""No GPU: the host stages of the quantile MCSE -- kmc_beta_quantile against scipy.special.betaincinv, kmc_quantile_mcse_ranks and
kmc_indicator_moments against tests/quantile_mcse_yardstick.py bit for bit, kmc_indicator_plan, the refusals of the two host-chain calls
that follow from the arguments alone, and the host header in a stand-alone program under the host sanitizers.

The Beta quantile.  Over ess in {1.5, 10, 1e3, 1e6, 2e9} x p in {0.001, 0.05, 0.5, 0.95, 0.999} x both tail probabilities the largest
relative disagreement with scipy 1.15 was measured as 1.43e-12 (at ess = 2e9, p = 0.05; below 4e-14 up to ess = 1e6); the test prints
it again.  The cap 1e-9 is a condition, not a measurement: at the S <= 1e5 of the GPU tests it bounds the error of a S by 1e-4."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.special import betaincinv

import quantile_mcse_yardstick as qy

ESS = (1.5, 10.0, 1e3, 1e6, 2e9)
PROBS = (0.001, 0.05, 0.5, 0.95, 0.999)


def bits(v):
    return np.float64(v).view(np.uint64)


def test_names_are_public(kmc):
    for name in ("quantile_mcse", "indicator_lags", "beta_quantile", "quantile_mcse_ranks", "indicator_moments", "indicator_plan"):
        assert name in kmc.__all__ and callable(getattr(kmc, name))
    assert callable(kmc.Sampler.quantile_mcse) and callable(kmc.Sampler.indicator_lags)
    import inspect
    assert inspect.signature(kmc.summarize_run).parameters["quantile_mcse"].default is False
    assert inspect.signature(kmc.Sampler.summary).parameters["quantile_mcse"].default is False
    from kissmcmc_jl_amd import _lib
    for sym in ("kmc_beta_quantile", "kmc_quantile_mcse_ranks", "kmc_indicator_moments", "kmc_indicator_plan", "kmc_sampler_indicator_lags",
                "kmc_chain_indicator_lags", "kmc_sampler_quantile_mcse", "kmc_chain_quantile_mcse"):
        assert sym in _lib.SYMBOLS and hasattr(_lib.lib(), sym)


def test_beta_quantile_against_scipy(kmc):
    worst = 0.0
    for ess in ESS:
        for p in PROBS:
            A, B = ess * p + 1.0, ess * (1.0 - p) + 1.0
            for tail in (qy.PHI_MINUS_1, qy.PHI_PLUS_1):
                got, want = kmc.beta_quantile(tail, A, B), float(betaincinv(A, B, tail))
                assert bits(got) == bits(kmc.beta_quantile(tail, A, B))                # equal inputs, equal bits
                rel = abs(got - want) / want
                print(f"ess {ess:g} p {p:g} tail {tail:.3f}: {got!r} scipy {want!r} rel {rel:.3e}")
                worst = max(worst, rel)
    print(f"largest relative disagreement with scipy: {worst:.3e}")
    assert worst <= 1e-9


def test_beta_quantile_at_the_ends_of_its_range(kmc):
    from kissmcmc_jl_amd import _lib
    top = 2.0 ** 31 + 1.0
    assert abs(kmc.beta_quantile(0.25, 1.0, 1.0) - 0.25) <= 1e-15                     # uniform
    for prob in (qy.PHI_MINUS_1, qy.PHI_PLUS_1):                                      # Beta(A, 1): x = prob^(1 / A); Beta(1, B): 1 - (1 - prob)^(1 / B)
        assert abs(kmc.beta_quantile(prob, top, 1.0) / np.exp(np.log(prob) / top) - 1.0) <= 1e-12
        assert abs(kmc.beta_quantile(prob, 1.0, top) / -np.expm1(np.log1p(-prob) / top) - 1.0) <= 1e-9
        x = kmc.beta_quantile(prob, top, top)
        assert abs(x / float(betaincinv(top, top, prob)) - 1.0) <= 1e-9 and abs(x - 0.5) < 1e-4
    for args in ((0.0, 2.0, 2.0), (1.0, 2.0, 2.0), (float("nan"), 2.0, 2.0), (0.5, 0.5, 2.0), (0.5, 2.0, float("inf")), (0.5, float("nan"), 2.0)):
        with pytest.raises(kmc.KmcError) as err:
            kmc.beta_quantile(*args)
        assert err.value.status == _lib.ERR_BAD_ARG


def test_ranks_and_moments_match_the_yardstick_bit_for_bit(kmc):
    """The index rule on the library's own a and b (scipy's differ in the last digits), A and B as the yardstick forms them; the moments
    at word edges, the ends of the count and the largest chain."""
    for S in (8, 1000, 99991, 2 ** 31 - 1):
        for ess in ESS:
            for p in PROBS:
                a, b, i1, i2 = kmc.quantile_mcse_ranks(S, p, ess)
                A, B, sa, sb = qy.beta_ab(p, ess)
                assert bits(a) == bits(kmc.beta_quantile(qy.PHI_MINUS_1, A, B)) and bits(b) == bits(kmc.beta_quantile(qy.PHI_PLUS_1, A, B))
                assert (i1, i2) == qy.ranks(S, a, b) and 0 <= i1 <= i2 <= S - 1
                if qy.margin(S, sa, sb) > 1e-4 * max(1.0, S / 1e5):                       # where scipy's a S, b S are clear of an integer: its ranks too
                    assert (i1, i2) == qy.ranks(S, sa, sb)
    for ess in (float("nan"), 0.0, -3.0):
        a, b, i1, i2 = kmc.quantile_mcse_ranks(100, 0.5, ess)
        assert np.isnan(a) and np.isnan(b) and (i1, i2) == (-1, -1)
    for h in (4, 5, 63, 64, 65, 1000, 2 ** 31 - 1):
        for k in sorted({0, 1, h // 3, h // 2, h - 1, h}):
            mu, s2 = kmc.indicator_moments(h, k)
            wmu, ws2 = qy.moments(h, k)
            assert bits(mu) == bits(wmu) and bits(s2) == bits(ws2), (h, k)
    for args in ((1, 0), (4, -1), (4, 5)):
        with pytest.raises(kmc.KmcError):
            kmc.indicator_moments(*args)
    for args in ((0, 0.5, 10.0), (100, 0.0, 10.0), (100, 1.0, 10.0), (100, float("nan"), 10.0)):
        with pytest.raises(kmc.KmcError):
            kmc.quantile_mcse_ranks(*args)


def test_indicator_plan(kmc):
    p = kmc.indicator_plan()
    assert list(p) == ["word_bits", "threads", "chunk_words", "lds_bytes"]
    assert p["word_bits"] == 64 and p["threads"] == 256 and p["chunk_words"] == 2048
    assert p["lds_bytes"] == 8 * p["chunk_words"] + 4 * p["threads"] <= 64 * 1024


def test_argument_checks_need_no_device(kmc):
    """Every refusal of the two host-chain calls that follows from the arguments alone comes before the device is touched (this test
    runs without one), and names the index and the value."""
    from kissmcmc_jl_amd import _lib
    L = _lib.lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    pd = lambda a: a.ctypes.data_as(dp)
    chain = np.zeros((10, 3, 2))
    out = [np.full((2, 2), -7.0) for _ in range(5)]
    T, flags = np.full((2, 2), -7, dtype=np.int64), np.full((2, 2), -7, dtype=np.int32)
    m, h = C.c_int64(-1), C.c_int64(-1)

    def whole(probs=(0.5, 0.9), ns=10, nw=3, first=0, mask=None, split=1, max_lag=0, nprobs=None, ch=chain, res=out):
        pr = np.asarray(probs, dtype=np.float64)
        mk = None if mask is None else np.asarray(mask, dtype=np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
        return L.kmc_chain_quantile_mcse(None if ch is None else pd(ch), None, ns, nw, 2, first, mk, split, max_lag, len(pr) if nprobs is None else nprobs,
                                         pd(pr) if pr.size else None, 0, *[None if res is None else pd(a) for a in out], T.ctypes.data_as(ip),
                                         flags.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(m), C.byref(h), None)

    err = lambda: L.kmc_last_error()
    bad = _lib.ERR_BAD_ARG
    assert whole(probs=(0.5, 1.0)) == bad and b"probs[1] = 1" in err()
    assert whole(probs=(0.0,)) == bad and b"probs[0] = 0" in err()
    assert whole(probs=(0.5, 0.5, float("nan"))) == bad and b"probs[2] = nan" in err()
    assert whole(probs=(0.5, float("inf"))) == bad and b"probs[1] = inf" in err()
    assert whole(probs=(-0.25,)) == bad and b"probs[0] = -0.25" in err()
    assert whole(probs=()) == bad and b"nprobs = 0" in err()
    assert whole(probs=(0.5,) * 17) == bad and b"nprobs = 17" in err()
    assert whole(nprobs=-1) == bad
    assert whole(ch=None) == bad
    assert whole(res=None) == bad
    assert whole(first=10) == bad and b"empty" in err()
    assert whole(mask=(0, 0, 0)) == bad and b"empty" in err()
    assert whole(first=4) == bad and b"h = 3" in err()                                 # 6 samples, split: 3 a chain
    assert whole(nw=1, ch=np.zeros((10, 1, 2)), split=0) == bad and b"m = 1" in err()
    assert whole(max_lag=5) == bad and b"max_lag" in err()                             # h = 5: max_lag <= 4
    assert whole(max_lag=2) == bad and b"max_lag" in err()
    assert m.value == -1 and h.value == -1 and all((a == -7.0).all() for a in out) and (T == -7).all() and (flags == -7).all()

    ones, counts = np.full((2, 2, 6), -7, dtype=np.int64), np.full((2, 2, 4), 7, dtype=np.uint64)
    thr = np.zeros((2, 2))

    def stage(nprobs=2, lag0=1, nlags=4, first=0, t=thr, o=ones, cnt=counts, ch=chain):
        return L.kmc_chain_indicator_lags(None if ch is None else pd(ch), None, 10, 3, 2, first, None, 1, nprobs, None if t is None else pd(t), lag0, nlags, 0,
                                          None if o is None else o.ctypes.data_as(ip), None if cnt is None else cnt.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          C.byref(m), C.byref(h))

    assert stage(nprobs=0) == bad and b"nprobs = 0" in err()
    assert stage(nprobs=17) == bad and b"nprobs = 17" in err()
    assert stage(t=None) == bad and stage(o=None) == bad and stage(cnt=None) == bad and stage(ch=None) == bad
    assert stage(lag0=0) == bad and b"[1, h - 1]" in err()
    assert stage(lag0=2, nlags=4) == bad and b"h = 5" in err()
    assert stage(nlags=-1) == bad
    assert stage(first=10) == bad and b"empty" in err()
    assert m.value == -1 and (ones == -7).all() and (counts == 7).all()
    th = np.zeros((3, 10, 2))
    with pytest.raises(kmc.KmcError, match=r"probs\[1\] = 1.5"):
        kmc.quantile_mcse(th, [0.5, 1.5])
    with pytest.raises(ValueError, match="thresholds"):
        kmc.indicator_lags(th, np.zeros((2, 3)))


def test_host_header_under_host_sanitizers(tmp_path):
    """The host header of the Beta quantile, the index rule and the indicator moments (csrc/kmc_quantile_host.hpp) in a stand-alone
    program of its own (tests/sanitize/beta_quantile_main.cpp), built with the host's address and undefined-behaviour sanitizers and run
    over the grid above.  Nothing of it is loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "beta_quantile_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(root, "kissmcmc.jl_amd", "csrc"), os.path.join(root, "tests", "sanitize", "beta_quantile_main.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 33 and lines[-1] == "bad 0" and lines[0].startswith("ess 1.5 p 0.001") and lines[24].startswith("ess 2000000000 p 0.999")
    for line in lines[:25]:                                                            # the program's values against scipy, like the library's
        t = line.split()
        ess, p_, a, b = float(t[1]), float(t[3]), float(t[5]), float(t[7])
        _, _, sa, sb = qy.beta_ab(p_, ess)
        assert abs(a / sa - 1.0) <= 1e-9 and abs(b / sb - 1.0) <= 1e-9
        assert (int(t[9]), int(t[11])) == qy.ranks(100000, a, b)
