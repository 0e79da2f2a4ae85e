"""The differential-evolution move (KMC_MOVE_DE, kmc.DEMove) without a device: the numpy yardstick's stream against the
oracle's Philox, the partner map, kmc_validate's refusals, and the new kmc_config fields across the C header, the ctypes
mirror and the Julia shim.  The sampling itself is tests/test_gpu_de_move.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import de_yardstick as yd
import validate_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_vectorised_philox_matches_the_oracle(oracle):
    rng = np.random.default_rng(1)
    for _ in range(64):
        ctr = [int(v) for v in rng.integers(0, 2 ** 32, 4, dtype=np.uint64)]
        key = [int(v) for v in rng.integers(0, 2 ** 32, 2, dtype=np.uint64)]
        got = yd.philox4x32_10(*[np.array([c], dtype=np.uint64) for c in ctr], *key)
        assert tuple(int(g[0]) for g in got) == oracle.philox4x32_10(ctr, key)


def test_draws_follow_the_documented_stream(oracle):
    seed, step, h = (7 << 32) | 0x1234ABCD, 2 * 41 + 1, 96
    walkers = np.arange(h, 2 * h)
    j, k, u, g = yd.draws(seed, step, walkers, h, 0.5, 1e-5)
    for i, w in enumerate(walkers[:16]):
        key = [(seed & 0xFFFFFFFF) ^ 0x44454D56, seed >> 32]
        w0, w1, w2, w3 = oracle.philox4x32_10([step & 0xFFFFFFFF, step >> 32, int(w), 0], key)
        v0 = oracle.philox4x32_10([step & 0xFFFFFFFF, step >> 32, int(w), 1], key)[0]
        jj = (w0 * h) >> 32
        kp = (w1 * (h - 1)) >> 32
        assert j[i] == jj and k[i] == kp + (kp >= jj)
        assert u[i] == ((((w2 << 20) | (w3 >> 12)) + 0.5) * 2.0 ** -52)
        assert g[i] == 0.5 * (1.0 + 1e-5 * (2.0 * ((v0 + 0.5) * 2.0 ** -32) - 1.0))
    assert np.all((u > 0) & (u < 1)) and np.all(np.abs(g / 0.5 - 1.0) <= 1e-5)


@pytest.mark.parametrize("h", [2, 3, 5, 50, 1000])
def test_partners_are_distinct_and_in_range(h):
    j, k, _, _ = yd.draws(3, 17, np.arange(20000), h, 1.0, 0.0)
    assert np.all(j != k)
    assert j.min() >= 0 and k.min() >= 0 and j.max() < h and k.max() < h


@pytest.mark.parametrize("h", [2, 4, 8, 1024])
def test_partner_map_is_exactly_uniform_for_power_of_two_halves(h):
    """Over the whole range of a 32-bit word, umulhi(w, h) hits every partner j exactly 2^32 / h times when h is a power of two;
    k' = umulhi(w1, h - 1) hits each of its h - 1 values floor or ceil(2^32 / (h - 1)) times, and k = k' + (k' >= j) never equals j.
    (Bucket sizes in closed form: the smallest w with umulhi(w, m) >= b is ceil(b 2^32 / m).)"""
    def sizes(m):
        edges = [-(-(b << 32) // m) for b in range(m + 1)]
        return [edges[i + 1] - edges[i] for i in range(m)]
    assert sizes(h) == [(1 << 32) // h] * h
    sk = sizes(h - 1)
    assert max(sk) - min(sk) <= 1 and sum(sk) == 1 << 32
    for jj in range(min(h, 16)):
        assert all(kp + (kp >= jj) != jj for kp in range(h - 1))


def _validate(kmc, **kw):
    from kissmcmc_jl_amd import _lib
    return validate_cases.validate(**dict(dict(nwalkers=64, ndim=4, move=_lib.MOVE_DE), **kw))


def test_de_config_validates(kmc):
    assert _validate(kmc) == (0, "")
    assert _validate(kmc, de_gamma0=0.7, de_sigma=0.0) == (0, "")
    assert _validate(kmc, move=0)[0] == 0


@pytest.mark.parametrize("kw", [dict(move=2), dict(move=-1), dict(de_gamma0=-0.1), dict(de_gamma0=float("inf")), dict(de_gamma0=float("nan")),
                                dict(de_sigma=-1e-6), dict(de_sigma=1.0), dict(de_sigma=float("nan")), dict(de_sigma=float("inf"))])
def test_bad_de_arguments_are_bad_arg(kmc, kw):
    from kissmcmc_jl_amd import _lib
    assert _validate(kmc, **kw)[0] == _lib.ERR_BAD_ARG


def test_stretch_config_ignores_de_fields(kmc):
    assert _validate(kmc, move=0, de_gamma0=-5.0, de_sigma=3.0)[0] == 0


@pytest.mark.parametrize("what", ["islands", "p2p", "shards", "dealt", "f32", "blobs"])
def test_de_refusals_are_unsupported_and_name_the_move(kmc, what):
    from kissmcmc_jl_amd import _lib
    kw = dict(islands=dict(flags=_lib.ISLANDS, nwalkers=256, island_size=64), p2p=dict(flags=_lib.P2P, shard_count=2),
              shards=dict(shard_count=2), dealt=dict(deal_count=2), f32=dict(dtype=_lib.F32), blobs=dict(flags=_lib.STORE_BLOBS))[what]
    st, msg = _validate(kmc, **kw)
    assert st == _lib.ERR_UNSUPPORTED, (st, msg)
    assert "KMC_MOVE_DE" in msg


def test_a_scale_is_still_validated_with_de(kmc):
    from kissmcmc_jl_amd import _lib
    assert _validate(kmc, a_scale=1.0)[0] == _lib.ERR_A_SCALE


def test_demove_python_object(kmc):
    m = kmc.DEMove()
    assert m.gamma0 is None and m.sigma == 1e-5 and m.gamma0_for(32) == 2.38 / 8.0
    from kissmcmc_jl_amd import _lib
    c = _lib.Config()
    m.apply(c)
    assert c.move == _lib.MOVE_DE and c.de_gamma0 == 0.0 and c.de_sigma == 1e-5
    for bad in (dict(gamma0=0.0), dict(gamma0=-1.0), dict(sigma=1.0), dict(sigma=-0.5)):
        with pytest.raises(ValueError):
            kmc.DEMove(**bad)
    assert "DEMove" in kmc.__all__


def test_new_fields_agree_across_header_ctypes_and_julia(tmp_path):
    from kissmcmc_jl_amd import _lib
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kissmcmc_hip.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(kmc_config), offsetof(kmc_config, move), offsetof(kmc_config, move_pad_),'
                   ' offsetof(kmc_config, de_gamma0), offsetof(kmc_config, de_sigma), (int)KMC_MOVE_STRETCH, (int)KMC_MOVE_DE);return 0;}\n')
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(_lib.Config), _lib.Config.move.offset, _lib.Config.move_pad_.offset, _lib.Config.de_gamma0.offset,
            _lib.Config.de_sigma.offset, _lib.MOVE_STRETCH, _lib.MOVE_DE]
    assert got == want
    jl = open(os.path.join(ROOT, "kissmcmc.jl_amd", "julia", "src", "KissMCMCHIP.jl")).read()
    m = re.search(r"Base\.@kwdef struct KmcConfig\n(.*?)\nend\n", jl, re.S)
    assert re.findall(r"^\s+(\w+)::", m.group(1), re.M)[-4:] == ["move", "move_pad_", "de_gamma0", "de_sigma"]
    consts = dict((n, int(v)) for n, v in re.findall(r"^const (KMC_MOVE_\w+) = Int32\((\d+)\)", jl, re.M))
    assert consts == {"KMC_MOVE_STRETCH": 0, "KMC_MOVE_DE": 1}
