"""The snooker move (KMC_MOVE_SNOOKER, kmc.DESnookerMove) and the DE / snooker mixtures (KMC_MOVE_MIX) without a device: the Python
objects and the config they write, the new constants and fields across the C header and the ctypes mirror, kmc_validate's answers,
and the numpy yardstick's own checks -- its partners, its member choice, its summation order and, as the check of the Hastings
factor, the stationary distribution it samples.  The kernels against the yardstick: tests/test_gpu_snooker_move.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import de_yardstick as yd
import snooker_yardstick as ys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the Python objects -------------------------------------------------------------------------------------------------
def test_snooker_python_object(kmc):
    from kissmcmc_jl_amd import _lib
    m = kmc.DESnookerMove()
    assert m.gamma == 1.7 and "DESnookerMove" in kmc.__all__ and "DESnookerMove" in repr(m)
    c = _lib.Config()
    m.apply(c)
    assert c.move == _lib.MOVE_SNOOKER and c.snooker_gamma == 1.7 and c.mix_count == 0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            kmc.DESnookerMove(gamma=bad)


def test_mixture_writes_the_config(kmc):
    from kissmcmc_jl_amd import _lib
    from kissmcmc_jl_amd.moves import apply_move, mixture_weights
    c = _lib.Config()
    apply_move([(kmc.DEMove(), 0.8), (kmc.DESnookerMove(), 0.2)], c)
    assert c.move == _lib.MOVE_MIX and c.mix_count == 2
    assert (c.mix_move0, c.mix_move1) == (_lib.MOVE_DE, _lib.MOVE_SNOOKER)
    assert (c.mix_weight0, c.mix_weight1) == (0.8, 0.2)                   # raw: the library normalises
    assert (c.mix_gamma0, c.mix_sigma0, c.mix_gamma1, c.mix_sigma1) == (0.0, 1e-5, 1.7, 0.0)
    c = _lib.Config()
    apply_move([(kmc.DEMove(gamma0=0.5, sigma=0.0), 1), (kmc.DEMove(gamma0=1.0), 2), (kmc.DESnookerMove(2.0), 3), (kmc.DESnookerMove(), 4)], c)
    assert c.mix_count == 4 and (c.mix_gamma0, c.mix_gamma1, c.mix_gamma2, c.mix_gamma3) == (0.5, 1.0, 2.0, 1.7)
    assert (c.mix_weight0, c.mix_weight3) == (1.0, 4.0)
    assert mixture_weights([0.8, 0.2]) == ys.mix_weights([0.8, 0.2])[0]
    c = _lib.Config()
    apply_move(None, c)
    assert c.move == _lib.MOVE_STRETCH and c.mix_count == 0


def test_bad_mixtures_are_refused_in_python(kmc):
    from kissmcmc_jl_amd import _lib
    from kissmcmc_jl_amd.moves import apply_move
    de, sn = kmc.DEMove(), kmc.DESnookerMove()
    for bad in ([(de, 1.0)], [(de, 1.0)] * 5, [(de, 0.0), (sn, 1.0)], [(de, -1.0), (sn, 1.0)], [(de, float("nan")), (sn, 1.0)],
                [(de, float("inf")), (sn, 1.0)], [(de, 1e308), (sn, 1e308)]):
        with pytest.raises(ValueError):
            apply_move(bad, _lib.Config())
    with pytest.raises(ValueError, match="stretch"):
        apply_move([(None, 0.5), (sn, 0.5)], _lib.Config())
    for bad in ("snooker", 3, [(de, 1.0), sn], [("de", 1.0), (sn, 1.0)]):
        with pytest.raises(TypeError):
            apply_move(bad, _lib.Config())


# ---- header, ctypes, kmc_validate ---------------------------------------------------------------------------------------
def test_new_constants_and_fields_agree_with_the_header(tmp_path):
    from kissmcmc_jl_amd import _lib
    fields = ["snooker_gamma", "mix_count", "mix_move", "mix_weight", "mix_gamma", "mix_sigma", "move", "de_sigma"]
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kissmcmc_hip.h"\nint main(void){printf("%zu %d %d %d %d %d", sizeof(kmc_config), '
                   '(int)KMC_MOVE_STRETCH, (int)KMC_MOVE_DE, (int)KMC_MOVE_SNOOKER, (int)KMC_MOVE_MIX, (int)KMC_MIX_MAX);'
                   + "".join(f'printf(" %zu", offsetof(kmc_config, {f}));' for f in fields)
                   + 'printf(" %zu %zu\\n", sizeof(((kmc_config*)0)->mix_move), sizeof(((kmc_config*)0)->mix_sigma));return 0;}\n')
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    K = _lib.Config
    want = [C.sizeof(K), _lib.MOVE_STRETCH, _lib.MOVE_DE, _lib.MOVE_SNOOKER, _lib.MOVE_MIX, _lib.MIX_MAX,
            K.snooker_gamma.offset, K.mix_count.offset, K.mix_move0.offset, K.mix_weight0.offset, K.mix_gamma0.offset, K.mix_sigma0.offset,
            K.move.offset, K.de_sigma.offset, 16, 32]
    assert got == want
    assert K.mix_move3.offset == K.mix_move0.offset + 12 and K.mix_sigma3.offset == K.mix_sigma0.offset + 24
    assert _lib.MOVE_STRETCH == 0 and len({_lib.MOVE_STRETCH, _lib.MOVE_DE, _lib.MOVE_SNOOKER, _lib.MOVE_MIX}) == 4


def _cfg(lib, **kw):
    c = lib.Config()
    c.dtype = lib.F64
    c.density = lib.GAUSSIAN_ISO
    c.params[0], c.params[1] = 0.0, 1.0
    c.nwalkers, c.ndim, c.ngenerations, c.nburnin, c.nthin = 64, 4, 10, 0, 1
    c.a_scale = 2.0
    c.shard_count = 1
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _validate(move, **kw):
    from kissmcmc_jl_amd import _lib
    from kissmcmc_jl_amd.moves import apply_move
    L = _lib.lib()
    c = _cfg(_lib)
    if move is not None:
        apply_move(move, c)
    for k, v in kw.items():
        setattr(c, k, v)
    st = L.kmc_validate(C.byref(c))
    return st, L.kmc_last_error().decode() if st else ""


def _mix(kmc):
    return [(kmc.DEMove(), 0.8), (kmc.DESnookerMove(), 0.2)]


def test_snooker_and_mixture_configs_validate(kmc):
    assert _validate(kmc.DESnookerMove()) == (0, "")
    assert _validate(kmc.DESnookerMove(), snooker_gamma=0.0) == (0, "")           # 0: the default, 1.7
    assert _validate(_mix(kmc)) == (0, "")
    assert _validate([(kmc.DEMove(), 1.0), (kmc.DEMove(gamma0=1.0, sigma=0.0), 1.0)]) == (0, "")   # one class, two parameter sets
    assert _validate(None, snooker_gamma=-3.0, mix_count=9)[0] == 0               # a stretch config ignores the new fields


@pytest.mark.parametrize("kw", [dict(snooker_gamma=-0.1), dict(snooker_gamma=float("nan")), dict(snooker_gamma=float("inf")), dict(ndim=1),
                                dict(nwalkers=4, ndim=2)])
def test_bad_snooker_arguments_are_bad_arg(kmc, kw):
    from kissmcmc_jl_amd import _lib
    assert _validate(kmc.DESnookerMove(), **kw)[0] == _lib.ERR_BAD_ARG


@pytest.mark.parametrize("kw", [dict(mix_count=1), dict(mix_count=5), dict(mix_weight0=0.0), dict(mix_weight1=-1.0), dict(mix_weight0=float("nan")),
                                dict(mix_weight1=float("inf")), dict(mix_move1=2), dict(mix_move0=4), dict(mix_sigma0=1.0), dict(mix_gamma1=-1.0),
                                dict(ndim=1)])
def test_bad_mixture_arguments_are_bad_arg(kmc, kw):
    from kissmcmc_jl_amd import _lib
    assert _validate(_mix(kmc), **kw)[0] == _lib.ERR_BAD_ARG


def test_a_stretch_member_is_unsupported_and_says_so(kmc):
    from kissmcmc_jl_amd import _lib
    st, msg = _validate(_mix(kmc), mix_move0=_lib.MOVE_STRETCH)
    assert st == _lib.ERR_UNSUPPORTED and "stretch member" in msg


@pytest.mark.parametrize("move,name", [("snooker", "KMC_MOVE_SNOOKER"), ("mix", "KMC_MOVE_MIX")])
@pytest.mark.parametrize("what", ["islands", "p2p", "shards", "dealt", "f32", "blobs"])
def test_refusals_are_unsupported_and_name_the_move(kmc, move, name, what):
    from kissmcmc_jl_amd import _lib
    kw = dict(islands=dict(flags=_lib.ISLANDS, nwalkers=256, island_size=64), p2p=dict(flags=_lib.P2P, shard_count=2),
              shards=dict(shard_count=2), dealt=dict(deal_count=2), f32=dict(dtype=_lib.F32), blobs=dict(flags=_lib.STORE_BLOBS))[what]
    st, msg = _validate(kmc.DESnookerMove() if move == "snooker" else _mix(kmc), **kw)
    assert st == _lib.ERR_UNSUPPORTED, (st, msg)
    assert name in msg


# ---- the yardstick's own checks -----------------------------------------------------------------------------------------
def test_snooker_draws_follow_the_documented_stream(oracle):
    seed, step, h = (9 << 32) | 0x0BADCAFE, 2 * 17 + 1, 57
    walkers = np.arange(h, 2 * h)
    z, z1, z2, u = ys.draws_snooker(seed, step, walkers, h)
    key = [(seed & 0xFFFFFFFF) ^ 0x44454D56, seed >> 32]
    for i, w in enumerate(walkers[:16]):
        w0, w1, w2, _ = oracle.philox4x32_10([step & 0xFFFFFFFF, step >> 32, int(w), 2], key)
        _, _, v2, v3 = oracle.philox4x32_10([step & 0xFFFFFFFF, step >> 32, int(w), 3], key)
        a = (w0 * h) >> 32
        others = [v for v in range(h) if v != a]
        b = others[(w1 * (h - 1)) >> 32]
        others = [v for v in others if v != b]
        c = others[(w2 * (h - 2)) >> 32]
        assert (z[i], z1[i], z2[i]) == (a, b, c)
        assert u[i] == ((((v2 << 20) | (v3 >> 12)) + 0.5) * 2.0 ** -52)


@pytest.mark.parametrize("h", [3, 4, 5, 7, 50, 1000])
def test_partners_are_distinct_and_in_range(h):
    z, z1, z2, u = ys.draws_snooker(3, 23, np.arange(20000), h)
    assert np.all(z != z1) and np.all(z != z2) and np.all(z1 != z2)
    for v in (z, z1, z2):
        assert v.min() >= 0 and v.max() < h
    assert np.all((u > 0) & (u < 1))
    if h <= 7:                                   # every ordered triple occurs
        assert len({(a, b, c) for a, b, c in zip(z, z1, z2)}) == h * (h - 1) * (h - 2)


def test_mix_choice_frequencies_follow_the_weights():
    """100 000 half-steps: the member counts are binomial, so each frequency lies within 5 sigma = 5 sqrt(p (1 - p) / n) of its weight."""
    n = 100000
    for weights in ([0.8, 0.2], [1.0, 2.0, 3.0, 4.0], [5.0, 1.0, 1e-300]):
        p, cum = ys.mix_weights(weights)
        got = ys.mix_choices(1234567, np.arange(n), cum)
        for i, pi in enumerate(p):
            assert abs(np.mean(got == i) - pi) <= 5.0 * math.sqrt(pi * (1.0 - pi) / n) + 1e-12, (weights, i)
        assert [ys.mix_choice(1234567, s, cum) for s in range(50)] == list(got[:50])
    assert np.all(ys.mix_choices(5, np.arange(n), ys.mix_weights([1.0, 1e-300])[1]) == 0)       # weight on the first member only
    assert len(set(ys.mix_choices(s, np.arange(64), ys.mix_weights([0.5, 0.5])[1]).tobytes() for s in range(4))) == 4   # keyed by the seed


def test_tree_T_is_a_sum_to_a_few_ulp():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 4, 5, 7, 8, 32, 33, 100, 1024, 1100, 4097):
        v = rng.standard_normal((6, n)) ** 2                      # positive terms, like d . d
        for row, t in zip(v, ys.T(v)):
            exact = math.fsum(row)
            assert abs(t - exact) <= (2 + math.ceil(math.log2(max(n, 2)))) * np.spacing(exact), n   # a tree of depth log2 n
    # padding further changes no bit, whatever the sign of a zero sum
    for row in ([-0.0], [-0.0, -0.0, -0.0], [1.5, -1.5, -0.0], [3.0, 1e-17, -3.0, 2.0, 7.0]):
        a = ys.T(np.array([row]))
        b = ys.T(np.array([row + [0.0] * (64 - len(row))]))
        assert a.tobytes() == b.tobytes()
    # the order is the pairwise one: ((a + b) + (c + 0))
    a, b, c = 1.0, 2.0 ** -53, 2.0 ** -53
    assert ys.T(np.array([[a, b, c]]))[0] == (a + b) + (c + 0.0) and ys.T(np.array([[b, c, a]]))[0] == (b + c) + (a + 0.0)


def test_mixture_with_all_weight_on_de_is_the_de_sampler():
    th = np.random.default_rng(2).standard_normal((48, 5))
    f = lambda X: -0.5 * np.sum(X * X, axis=1)
    want = yd.emcee_de(f, th, 25, 5, 2, seed=77)
    got = ys.emcee_moves(f, th, 25, 5, 2, seed=77, move=[(ys.DE(), 1.0), (ys.Snooker(), 1e-300)])
    for k in ("pos", "logp", "nacc", "chain", "chain_logp"):
        np.testing.assert_array_equal(got[k], want[k])
    assert np.all(got["members"] == 0)
    alone = ys.emcee_moves(f, th, 25, 5, 2, seed=77, move=ys.DE())
    np.testing.assert_array_equal(alone["pos"], want["pos"])


def _stationary(move, seed, hastings=None):
    """64 walkers on the 3-D unit Gaussian, 1 500 generations, 300 burned: pooled mean and variance per dimension."""
    nw, nd, G, nb = 64, 3, 1500, 300
    th = np.random.default_rng(seed).standard_normal((nw, nd))
    f = lambda X: -0.5 * np.sum(X * X, axis=1)
    old = ys.HASTINGS_DIMS
    if hastings is not None:
        ys.HASTINGS_DIMS = hastings
    try:
        r = ys.emcee_moves(f, th, G, nb, 1, seed=seed, move=move)
    finally:
        ys.HASTINGS_DIMS = old
    mean = r["sum"] / r["n"]
    return mean, r["sumsq"] / r["n"] - mean ** 2, r


MIX = [(ys.DE(), 0.8), (ys.Snooker(), 0.2)]


@pytest.mark.parametrize("move", [ys.Snooker(), MIX], ids=["snooker", "mixture"])
def test_stationary_mean_and_variance_of_the_unit_gaussian(move):
    """The check that the Hastings factor (ndim - 1) log|1 + s| is right.  76 800 pooled samples with tau_int of 10 to 30
    generations are some 2 500 to 7 500 independent ones: the standard error of a variance is sqrt(2 / 2 500) = 0.028 at worst, of a
    mean 0.02; the bounds are 0.1 and 0.08, four sigma of the worst case.  Without the factor (test below) the variance of the
    snooker chain is off by several times the bound."""
    mean, var, r = _stationary(move, 101)
    assert np.all(np.abs(mean) < 0.08) and np.all(np.abs(var - 1.0) < 0.1), (mean, var)
    acc = r["nacc"].sum() / (64 * 1200)
    assert 0.1 < acc < 0.9
    if isinstance(move, list):
        assert 0.1 < np.mean(r["members"] == 1) < 0.3


def test_the_stationary_check_sees_a_wrong_hastings_factor():
    """Dropping (ndim - 1) from the accept test must fail the same check: it then samples another distribution."""
    mean, var, _ = _stationary(ys.Snooker(), 101, hastings=lambda nd: 0)
    assert not np.all(np.abs(var - 1.0) < 0.1), var
