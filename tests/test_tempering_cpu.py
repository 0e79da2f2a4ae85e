"""CPU: parallel tempering without a GPU -- the numpy yardstick (tests/tempering_yardstick.py) checked on its own (rung 0 of a ladder
that never swaps is the oracle's stretch run and de_yardstick's DE run, bit for bit; the swap schedule; what a sweep conserves), the
ladder helper, the Python-side argument errors, the new config fields in the header, the ctypes mirror and kmc_validate.  The
sampling itself is tests/test_gpu_tempering.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import de_yardstick as yd
import snooker_yardstick as sy
import tempering_yardstick as ty
import validate_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAUSS, ROSEN = 0, 2


def test_fma_is_the_c_fma():
    r = np.random.default_rng(0)
    a, b, c = r.standard_normal(20000), r.standard_normal(20000) * 3.0, r.standard_normal(20000) * 1e-3
    c[::7] = -(a * b)[::7]                                     # cancellation: what a fused multiply-add is for
    libm = C.CDLL("libm.so.6")
    libm.fma.restype = C.c_double
    libm.fma.argtypes = [C.c_double] * 3
    want = np.array([libm.fma(x, y, z) for x, y, z in zip(a, b, c)])
    np.testing.assert_array_equal(ty.fma(a, b, c), want)


@pytest.mark.parametrize("dens,params,nw,nd", [(GAUSS, [0.0, 1.0], 64, 4), (ROSEN, [1.0, 100.0, 20.0], 48, 7)])
def test_rung0_without_swaps_is_the_oracles_stretch_run(oracle, dens, params, nw, nd):
    G, nburn, nthin, seed = 25, 6, 2, 5
    th = np.random.default_rng(nd).standard_normal((nw, nd)) * 0.5 + (1.0 if dens == ROSEN else 0.0)
    ref = oracle.emcee(oracle.make_config(dens, params, nw, nd, G, nburn, nthin, 2.0, seed), th)
    assert ref["status"] == 0
    f = lambda X: oracle.logpdf_batch(dens, params, X)
    got = ty.emcee_tempered(f, th, [1.0, 0.5, 0.2], G, nburn, nthin, seed=seed, swap_every=0)
    np.testing.assert_array_equal(got["pos"][0], ref["final_pos"])
    np.testing.assert_array_equal(got["nacc"][0], ref["naccept"])
    np.testing.assert_array_equal(got["chain"], ref["chain"])
    np.testing.assert_allclose(got["logp"][0], ref["final_logp"], rtol=1e-12, atol=1e-12)
    assert not np.array_equal(got["pos"][1], got["pos"][0]) and got["nswap"].sum() == 0


def test_rung0_without_swaps_is_the_de_yardstick(oracle):
    nw, nd, G = 64, 5, 20
    th = np.random.default_rng(1).standard_normal((nw, nd))
    f = lambda X: oracle.logpdf_batch(GAUSS, [0.0, 1.0], X)
    want = yd.emcee_de(f, th, G, 4, 1, seed=9)
    got = ty.emcee_tempered(f, th, [1.0, 0.3], G, 4, 1, seed=9, move=sy.DE(), swap_every=0)
    for k in ("pos", "logp", "nacc"):
        np.testing.assert_array_equal(got[k][0], want[k])
    np.testing.assert_array_equal(got["chain"], want["chain"])
    np.testing.assert_array_equal(got["chain_logp"], want["chain_logp"])
    want = sy.emcee_moves(f, th, G, 4, 1, seed=9, move=[(sy.DE(), 0.5), (sy.Snooker(), 0.5)])
    got = ty.emcee_tempered(f, th, [1.0, 0.3], G, 4, 1, seed=9, move=[(sy.DE(), 0.5), (sy.Snooker(), 0.5)], swap_every=0)
    np.testing.assert_array_equal(got["pos"][0], want["pos"])
    np.testing.assert_array_equal(got["nacc"][0], want["nacc"])


def test_the_schedule_never_puts_a_rung_into_two_pairs():
    for T in range(2, 12):
        seen = set()
        for n in range(6):
            lower = ty.swap_pairs(n, T)
            rungs = [t for t in lower] + [t + 1 for t in lower]
            assert len(set(rungs)) == len(rungs) and all(0 <= t < T for t in rungs)
            assert all(t % 2 == n % 2 for t in lower)
            seen.update(lower)
        assert seen == set(range(T - 1))                       # two consecutive sweeps attempt every neighbouring pair


def test_a_sweep_conserves_the_ladders_rows():
    r = np.random.default_rng(3)
    T, nw, nd = 5, 32, 3
    betas = np.array([1.0, 0.6, 0.3, 0.1, 0.02])
    pos = r.standard_normal((T, nw, nd))
    logp = -0.5 * (pos ** 2).sum(axis=2)
    before = sorted((tuple(p), l) for p, l in zip(pos.reshape(-1, nd), logp.reshape(-1)))
    cols = [sorted((tuple(pos[t, w]), logp[t, w]) for t in range(T)) for w in range(nw)]
    total = np.zeros(T - 1, dtype=np.int64)
    for n in range(4):
        total += ty.sweep(pos, logp, betas, 7, n)
    assert sorted((tuple(p), l) for p, l in zip(pos.reshape(-1, nd), logp.reshape(-1))) == before
    assert [sorted((tuple(pos[t, w]), logp[t, w]) for t in range(T)) for w in range(nw)] == cols      # same-index exchange: a walker keeps its half
    np.testing.assert_array_equal(logp, -0.5 * (pos ** 2).sum(axis=2))                                # the log-density travels with its row
    assert np.all(total > 0) and np.all(total <= 2 * nw)              # (every pair was attempted in two of the four sweeps)


def test_a_checkpoint_resumes_the_yardstick(oracle):
    f = lambda X: oracle.logpdf_batch(GAUSS, [0.0, 1.0], X)
    th = np.random.default_rng(5).standard_normal((32, 3))
    kw = dict(nburnin=3, nthin=1, seed=2, swap_every=3)
    whole = ty.emcee_tempered(f, th, [1.0, 0.4, 0.1], 20, **kw)
    part = ty.emcee_tempered(f, th, [1.0, 0.4, 0.1], 7, **kw)
    rest = ty.emcee_tempered(f, None, [1.0, 0.4, 0.1], 20, start=part, **kw)
    for k in ("pos", "logp", "nacc", "nswap"):
        np.testing.assert_array_equal(rest[k], whole[k])
    np.testing.assert_allclose(rest["logp_sum"], whole["logp_sum"], rtol=1e-13)


def test_geometric_betas_and_argument_errors():
    import kissmcmc_jl_amd as kmc
    from kissmcmc_jl_amd import _lib
    from kissmcmc_jl_amd.tempering import apply_tempering, check_betas
    b = kmc.geometric_betas(5, 0.01)
    assert b[0] == 1.0 and b[-1] == 0.01 and np.all(np.diff(b) < 0)
    np.testing.assert_allclose(b[1:] / b[:-1], 0.01 ** 0.25, rtol=1e-14)
    assert "geometric_betas" in kmc.__all__
    for bad in (dict(ntemps=1, beta_min=0.1), dict(ntemps=65, beta_min=0.1), dict(ntemps=4, beta_min=0.0), dict(ntemps=4, beta_min=1.0)):
        with pytest.raises(ValueError):
            kmc.geometric_betas(**bad)
    for bad in ([1.0], [0.9, 0.5], [1.0, 1.0], [1.0, 0.5, 0.6], [1.0, 0.0], [1.0, -0.1], [1.0, float("nan")], [[1.0, 0.5]], [1.0] + [0.5] * 64):
        with pytest.raises(ValueError):
            check_betas(bad)
    c = _lib.Config()
    assert apply_tempering(c) is None and (c.ntemps, c.swap_every) == (0, 0) and not c.betas
    keep = apply_tempering(c, betas=[1.0, 0.5, 0.25], swap_every=3)
    assert (c.ntemps, c.swap_every) == (3, 3) and c.betas == keep.ctypes.data
    keep = apply_tempering(c, ntemps=4, beta_min=0.1)
    assert c.ntemps == 4 and c.swap_every == 1 and keep[-1] == 0.1
    for bad in (dict(ntemps=4), dict(beta_min=0.1), dict(betas=[1.0, 0.5], ntemps=3), dict(betas=[1.0, 0.5], swap_every=-1),
                dict(betas=[1.0, 0.5], swap_every=1.5)):
        with pytest.raises(ValueError):
            apply_tempering(_lib.Config(), **bad)


def test_new_fields_agree_with_the_header(tmp_path):
    from kissmcmc_jl_amd import _lib
    fields = ["mix_sigma", "betas", "ntemps", "swap_every", "move"]
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kissmcmc_hip.h"\nint main(void){printf("%zu %d", sizeof(kmc_config), (int)KMC_TEMPS_MAX);'
                   + "".join(f'printf(" %zu", offsetof(kmc_config, {f}));' for f in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    K = _lib.Config
    assert got == [C.sizeof(K), _lib.TEMPS_MAX, K.mix_sigma0.offset, K.betas.offset, K.ntemps.offset, K.swap_every.offset, K.move.offset]
    assert K.betas.offset == K.mix_sigma3.offset + 8 and K.move.offset == K.swap_every.offset + 4
    assert {"kmc_sampler_get_rung_state", "kmc_sampler_set_rung_state", "kmc_sampler_get_swaps"} <= set(_lib.SYMBOLS)


def _validate(**kw):
    return validate_cases.validate(**dict(dict(nwalkers=64, ndim=4), **kw))


def test_kmc_validate_on_ladders_and_refusals():
    from kissmcmc_jl_amd import _lib
    assert _validate()[0] == _lib.OK and _validate(ntemps=0)[0] == _lib.OK and _validate(ntemps=1, swap_every=5)[0] == _lib.OK
    assert _validate(betas=[1.0, 0.5, 0.1], swap_every=2)[0] == _lib.OK
    for bad, word in ((dict(betas=[0.9, 0.5]), "betas[0]"), (dict(betas=[1.0, 0.5, 0.5]), "decreasing"), (dict(betas=[1.0, 0.0]), "betas"),
                      (dict(betas=[1.0, -1.0]), "betas"), (dict(betas=[1.0, float("inf")]), "betas"), (dict(betas=[1.0] + [0.9 ** (i + 1) for i in range(64)]), "ntemps"),
                      (dict(ntemps=3), "betas"), (dict(ntemps=-1), "ntemps"), (dict(betas=[1.0, 0.5], swap_every=-1), "swap_every"),
                      (dict(betas=[1.0, 0.5], nwalkers=1 << 30), "ntemps * nwalkers")):
        st, msg = _validate(**bad)
        assert st == _lib.ERR_BAD_ARG and word in msg, (bad, st, msg)
    for kw in (dict(dtype=_lib.F32), dict(flags=_lib.ISLANDS, island_size=64), dict(flags=_lib.P2P), dict(shard_count=2), dict(deal_count=2),
               dict(density=_lib.HOST_DENSITY, host_logpdf=1)):
        st, msg = _validate(betas=[1.0, 0.5], **kw)
        assert st == _lib.ERR_UNSUPPORTED and "tempering" in msg, (kw, st, msg)
