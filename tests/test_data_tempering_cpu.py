"""Likelihood tempering (kmc.Sampler(DataDensity, betas=..., temper="likelihood") / kmc_config.temper_mode) without a device: the
numpy yardstick against tempering_yardstick, thermodynamic integration on an analytic curve, the Python layer's and kmc_validate's
argument checks, the header / ctypes / Julia mirrors, and the condition on the evidence test's ladder.  The sampling itself is
tests/test_gpu_data_tempering.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import data_tempering_yardstick as dy
import snooker_yardstick as sy
import tempering_yardstick as ty
from test_data_density_cpu import REG_TERM
from test_gpu_data_density import reg_data, reg_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MOVES = {"stretch": None, "de": sy.DE(), "snooker": sy.Snooker(), "mix": [(sy.DE(), 0.8), (sy.Snooker(), 0.2)]}


def gauss_prior(X):
    return -0.5 * (X * X).sum(axis=1)


@pytest.mark.parametrize("mv", ["stretch", "de", "snooker", "mix"])
def test_rung0_without_swaps_is_the_whole_mode_yardstick_on_the_posterior(mv):
    """beta = 1.0: q = pri + 1.0 * S has the bits of pri + S, so rung 0 of a ladder that never swaps equals
    tempering_yardstick.emcee_tempered given pri + S as its log-density, bit for bit."""
    nw, nd, G = 32, 3, 12
    D, beta = reg_data(37, nd, 2)
    f2 = dy.data_logpdf(lambda X: reg_terms(X, D, 2.0), gauss_prior)
    f1 = lambda X: dy.posterior(*f2(X))
    th = beta + 0.05 * np.random.default_rng(1).standard_normal((nw, nd))
    betas = [1.0, 0.4, 0.0]
    got = dy.emcee_data_tempered(f2, th, betas, G, 3, 2, seed=5, move=MOVES[mv], swap_every=0)
    want = ty.emcee_tempered(f1, th, [1.0, 0.4], G, 3, 2, seed=5, move=MOVES[mv], swap_every=0)
    for k in ("pos", "logp", "nacc"):
        np.testing.assert_array_equal(got[k][0], want[k][0], err_msg=k)
    np.testing.assert_array_equal(got["chain"], want["chain"])
    np.testing.assert_array_equal(got["chain_logp"], want["chain_logp"])
    np.testing.assert_array_equal(got["logp"], got["logprior"] + got["loglike"])
    assert got["nacc"][0].sum() > 0 and not np.array_equal(got["pos"][1], got["pos"][0])
    # the prior rung moves by the prior alone: its accept decisions do not depend on the data
    f2b = dy.data_logpdf(lambda X: 7.0 * reg_terms(X, D, 2.0), gauss_prior)
    other = dy.emcee_data_tempered(f2b, th, betas, G, 3, 2, seed=5, move=MOVES[mv], swap_every=0)
    np.testing.assert_array_equal(other["pos"][2], got["pos"][2])


def test_yardstick_checkpoint_resumes_bit_for_bit_and_sweeps_exchange_all_four_arrays():
    nw, nd, G = 32, 3, 14
    D, beta = reg_data(20, nd, 3)
    f2 = dy.data_logpdf(lambda X: reg_terms(X, D, 2.0), gauss_prior)
    th = beta + 0.3 * np.random.default_rng(2).standard_normal((nw, nd))
    betas = [1.0, 0.5, 0.1, 0.0]
    whole = dy.emcee_data_tempered(f2, th, betas, G, 2, 1, seed=9, swap_every=3)
    part = dy.emcee_data_tempered(f2, th, betas, 7, 2, 1, seed=9, swap_every=3)
    rest = dy.emcee_data_tempered(f2, None, betas, G, 2, 1, seed=9, swap_every=3, start=part)
    for k in ("pos", "logp", "loglike", "logprior", "nacc", "nswap", "loglike_sum"):
        np.testing.assert_array_equal(rest[k], whole[k], err_msg=k)
    assert whole["nswap"].sum() > 0
    for t in range(4):                                     # S and the prior travelled with their rows
        pri, S = f2(whole["pos"][t])
        np.testing.assert_array_equal(whole["loglike"][t], S)
        np.testing.assert_array_equal(whole["logprior"][t], pri)
    v = np.random.default_rng(0).standard_normal(100)
    assert abs(dy.block_sum256(v) - v.sum()) < 1e-12


def test_thermodynamic_integration_on_an_analytic_curve(kmc):
    """<S>_beta = 3 beta^2 - 2: the integral over [0, 1] is -1; the trapezoid over beta_k = k / 8 overshoots by sum h^3 / 12 f'' =
    8 * (1/8)^3 / 12 * 6 = 1/128, over every second rung by 4 * (1/4)^3 / 12 * 6 = 1/32: err = 1/32 - 1/128."""
    b = np.arange(8, -1, -1) / 8.0
    logz, err = kmc.thermodynamic_integration(b, 3.0 * b * b - 2.0)
    assert abs(logz - (-1.0 + 1.0 / 128)) < 1e-14 and abs(err - (1.0 / 32 - 1.0 / 128)) < 1e-14
    up = kmc.thermodynamic_integration(b[::-1], (3.0 * b * b - 2.0)[::-1])       # the order the ladder is given in does not matter
    assert up == (logz, err)
    # an even number of rungs: every second rung from beta = 1 down, and the lowest one
    b4 = np.array([1.0, 0.5, 0.25, 0.0])
    m4 = np.array([4.0, 2.0, 1.0, 0.0])                                            # linear: both trapezoids are exact
    assert kmc.thermodynamic_integration(b4, m4) == (2.0, 0.0)
    m4 = np.array([4.0, 0.0, 1.0, 0.0])
    full = 0.5 * (4.0 + 0.0) * 0.5 + 0.5 * (0.0 + 1.0) * 0.25 + 0.5 * 1.0 * 0.25
    coarse = 0.5 * (4.0 + 1.0) * 0.75 + 0.5 * 1.0 * 0.25
    assert kmc.thermodynamic_integration(b4, m4) == (full, abs(full - coarse))
    # a ladder that stops above 0 integrates from there
    assert kmc.thermodynamic_integration([1.0, 0.5], [2.0, 2.0]) == (1.0, 0.0)
    for bad in (([1.0], [0.0]), ([1.0, 0.5], [0.0]), ([1.0, 1.0], [0.0, 0.0])):
        with pytest.raises(ValueError):
            kmc.thermodynamic_integration(*bad)
    assert "thermodynamic_integration" in kmc.__all__


def test_python_layer_argument_checks():
    from kissmcmc_jl_amd import _lib
    from kissmcmc_jl_amd.tempering import apply_tempering
    c = _lib.Config()
    keep = apply_tempering(c, betas=[1.0, 0.5, 0.0], temper="likelihood")
    assert c.temper_mode == _lib.TEMPER_LIKELIHOOD == 1 and c.ntemps == 3 and keep[-1] == 0.0
    apply_tempering(c, betas=[1.0, 0.5])
    assert c.temper_mode == _lib.TEMPER_WHOLE == 0
    apply_tempering(c, betas=[1.0, 0.5], temper="whole")
    assert c.temper_mode == _lib.TEMPER_WHOLE
    apply_tempering(c, ntemps=4, beta_min=0.1, temper="likelihood")
    assert c.temper_mode == _lib.TEMPER_LIKELIHOOD and c.ntemps == 4
    for bad in (dict(betas=[1.0, 0.5], temper="prior"),                 # an unknown temper value
                dict(temper="likelihood"),                              # temper="likelihood" without a ladder
                dict(betas=[1.0, 0.0, 0.0], temper="likelihood"),       # beta = 0 anywhere but last
                dict(betas=[1.0, 0.0, -0.5], temper="likelihood"),
                dict(betas=[1.0, 0.5, 0.0]),                            # beta = 0 in whole mode
                dict(betas=[1.0, 0.5, 0.0], temper="whole")):
        with pytest.raises(ValueError):
            apply_tempering(_lib.Config(), **bad)


def _validate(kmc, density="data", **kw):
    from kissmcmc_jl_amd import _lib
    L = _lib.lib()
    c = _lib.Config()
    c.dtype = _lib.F64
    keep_d = kmc.DataDensity(REG_TERM, np.zeros((8, 3)), params=[1.0])
    if density == "data":
        c.density, c.user_density = _lib.DATA_DENSITY, keep_d.user_handle
    else:
        c.density = _lib.GAUSSIAN_ISO
        c.params[0], c.params[1] = 0.0, 1.0
    c.nwalkers, c.ndim, c.ngenerations, c.nburnin, c.nthin, c.a_scale, c.shard_count = 16, 3, 10, 0, 1, 2.0, 1
    betas = kw.pop("betas", None)
    keep = None
    if betas is not None:
        keep = (C.c_double * len(betas))(*betas)
        c.betas, c.ntemps = C.cast(keep, C.c_void_p), len(betas)
    for k, v in kw.items():
        setattr(c, k, v)
    st = L.kmc_validate(C.byref(c))
    return st, L.kmc_last_error().decode()


def test_kmc_validate_on_the_tempering_mode(kmc):
    from kissmcmc_jl_amd import _lib
    LIKE = _lib.TEMPER_LIKELIHOOD
    assert _validate(kmc, betas=[1.0, 0.5, 0.1], temper_mode=LIKE)[0] == _lib.OK
    assert _validate(kmc, betas=[1.0, 0.5, 0.0], temper_mode=LIKE, swap_every=2)[0] == _lib.OK
    for mv in (_lib.MOVE_DE, _lib.MOVE_SNOOKER):
        assert _validate(kmc, betas=[1.0, 0.0], temper_mode=LIKE, move=mv)[0] == _lib.OK
    for bad, word in ((dict(betas=[1.0, 0.0, 0.0], temper_mode=LIKE), "betas"), (dict(betas=[1.0, 0.5, -0.1], temper_mode=LIKE), "betas"),
                      (dict(temper_mode=LIKE), "ladder"), (dict(betas=[1.0, 0.5], temper_mode=2), "temper_mode")):
        st, msg = _validate(kmc, **bad)
        assert st == _lib.ERR_BAD_ARG and word in msg, (bad, st, msg)
    st, msg = _validate(kmc, density="gauss", betas=[1.0, 0.0])                  # beta = 0 in whole mode: a bad argument, as before
    assert st == _lib.ERR_BAD_ARG and "> 0" in msg
    # refusals name tempering: another density in likelihood mode; a data density in the default mode (pointing to the new one)
    st, msg = _validate(kmc, density="gauss", betas=[1.0, 0.5], temper_mode=LIKE)
    assert st == _lib.ERR_UNSUPPORTED and "tempering" in msg and "KMC_DATA_DENSITY" in msg
    st, msg = _validate(kmc, betas=[1.0, 0.5])
    assert st == _lib.ERR_UNSUPPORTED and "tempering" in msg and 'temper="likelihood"' in msg
    for kw, what in ((dict(dtype=_lib.F32), "KMC_F32"), (dict(flags=_lib.ISLANDS, island_size=64), "island"), (dict(flags=_lib.P2P, shard_count=2), "P2P"),
                     (dict(shard_count=2), "shard"), (dict(deal_count=2), "dealt"), (dict(flags=_lib.STORE_BLOBS), "blobs")):
        st, msg = _validate(kmc, betas=[1.0, 0.5], temper_mode=LIKE, **kw)
        assert st == _lib.ERR_UNSUPPORTED and what.lower() in msg.lower(), (kw, st, msg)


def test_new_field_constants_and_calls_agree_across_header_ctypes_and_julia(tmp_path):
    from kissmcmc_jl_amd import _lib
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kissmcmc_hip.h"\nint main(void){printf("%zu %zu %zu %zu %d %d\\n", sizeof(kmc_config), '
                   'offsetof(kmc_config, temper_mode), offsetof(kmc_config, deal_count), offsetof(kmc_config, snooker_gamma), '
                   '(int)KMC_TEMPER_WHOLE, (int)KMC_TEMPER_LIKELIHOOD);return 0;}\n')
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    K = _lib.Config
    assert got == [C.sizeof(K), K.temper_mode.offset, K.deal_count.offset, K.snooker_gamma.offset, _lib.TEMPER_WHOLE, _lib.TEMPER_LIKELIHOOD]
    assert K.temper_mode.offset == K.deal_count.offset + 4 and _lib.TEMPER_WHOLE == 0
    assert {"kmc_sampler_get_rung_loglike", "kmc_sampler_set_rung_loglike_sum"} <= set(_lib.SYMBOLS)
    jl = open(os.path.join(ROOT, "kissmcmc.jl_amd", "julia", "src", "KissMCMCHIP.jl")).read()
    assert "const KMC_TEMPER_WHOLE, KMC_TEMPER_LIKELIHOOD = Int32(0), Int32(1)" in jl
    sig = re.search(r"function emcee\(pdf::DeviceLogPdf, theta0s;(.*?)\)\s*\n\s+ladder", jl, re.S).group(1)
    assert "temper=:whole" in sig and "temper_mode=(temper == :likelihood ? KMC_TEMPER_LIKELIHOOD : KMC_TEMPER_WHOLE)" in jl


def test_the_evidence_ladder_has_an_analytic_trapezoid_error_under_0_05_nat(kmc):
    """A condition on the INPUTS of test_gpu_data_tempering.py's evidence test, from the closed forms alone."""
    m = dy.EvidenceModel()
    assert m.betas[0] == 1.0 and m.betas[-1] == 0.0 and np.all(np.diff(m.betas) < 0) and m.betas.size == 24
    ana = np.array([m.mean_loglike(b) for b in m.betas])
    trap, err = kmc.thermodynamic_integration(m.betas, ana)
    print("analytic trapezoid", trap, "exact log Z", m.log_z(), "every-second-rung estimate", err)
    assert abs(trap - m.log_z()) < 0.05
    # the closed form of <S>_beta against a direct Gaussian quadrature of the posterior at one beta (10^5 draws: 3 sigma of the mean)
    beta = float(m.betas[5])
    cov = np.linalg.inv(np.eye(2) / m.s ** 2 + beta * m.p * m.A.T @ m.A)
    th = np.random.default_rng(0).multivariate_normal(cov @ (beta * m.p * m.A.T @ m.y), cov, size=100000)
    S = m.term_fn(th).sum(axis=1)
    assert abs(S.mean() - m.mean_loglike(beta)) < 4.0 * S.std() / np.sqrt(len(S))
