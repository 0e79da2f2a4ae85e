"""Data densities (KMC_DATA_DENSITY, kmc.DataDensity) without a device: the value contract's pairwise tree, creation-time
validation and compile errors, the C constant.  The sampling itself is tests/test_gpu_data_density.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REG_TERM = "double mu = x[0]; for (int k = 1; k < n; ++k) mu += x[k] * d[k - 1]; double r = d[n - 1] - mu; return -0.5 * p[0] * r * r;"


def pairwise(T):
    """The contract's tree (include/kissmcmc_hip.h, kmc_data_density_create) over the columns of T [nrows, ndata]."""
    while T.shape[1] > 1:
        n = T.shape[1]
        S = T[:, 0:n - 1:2] + T[:, 1:n:2]
        T = np.concatenate([S, T[:, -1:]], axis=1) if n % 2 else S
    return T[:, 0]


def recursive(t):
    """The same tree by its recursive definition: the first 2^k elements (largest power of two below n) + the rest."""
    n = len(t)
    if n == 1:
        return t[0]
    k = 1
    while 2 * k < n:
        k *= 2
    return recursive(t[:k]) + recursive(t[k:])


def test_pairwise_restatement_equals_recursive_definition():
    rng = np.random.default_rng(5)
    sizes = sorted(set([1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]) | set(rng.integers(1, 1026, 40).tolist()))
    for n in sizes:
        T = rng.standard_normal((3, n)) * 10.0 ** rng.integers(-8, 9, (3, n))
        got = pairwise(T)
        for r in range(3):
            assert got[r] == recursive(list(T[r])), n


def test_header_constant_matches_binding(kmc):
    from kissmcmc_jl_amd import _lib
    txt = open(os.path.join(ROOT, "include", "kissmcmc_hip.h")).read()
    assert int(re.search(r"KMC_DATA_DENSITY\s*=\s*(\d+)", txt).group(1)) == _lib.DATA_DENSITY == 102
    assert "kmc_data_density_create" in _lib.SYMBOLS and hasattr(_lib.lib(), "kmc_data_density_create")


def _create(_lib, term, prior, data, ndata, ncols):
    h = C.c_void_p()
    dp = None if data is None else np.ascontiguousarray(data, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    st = _lib.lib().kmc_data_density_create(term.encode(), prior.encode() if prior else None, dp, ndata, ncols, C.byref(h))
    if st == _lib.OK:
        _lib.lib().kmc_user_density_destroy(h)
    return st, _lib.lib().kmc_last_error().decode()


def test_creation_validates_its_arguments(kmc):
    from kissmcmc_jl_amd import _lib
    D = np.zeros((10, 3))
    assert _create(_lib, REG_TERM, None, D, 10, 3)[0] == _lib.OK
    assert _create(_lib, REG_TERM, "return x[0] > 0 ? 0.0 : -INFINITY;", D, 10, 3)[0] == _lib.OK
    st, msg = _create(_lib, REG_TERM, None, None, 10, 3)
    assert st == _lib.ERR_BAD_ARG and "NULL" in msg
    st, msg = _create(_lib, REG_TERM, None, D, 0, 3)
    assert st == _lib.ERR_BAD_ARG and "ndata" in msg
    st, msg = _create(_lib, REG_TERM, None, D, 10, 0)
    assert st == _lib.ERR_BAD_ARG and "ncols" in msg
    st, msg = _create(_lib, REG_TERM, None, np.zeros((10, 17)), 10, 17)
    assert st == _lib.ERR_BAD_ARG and "ncols" in msg
    assert _create(_lib, REG_TERM, None, np.zeros((2, 16)), 2, 16)[0] == _lib.OK
    with pytest.raises(ValueError):
        kmc.DataDensity(REG_TERM, D, params=range(7))
    with pytest.raises(ValueError):
        kmc.DataDensity(REG_TERM, np.zeros((2, 2, 2)))
    d = kmc.DataDensity(REG_TERM, np.arange(6.0), params=[2.0])       # a vector: one column
    assert d.data.shape == (6, 1) and d.params() == [2.0]


def test_broken_bodies_report_the_compiler_message(kmc):
    from kissmcmc_jl_amd import _lib
    with pytest.raises(kmc.KmcError, match="undeclared identifier 'zz'") as e:
        kmc.DataDensity("return x[0] * zz;", np.zeros((4, 2)))
    assert e.value.status == _lib.ERR_BAD_ARG
    with pytest.raises(kmc.KmcError, match="does not compile") as e:
        kmc.DataDensity(REG_TERM, np.zeros((4, 2)), prior="return x[0] +;")
    assert e.value.status == _lib.ERR_BAD_ARG


def test_validation_of_configs_needs_no_device(kmc):
    from kissmcmc_jl_amd import _lib
    L = _lib.lib()
    d = kmc.DataDensity(REG_TERM, np.zeros((8, 3)), params=[1.0])

    def cfg(**kw):
        c = _lib.Config()
        c.dtype, c.density, c.user_density = _lib.F64, _lib.DATA_DENSITY, d.user_handle
        c.nwalkers, c.ndim, c.ngenerations, c.nburnin, c.nthin, c.a_scale, c.seed = 16, 3, 10, 0, 1, 2.0, 1
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    assert L.kmc_validate(C.byref(cfg())) == _lib.OK
    assert L.kmc_validate(C.byref(cfg(user_density=None))) == _lib.ERR_BAD_ARG
    e = kmc.ExprDensity("-0.5*x*x")
    assert L.kmc_validate(C.byref(cfg(user_density=e.user_handle))) == _lib.ERR_BAD_ARG          # not a data handle
    assert L.kmc_validate(C.byref(cfg(density=_lib.USER_DENSITY))) == _lib.ERR_BAD_ARG             # a data handle as a user density
    for kw, what in [(dict(dtype=_lib.F32), "KMC_F32"), (dict(flags=_lib.ISLANDS, island_size=64), "island"), (dict(flags=_lib.P2P, shard_count=2), "P2P"),
                     (dict(shard_count=2), "sharding"), (dict(deal_count=2), "dealt"), (dict(flags=_lib.STORE_BLOBS), "blobs"),
                     (dict(ndim=33, nwalkers=70), "ndim")]:
        assert L.kmc_validate(C.byref(cfg(**kw))) == _lib.ERR_UNSUPPORTED, what
        assert what.lower() in L.kmc_last_error().decode().lower(), what
