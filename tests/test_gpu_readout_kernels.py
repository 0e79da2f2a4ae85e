"""The chain read-out kernels (csrc/kmc_copy_kernels.hpp: chain_by_walker, rows_compact) element by element, on data in which
every element is unique, in every regime of the tile planner by_walker_tile(nd) and of launch_by_walker -- through
kmc_debug_chain_by_walker / kmc_debug_rows_compact, which run the library's own launch code on the caller's arrays.

The tests over a real sampler (test_gpu_chain_by_walker.py) compare two read-outs of one run: rejected moves repeat rows, so a
wrong sample index inside a tile is invisible for a large share of the elements, and they reach ndim <= 200 only.  Here
src[k][w][c] = its own linear index + 1 (exact in float below 2^24), the pad columns c >= nd hold NaN, the destination is
pre-filled with a sentinel and is 4 096 doubles longer than the call may write, and the WHOLE destination is compared, exactly,
with a numpy transposition: a misplaced element, a leaked pad value, a write into a stride gap or past the end and an element
left unwritten all fail the one comparison."""
import ctypes as C

import numpy as np
import pytest

SENTINEL = -1.0          # (the source holds positive integers and NaN)
SLACK = 4096             # doubles of the destination beyond what a call may write


def tile(nd):
    """(TW, TK) of by_walker_tile(nd), restated from the regime table above it: walkers x samples of one LDS tile."""
    if nd <= 200:
        return min(64, max(1, 7680 // (32 * nd + 1))), 32
    if nd <= 3000:
        return 1, 6000 // nd
    if nd <= 3839:
        return 2, 1
    return 1, 1           # 3840 ... 4096: still the tiled branch; beyond: column windows of 4 096


# the table of the planner's comment, for every row length used below: a restatement that drifts from it (or a table edited to
# follow a moved regime boundary) shows here, not as a regime silently no longer covered
TABLE = {1: (64, 32), 2: (64, 32), 7: (34, 32), 32: (7, 32), 33: (7, 32), 200: (1, 32),
         201: (1, 29), 1500: (1, 4), 2999: (1, 2), 3000: (1, 2),
         3001: (2, 1), 3839: (2, 1),
         3840: (1, 1), 4096: (1, 1),
         4097: (1, 1), 8193: (1, 1)}


def test_tile_restatement_matches_the_planner_table():
    for nd, want in TABLE.items():
        assert tile(nd) == want, nd
    # the regime boundaries themselves
    assert [tile(nd)[1] for nd in (200, 201, 206, 207, 3000, 3001)] == [32, 29, 29, 28, 2, 1]
    assert [tile(nd)[0] for nd in (3000, 3001, 3839, 3840)] == [1, 2, 2, 1]


def make_src(K, nl, ld, nd, dtype=np.float64):
    src = (np.arange(K * nl * ld, dtype=np.float64) + 1.0).reshape(K, nl, ld)
    src[:, :, nd:] = np.nan
    if dtype == np.float32:
        assert K * nl * ld < 2 ** 24          # every value exact in float
    return np.ascontiguousarray(src.astype(dtype))


def run_by_walker(src, nd, w0=0, nw=None, gap=0):
    """The device transposition and its numpy statement, both over the whole destination."""
    from kissmcmc_jl_amd import _lib
    K, nl, ld = src.shape
    nw = nl - w0 if nw is None else nw
    stride = K * nd + gap
    dst_len = (nw - 1) * stride + K * nd + gap + SLACK
    dst = np.full(dst_len, SENTINEL)
    _lib.check(_lib.lib().kmc_debug_chain_by_walker(src.ctypes.data_as(C.c_void_p), int(src.dtype == np.float32), K, nl, ld, nd, w0, nw, stride,
                                                    dst.ctypes.data_as(C.POINTER(C.c_double)), dst_len, 0))
    exp = np.full(dst_len, SENTINEL)
    for w in range(nw):                        # exp[w * dst_stride + k * nd + c] = src[k][w0 + w][c]
        exp[w * stride:w * stride + K * nd] = src[:, w0 + w, :nd].astype(np.float64).reshape(-1)
    return dst, exp


def shape_of(nd, nl=None, K=None):
    """One whole tile plus one ragged tile, in walkers and in samples."""
    tw, tk = tile(nd)
    return (tk + 1 if K is None else K), (2 * tw + 1 if nl is None else nl)


# (nd, ld, nl, K): None = 2 TW + 1 walkers, TK + 1 samples
REGIMES = [
    pytest.param(1, 1, None, None, id="logp-rows-nd1"),
    pytest.param(7, 8, None, None, id="padded-nd7"),
    pytest.param(33, 34, None, None, id="padded-nd33"),
    pytest.param(2, 2, None, None, id="dense-nd2"),
    pytest.param(32, 32, None, None, id="dense-nd32"),
    pytest.param(200, 200, None, None, id="dense-nd200-TW1"),
    pytest.param(201, 202, None, None, id="TK29-nd201"),
    pytest.param(1500, 1500, None, None, id="TK4-nd1500"),
    pytest.param(2999, 3000, None, None, id="TK2-nd2999"),
    pytest.param(3001, 3002, 5, 3, id="TW2-nd3001"),
    pytest.param(3839, 3840, 5, 3, id="TW2-nd3839"),
    pytest.param(3840, 3840, None, None, id="last-tiled-nd3840"),
    pytest.param(4096, 4096, None, None, id="last-tiled-nd4096"),
    pytest.param(4097, 4098, 3, 3, id="windows-nd4097"),
    pytest.param(8193, 8194, 3, 3, id="windows-nd8193"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("nd,ld,nl,K", REGIMES)
def test_by_walker_every_tile_regime(kmc, nd, ld, nl, K):
    K, nl = shape_of(nd, nl, K)
    dst, exp = run_by_walker(make_src(K, nl, ld, nd), nd)
    np.testing.assert_array_equal(dst, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("nd,ld", [(7, 8), (201, 202), (4097, 4098)])
def test_by_walker_float_source(kmc, nd, ld):
    K, nl = shape_of(nd, 3 if nd > 4096 else None, 3 if nd > 4096 else None)
    dst, exp = run_by_walker(make_src(K, nl, ld, nd, np.float32), nd)
    np.testing.assert_array_equal(dst, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("nd,ld,K", [(7, 8, None), (3001, 3002, 3)])
def test_by_walker_piece_of_walkers(kmc, nd, ld, K):
    """Walkers [3, nl - 2) of a larger ensemble: the piece still spans two whole tiles and a ragged one."""
    tw, _ = tile(nd)
    nl = 2 * tw + 1 + 5
    K, _ = shape_of(nd, nl, K)
    dst, exp = run_by_walker(make_src(K, nl, ld, nd), nd, w0=3, nw=nl - 5)
    np.testing.assert_array_equal(dst, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("nd,ld", [(1, 1), (32, 32), (4097, 4098)])
def test_by_walker_wide_destination_stride(kmc, nd, ld):
    """dst_stride = K * nd + 5 (a block of a streamed chain has nsamples * nd): the gaps between walkers keep the sentinel."""
    K, nl = shape_of(nd, 3 if nd > 4096 else None, 3 if nd > 4096 else None)
    dst, exp = run_by_walker(make_src(K, nl, ld, nd), nd, gap=5)
    np.testing.assert_array_equal(dst, exp)


@pytest.mark.gpu
def test_by_walker_sample_slices(kmc):
    """More than 65 535 sample tiles (gridDim.y): launch_by_walker goes on in a second launch with source and destination shifted --
    what metropolis enters with one chain and 2.1 M samples.  34 MB each way."""
    K = 65535 * 32 + 33
    assert -(-K // tile(1)[1]) > 65535
    dst, exp = run_by_walker(make_src(K, 2, 1, 1), 1)
    np.testing.assert_array_equal(dst, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("nd,ld", [(1, 1), (201, 202), (4097, 4098)])
@pytest.mark.parametrize("what", ["K1", "nw1", "nl1"])
def test_by_walker_degenerate(kmc, nd, ld, what):
    K, nl = shape_of(nd)
    if what == "K1":
        dst, exp = run_by_walker(make_src(1, nl, ld, nd), nd)
    elif what == "nw1":
        dst, exp = run_by_walker(make_src(K, nl, ld, nd), nd, w0=1, nw=1)
    else:
        dst, exp = run_by_walker(make_src(K, 1, ld, nd), nd)
    np.testing.assert_array_equal(dst, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,ld,nd", [(1, 2, 1), (257, 8, 7), (1000, 34, 33), (3, 4098, 4097),
                                        (300000, 8, 7)])         # rows * nd > 8192 * 256: a second trip of the grid-stride loop
def test_rows_compact(kmc, rows, ld, nd):
    from kissmcmc_jl_amd import _lib
    if rows == 300000:
        assert rows * nd > 8192 * 256
    src = make_src(1, rows, ld, nd)[0]
    dst_len = rows * nd + SLACK
    dst = np.full(dst_len, SENTINEL)
    dp = C.POINTER(C.c_double)
    _lib.check(_lib.lib().kmc_debug_rows_compact(src.ctypes.data_as(dp), rows, ld, nd, dst.ctypes.data_as(dp), dst_len, 0))
    exp = np.full(dst_len, SENTINEL)
    exp[:rows * nd] = src[:, :nd].reshape(-1)
    np.testing.assert_array_equal(dst, exp)


def test_debug_entries_refuse_bad_arguments_before_the_device(kmc):
    """Every bound of the two entries is KMC_ERR_BAD_ARG with a message, checked before the device is asked for: a wrong call
    from a test is an error, never a fault.  No device needed."""
    from kissmcmc_jl_amd import _lib
    L = _lib.lib()
    dp = C.POINTER(C.c_double)
    src, dst = np.ones(12), np.full(64, SENTINEL)
    ok = dict(src=src.ctypes.data_as(C.c_void_p), is_float=0, K=2, nl=3, ld=2, nd=2, w0=0, nw=3, stride=4, dst=dst.ctypes.data_as(dp), dst_len=12)

    def bw(**kw):
        a = dict(ok, **kw)
        st = L.kmc_debug_chain_by_walker(a["src"], a["is_float"], a["K"], a["nl"], a["ld"], a["nd"], a["w0"], a["nw"], a["stride"], a["dst"], a["dst_len"], 0)
        return st, L.kmc_last_error().decode()

    assert bw()[0] in (_lib.OK, _lib.ERR_NO_DEVICE)                      # the base call itself passes every check
    for bad in (dict(nd=0), dict(nd=-1), dict(nd=3), dict(ld=1), dict(w0=-1), dict(w0=1), dict(nw=4), dict(w0=3, nw=1), dict(nw=0), dict(K=0), dict(nl=0),
                dict(stride=3), dict(dst_len=11), dict(stride=6, dst_len=15), dict(dst_len=0), dict(src=None), dict(dst=None), dict(is_float=2),
                dict(ld=2 ** 31), dict(nl=2 ** 31, nw=1), dict(nd=65535 * 4096 + 1, ld=65535 * 4096 + 1, stride=2 ** 40, dst_len=2 ** 50),
                dict(K=2 ** 40, nl=2 ** 30, stride=2 ** 41, dst_len=2 ** 60), dict(stride=2 ** 62, dst_len=2 ** 62)):
        st, msg = bw(**bad)
        assert st == _lib.ERR_BAD_ARG and msg.startswith("kmc_debug_chain_by_walker: "), (bad, st, msg)
    np.testing.assert_array_equal(dst[12:], SENTINEL)

    okc = dict(src=src.ctypes.data_as(dp), rows=3, ld=4, nd=3, dst=dst.ctypes.data_as(dp), dst_len=9)

    def rc(**kw):
        a = dict(okc, **kw)
        return L.kmc_debug_rows_compact(a["src"], a["rows"], a["ld"], a["nd"], a["dst"], a["dst_len"], 0), L.kmc_last_error().decode()

    assert rc()[0] in (_lib.OK, _lib.ERR_NO_DEVICE)
    for bad in (dict(nd=0), dict(nd=5), dict(ld=2), dict(rows=0), dict(rows=-1), dict(dst_len=8), dict(src=None), dict(dst=None),
                dict(ld=2 ** 31, dst_len=64), dict(rows=2 ** 61, dst_len=2 ** 62)):
        st, msg = rc(**bad)
        assert st == _lib.ERR_BAD_ARG and msg.startswith("kmc_debug_rows_compact: "), (bad, st, msg)
