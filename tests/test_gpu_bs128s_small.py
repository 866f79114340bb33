"""The k = 128 queue launch (extend_gf8_bs128s_kernel, kernels_gf8_bs.hip bs_split_wave)
at the smallest batches that still reach it, every square against the oracle:

  13 squares of k = 128, S = 512   the first count above the latency form's split_max
                                   (12): the instantiation with fixed per-lane offsets;
  16 squares of k = 128, S = 192   S does not divide the 2 KiB set width: the general
                                   instantiation, sets straddle shares;
  14 squares of k = 65,  S = 64    symbols e >= k are out of range (zero inputs, no
                                   stores); this k goes to the two passes, which share
                                   the object and the load / store helpers.

Each shape runs through the product library (the body production launches: h1 copied
from its landing registers P into X[8..15], the next set's h1 loads issued after T0 and
the small IFFT of h0) and, in the diagnostic library, through every variant of the top
of the set by name: 59000 / 59007 copies with the loads at the top of the set (the body
up to round 7; fixed offsets / general), 59001 / 59002 the first transpose stage of h1 reading P instead of the copies
(fixed offsets / general), 59003 / 59005 production's body, 59004 / 59006 from P with
the late loads.  The launch takes the instantiation from the mode, so each mode runs
only on the shape it is built for."""
import ctypes

import numpy as np
import pytest

import oracle
import rsmt2d_amd as R

pytestmark = pytest.mark.gpu

SHAPES = [(128, 512, 13), (128, 192, 16), (65, 64, 14)]


def check_squares(got, k):
    for j in range(got.shape[0]):
        assert np.array_equal(got[j], oracle.extend_square(got[j, :k, :k].copy(), nthreads=8)), j


@pytest.mark.parametrize("k,S,count", SHAPES)
def test_product_library(lib, k, S, count):
    ctx = R.device_context(0)
    W = 2 * k
    n = W * W * S * count
    buf = R.DeviceBuffer(n)
    buf.fill_random(0xB5 + k + S)  # the parity quadrants start as garbage
    R._check(lib.rsm_extend_squares_dev(ctx, buf.ptr, k, S, count, None))
    R._check(lib.rsm_sync(ctx))
    check_squares(buf.download(n).reshape(count, W, W, S), k)
    buf.free()


def test_two_streams_at_once(lib):
    """Two launches of the first shape in flight together (each stream has its own queue
    words): neither may see the other's items or signals."""
    k, S, count = SHAPES[0]
    ctx = R.device_context(0)
    W = 2 * k
    n = W * W * S * count
    bufs = [R.DeviceBuffer(n) for _ in range(2)]
    streams = []
    for i, b in enumerate(bufs):
        b.fill_random(0x2500 + i)
        s = ctypes.c_void_p()
        R._check(lib.rsm_stream_create(ctx, ctypes.byref(s)))
        streams.append(s.value)
    R._check(lib.rsm_sync(ctx))
    try:
        for _ in range(2):  # the second round re-uses each stream's self-re-zeroed queue words
            for b, s in zip(bufs, streams):
                R._check(lib.rsm_extend_squares_dev(ctx, b.ptr, k, S, count, s))
        for s in streams:
            R._check(lib.rsm_stream_check(ctx, s))
        for b in bufs:
            check_squares(b.download(n).reshape(count, W, W, S), k)
    finally:
        for s in streams:
            R._check(lib.rsm_stream_destroy(ctx, s))
        for b in bufs:
            b.free()


@pytest.fixture(scope="module")
def dl():
    return R.diag_library()


MODES = [(59000, 0), (59001, 0), (59003, 0), (59004, 0),   # fixed per-lane offsets
         (59002, 1), (59005, 1), (59006, 1), (59007, 1),   # general instantiation
         (59000, 2), (59001, 2)]                           # the two passes beside them


@pytest.mark.parametrize("mode,k,S,count", [(m, *SHAPES[i]) for m, i in MODES])
def test_set_bodies_by_name(dl, mode, k, S, count):
    chk = lambda rc: R._check_with(dl, rc)
    h = ctypes.c_void_p()
    chk(dl.rsm_ctx_create(0, ctypes.byref(h)))
    ctx = h.value
    W = 2 * k
    n = W * W * S * count
    p = ctypes.c_void_p()
    chk(dl.rsm_dev_alloc(ctx, n, ctypes.byref(p)))
    try:
        chk(dl.rsm_dev_fill_random(ctx, p.value, n, 0x5900 + mode + S))
        chk(dl.rsm_sync(ctx))
        chk(dl.rsm_diag_set_bs_mode(mode, 1, 0))
        chk(dl.rsm_extend_squares_dev(ctx, p.value, k, S, count, None))
        chk(dl.rsm_sync(ctx))
        got = np.empty(n, np.uint8)
        chk(dl.rsm_memcpy(ctx, got.ctypes.data, p.value, n, 1))
        check_squares(got.reshape(count, W, W, S), k)
    finally:
        chk(dl.rsm_diag_set_bs_mode(40, 1, 0))
        dl.rsm_dev_free(ctx, p.value)
        dl.rsm_ctx_destroy(ctx)
