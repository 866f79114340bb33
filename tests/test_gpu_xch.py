"""The k = 128 set body's exchange (64-bit stores, the tail of the large layers inside
the read statements; kernels_gf8_bs.hip bs_split_wave) on the GPU: every square of
every batch bit-exact against the oracle.  All cases go through rsm_extend_squares_dev
with rsm_ctx_set_split_max(ctx, 0), so batches the queue kernel accepts run on it
(rsm_runtime.cpp extend_squares: k = 128 with k * S a multiple of 2 KiB; any other k takes
the two passes, whose kernels this exchange is not part of)."""
import ctypes

import numpy as np
import pytest

import oracle
import rsmt2d_amd as R

pytestmark = pytest.mark.gpu


def extend_and_check(lib, k, S, count, seed):
    ctx = R.device_context(0)
    W = 2 * k
    sq = W * W * S
    buf = R.DeviceBuffer(sq * count)
    buf.fill_random(seed)  # the parity quadrants start as garbage
    R._check(lib.rsm_sync(ctx))
    prev = ctypes.c_int(0)
    R._check(lib.rsm_ctx_set_split_max(ctx, 0, ctypes.byref(prev)))
    try:
        R._check(lib.rsm_extend_squares_dev(ctx, buf.ptr, k, S, count, None))
        R._check(lib.rsm_sync(ctx))
    finally:
        R._check(lib.rsm_ctx_set_split_max(ctx, prev.value, None))
    for j in range(count):  # every square
        got = buf.download(sq, j * sq).reshape(W, W, S)
        assert np.array_equal(got, oracle.extend_square(got[:k, :k].copy(), nthreads=8)), (k, S, count, j)


def test_many_consecutive_sets_per_workgroup(lib):
    """k = 128, S = 512, 16 squares: 1,536 sets on 256 workgroups, so every workgroup
    runs several sets back to back -- a read of one set's last exchange that a store
    of the next set's first could overtake (a barrier missing across the back-edge)
    would corrupt squares here."""
    extend_and_check(lib, 128, 512, 16, 0xC401)


@pytest.mark.parametrize("count", [1, 2])
def test_prologue_and_exit_paths(lib, count):
    """k = 128, S = 512, 1 and 2 squares (96 / 192 sets): most workgroups run one set
    or none."""
    extend_and_check(lib, 128, 512, count, 0xC410 + count)


def test_general_lane_geometry(lib):
    """k = 128, S = 192, 13 squares: S does not divide the 2 KiB set width, so the queue
    kernel's instantiation with per-lane division (not the fixed per-lane offsets of
    the S = 512 shape) runs the same set body."""
    extend_and_check(lib, 128, 192, 13, 0xC420)


def test_smaller_square_same_call(lib):
    """k = 65, S = 192, 13 squares through the same call: the dispatch sends every
    k < 128 to the two passes (the queue launch needs k = 128), which must keep
    working beside the changed kernel in the same object."""
    extend_and_check(lib, 65, 192, 13, 0xC430)
