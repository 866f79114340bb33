"""GPU: every kernel form against the algebraic definition of the code, bit-exact.

No oracle in between: the expected bytes come from ``rs_definition`` (Lagrange / Cauchy
over the field polynomials and the Cantor bases), which shares no machinery -- FFT,
skew tables, Walsh transform -- with the kernels or with ``oracle/leopard_oracle.c``.
Each case is the smallest shape that reaches its form; the docstrings name the kernel,
read from the dispatch code (rsm_runtime.cpp extend_squares / extend_squares_split /
launch_encode, kernels_gf8.hip launch_encode_gf8 / launch_encode_gf8_split,
kernels_gf8_bs.hip bs128_applicable / bs128_queue_applicable, kernels_gf16.hip
launch_encode_gf16).  Whole squares are compared where the definition costs under about
2 s of CPU; otherwise rows of Q1 and columns of Q2 / Q3 are sampled: always first, last
and k // 2, plus those next to a 2 KiB set boundary of the bit-sliced kernels.
"""
import ctypes

import numpy as np
import pytest

import rs_definition as rsd
import rsmt2d_amd as R

pytestmark = pytest.mark.gpu

FULL_BUDGET = 250e6  # symbol products of a whole-square definition (about 2 s of CPU)


def _rng(*key):
    return np.random.default_rng([0xDEF1] + [int(x) for x in key])


def _batch(k, S, count, seed):
    """[count][2k][2k][S]: random Q0, random non-zero filler in Q1..Q3 (a cell the
    kernel fails to write cannot match by accident)."""
    W = 2 * k
    g = _rng(seed, k, S, count)
    batch = g.integers(1, 256, (count, W, W, S), dtype=np.uint8)
    batch[:, :k, :k] = g.integers(0, 256, (count, k, k, S), dtype=np.uint8)
    return batch


def _extend(lib, ctx, batch, k, S):
    count = batch.shape[0]
    buf = R.DeviceBuffer(batch.nbytes)
    try:
        buf.upload(batch)
        R._check(lib.rsm_extend_squares_dev(ctx, buf.ptr, k, S, count, None))
        R._check(lib.rsm_sync(ctx))
        return buf.download(batch.nbytes).reshape(batch.shape)
    finally:
        buf.free()


def _sample(k, S):
    """first, last, k // 2 and the vectors around the first 2 KiB set boundary"""
    b = 2048 // S
    return sorted({0, k // 2, k - 1} | {i for i in (b - 1, b, b + 1) if 0 <= i < k})


def _check_square(got, ods, k, S):
    """got [2k][2k][S] against the definition: whole, or sampled (module docstring)."""
    assert np.array_equal(got[:k, :k], ods), "Q0 changed"
    nsym = S if rsd.field_bits(k) == 8 else S // 2
    if 3.0 * k ** 3 * nsym <= FULL_BUDGET:
        assert np.array_equal(got, rsd.extend_square(ods))
        return
    idx = _sample(k, S)
    q1_rows, q2_cols, q3_cols = rsd.extend_square(ods, rows=idx, cols=idx)
    assert np.array_equal(got[idx, k:], q1_rows), "Q1 rows"
    assert np.array_equal(got[k:, idx], q2_cols), "Q2 columns"
    assert np.array_equal(got[k:][:, [k + c for c in idx]], q3_cols), "Q3 columns"


def _check_batch(got, batch, k, S):
    count = batch.shape[0]
    for q in sorted({0, count - 1}):
        _check_square(got[q], batch[q, :k, :k], k, S)


# ---------------------------------------------------------------------------
# Codec.Encode
# ---------------------------------------------------------------------------
def _encode_case(k, S, rows=None):
    data = _rng(1, k, S).integers(0, 256, (k, S), dtype=np.uint8)
    got = R.NewLeoRSCodec().Encode([d.tobytes() for d in data])
    assert len(got) == k
    if rows is None:
        assert got == rsd.encode(data)
    else:
        assert [got[r] for r in rows] == rsd.parity_shares(data, rows)


@pytest.mark.parametrize("S", [64, 320])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 9, 17, 33, 64])
def test_encode_byte_table(lib, k, S):
    """k <= 64: the copy path of rsm_encode, launch_encode_gf8 -> encode_gf8_kernel<M>
    (one wave per codeword chunk), M = 1 .. 64; S = 320 ends on a partial 256-byte chunk."""
    _encode_case(k, S)


@pytest.mark.parametrize("k", [65, 128])
def test_encode_gf8_m128(lib, k):
    """65 <= k <= 128: rsm_encode runs zero-copy on the pinned staging buffer,
    launch_encode_gf8_split(nw = 16) -> encode_gf8_split16_kernel (where the runtime cannot
    map the buffer: launch_encode -> encode_gf8_bs128u_kernel)."""
    _encode_case(k, 64)


@pytest.mark.parametrize("S", [64, 576])
@pytest.mark.parametrize("k", [129, 256, 257, 512])
def test_encode_gf16_single_pass(lib, k, S):
    """GF(2^16), m = 256: enc16h_kernel<0>; m = 512: enc16h512_kernel<0> (run_encode<M>);
    S = 576 is nine 64-byte blocks, so the last 256-byte chunk is partial."""
    _encode_case(k, S)


@pytest.mark.parametrize("k", [513, 1025])
def test_encode_gf16_multi_pass(lib, k):
    """m >= 1024: run_encode_generic, g16_pass_kernel over the stream's work arrays
    (m = 1024: three bit groups; m = 2048: the top group has three bits); all parity."""
    _encode_case(k, 64)


def test_encode_gf16_k32768(lib):
    """The reference's largest codeword (m = 32768, g16_pass_kernel, four bit groups):
    16 sampled parity shares, always 0, 1, k // 2 and k - 1."""
    k = 32768
    rows = rsd.sample_indices(k, 16, always=(0, 1, k // 2, k - 1))
    assert len(rows) >= 16 and {0, 1, k // 2, k - 1} <= set(rows)
    _encode_case(k, 64, rows)


# ---------------------------------------------------------------------------
# rsm_extend_squares_dev
# ---------------------------------------------------------------------------
EXTEND_CASES = {
    # (k, S, count): the form the dispatch code sends it to
    (9, 64, 1): "encode_gf8_splitm_kernel<16, 4>",
    (33, 320, 2): "encode_gf8_splitm_kernel<64, 8>",
    (64, 64, 1): "encode_gf8_splitm_kernel<64, 8>",
    (16, 64, 65): "encode_gf8_kernel<16>, two passes",
    (65, 64, 1): "encode_gf8_split16_kernel, two launches",
    (128, 1024, 1): "encode_gf8_split16_kernel, two launches",
    (65, 64, 2): "encode_gf8_split_kernel<8>",
    (65, 64, 13): "encode_gf8_bs128u_kernel per pass",
    (100, 192, 13): "encode_gf8_bs128u_kernel per pass",
    (128, 64, 13): "extend_gf8_bs128q queue launch",
    (128, 192, 13): "extend_gf8_bs128q queue launch",
    (129, 64, 1): "enc16h_kernel",
}


@pytest.mark.parametrize("k,S,count", sorted(EXTEND_CASES))
def test_extend_squares_dev_forms(lib, k, S, count):
    """rsm_extend_squares_dev at the default split_max (12), by case (EXTEND_CASES):

    * (9, 64, 1), (33, 320, 2), (64, 64, 1): 9 <= k <= 64 and count <= 64 -> extend_squares_split
      -> encode_gf8_splitm_kernel<M, NW> (M = 16, 64, 64).
    * (16, 64, 65): past kSplitSmallBatch = 64 squares -> the two byte-table passes,
      encode_gf8_kernel<16>.
    * (65, 64, 1): asked for as the one-launch fused split, but split_fused_enabled() is
      false in the product library (the fused form is diagnostic-only), so this is the
      nearest shape the product reaches: two launches of encode_gf8_split16_kernel
      (test_extend_split_one_launch_diag runs the fused form through the diagnostic library).
    * (128, 1024, 1): 3 k ceil(S / 256) = 1536 workgroups; two launches of the 16-wave
      encode_gf8_split16_kernel (count == 1 -> kSplitWavesOne).
    * (65, 64, 2): count > 1 -> encode_gf8_split_kernel<8>, two launches.
    * (65, 64, 13), (100, 192, 13): count > split_max and k != 128, so no queue launch
      (bs128_queue_applicable): two passes of encode_gf8_bs128u_kernel, whose 2 KiB sets
      straddle codewords (k S is no multiple of 2048 at k = 65; S = 192 does not divide it).
    * (128, 64, 13), (128, 192, 13): one queue-driven launch (extend_squares_queue,
      launch_extend_gf8_bs128_queue); S = 192 takes the per-lane division.
    * (129, 64, 1): GF(2^16), m = 256: enc16h_kernel per pass.
    First and last square of each batch are compared."""
    ctx = R.device_context(0)
    batch = _batch(k, S, count, 2)
    got = _extend(lib, ctx, batch, k, S)
    _check_batch(got, batch, k, S)


def test_extend_split_one_launch_diag():
    """The one-launch fused split at (65, 64, 1) -- 3 k ceil(S / 256) = 195 workgroups,
    resident at once -- exists in the DIAGNOSTIC library only (rsm_diag_set_split_fused;
    launch_extend_gf8_split_fused -> encode_gf8_split_kernel<8> with p.fused): the same
    definition, through that library's own context."""
    k, S = 65, 64
    dl = R.diag_library()
    batch = _batch(k, S, 1, 5)
    ctx, p = ctypes.c_void_p(), ctypes.c_void_p()
    R._check_with(dl, dl.rsm_ctx_create(0, ctypes.byref(ctx)))
    try:
        R._check_with(dl, dl.rsm_dev_alloc(ctx, batch.nbytes, ctypes.byref(p)))
        R._check_with(dl, dl.rsm_memcpy(ctx, p, batch.ctypes.data, batch.nbytes, 0))
        R._check_with(dl, dl.rsm_diag_set_split_fused(1))
        try:
            R._check_with(dl, dl.rsm_extend_squares_dev(ctx, p, k, S, 1, None))
            R._check_with(dl, dl.rsm_diag_queue_check(ctx, None))
            R._check_with(dl, dl.rsm_sync(ctx))
        finally:
            R._check_with(dl, dl.rsm_diag_set_split_fused(0))
        got = np.empty_like(batch)
        R._check_with(dl, dl.rsm_memcpy(ctx, got.ctypes.data, p, batch.nbytes, 1))
        dl.rsm_dev_free(ctx, p)
    finally:
        dl.rsm_ctx_destroy(ctx)
    _check_batch(got, batch, k, S)


def test_extend_phases(lib):
    """rsm_extend_squares_phase_dev at (128, 64, 2): phase 1 is the row pass alone
    (encode_gf8_bs128u_kernel, MODE 104) -- Q1 equals the definition, Q2 / Q3 still hold
    the pre-filled bytes -- then phase 2 the column pass (MODE 184, sets walked in
    reverse)."""
    k, S, count = 128, 64, 2
    ctx = R.device_context(0)
    batch = _batch(k, S, count, 3)
    buf = R.DeviceBuffer(batch.nbytes)
    try:
        buf.upload(batch)
        R._check(lib.rsm_extend_squares_phase_dev(ctx, buf.ptr, k, S, count, 1, None))
        R._check(lib.rsm_sync(ctx))
        mid = buf.download(batch.nbytes).reshape(batch.shape)
        assert np.array_equal(mid[:, k:], batch[:, k:]), "phase 1 touched Q2 / Q3"
        assert np.array_equal(mid[:, :k, :k], batch[:, :k, :k]), "phase 1 touched Q0"
        for q in range(count):
            # all of Q1: k codewords of k shares
            want = rsd.encode_vectors(batch[q, :k, :k])
            assert np.array_equal(mid[q, :k, k:], want), ("Q1", q)
        R._check(lib.rsm_extend_squares_phase_dev(ctx, buf.ptr, k, S, count, 2, None))
        R._check(lib.rsm_sync(ctx))
        got = buf.download(batch.nbytes).reshape(batch.shape)
    finally:
        buf.free()
    assert np.array_equal(got[:, :k], mid[:, :k]), "phase 2 touched the top half"
    _check_batch(got, batch, k, S)


# ---------------------------------------------------------------------------
# the wide forms (64-bit per-symbol bases), forced by a lowered offset limit
# ---------------------------------------------------------------------------
@pytest.fixture
def pctx(lib):
    """A private context: its limits are lowered, the shared one keeps the defaults."""
    h = ctypes.c_void_p()
    R._check(lib.rsm_ctx_create(0, ctypes.byref(h)))
    yield h.value
    lib.rsm_ctx_destroy(h.value)


@pytest.mark.parametrize("k,S", [(64, 64), (200, 64)])
def test_extend_wide_forms(lib, pctx, k, S):
    """offset_limit = 1 makes narrow_ok false for every codeword: (64, 64) runs
    encode_gf8_wide_kernel<64> for both passes, (200, 64) the multi-pass GF(2^16)
    g16_pass_kernel at m = 256 (launch_encode sets wide for k <= 512 as well)."""
    batch = _batch(k, S, 2, 4)
    R._check(lib.rsm_ctx_set_limits(pctx, 1, 0))
    try:
        got = _extend(lib, pctx, batch, k, S)
    finally:
        R._check(lib.rsm_ctx_set_limits(pctx, 0, 0))
    _check_batch(got, batch, k, S)
