"""GPU: no store outside the operand, from bases that are only 64-byte aligned.

Every other device test hands the kernels a buffer straight from rsm_dev_alloc and
compares only its own bytes, so a tail store past the last share of the last square would
land in allocator slack unnoticed -- and the bit-sliced 2 KiB sets straddle codewords and
squares, the split / GF(2^16) forms work in 256-byte chunks on 64-byte shares.  A caller
that sub-allocates (a cgo arena) also passes bases that are 64-byte but not 128-byte
aligned.

Here every operand sits inside one allocation between a front guard of 4096 + 64 bytes
and a back guard of 8192 bytes, both filled with a seeded non-constant pattern.  After the
call: both guards byte-identical, the operand equal to the oracle (a full compare: this
file is about addressing; the oracle is pinned by tests/test_definition_cpu.py), and every
input-only region unchanged.  The kernels' global loads and stores are at most 16 bytes
wide (uint4 / dwordx4), so no entry needs more than the 64-byte alignment a share has;
rsm_proof_nodes_dev / rsm_proofs_dev keep their documented 16-byte alignment, which the
4096 + 64 offset satisfies.
"""
import ctypes
import os

import numpy as np
import pytest

import oracle
import proof_verify as V
import rsmt2d_amd as R
from oracle import crossword, nmt

pytestmark = pytest.mark.gpu
CPU = min(16, os.cpu_count() or 1)
FRONT, BACK = 4096 + 64, 8192


def _rng(*key):
    return np.random.default_rng([0x6A2D] + [int(x) for x in key])


class Guarded:
    """front guard | operand | back guard in ONE DeviceBuffer; ``ptr`` is the operand."""

    def __init__(self, operand, seed):
        operand = np.ascontiguousarray(operand)
        self.shape, self.dtype = operand.shape, operand.dtype
        self.sent = operand.reshape(-1).view(np.uint8).copy()
        g = _rng(0x9A, seed, self.sent.size)
        self.front = g.integers(0, 256, FRONT, dtype=np.uint8)
        self.back = g.integers(0, 256, BACK, dtype=np.uint8)
        self.buf = R.DeviceBuffer(FRONT + self.sent.size + BACK)
        self.buf.upload(np.concatenate([self.front, self.sent, self.back]))
        self.ptr = self.buf.ptr + FRONT
        assert self.ptr % 128 == 64, "the operand base is meant to be 64- but not 128-byte aligned"

    def result(self):
        """Checks both guards; returns the operand as it is now."""
        got = self.buf.download()
        n = self.sent.size
        assert np.array_equal(got[:FRONT], self.front), "a store landed before the operand"
        assert np.array_equal(got[FRONT + n:], self.back), "a store landed past the operand"
        return got[FRONT:FRONT + n].view(self.dtype).reshape(self.shape)

    def unchanged(self):
        """Guards intact and the operand (an input-only region) byte-identical."""
        return np.array_equal(self.result().reshape(-1).view(np.uint8), self.sent)

    def free(self):
        self.buf.free()


def _filled_batch(k, S, count, seed):
    """[count][2k][2k][S]: random Q0, random filler elsewhere."""
    return _rng(seed, k, S, count).integers(0, 256, (count, 2 * k, 2 * k, S), dtype=np.uint8)


@pytest.mark.parametrize("k,S,count", [(65, 64, 1), (65, 64, 13), (127, 320, 2), (128, 64, 13), (33, 64, 1),
                                       (16, 64, 65), (129, 64, 1), (257, 64, 1)])
def test_extend_squares_guarded(lib, k, S, count):
    """rsm_extend_squares_dev: the 16-wave split (65, 64, 1), the per-pass bit-sliced sets
    (65, 64, 13: 65 * 64 bytes per row, so sets straddle rows and squares), the 8-wave
    split with a partial chunk (127, 320, 2), the queue launch (128, 64, 13), splitm
    (33, 64, 1), the byte-table passes (16, 64, 65), GF(2^16) m = 256 and m = 512."""
    ctx = R.device_context(0)
    batch = _filled_batch(k, S, count, 1)
    g = Guarded(batch, 1)
    try:
        R._check(lib.rsm_extend_squares_dev(ctx, g.ptr, k, S, count, None))
        R._check(lib.rsm_sync(ctx))
        got = g.result()
    finally:
        g.free()
    for q in range(count):
        assert np.array_equal(got[q], oracle.extend_square(batch[q, :k, :k], nthreads=CPU)), q


def test_extend_rows_cols_partial_guarded(lib):
    """rsm_extend_rows_dev / rsm_extend_cols_dev on a partial range of a (100, 192)
    square (encode_gf8_bs128u_kernel over nrows * 192 bytes: a ragged last set): the
    range equals the oracle, every other row / column keeps its bytes."""
    k, S = 100, 192
    W = 2 * k
    ctx = R.device_context(0)
    sq = _filled_batch(k, S, 1, 2)[0]
    want = oracle.extend_square(sq[:k, :k], nthreads=CPU)
    row0, nrows = 7, 50
    g = Guarded(sq, 2)
    try:
        R._check(lib.rsm_extend_rows_dev(ctx, g.ptr, k, S, row0, nrows, None))
        R._check(lib.rsm_sync(ctx))
        got = g.result()
    finally:
        g.free()
    exp = sq.copy()
    exp[row0:row0 + nrows, k:] = want[row0:row0 + nrows, k:]
    assert np.array_equal(got, exp)
    # columns 30 .. 149 (Q0 and Q1 columns) of a square whose top half is complete
    col0, ncols = 30, 120
    sq2 = sq.copy()
    sq2[:k] = want[:k]
    g = Guarded(sq2, 3)
    try:
        R._check(lib.rsm_extend_cols_dev(ctx, g.ptr, k, S, col0, ncols, None))
        R._check(lib.rsm_sync(ctx))
        got = g.result()
    finally:
        g.free()
    exp = sq2.copy()
    exp[k:, col0:col0 + ncols] = want[k:, col0:col0 + ncols]
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("k,S,count", [(100, 192, 5), (256, 64, 3)])
def test_encode_batch_guarded(lib, k, S, count):
    """rsm_encode_batch_dev with cw_stride > k * share_stride: the gaps between the
    codewords are guard bytes too, in d_out (kept) and in d_in (input-only, with the data).
    (100, 192, 5): encode_gf8_bs128u_kernel; (256, 64, 3): enc16h_kernel."""
    ctx = R.device_context(0)
    share_stride = S
    cw_stride = k * share_stride + 192
    n = count * cw_stride
    src = _rng(4, k, S).integers(0, 256, n, dtype=np.uint8)
    dst = _rng(5, k, S).integers(0, 256, n, dtype=np.uint8)
    gi, go = Guarded(src, 4), Guarded(dst, 5)
    try:
        R._check(lib.rsm_encode_batch_dev(ctx, gi.ptr, go.ptr, k, S, count, cw_stride, share_stride, None))
        R._check(lib.rsm_sync(ctx))
        got = go.result()
        assert gi.unchanged(), "d_in changed"
    finally:
        gi.free()
        go.free()
    exp = dst.copy()
    for q in range(count):
        cw = src[q * cw_stride:q * cw_stride + k * S].reshape(k, S)
        par = oracle.encode([s.tobytes() for s in cw])
        exp[q * cw_stride:q * cw_stride + k * S] = np.frombuffer(b"".join(par), np.uint8)
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("k,S", [(65, 64), (200, 64)])
def test_decode_vectors_guarded(lib, k, S, axis):
    """rsm_decode_vectors_dev over every vector, each missing 1 .. k cells:
    decode_gf8_split_kernel (65, 64), errloc16_kernel + dec16f_kernel (200, 64)."""
    ctx = R.device_context(0)
    W = 2 * k
    g = _rng(6, k, S, axis)
    full = oracle.extend_square(g.integers(0, 256, (k, k, S), dtype=np.uint8), nthreads=CPU)
    pres = np.ones((W, W), np.uint8)
    for v in range(W):
        lost = g.choice(W, size=int(g.integers(1, k + 1)), replace=False)
        if axis == 0:
            pres[v, lost] = 0
        else:
            pres[lost, v] = 0
    ge, gp = Guarded(full * pres[:, :, None], 6), Guarded(pres, 7)
    gi = Guarded(np.arange(W, dtype=np.uint32), 8)
    try:
        R._check(lib.rsm_decode_vectors_dev(ctx, ge.ptr, gp.ptr, k, S, axis, gi.ptr, W, None))
        R._check(lib.rsm_sync(ctx))
        got = ge.result()
        assert gp.unchanged() and gi.unchanged(), "presence / indices changed"
    finally:
        for x in (ge, gp, gi):
            x.free()
    assert np.array_equal(got, full)


def _tree_params(tree, k):
    return R.NmtParams(29, 1, k) if tree == "nmt" else None


def _want_root(sq, p, axis, index):
    vec = V.vector(sq, axis, index)
    return crossword.merkle_root(vec) if p is None else nmt.erasured_root(vec, index, p.square_size, p.namespace_size)


@pytest.mark.parametrize("W,count", [(6, 3), (130, 2)])
@pytest.mark.parametrize("tree", ["default", "nmt"])
def test_roots_squares_guarded(lib, tree, W, count):
    """rsm_roots_squares_dev / rsm_nmt_roots_squares_dev: the roots (and the NMT statuses)
    between guards, the squares input-only."""
    ctx = R.device_context(0)
    k, S = W // 2, 64
    p = _tree_params(tree, k)
    nl = 32 if p is None else 2 * p.namespace_size + 32
    batch = np.stack([V.sorted_q0_square(k, S, 29, 800 + W + q) for q in range(count)])
    ge = Guarded(batch, 9)
    gr = Guarded(_rng(10, W).integers(0, 256, count * 2 * W * nl, dtype=np.uint8), 10)
    gs = Guarded(np.full(count * 2 * W, 0xFFFFFFFF, np.uint32), 11)
    try:
        if p is None:
            R._check(lib.rsm_roots_squares_dev(ctx, ge.ptr, W, S, count, gr.ptr, None))
        else:
            R._check(lib.rsm_nmt_roots_squares_dev(ctx, ge.ptr, W, S, count, ctypes.byref(p), gr.ptr, gs.ptr, None))
        R._check(lib.rsm_sync(ctx))
        roots = gr.result().tobytes()
        status = gs.result()
        assert ge.unchanged(), "the squares changed"
    finally:
        for x in (ge, gr, gs):
            x.free()
    if p is None:
        assert (status == 0xFFFFFFFF).all()  # (not passed to the DefaultTree call)
    else:
        assert not status.any()
    for q in range(count):
        for a in (0, 1):
            for i in range(W):
                t = (q * 2 + a) * W + i
                assert roots[t * nl:(t + 1) * nl] == _want_root(batch[q], p, a, i), (q, a, i)


@pytest.mark.parametrize("W", [6, 70])
@pytest.mark.parametrize("tree", ["default", "nmt"])
def test_proofs_guarded(lib, tree, W):
    """rsm_proof_nodes_dev + rsm_proofs_dev: the node store, the roots / statuses, the
    records and the gathered shares each between guards (bases 16-byte aligned, as
    documented, but not 128-byte aligned); the squares input-only.  Records equal the
    host restatement and verify against the oracle root of their tree."""
    ctx = R.device_context(0)
    k, S, count = W // 2, 64, 2
    p = _tree_params(tree, k)
    pp = ctypes.byref(p) if p is not None else None
    nl = 32 if p is None else 2 * p.namespace_size + 32
    batch = np.stack([V.sorted_q0_square(k, S, 29, 900 + W + q) for q in range(count)])
    if W <= 6:
        samples = [(q, a, i, x) for q in range(count) for a in (0, 1) for i in range(W) for x in range(W)]
    else:
        g = _rng(12, W)
        samples = sorted({(q, a, i, x) for q in (0, count - 1) for a in (0, 1) for i in (0, W - 1) for x in (0, W - 1)} |
                         {(int(g.integers(count)), int(g.integers(2)), int(g.integers(W)), int(g.integers(W)))
                          for _ in range(48)})
    n = len(samples)
    rb = int(lib.rsm_proof_record_bytes(W, pp))
    assert rb == V.record_bytes(W, nl)
    nbytes = int(lib.rsm_proof_nodes_bytes(W, pp, count))
    assert nbytes > 0
    ge = Guarded(batch, 13)
    gn = Guarded(_rng(14, W).integers(0, 256, nbytes, dtype=np.uint8), 14)
    gr = Guarded(_rng(15, W).integers(0, 256, count * 2 * W * nl, dtype=np.uint8), 15)
    gs = Guarded(np.full(count * 2 * W, 0xFFFFFFFF, np.uint32), 16)
    gc = Guarded(_rng(17, W).integers(0, 256, n * rb, dtype=np.uint8), 17)
    gh = Guarded(_rng(18, W).integers(0, 256, n * S, dtype=np.uint8), 18)
    try:
        arr = (R.Sample * n)(*[R.Sample(*s) for s in samples])
        R._check(lib.rsm_proof_nodes_dev(ctx, ge.ptr, W, S, count, pp, gn.ptr, gr.ptr, gs.ptr, None))
        R._check(lib.rsm_proofs_dev(ctx, gn.ptr, ge.ptr, W, S, count, pp, arr, n, gc.ptr, gh.ptr, None))
        R._check(lib.rsm_sync(ctx))
        gn.result()  # (the store is opaque: only its guards)
        roots = gr.result().tobytes()
        assert not gs.result().any()
        records = gc.result().tobytes()
        shares = gh.result().tobytes()
        assert ge.unchanged(), "the squares changed"
    finally:
        for x in (ge, gn, gr, gs, gc, gh):
            x.free()
    want_roots = {}
    for i, (q, a, idx, pos) in enumerate(samples):
        vec = V.vector(batch[q], a, idx)
        assert shares[i * S:(i + 1) * S] == vec[pos], (q, a, idx, pos)
        if (q, a, idx) not in want_roots:
            want_roots[(q, a, idx)] = _want_root(batch[q], p, a, idx)
        root = want_roots[(q, a, idx)]
        t = (q * 2 + a) * W + idx
        assert roots[t * nl:(t + 1) * nl] == root, (q, a, idx)
        rec = records[i * rb:(i + 1) * rb]
        keep, ptrs, _ = R._bufs(vec)
        host = ctypes.create_string_buffer(rb)
        if p is None:
            assert lib.rsm_default_tree_prove(ptrs, W, S, pos, host, None) == 0
        else:
            assert lib.rsm_nmt_tree_prove(pp, idx, ptrs, W, S, pos, host, None) == 0
        assert rec == host.raw, (q, a, idx, pos)
        nodes, mask = V.parse_record(rec, nl)
        if p is None:
            assert V.verify_default(root, [vec[pos]] + nodes, pos, W), (q, a, idx, pos)
        else:
            assert V.verify_nmt(root, vec[pos], nodes, mask, pos, idx, k, 29), (q, a, idx, pos)
