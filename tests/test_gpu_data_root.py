"""GPU: the data root on the device -- rsm_data_roots_dev (build), rsm_root_proofs_dev
(gather), rsm_proofs_verify_data_root_dev (the chained verifier) and the device path of
ExtendedDataSquare.DataRoot() -- against tests/data_root.py (RFC 6962's recursive split in
hashlib) and the host restatements."""
import ctypes

import numpy as np
import pytest

import rsmt2d_amd as R
import data_root as DR
import device_calls as D
import proof_status as P
import proof_verify as V

pytestmark = pytest.mark.gpu

GUARD = 4096


class Guarded:
    """front band | operand | back band in one DeviceBuffer, the operand `skew` bytes past
    a 64-byte boundary."""

    def __init__(self, data, skew):
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        g = np.random.default_rng([0x4452, len(data), skew])
        self.front, self.n = GUARD + skew, len(data)
        self.sent = g.integers(0, 256, self.front + self.n + GUARD, dtype=np.uint8)
        self.sent[self.front:self.front + self.n] = data
        self.buf = R.DeviceBuffer(len(self.sent))
        self.buf.upload(self.sent)
        self.ptr = self.buf.ptr + self.front

    def result(self):
        got = self.buf.download()
        assert np.array_equal(got[:self.front], self.sent[:self.front]), "a store landed before the operand"
        assert np.array_equal(got[self.front + self.n:], self.sent[self.front + self.n:]), "a store landed past the operand"
        return got[self.front:self.front + self.n]

    def unchanged(self):
        return np.array_equal(self.result(), self.sent[self.front:self.front + self.n])

    def free(self):
        self.buf.free()


def root_table(width, root_len, count, seed):
    return np.random.default_rng([0x5254, width, root_len, seed]).integers(0, 256, (count, 2 * width, root_len), dtype=np.uint8)


def picked_refs(width, count):
    """Every root of a small square; of a wide one both ends and the middle of each axis
    of each square, and 48 seeded ones."""
    if width <= 130:
        return [(q, a, i) for q in range(count) for a in (0, 1) for i in range(width)]
    s = {(q, a, i) for q in range(count) for a in (0, 1) for i in (0, 1, width // 2 - 1, width // 2, width - 2, width - 1)}
    g = np.random.default_rng(width)
    s |= {(int(g.integers(count)), int(g.integers(2)), int(g.integers(width))) for _ in range(48)}
    return sorted(s)


# 130: 260 leaves, more than one workgroup pass; 1024 x 96: the NMT limit; 2048 x 32: the
# DefaultTree limit; width 34 also at the padding-class edges of the 1 + root_len byte leaf
@pytest.mark.parametrize("width,root_len", [(1, 32), (3, 32), (3, 90), (34, 32), (34, 54), (34, 56), (34, 64), (34, 90),
                                            (130, 32), (130, 90), (1024, 96), (2048, 32)])
def test_build_and_gather(lib, width, root_len):
    count = 3
    ctx = R.device_context(0)
    table = root_table(width, root_len, count, 1)
    trees = [DR.RfcTree([r.tobytes() for r in table[q]]) for q in range(count)]
    refs = picked_refs(width, count)
    n, rb = len(refs), int(lib.rsm_data_root_record_bytes(width))
    assert rb == DR.record_bytes(width)
    nbytes = int(lib.rsm_data_root_nodes_bytes(width, count))
    # every level of the picture, carried-up copies included
    assert nbytes == count * 32 * sum(-(-2 * width // (1 << l)) for l in range(DR.levels(2 * width) + 1))
    g_roots = Guarded(table, 3)  # byte-aligned roots
    g_dr, g_dr2 = Guarded(np.full(count * 32, 0xEE, np.uint8), 1), Guarded(np.full(count * 32, 0xEE, np.uint8), 5)
    g_nodes = Guarded(np.full(nbytes, 0xDD, np.uint8), 0)
    g_rec = Guarded(np.full(n * rb, 0xCC, np.uint8), 2)
    try:
        arr = (R.RootRef * n)(*[R.RootRef(*r) for r in refs])
        R._check(lib.rsm_data_roots_dev(ctx, g_roots.ptr, width, root_len, count, g_dr.ptr, g_nodes.ptr, None))
        R._check(lib.rsm_data_roots_dev(ctx, g_roots.ptr, width, root_len, count, g_dr2.ptr, None, None))  # no store
        R._check(lib.rsm_root_proofs_dev(ctx, g_nodes.ptr, width, count, arr, n, g_rec.ptr, None))
        del arr  # copied before the call returned
        R._check(lib.rsm_sync(ctx))
        want = b"".join(t.root() for t in trees)
        assert g_dr.result().tobytes() == want
        assert g_dr2.result().tobytes() == want
        assert g_roots.unchanged()
        g_nodes.result()  # only the bands are checked: the store is opaque
        rec = g_rec.result().tobytes()
        for i, (q, a, idx) in enumerate(refs):
            assert rec[i * rb:(i + 1) * rb] == DR.record_of(trees[q], width, a, idx), (q, a, idx)
    finally:
        for g in (g_roots, g_dr, g_dr2, g_nodes, g_rec):
            g.free()


def test_build_and_gather_argument_errors(lib):
    ctx = R.device_context(0)
    width, root_len = 6, 32
    table = root_table(width, root_len, 1, 2)
    g_roots = Guarded(table, 0)
    g_dr = Guarded(np.full(32, 0xEE, np.uint8), 0)
    g_nodes = Guarded(np.full(int(lib.rsm_data_root_nodes_bytes(width, 1)), 0xDD, np.uint8), 0)
    g_rec = Guarded(np.full(4 * DR.record_bytes(width), 0xCC, np.uint8), 0)
    try:
        def build(width=width, root_len=root_len, count=1, nodes=g_nodes.ptr):
            return lib.rsm_data_roots_dev(ctx, g_roots.ptr, width, root_len, count, g_dr.ptr, nodes, None)

        def gather(refs, n=None, width=width, count=1):
            arr = (R.RootRef * max(len(refs), 1))(*[R.RootRef(*r) for r in refs])
            return lib.rsm_root_proofs_dev(ctx, g_nodes.ptr, width, count, arr, len(refs) if n is None else n, g_rec.ptr, None)

        assert build(count=0) == 0
        assert build(width=2049) == R.RSM_EUNSUPPORTED
        assert build(width=0) == R.RSM_EINVAL
        assert build(root_len=31) == R.RSM_EINVAL and build(root_len=97) == R.RSM_EINVAL
        assert build(nodes=g_nodes.ptr + 8) == R.RSM_EINVAL  # d_nodes must be 16-byte aligned
        assert gather([(0, 0, 0)], n=0) == 0
        assert gather([(0, 0, 0)], width=2049) == R.RSM_EUNSUPPORTED
        for bad in [(1, 0, 0), (0, 2, 0), (0, 0, width)]:
            assert gather([(0, 1, width - 1), bad]) == R.RSM_EINVAL
            assert b"ref 1" in lib.rsm_last_error()
        R._check(lib.rsm_sync(ctx))
        assert g_dr.unchanged() and g_nodes.unchanged() and g_rec.unchanged() and g_roots.unchanged()  # nothing stored
        assert build() == 0 and gather([(0, 1, width - 1)]) == 0
        R._check(lib.rsm_sync(ctx))
        assert g_dr.result().tobytes() == DR.mth([r.tobytes() for r in table[0]])
    finally:
        for g in (g_roots, g_dr, g_nodes, g_rec):
            g.free()


# ---- the chain: extend -> node store and roots -> data roots and their store -> share
# proofs and root proofs -> the chained verifier ------------------------------------------
TREES = [("default", 0), ("nmt", 29), ("nmt", 12)]
S = 64


def extended_batch(lib, k, ns, seed, count=2):
    """`count` squares extended on the device from namespace-sorted original squares."""
    ctx = R.device_context(0)
    W = 2 * k
    batch = np.zeros((count, W, W, S), np.uint8)
    for q in range(count):
        batch[q, :k, :k] = V.sorted_q0_square(k, S, max(ns, 8), seed + q)[:k, :k]
    buf = R.DeviceBuffer(batch.nbytes)
    try:
        buf.upload(batch.reshape(-1))
        R._check(lib.rsm_extend_squares_dev(ctx, buf.ptr, k, S, count, None))
        R._check(lib.rsm_sync(ctx))
        return buf.download().reshape(count, W, W, S).copy()
    finally:
        buf.free()


def device_chain(lib, items, W, p, roots=None, count=None):
    """Statuses of rsm_proofs_verify_data_root_dev over `items`.  With `roots`
    ([count][2][W][root_len] bytes) the data roots and the root records are the device's own
    (rsm_data_roots_dev, rsm_root_proofs_dev; also returned); otherwise each item brings its
    root record and its data root, the latter in a slot of its own: the verifier uses
    `square` for that lookup only."""
    ctx = R.device_context(0)
    n = len(items)
    pp = ctypes.byref(p) if p is not None else None
    rb = DR.record_bytes(W)
    g_sh = Guarded(np.frombuffer(b"".join(it.share for it in items), np.uint8), 0)
    g_rec = Guarded(np.frombuffer(b"".join(it.record for it in items), np.uint8), 2)
    g_st = Guarded(np.full(n, 0xDEADBEEF, np.uint32), 4)
    bufs = [g_sh, g_rec, g_st]
    try:
        if roots is not None:
            samples = [it.sample for it in items]
            g_roots = Guarded(np.frombuffer(roots, np.uint8), 1)
            g_dr = Guarded(np.zeros(count * 32, np.uint8), 3)
            g_nodes = Guarded(np.zeros(int(lib.rsm_data_root_nodes_bytes(W, count)), np.uint8), 0)
            g_rrec = Guarded(np.zeros(n * rb, np.uint8), 6)
            bufs += [g_roots, g_dr, g_nodes, g_rrec]
            refs = (R.RootRef * n)(*[R.RootRef(*s[:3]) for s in samples])
            R._check(lib.rsm_data_roots_dev(ctx, g_roots.ptr, W, len(roots) // (count * 2 * W), count, g_dr.ptr,
                                            g_nodes.ptr, None))
            R._check(lib.rsm_root_proofs_dev(ctx, g_nodes.ptr, W, count, refs, n, g_rrec.ptr, None))
        else:
            samples = [(i,) + tuple(it.sample[1:]) for i, it in enumerate(items)]
            count = n
            g_dr = Guarded(np.frombuffer(b"".join(it.data_root for it in items), np.uint8), 3)
            g_rrec = Guarded(np.frombuffer(b"".join(it.root_record for it in items), np.uint8), 6)
            bufs += [g_dr, g_rrec]
        arr = (R.Sample * n)(*[R.Sample(*s) for s in samples])
        R._check(lib.rsm_proofs_verify_data_root_dev(ctx, g_sh.ptr, g_rec.ptr, g_rrec.ptr, g_dr.ptr, W, S, count, pp, arr,
                                                     n, g_st.ptr, None))
        R._check(lib.rsm_sync(ctx))
        assert g_sh.unchanged() and g_rec.unchanged()
        return list(g_st.result().view(np.uint32)), g_dr.result().tobytes(), g_rrec.result().tobytes()
    finally:
        for g in bufs:
            g.free()


def host_chain_status(lib, p, W, it):
    st = ctypes.c_uint32(0xDEAD)
    sm = R.Sample(*it.sample)
    rc = lib.rsm_sample_verify_data_root(ctypes.byref(p) if p is not None else None, W, ctypes.byref(sm), it.share,
                                         len(it.share), it.record, it.root_record, it.data_root, ctypes.byref(st))
    assert rc == 0
    return st.value


@pytest.mark.parametrize("tree,ns", TREES)
@pytest.mark.parametrize("k", [2, 3, 17])
def test_chain(lib, k, tree, ns):
    W, count = 2 * k, 2
    p = R.NmtParams(ns, 1, k) if tree == "nmt" else None
    batch = extended_batch(lib, k, ns, 31 * k + ns, count)
    samples = D.all_samples(W, count) if k <= 3 else D.picked_samples(W, k + ns, count, 256)
    dev = D.Dev(lib, batch, p, samples)  # node store, roots, share proofs and shares, on the device
    assert not dev.status.any()
    ch = DR.Chain(P.Squares(batch, p))
    assert dev.roots == b"".join(b"".join(r) for r in ch.roots)
    # everything from the device's own calls: all of it verifies
    served = [DR.ChainItem("served", dev.share(i), dev.record(i), None, None, s) for i, s in enumerate(samples)]
    got, data_roots, rrecs = device_chain(lib, served, W, p, roots=dev.roots, count=count)
    assert data_roots == b"".join(ch.data_roots)
    rb = DR.record_bytes(W)
    for i, s in enumerate(samples):
        assert rrecs[i * rb:(i + 1) * rb] == ch.root_record(*s[:3]), s
    assert got == [DR.OK] * len(samples)
    # one batch with every hostile variant, status for status with the helper and the host
    picked = sorted(set(P.picked_samples(W, 7 * k + ns, count, 6)))
    picked += [s for s in [(1, 0, 0, 0), (0, 1, k - 1, 1)] if s not in picked]  # quadrant-0 samples: sibling order
    items = ch.items(picked)
    want = ch.expect(items)
    assert {DR.OK, DR.MALFORMED, DR.ROOT} | ({DR.ORDER} if ns else set()) == set(want)
    labels = {it.label for it in items}
    assert {"share bit", "another square's data root", "row as column", "column as row"} <= labels
    if ns:
        assert all(w == DR.ORDER for it, w in zip(items, want) if it.label == "sibling order broken")
        assert "sibling order broken" in labels
    got, _, _ = device_chain(lib, items, W, p)
    for it, g, w in zip(items, got, want):
        assert g == w, (it.sample, it.label, g, w)
        assert host_chain_status(lib, p, W, it) == w, (it.sample, it.label)


@pytest.mark.parametrize("tree,ns", TREES)
def test_eds_data_root_on_the_device(lib, tree, ns):
    k = 3
    W = 2 * k
    ods = V.sorted_q0_square(k, S, max(ns, 8), 500 + ns)[:k, :k]
    ctor = R.NewDefaultTree if tree == "default" else R.newErasuredNamespacedMerkleTreeConstructor(k, ns)
    codec = R.NewLeoRSCodec()
    eds = R.ComputeExtendedDataSquare([ods[r, c].tobytes() for r in range(k) for c in range(k)], codec, ctor)
    roots = eds.Roots()
    dr = eds.DataRoot()  # the device path: a context and a complete square
    assert dr == DR.mth(roots)
    host = R.ImportExtendedDataSquare(eds.Flattened(), codec, ctor)  # no context: the host path
    assert host.DataRoot() == dr
    # a changed parity cell (any bytes are a parity share's: its namespace is 0xFF..)
    new = bytes(b ^ 0x5A for b in eds.GetCell(W - 1, W - 2))
    eds.setCell(W - 1, W - 2, new)
    roots2, dr2 = eds.Roots(), eds.DataRoot()
    assert dr2 != dr and dr2 == DR.mth(roots2)
    for axis, i in [(0, W - 1), (1, W - 2), (0, 0), (1, W - 1)]:
        pr = eds.RootProof(axis, i)
        assert pr.record() == DR.record_of(roots2, W, axis, i)
        assert pr.verify(roots2[axis * W + i], dr2) == DR.OK
        assert pr.verify(roots2[axis * W + i], dr) == DR.ROOT
