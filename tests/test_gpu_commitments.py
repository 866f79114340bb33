"""GPU: blob share commitments on the device -- rsm_blob_commitments_dev (from blob
shares) and rsm_commitments_dev (from the NMT node store), against the hashlib model
(tests/commitments.py), at the smallest shapes that reach each kernel form.  The subtree
pass changes form at two sizes: 1 (a copy) | 2 .. 128 (packed into waves) | 256 .. 1024 (a
workgroup each); the fold runs passes of 256 lanes, so root counts sit around 256 and its
multiples.  Every output is written between guard bands (commit_calls)."""
import ctypes

import numpy as np
import pytest

import commit_calls as K
import commitments as C
import rsmt2d_amd as R

pytestmark = pytest.mark.gpu

ZERO = b"\x00" * 32


def params(ns, k=1, ig=True):
    return R.NmtParams(ns, int(ig), k)


# ---- exhaustive small ---------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2, 64])
@pytest.mark.parametrize("ns", [8, 29])
def test_every_aligned_blob_of_two_small_squares(lib, ns, t):
    k, S = 8, 64
    batch = np.stack([C.make_square(k, S, ns, 10 + q, tail=3 * q) for q in range(2)])
    p = params(ns, k)
    blobs = [(q, s, n) for q in range(2) for s, n in C.aligned_blobs(k, t)]
    levels = [{}, {}]
    want_roots = [C.square_subtree_roots(batch[q], k, ns, s, n, t, True, levels[q]) for q, s, n in blobs]
    want = [C.mth(r) for r in want_roots]
    store = K.Store(lib, batch, p)
    try:
        assert not store.tree_status.any()
        rc, com, st, roots = store.commitments(blobs, t)
        assert rc == 0 and st == [0] * len(blobs)
        assert com == want
        assert roots == want_roots
        rc2, com2, st2, _ = store.commitments(blobs, t, want_roots=False)
        assert (rc2, com2, st2) == (0, want, st)
    finally:
        store.free()
    # the same shares copied out of the ODS, through the shares path: byte for byte
    rc, com3, st3 = K.shares_path(lib, params(ns), S, [C.ods_shares(batch[q], k, s, n) for q, s, n in blobs], t, lead=1)
    assert rc == 0 and st3 == [0] * len(blobs)
    assert com3 == com


def test_unaligned_starts_take_the_shares_path_only(lib):
    k, S, ns, t = 8, 64, 29, 1
    sq = C.make_square(k, S, ns, 20)
    aligned = set(C.aligned_blobs(k, t))
    odd = [(s, n) for s, n in C.all_blobs(k) if (s, n) not in aligned][::3]
    assert odd
    shares = [C.ods_shares(sq, k, s, n) for s, n in odd]
    rc, com, st = K.shares_path(lib, params(ns), S, shares, t)
    assert rc == 0 and st == [0] * len(odd)
    assert com == [C.commitment(sh, ns, t) for sh in shares]
    store = K.Store(lib, sq[None], params(ns, k))
    try:
        good = (0, 0, 4)
        for at in (0, 2):
            blobs = [good] * 3
            blobs[at] = (0,) + odd[5]
            rc, _, _, _ = store.commitments(blobs, t)
            assert rc == R.RSM_EINVAL
            assert ("blob %d " % at) in (lib.rsm_last_error() or b"").decode()
    finally:
        store.free()


# ---- root counts around the fold's passes ------------------------------------------------
def test_root_counts_around_the_fold_passes(lib):
    k, S, ns, t = 64, 64, 29, 1 << 20
    lens = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 4095, 4096]
    sq = C.make_square(k, S, ns, 30, distinct=40)
    starts = [(i * 997) % (k * k - n + 1) for i, n in enumerate(lens)]
    assert all(C.width(n, t) == 1 for n in lens)
    levels = {}
    want = [C.square_commitment(sq, k, ns, s, n, t, True, levels) for s, n in zip(starts, lens)]
    shares = [C.ods_shares(sq, k, s, n) for s, n in zip(starts, lens)]
    assert want == [C.commitment(sh, ns, t) for sh in shares]
    store = K.Store(lib, sq[None], params(ns, k))
    try:
        rc, com, st, roots = store.commitments([(0, s, n) for s, n in zip(starts, lens)], t)
        assert rc == 0 and st == [0] * len(lens) and com == want
        assert [len(r) for r in roots] == lens
        # 4097 shares do not fit this ODS (k * k = 4096): the store path owes RSM_EINVAL here; its
        # RSM_EUNSUPPORTED for 4097 roots is pinned at k = 128 in tests/test_commitments_cpu.py
        assert store.commitments([(0, 0, 4096), (0, 0, 4097)], t)[0] == R.RSM_EINVAL
    finally:
        store.free()
    rc, com2, st2 = K.shares_path(lib, params(ns), S, shares, t)
    assert rc == 0 and st2 == [0] * len(lens) and com2 == want
    rc, _, _ = K.shares_path(lib, params(ns), S, [K.make_blob(4097, S, ns, 31)], t)
    assert rc == R.RSM_EUNSUPPORTED


# ---- subtree sizes on both sides of every change of form ------------------------------------
@pytest.mark.parametrize("n,t,sizes", [
    (127, 1, {16, 8, 4, 2, 1}),             # copy | wave forms of 2 .. 16
    (2048, 2, {64}),
    (3072, 3, {64}),
    (16384 + 256 + 128 + 2 + 1, 64, {256, 128, 2, 1}),  # the last wave size and the first workgroup size
    ((1 << 18) + 1024 + 300, 256, {1024, 256, 32, 8, 4}),  # the widest form: 1024 leaves in one workgroup
])
def test_subtree_sizes_through_the_shares_path(lib, n, t, sizes):
    S, ns = 64, 29
    w = C.width(n, t)
    assert set(C.sizes(n, w)) == sizes
    blob = K.make_blob(n, S, ns, n)
    small = K.make_blob(5, S, ns, 1)  # a neighbour of another shape in the same batch
    want = [C.commitment(list(blob), ns, t), C.commitment(list(small), ns, t)]
    rc, com, st = K.shares_path(lib, params(ns), S, [blob, small], t)
    assert rc == 0 and st == [0, 0]
    assert com == want


def test_ignore_max_and_other_namespace_sizes_through_the_shares_path(lib):
    S, t = 64, 2
    for ns, ig in ((1, True), (8, False), (32, True), (29, False)):
        blob = K.make_blob(300, S, ns, ns)
        blob[-9:, :ns] = 0xFF  # tail padding
        rc, com, st = K.shares_path(lib, params(ns, 1, ig), S, [blob], t)
        assert (rc, st) == (0, [0])
        assert com == [C.commitment(list(blob), ns, t, ig)], (ns, ig)


def test_wide_subtrees_through_the_store_path(lib):
    """minsq binds the width, so w = 512 needs a blob of more than 256^2 shares: one blob
    of a k = 512 square, read off levels 9, 8, 1 and 0 of 130 row trees."""
    k, S, ns, t = 512, 64, 29, 1
    n, start = 65536 + 512 + 256 + 3, 512 * 5
    assert C.width(n, t) == 512 and set(C.sizes(n, 512)) == {512, 256, 2, 1}
    sq = C.make_square(k, S, ns, 40, distinct=30)
    want_roots = C.square_subtree_roots(sq, k, ns, start, n, t)
    store = K.Store(lib, sq[None], params(ns, k))
    try:
        rc, com, st, roots = store.commitments([(0, start, n)], t)
        assert (rc, st) == (0, [0])
        assert roots == [want_roots] and com == [C.mth(want_roots)]
    finally:
        store.free()


# ---- Celestia's shape -------------------------------------------------------------------
def test_celestia_shape(lib):
    k, S, ns, t = 128, 512, 29, 64
    lens = [1, 64, 65, 129, 8192, 16384]
    batch = np.stack([C.make_square(k, S, ns, 50 + q, distinct=12, tail=100 * q) for q in range(2)])
    blobs = [(q, 0 if n == k * k else C.width(n, t) * (3 + q), n) for q in range(2) for n in lens]
    assert len(C.sizes(16384, C.width(16384, t))) == 128
    shares = [C.ods_shares(batch[q], k, s, n) for q, s, n in blobs]
    want = [C.commitment(sh, ns, t) for sh in shares]
    store = K.Store(lib, batch, params(ns, k))
    try:
        rc, com, st, _ = store.commitments(blobs, t, want_roots=False)
        assert rc == 0 and st == [0] * len(blobs) and com == want
    finally:
        store.free()
    rc, com2, st2 = K.shares_path(lib, params(ns), S, shares, t)
    assert rc == 0 and st2 == [0] * len(blobs) and com2 == want
    # the object: Commitment reads the cached node store, CreateCommitment hashes the shares
    ods = [batch[0, r, c].tobytes() for r in range(k) for c in range(k)]
    eds = R.ComputeExtendedDataSquare(ods, R.NewLeoRSCodec(), R.newErasuredNamespacedMerkleTreeConstructor(k, ns))
    p = params(ns, k)
    for (q, s, n), w in list(zip(blobs, want))[:len(lens)]:
        assert eds.Commitment(s, n, t) == w, n
        if n in (65, 16384):
            assert R.CreateCommitment(ods[s:s + n], p, t) == w
            assert R.CreateCommitment(ods[s:s + n], p, t, device=None) == w
    roots = eds.SubtreeRoots(blobs[3][1], 129, t)
    assert roots == C.subtree_roots(shares[3], ns, t) and C.mth(roots) == want[3]


def test_square_object_gives_the_same_on_both_paths(lib):
    """A computed square has a context and takes the cached node store; its imported copy has
    none and takes the host restatement."""
    k, S, ns, t = 8, 64, 29, 2
    sq = C.make_square(k, S, ns, 55, tail=5)
    tree = R.newErasuredNamespacedMerkleTreeConstructor(k, ns)
    dev = R.ComputeExtendedDataSquare([sq[r, c].tobytes() for r in range(k) for c in range(k)], R.NewLeoRSCodec(), tree)
    host = R.ImportExtendedDataSquare(dev.Flattened(), R.NewLeoRSCodec(), tree)
    levels = {}
    for start, n in C.aligned_blobs(k, t)[::9]:
        roots = C.square_subtree_roots(sq, k, ns, start, n, t, True, levels)
        assert dev.SubtreeRoots(start, n, t) == roots == host.SubtreeRoots(start, n, t)
        assert dev.Commitment(start, n, t) == C.mth(roots) == host.Commitment(start, n, t)
    for eds in (dev, host):
        with pytest.raises(R.RSMError) as e:
            eds.Commitment(1, 4, t)
        assert e.value.code == R.RSM_EINVAL


# ---- status words -----------------------------------------------------------------------
def test_a_failing_row_fails_the_blobs_that_touch_it(lib):
    k, S, ns, t = 8, 64, 29, 2
    sq = C.make_square(k, S, ns, 60, distinct=20)
    sq[3, 5, :ns] = 0  # row 3 out of order
    blobs = [(0, s, n) for s, n in C.aligned_blobs(k, t)][::7]
    touching = [s // k <= 3 <= (s + n - 1) // k for _, s, n in blobs]
    assert any(touching) and not all(touching)
    levels = {}
    store = K.Store(lib, sq[None], params(ns, k))
    try:
        assert [i for i, x in enumerate(store.tree_status[0][:2 * k]) if x] == [3]  # the row trees' words
        rc, com, st, _ = store.commitments(blobs, t)
        assert rc == 0
        for (_, s, n), hit, c, word in zip(blobs, touching, com, st):
            if hit:
                assert (c, word) == (ZERO, R.RSM_COMMIT_TREE), (s, n)
            else:
                assert (c, word) == (C.square_commitment(sq, k, ns, s, n, t, True, levels), 0), (s, n)
    finally:
        store.free()


def test_a_violation_inside_a_subtree_fails_its_blob_only(lib):
    S, ns, t = 64, 29, 4
    n = 1024 + 64 + 5  # w = 64 (minsq): 17 subtrees of 64, then 4 and 1
    assert C.runs(n, t)[-3:] == [(1024, 64), (1088, 4), (1092, 1)]
    base = K.make_blob(n, S, ns, 70)
    low = np.zeros(ns, np.uint8)
    blobs, expect = [], []
    for at in (1, 64 * 8 + 63, 1088 + 3, None, 64, 1088, 1092):  # first, middle, last subtree | clean | run boundaries
        b = base.copy()
        if at is not None:
            b[at, :ns] = low
        blobs.append(b)
        inside = at in (1, 64 * 8 + 63, 1088 + 3)
        expect.append((ZERO, R.RSM_COMMIT_ORDER) if inside else (C.commitment(list(b), ns, t), 0))
        if inside:
            with pytest.raises(C.OrderError):
                C.commitment(list(b), ns, t)
    rc, com, st = K.shares_path(lib, params(ns), S, blobs, t)
    assert rc == 0
    assert list(zip(com, st)) == expect
    # a wide subtree (the workgroup form) out of order at its last pair
    n2, t2 = 16384 + 256, 64
    assert C.width(n2, t2) == 256
    wide = K.make_blob(n2, S, ns, 71)
    wide[256 * 7 + 255, :ns] = low
    rc, com, st = K.shares_path(lib, params(ns), S, [wide, blobs[3]], t2)
    assert rc == 0 and (com[0], st[0]) == (ZERO, R.RSM_COMMIT_ORDER)
    assert (com[1], st[1]) == (C.commitment(list(blobs[3]), ns, t2), 0)


# ---- composition ------------------------------------------------------------------------
def test_subtree_roots_are_the_nodes_the_range_proofs_stand_on(lib):
    k, S, ns, t = 16, 64, 29, 10
    sq = C.make_square(k, S, ns, 80, distinct=9)
    p = params(ns, k)
    start, n = 8 * 3, 8 * 9 + 7  # w = 8: nine subtrees of 8, then 4, 2, 1, over five rows
    assert C.width(n, t) == 8
    store = K.Store(lib, sq[None], p)
    buf = R.DeviceBuffer(sq.nbytes)
    try:
        rc, com, st, roots = store.commitments([(0, start, n)], t)
        assert (rc, st) == (0, [0])
        assert C.mth(roots[0]) == com[0] == C.commitment(C.ods_shares(sq, k, start, n), ns, t)
        buf.upload(sq.reshape(-1))
        queries = [(0, R.Row, (start + at) // k, (start + at) % k, (start + at) % k + z) for at, z in C.runs(n, t)]
        proofs = R.prove_ranges_dev(buf, 2 * k, S, queries, nmt=p)
        for pr, q, root in zip(proofs, queries, roots[0]):
            assert pr.verify(store.roots[0, 0, q[2]].tobytes()) == R.RSM_PROOF_OK
            assert C.nmt.nmt_root([sh[:ns] + sh for sh in pr.shares], ns, True) == root
    finally:
        buf.free()
        store.free()


# ---- entry-point behaviour ----------------------------------------------------------------
def test_nothing_to_do_launches_nothing(lib):
    ctx, p = R.device_context(0), params(29, 8)
    g = K.Guarded(64, 0, 90)
    try:
        assert lib.rsm_blob_commitments_dev(ctx, g.ptr, 64, ctypes.byref(p), 64, (ctypes.c_uint32 * 1)(0), 0, g.ptr, g.ptr, g.ptr,
                                            None) == 0
        arr = (R.BlobRef * 1)(R.BlobRef(0, 0, 1))
        assert lib.rsm_commitments_dev(ctx, g.ptr, g.ptr, 16, 1, ctypes.byref(p), 64, arr, 0, g.ptr, g.ptr, g.ptr, g.ptr,
                                       None) == 0
        assert lib.rsm_commitments_dev(ctx, g.ptr, g.ptr, 16, 0, ctypes.byref(p), 64, arr, 1, g.ptr, g.ptr, g.ptr, g.ptr,
                                       None) == 0
        R._check(lib.rsm_sync(ctx))
        assert np.array_equal(g.result(), g.untouched(0, 64))
    finally:
        g.free()


def test_work_bytes_is_zero_exactly_at_the_unsupported_shapes(lib):
    p = ctypes.byref(params(29))
    f = lib.rsm_commit_work_bytes
    assert f(1, 1, p) > 0 and f(1 << 24, 1 << 24, p) > 0
    assert f((1 << 24) + 1, 1, p) == 0 and f(4, 5, p) == 0 and f(4, 4, None) == 0
    assert f(4, 4, ctypes.byref(params(33))) == 0
