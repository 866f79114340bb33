"""GPU: the DefaultTree kernels (kernels_sha.hip tree_root_kernel<4 | 2 | 1>,
tree_nodes_kernel, proof_verify_kernel) by width class (tests/default_tree_classes.py):
odd widths (the height-0 carried subtree, a raw leaf digest carried up, waves of the batch
form that hold row and column trees together and a last wave with fewer trees than the
others), both sides of the widths where the batch form changes its trees per wave (177 |
178, 385 | 386) and the node store its trees per workgroup (256 | 257) and its passes per
level (514), widths with a carried subtree at every height, and the width limit 2048 with
its 133,120 bytes of LDS.

Every compare is byte for byte against hashlib (two statements of the tree, held to each
other), never against another device call alone.  The host restatements meet the same
widths in tests/test_default_tree_classes_cpu.py."""
import ctypes

import numpy as np
import pytest

import default_tree_classes as C
import proof_status as P
import rsmt2d_amd as R
from device_calls import Dev, all_samples, check_samples, committed_roots, device_statuses

pytestmark = pytest.mark.gpu
S = C.S


def device_roots(lib, b, single=False):
    """[count][2W][32]: rsm_roots_squares_dev over the batch, or rsm_roots_dev (`single`, one
    square); the output starts as 0xA5 bytes."""
    count, W, _, S_ = b.shape
    assert count == 1 or not single
    d, out = R.DeviceBuffer(b.nbytes), R.DeviceBuffer(count * 2 * W * 32)
    try:
        d.upload(b.reshape(-1))
        out.upload(np.full(count * 2 * W * 32, 0xA5, np.uint8))
        if single:
            R._check(lib.rsm_roots_dev(d.ctx, d.ptr, W, S_, out.ptr, None))
        else:
            R._check(lib.rsm_roots_squares_dev(d.ctx, d.ptr, W, S_, count, out.ptr, None))
        R._check(lib.rsm_sync(d.ctx))
        return out.download().reshape(count, 2 * W, 32)
    finally:
        d.free()
        out.free()


def assert_roots(got, want, what):
    """got, want: [2W][32]; names the trees that differ."""
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), (what, "trees with another root:", len(bad), bad[:16].tolist())


def assert_sampled(got, want, what):
    """got: [2W][32]; want: {tree: root}."""
    bad = [t for t, r in want.items() if got[t].tobytes() != r]
    assert not bad, (what, "trees with another root:", bad)


# --- rsm_roots_dev: one square, tree_root_kernel<1, true> ------------------------------------
ODD = [3, 5, 7, 9, 33, 127, 129, 255, 257]
EVERY_HEIGHT = [126, 254, 510]   # a carried subtree at every height but the top
PAST_POWER = [258, 514]          # 2^n + 2: one carried pair under a perfect tree


@pytest.mark.parametrize("W", ODD + EVERY_HEIGHT + PAST_POWER)
def test_roots_one_square(lib, W):
    assert C.root_form(W, 1)[0] == 1
    got = device_roots(lib, C.batch(W, 1), single=True)
    assert_roots(got[0], C.batch_roots(W, 1)[0], ("rsm_roots_dev", W))


def test_roots_one_square_of_long_shares(lib):
    """S = 1088: 18 SHA blocks per leaf, an odd width."""
    W, S_ = 33, 1088
    got = device_roots(lib, C.batch(W, 1, S_), single=True)
    assert_roots(got[0], C.batch_roots(W, 1, S_)[0], ("rsm_roots_dev", W, S_))


@pytest.mark.parametrize("W", [2047, 2048])
def test_roots_one_square_at_the_width_limit(lib, W):
    """The widest squares the entry point takes: 132,992 and 133,120 bytes of LDS per
    workgroup; the first and last workgroup's trees, those around the axis boundary and 16
    seeded ones against hashlib, and no root left unwritten."""
    assert C.root_form(W, 1)[:2] == (1, {2047: 132992, 2048: C.LATENCY_LDS_2048}[W])
    b = C.make_batch(W, 1)
    want = C.sampled_roots(b[0], C.sampled_trees(W, 1))
    got = device_roots(lib, b, single=True)
    assert_sampled(got[0], want, ("rsm_roots_dev", W))
    assert not (got[0] == 0xA5).all(axis=1).any()
    assert len({r.tobytes() for r in got[0]}) == 2 * W


def test_unsupported_widths(lib):
    ctx = R.device_context(0)
    small = R.DeviceBuffer(1 << 16)
    try:
        for W in (1, 2049):
            assert lib.rsm_roots_dev(ctx, small.ptr, W, S, small.ptr, None) == R.RSM_EUNSUPPORTED
            assert lib.rsm_roots_squares_dev(ctx, small.ptr, W, S, 2, small.ptr, None) == R.RSM_EUNSUPPORTED
        R._check(lib.rsm_sync(ctx))
    finally:
        small.free()


# --- rsm_roots_squares_dev: the batch form ----------------------------------------------------
@pytest.mark.parametrize("W", [176, 177, 178, 384, 385, 386, 3, 5, 514])
def test_roots_batch_of_three(lib, W):
    """Every root of every square.  177 and 385 are the last widths of their class, and odd:
    one wave holds the last row and the first columns; at four trees per wave the last wave
    has two.  3 and 5: fewer trees than one workgroup holds."""
    tpw, lds, blocks = C.root_form(W, 3)
    assert tpw == C.TREES_PER_WAVE[W]
    if W & 1:
        assert W % tpw != 0  # a wave with rows and columns
        assert tpw == 2 or (2 * W) % tpw == 2  # four trees per wave: the last wave has two
    got = device_roots(lib, C.batch(W, 3))
    want = C.batch_roots(W, 3)
    for q in range(3):
        assert_roots(got[q], want[q], ("rsm_roots_squares_dev", W, "square", q, "trees per wave", tpw))


def test_roots_batch_of_two_wide(lib):
    """W = 1026, one tree per wave with more than one square: sampled trees of each."""
    W = 1026
    assert C.root_form(W, 2)[0] == 1
    b = C.make_batch(W, 2)
    got = device_roots(lib, b)
    for q in range(2):
        assert_sampled(got[q], C.sampled_roots(b[q], C.sampled_trees(W, 1, seed=q)), ("rsm_roots_squares_dev", W, q))
        assert not (got[q] == 0xA5).all(axis=1).any()
    assert not (got[0] == got[1]).all(axis=1).any()


def test_roots_batch_entry_with_one_square(lib):
    """count = 1 through rsm_roots_squares_dev takes the latency form."""
    W = 386
    got = device_roots(lib, C.batch(W, 3)[:1])
    assert_roots(got[0], C.batch_roots(W, 3)[0], ("rsm_roots_squares_dev, count = 1", W))


# --- node store and gather --------------------------------------------------------------------
def check_store(lib, b, samples, want_roots):
    """rsm_proof_nodes_dev + rsm_proofs_dev: d_roots equal to hashlib (want_roots: [2W][32]
    per square, or {tree: root}) and to rsm_roots_squares_dev, records equal to the host
    prover's and accepted by the independent verifier against the oracle root."""
    count, W = b.shape[:2]
    dev = Dev(lib, b, None, samples)
    got = np.frombuffer(dev.roots, np.uint8).reshape(count, 2 * W, 32)
    for q in range(count):
        if isinstance(want_roots[q], dict):
            assert_sampled(got[q], want_roots[q], ("node store", W, q))
        else:
            assert_roots(got[q], want_roots[q], ("node store", W, q))
    assert dev.roots == dev.roots_ref and not dev.status.any()
    check_samples(lib, dev, b, None, samples)
    return dev


@pytest.mark.parametrize("W", [3, 5, 7, 9])
def test_node_store_small_odd_widths(lib, W):
    assert C.nodes_form(W)[0] == 32
    check_store(lib, C.batch(W, 1), all_samples(W), C.batch_roots(W, 1))


@pytest.mark.parametrize("W", [33, 255, 257, 258, 510, 514])
def test_node_store(lib, W):
    """Both sides of the trees-per-workgroup boundary (255: two trees, 257: one), the first
    width with a second 256-lane pass (514: one active lane in it), a carry at every height
    (510); the samples hold position W - 1, the carried leaf of an odd width, on four trees
    of each axis."""
    assert C.nodes_form(W) == C.NODES_FORMS[W]
    samples = C.class_samples(W)
    assert len({(a, i) for (_, a, i, p) in samples if p == W - 1}) >= 8
    check_store(lib, C.batch(W, 1), samples, C.batch_roots(W, 1))


def test_node_store_widest_odd(lib):
    """W = 2047: four passes per level, a carry at every height, the raw leaf carried up
    eleven levels."""
    W = 2047
    assert C.nodes_form(W) == C.NODES_FORMS[W]
    b = C.make_batch(W, 1)
    g = np.random.default_rng(W)
    samples = [(0, 0, 0, W - 1), (0, 1, W - 1, W - 1), (0, 0, W - 1, 0), (0, 1, 0, W - 2), (0, 0, 1023, 1024),
               (0, 1, 1024, 1023), (0, 0, 5, W - 1)]
    samples += [(0, int(g.integers(2)), int(g.integers(W)), int(g.integers(W))) for _ in range(5)]
    trees = set(C.sampled_trees(W, 1)) | {a * W + i for (_, a, i, _p) in samples}
    dev = check_store(lib, b, samples, [C.sampled_roots(b[0], sorted(trees))])
    assert P.proof_shape(W, W - 1)[0] == 10 and int.from_bytes(dev.record(0)[:4], "little") == 10


# --- rsm_proofs_verify_dev at odd widths ------------------------------------------------------
@pytest.mark.parametrize("W", [3, 5, 7, 9])
def test_verify_odd_widths(lib, W):
    """All 2 W^2 samples of three squares, every mutation: status for status."""
    sq = C.proof_squares(W, 3)
    items = sq.items(all_samples(W, 3))
    if len(items) % 256 == 0:
        items.append(items[0])
    want = P.expect(items, W, None)
    got = device_statuses(items, W, S, None, committed_roots(sq))
    bad = [(it.label, it.sample, g, w) for it, g, w in zip(items, got, want) if g != w]
    assert not bad, (len(bad), bad[:8])
    assert want.count(P.OK) >= 3 * 2 * W * W
    P.assert_covers(want, None)


# --- prove -> verify on device buffers at the last two-trees-per-wave width --------------------
def test_round_trip_on_device_at_385(lib):
    """Roots from the batch root kernel (held to hashlib), records and shares from the node
    store and the gather; nothing but the roots' check leaves the device.  One flipped share
    byte is reported as ROOT, and nothing else."""
    W, count = 385, 2
    b = C.batch(W, 3)[:count]
    samples = C.class_samples(W, count, n=600)
    n = len(samples)
    ctx = R.device_context(0)
    rb = int(lib.rsm_proof_record_bytes(W, None))
    bufs = [R.DeviceBuffer(b.nbytes), R.DeviceBuffer(int(lib.rsm_proof_nodes_bytes(W, None, count))),
            R.DeviceBuffer(n * rb), R.DeviceBuffer(n * S), R.DeviceBuffer(count * 2 * W * 32)]
    d, nodes, recs, shs, roots = bufs
    try:
        d.upload(b.reshape(-1))
        arr = (R.Sample * n)(*[R.Sample(*s) for s in samples])
        R._check(lib.rsm_proof_nodes_dev(ctx, d.ptr, W, S, count, None, nodes.ptr, None, None, None))
        R._check(lib.rsm_proofs_dev(ctx, nodes.ptr, d.ptr, W, S, count, None, arr, n, recs.ptr, shs.ptr, None))
        R._check(lib.rsm_roots_squares_dev(ctx, d.ptr, W, S, count, roots.ptr, None))
        R._check(lib.rsm_sync(ctx))
        got = roots.download().reshape(count, 2 * W, 32)
        for q in range(count):
            assert_roots(got[q], C.batch_roots(W, 3)[q], ("round trip roots", q))
        st = R.verify_samples_dev(shs, recs, roots, W, S, samples, count=count)
        assert not st.any(), np.nonzero(st)[0][:8]
        victim = next(i for i, s in enumerate(samples) if s[0] == 1 and s[3] == W - 1)
        byte = shs.download(1, victim * S + S - 1)
        shs.upload(byte ^ 0x10, victim * S + S - 1)
        st = R.verify_samples_dev(shs, recs, roots, W, S, samples, count=count)
        assert st[victim] == P.ROOT and np.count_nonzero(st) == 1
    finally:
        for x in bufs:
            x.free()
