"""TEST INFRASTRUCTURE ONLY -- the share sizes and the two "long compare" shapes that
tests/test_gpu_share_sizes.py, tests/test_share_sizes_cpu.py and tests/test_gpu_streams.py
share.  Importing this module touches no GPU, and nothing here computes an expectation with
the library under test.

Almost every device test of the proof, Repair and fraud-proof calls runs at 64-byte shares.
The ABI takes any multiple of 64 and Celestia's share is 512 bytes; at 64 bytes the loops
that depend on the share size run their shortest path only.  Each class below is the
smallest size that reaches what its docstring names.
"""
import functools

import numpy as np

import commitments as C
import data_root as DR
import ns_proofs as H
import oracle
import proof_status as P
import proof_verify as V
import range_proofs as M
import rsmt2d_amd as R
from range_calls import data_root_tree, square_roots

K = 8  # the square every family runs on unless its test says otherwise
NS = 29  # Celestia's namespace size


class Class128:
    """S = 128, eight 16-byte words: the smallest share that is not 64 bytes.  A constant 64
    (or a word count of 4) standing where the share size belongs gives a wrong answer here:
    scatter_apply_kernel's `S / 16` copy bound, vectors_gather_kernel's `per = S / 16`, the
    `W * W * S` strides of the Repair and fraud-proof work areas.  The leaf message of an
    NMT with 29-byte namespaces is 1 + 29 + 128 = 158 bytes: three SHA-256 blocks (two at
    S = 64)."""
    S = 128


class Class512:
    """S = 512: Celestia's share.  With ns = 29 the NMT leaf message is 1 + 29 + 512 = 542
    bytes; with the 0x80 byte and the 8-byte length that is 551 bytes, nine 64-byte blocks --
    the block loop production runs in share_leaf_hash, list_leaf_hash_kernel,
    commit_leaf_kernel<NS29> and the range verifier's per-lane share hashing.  A DefaultTree
    leaf (1 + 512 bytes) is nine blocks as well."""
    S = 512


class Class1088:
    """S = 1088, 68 sixteen-byte words: the smallest multiple of 64 past 1024 bytes, so the
    64-lane copy loops (`for (w = lane; w < S / 16; w += 64)`) make a second trip, with a
    four-lane tail.  The DefaultTree leaf message is 1 + 1088 = 1089 bytes: seventeen whole
    blocks -- an odd number, where 64, 128 and 512 give 1, 2 and 8 -- and one byte in the
    padded eighteenth; the NMT leaf (1 + 29 + 1088 = 1118 bytes) is eighteen blocks too.
    tests/test_gpu_default_tree_classes.py uses this size for the same reasons."""
    S = 1088


CLASSES = (Class128, Class512, Class1088)
SIZES = tuple(c.S for c in CLASSES)


def sha_blocks(message_bytes):
    """64-byte blocks SHA-256 runs over a message: its bytes, 0x80 and the 8-byte length."""
    return (message_bytes + 9 + 63) // 64


# 1 + ns + S with ns = 29, and the DefaultTree's 1 + S
assert [sha_blocks(1 + NS + s) for s in (64,) + SIZES] == [2, 3, 9, 18]
assert [sha_blocks(1 + s) for s in (64,) + SIZES] == [2, 3, 9, 18]
assert [s // 16 for s in SIZES] == [8, 32, 68] and 68 == 64 + 4

# ---- the long compares -----------------------------------------------------------------
#: launch_repair_compare_squares: at most 1024 blocks of 256 lanes, one 16-byte word a lane
REPAIR_COMPARE_TRIP = 1024 * 256
#: launch_compare (rsm_dev_equal): at most 4096 blocks of 256 lanes
DEV_EQUAL_TRIP = 4096 * 256


def square_words(k, S):
    return (2 * k) ** 2 * S // 16


def _long_repair_shape():
    """The smallest (k, S), k from the widths repair_cases is run at (8 and 65) and S from the
    classes above, whose square is longer than one trip of repair_compare_squares_kernel and
    no multiple of it, so the last trip is ragged."""
    for k, S in sorted(((k, S) for k in (8, 65) for S in SIZES), key=lambda x: square_words(*x)):
        w = square_words(k, S)
        if w > REPAIR_COMPARE_TRIP and w % REPAIR_COMPARE_TRIP:
            return k, S
    raise AssertionError("no long shape")


#: k = 65, S = 512: 130 * 130 * 32 = 540,800 words = 2.06 trips of 262,144 (8.25 MiB; the
#: largest square on which a test asked for a difference before was 1.08 MB).  S = 128 is
#: 135,200 words, half a trip; k = 8 never gets there (256 cells).
LONG_REPAIR = _long_repair_shape()
assert LONG_REPAIR == (65, 512) and square_words(65, 512) == 540800
assert square_words(65, 128) == 135200 < REPAIR_COMPARE_TRIP and square_words(8, 1088) < REPAIR_COMPARE_TRIP
assert 2 * REPAIR_COMPARE_TRIP < 540800 < 3 * REPAIR_COMPARE_TRIP and round(540800 / REPAIR_COMPARE_TRIP, 2) == 2.06

#: rsm_dev_equal: one trip (16 MiB), one more block of 256 words and one word
DEV_EQUAL_BYTES = (16 << 20) + (4 << 10) + 16
assert DEV_EQUAL_BYTES // 16 == DEV_EQUAL_TRIP + 256 + 1 and DEV_EQUAL_BYTES % 16 == 0
#: the words a test flips: the first, the last of the first trip, the first of the second
#: trip (thread 0 of block 0 again) and the last (thread 0 of block 1: the ragged end)
DEV_EQUAL_WORDS = (0, DEV_EQUAL_TRIP - 1, DEV_EQUAL_TRIP, DEV_EQUAL_BYTES // 16 - 1)


def trip_of(word, trip=REPAIR_COMPARE_TRIP):
    return word // trip


def differing_trips(given, k, S):
    """The trips of repair_compare_squares_kernel in which a complete [2k][2k][S] square
    differs from the re-extension of its own original quadrant (oracle codec)."""
    again = oracle.extend_square(np.ascontiguousarray(given[:k, :k]), nthreads=8)
    words = np.flatnonzero((np.asarray(given) != again).reshape(-1, 16).any(axis=1))
    return sorted({int(w) // REPAIR_COMPARE_TRIP for w in words})


def parity_flips(k, S):
    """(row, column, byte) of single bytes to flip in a complete valid square so that exactly
    one 16-byte word differs from the re-extension: the cell must be a parity cell (a changed
    original cell changes its whole row and column of the re-extension).  The first parity
    cell (first trip), the last parity cell wholly inside the first trip, the first parity
    cell wholly inside the second trip, and the last byte of the square (the ragged trip)."""
    W, per = 2 * k, S // 16

    def parity(cell):
        return cell // W >= k or cell % W >= k

    first = next(c for c in range(W * W) if parity(c))
    last_in_first = next(c for c in range(REPAIR_COMPARE_TRIP // per - 1, -1, -1) if parity(c))
    first_in_second = next(c for c in range(-(-REPAIR_COMPARE_TRIP // per), W * W) if parity(c))
    out = [(first // W, first % W, 0), (last_in_first // W, last_in_first % W, S - 1),
           (first_in_second // W, first_in_second % W, 0), (W - 1, W - 1, S - 1)]
    trips = [trip_of(((r * W + c) * S + b) // 16) for r, c, b in out]
    assert trips == [0, 0, 1, square_words(k, S) // REPAIR_COMPARE_TRIP], trips
    return out


# ---- the cases both test files run (models only; built once per process) ----------------
TREES = ("default", "nmt")


def tree_ns(tree):
    return NS if tree == "nmt" else 0


@functools.lru_cache(maxsize=None)
def proof_squares(S, tree):
    """(batch [2][W][W][S], proof_status.Squares, data_root.Chain) at k = K: two squares, so a
    sample's square index matters."""
    p = R.NmtParams(NS, 1, K) if tree == "nmt" else None
    batch = np.stack([V.sorted_q0_square(K, S, NS, 0x5120 + S + q) for q in range(2)])
    batch.setflags(write=False)
    sq = P.Squares(batch, p)
    return batch, sq, DR.Chain(sq)


@functools.lru_cache(maxsize=None)
def verify_items(S, tree):
    """(items, statuses owed) of rsm_proofs_verify_dev: every proof_status mutation of the
    corner, k-boundary and 12 seeded samples of proof_squares."""
    _, sq, _ = proof_squares(S, tree)
    items = sq.items(P.picked_samples(sq.W, S, sq.count, 12))
    if len(items) % 256 == 0:
        items.append(items[0])
    return items, P.expect(items, sq.W, sq.p)


@functools.lru_cache(maxsize=None)
def chain_items(S, tree):
    """(items, statuses owed) of rsm_proofs_verify_data_root_dev: every data_root chain
    mutation of eight samples, two of them in quadrant 0 (sibling order)."""
    _, sq, ch = proof_squares(S, tree)
    picked = sorted(set(P.picked_samples(sq.W, 7 * S, sq.count, 0)))[::3]
    picked += [s for s in [(1, 0, 0, 0), (0, 1, K - 1, 1)] if s not in picked]
    items = ch.items(picked)
    return items, ch.expect(items)


def sorted_vector(W, ns, S, bounds, seed):
    """W shares of S bytes whose namespaces 00..01, 00..02, .. change at the positions
    `bounds`."""
    rng = np.random.default_rng([seed, W, ns, S])
    out, v = [], 1
    for pos in range(W):
        v += pos in bounds
        out.append(bytes(ns - 1) + bytes([v]) + rng.integers(0, 256, S - ns, dtype=np.uint8).tobytes())
    return out


#: an odd width with a range of 66 leaves ([1, 67): two passes of a wave and a two-lane tail)
ODD_W, ODD_BOUNDS = 67, (1,)


def range_square(k, ns, S):
    sq = M.square(k, ns, S, 0x7A00 + S)
    sq.setflags(write=False)
    return sq


RANGES_K8 = ((0, 16), (1, 3), (7, 9), (15, 16), (3, 12))
#: k = 40 (W = 80, no power of two): ranges of 72 and 80 leaves, more than a wave's 64 lanes,
#: and one that ends the vector
LONG_RANGE_K, RANGES_LONG = 40, ((3, 75), (0, 80), (64, 80))


@functools.lru_cache(maxsize=None)
def range_world(k, ns, S):
    """(square, row trees, column trees, data-root tree) by the model."""
    sq = range_square(k, ns, S)
    rows, cols = square_roots(sq, k, ns)
    return sq, rows, cols, data_root_tree(rows, cols)


@functools.lru_cache(maxsize=None)
def range_cases(ns, S):
    """(cases, root records, chained statuses owed, data root) at k = K: range_proofs' hostile
    set over rows 0, k - 1, k and W - 1 of range_square; every case with its row's root
    record, and the valid ones also with a root record whose first node has a flipped bit."""
    k, W = K, 2 * K
    sq, rows, cols, drt = range_world(k, ns, S)
    dr = drt.root()
    cases, rrecs, musts = [], [], []
    for index in (0, k - 1, k, W - 1):
        leaves = H.vector_shares(sq, 0, index)
        good = DR.record_of(drt, W, 0, index)
        bad = good[:8] + bytes([good[8] ^ 4]) + good[9:]
        for start, end in RANGES_K8:
            for c in M.hostile(rows[index], W, ns, True, index, k, start, end, leaves[start:end], rows[(index + 1) % W].root):
                for rrec in (good, bad) if c.name == "valid" else (good,):
                    cases.append(c)
                    rrecs.append(rrec)
                    if c.name in ("asked of the next vector", "root bit"):
                        musts.append(None)  # they change the root table's entry, which the chained form has not
                    else:
                        musts.append(M.chained_status(W, ns, True, 0, c.index, k, c.start, c.end, c.shares, c.record, rrec, dr))
    return cases, rrecs, musts, dr


@functools.lru_cache(maxsize=None)
def commitment_square(S):
    sq = C.make_square(K, S, NS, 0xC0 + S, tail=3)
    sq.setflags(write=False)
    return sq


COMMIT_THRESHOLDS = (1, 2, 64)


@functools.lru_cache(maxsize=None)
def commitment_wants(S, t):
    """(blobs [(start, len)], subtree roots per blob, commitments) of every aligned blob of
    commitment_square by the model."""
    sq = commitment_square(S)
    blobs = C.aligned_blobs(K, t)
    levels = {}
    roots = [C.square_subtree_roots(sq, K, NS, s, n, t, True, levels) for s, n in blobs]
    return blobs, roots, [C.mth(r) for r in roots]
