"""TEST INFRASTRUCTURE ONLY -- blob share commitments in hashlib, the checker for the host
restatements (merkle.cpp rsm_blob_commitment / rsm_square_commitment) and the device
kernels (kernels_commit.hip).  The definition (include/rsmt2d_hip.h "share commitments") is
stated twice: from the blob's own runs (`commitment`: an NMT over each run of the mountain
range, oracle/nmt.py) and from the row trees' levels (`square_commitment`: the levels of
each touched row's tree, the blob's nodes read off at (level, j)); both end in the RFC 6962
root of tests/data_root.py (`mth`).  Importing this module touches no GPU."""
import math

from data_root import mth
from oracle import nmt


class OrderError(Exception):
    """A push-order error inside a subtree (RSM_COMMIT_ORDER) or a row (RSM_COMMIT_TREE)."""


def pow2ceil(x: int) -> int:
    p = 1
    while p < x:
        p *= 2
    return p


def minsq(n: int) -> int:
    s = math.isqrt(n)
    return pow2ceil(s if s * s == n else s + 1)


def width(n: int, t: int) -> int:
    return min(pow2ceil(-(-n // t)), minsq(n))


def sizes(n: int, w: int):
    out = []
    while n > 0:
        z = w if n >= w else 1 << (n.bit_length() - 1)
        out.append(z)
        n -= z
    return out


def runs(n: int, t: int):
    """(first share, size) of every subtree of a blob of n shares."""
    at, out = 0, []
    for z in sizes(n, width(n, t)):
        out.append((at, z))
        at += z
    return out


def subtree_roots(shares, ns: int, t: int, ig: bool = True):
    """r_0 .. r_{M-1} from the blob's own runs; OrderError on a violation inside a run."""
    out = []
    for at, z in runs(len(shares), t):
        try:
            out.append(nmt.nmt_root([bytes(s[:ns]) + bytes(s) for s in shares[at:at + z]], ns, ig))
        except nmt.NmtError as e:
            raise OrderError(str(e))
    return out


def commitment(shares, ns: int, t: int, ig: bool = True) -> bytes:
    return mth(subtree_roots(shares, ns, t, ig))


def row_levels(row_shares, k: int, ns: int, ig: bool = True):
    """Levels 0 .. log2(2k) of a row's tree in the level picture: leaf p under its own
    namespace for p < k, the parity namespace after; level l + 1 joins the pairs of level l
    (2k is a power of two: no node is carried up).  OrderError where the tree fails."""
    try:
        prev = None
        lv = []
        for p, sh in enumerate(row_shares):
            name = bytes(sh[:ns]) if p < k else b"\xff" * ns
            if prev is not None and name < prev:
                raise nmt.NmtError("invalid push order")
            prev = name
            lv.append(nmt.hash_leaf(name + bytes(sh), ns))
        out = [lv]
        while len(lv) > 1:
            lv = [nmt.hash_node(lv[2 * j], lv[2 * j + 1], ns, ig) for j in range(len(lv) // 2)]
            out.append(lv)
        return out
    except nmt.NmtError as e:
        raise OrderError(str(e))


def square_subtree_roots(sq, k: int, ns: int, start: int, length: int, t: int, ig: bool = True, levels=None):
    """The subtree roots of the blob at ODS shares [start, start + length) of the [2k][2k][S]
    square `sq`, as nodes of its row trees.  `levels`: a dict row -> row_levels to share."""
    w = width(length, t)
    assert start % w == 0 and start + length <= k * k and w <= k
    levels = {} if levels is None else levels
    out = []
    for at, z in runs(length, t):
        p = start + at
        row, col, lvl = p // k, p % k, z.bit_length() - 1
        assert col % z == 0 and col + z <= k, "a subtree crosses a row"
        if row not in levels:
            levels[row] = row_levels([sq[row, c].tobytes() for c in range(2 * k)], k, ns, ig)
        out.append(levels[row][lvl][col >> lvl])
    return out


def square_commitment(sq, k: int, ns: int, start: int, length: int, t: int, ig: bool = True, levels=None) -> bytes:
    return mth(square_subtree_roots(sq, k, ns, start, length, t, ig, levels))


def aligned_blobs(k: int, t: int):
    """Every (start, len) of a k x k ODS whose start is a multiple of the blob's width."""
    return [(s, n) for n in range(1, k * k + 1) for s in range(0, k * k - n + 1, width(n, t))]


def all_blobs(k: int):
    return [(s, n) for n in range(1, k * k + 1) for s in range(0, k * k - n + 1)]


def make_square(k: int, S: int, ns: int, seed: int, distinct: int = 5, tail: int = 0):
    """A [2k][2k][S] uint8 square whose ODS namespaces are non-decreasing in row-major order
    (`distinct` different ones, so subtrees span several), the last `tail` ODS shares under
    the parity namespace 0xFF.. (tail padding).  The commitments read quadrant 0 only: the
    other quadrants hold seeded bytes, not an extension."""
    import numpy as np
    g = np.random.default_rng([0xC0, seed, k, S, ns])
    sq = g.integers(0, 256, (2 * k, 2 * k, S), dtype=np.uint8)
    pool = np.sort(g.integers(0, 255, (distinct, ns), dtype=np.uint8).view([("", np.uint8)] * ns), axis=0)
    pool = pool.view(np.uint8).reshape(distinct, ns)
    pick = np.sort(g.integers(0, distinct, k * k))
    names = pool[pick]
    if tail:
        names[k * k - tail:] = 0xFF
    sq[:k, :k, :ns] = names.reshape(k, k, ns)
    return sq


def ods_shares(sq, k: int, start: int, length: int):
    return [sq[p // k, p % k].tobytes() for p in range(start, start + length)]


# values derived from the definition by hand, not from any implementation
WIDTHS = {(1, 64): 1, (64, 64): 1, (65, 64): 2, (129, 64): 4, (16384, 64): 128, (4, 1): 2, (9, 1): 4, (1024, 1 << 20): 1}
SIZES = {(11, 4): [4, 4, 2, 1], (19, 8): [8, 8, 2, 1], (5, 8): [4, 1]}
