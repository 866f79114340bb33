"""TEST INFRASTRUCTURE ONLY -- squares whose quadrant-0 namespaces have structure (the
shared helpers of tests/test_nmt_layouts_cpu.py and tests/test_gpu_nmt_layouts.py).
Uniform random namespaces never repeat, are always told apart by byte 0 and never
equal the parity namespace 0xFF..; a Celestia square does all three.  Nothing here
calls the library under test: the expectations come from oracle/nmt.py.

A layout is a row-major, non-decreasing sequence of k*k namespaces, so every row and
every column of quadrant 0 is sorted.  The tree kernels take any [2k][2k][S] buffer
(they do not check that it is an extension), so the payload and the three parity
quadrants are seeded random bytes.

  single    one namespace everywhere: every node has min == max
  runs      Celestia-shaped: reserved namespaces 00..00 01 / 02 / 04, then version-0
            user namespaces (leading zeros, a random tail of up to 10 bytes) in runs of
            irregular length that cross row ends, then a final run of 0xFF..
  ladder:p  every byte constant but byte p, which does not decrease (strictly
            increasing while k*k <= 256): only byte p ever decides a compare
  carry     pairs ..vv FF FF.. -> ..vv+1 00 00..: an earlier byte rises while every
            later byte falls, at every byte position in turn
  max_tail  a ladder on the last byte whose last m entries are 0xFF.. (k >= 3: one row
            ends in such cells, the last row is nothing else, row 0 has none)
  near_max  a ladder, then FF..FF 00 cells whose payload goes on with 0xFF (NOT the
            parity namespace), then 0xFF.. cells with random payload (the parity
            namespace)
"""
import zlib

import numpy as np

from oracle import nmt

LAYOUTS = ("single", "runs", "carry", "max_tail", "near_max")  # and "ladder:p", p in 0..ns-1


def all_layouts(ns):
    return list(LAYOUTS) + ["ladder:%d" % p for p in range(ns)]


def max_tail_len(k):
    """Trailing 0xFF.. cells of max_tail: the last row and the end of the row before."""
    return 1 if k == 1 else k + max(k // 2, 1)


def _ladder(n, ns, p, rng):
    seq = np.empty((n, ns), np.uint8)
    seq[:] = rng.integers(0, 256, ns, dtype=np.uint8)
    if ns > 1 and p != 0:
        seq[:, 0] = min(int(seq[0, 0]), 0xFE)  # below the near-max and parity namespaces
    if n <= 256:
        seq[:, p] = int(rng.integers(0, 256 - n + 1)) + np.arange(n)
    else:
        seq[:, p] = np.arange(n) * 256 // n
    return seq


def _int_ns(x, ns):
    return np.frombuffer(int(x).to_bytes(ns, "big"), np.uint8)


def _carry(n, ns):
    pos = list(range(ns - 2, -1, -1)) or [0]  # the byte that rises; ns == 1 has only byte 0
    seq = np.empty((n, ns), np.uint8)
    x = 0
    for i in range(0, n, 2):
        p = pos[(i // 2) % len(pos)]
        x |= (1 << (8 * (ns - 1 - p))) - 1  # every later byte 0xFF
        if ns == 1 and i:
            x += 1                          # no later byte: keep neighbouring pairs apart
        seq[i] = _int_ns(x, ns)
        x += 1                              # byte p + 1, every later byte 0x00
        if i + 1 < n:
            seq[i + 1] = _int_ns(x, ns)
    return seq


def _runs(n, k, ns, rng):
    n_ff = 0 if n < 4 else (k + 2 if k >= 3 else 1)
    n_res = min(4, (n - n_ff) // 2)
    n_user = n - n_ff - n_res
    seq = np.zeros((n, ns), np.uint8)
    seq[:n_res, ns - 1] = [1, 2, 2, 4][:n_res]
    lens = []
    while sum(lens) < n_user:
        lens.append(int(rng.integers(1, min(k, 36) + 4)))  # up to a row and more; capped for wide squares
    tail = min(10, ns - 1) if ns > 1 else 1  # byte 0 = 0 wherever there is more than one byte
    tails = rng.integers(0, 256, (len(lens), tail), dtype=np.uint8)
    tails[:, 0] = 5 + tails[:, 0] % 250  # above the reserved ones, below 0xFF..
    tails = tails[np.lexsort(tails[:, ::-1].T)]
    user = np.zeros((sum(lens), ns), np.uint8)
    user[:, ns - tail:] = np.repeat(tails, lens, axis=0)
    seq[n_res:n_res + n_user] = user[:n_user]
    seq[n_res + n_user:] = 0xFF
    return seq


def namespaces(k, ns, layout, rng):
    """The layout's k*k namespaces, uint8[k*k][ns], non-decreasing."""
    n = k * k
    if layout == "single":
        seq = np.empty((n, ns), np.uint8)
        seq[:] = rng.integers(0, 256, ns, dtype=np.uint8)
        seq[:, 0] &= 0x7F
    elif layout == "runs":
        seq = _runs(n, k, ns, rng)
    elif layout.startswith("ladder:"):
        seq = _ladder(n, ns, int(layout[7:]), rng)
    elif layout == "carry":
        seq = _carry(n, ns)
    elif layout == "max_tail":
        m = max_tail_len(k)
        seq = _ladder(n, ns, ns - 1, rng)
        if ns == 1:
            seq[:, 0] = np.minimum(seq[:, 0], 0xFE)
        seq[n - m:] = 0xFF
    elif layout == "near_max":
        third = max(n // 3, 1)
        seq = _ladder(n, ns, ns - 1, rng)
        seq[third:2 * third] = near_max_ns(ns)
        seq[2 * third:] = 0xFF
        seq = seq[np.lexsort(seq[:, ::-1].T)]  # ns == 1: the near-max namespace is 00
    else:
        raise ValueError("unknown layout %r" % (layout,))
    as_bytes = [bytes(x) for x in seq]
    assert as_bytes == sorted(as_bytes), "layout %s is not sorted" % layout
    return seq


def near_max_ns(ns):
    return np.frombuffer(b"\xff" * (ns - 1) + b"\x00", np.uint8)


def square(k, ns, S, layout, seed):
    """uint8[2k][2k][S]: seeded random bytes, quadrant 0's first ns bytes from `layout`."""
    rng = np.random.default_rng([seed, k, ns, S, zlib.crc32(layout.encode())])
    sq = rng.integers(0, 256, (2 * k, 2 * k, S), dtype=np.uint8)
    seq = namespaces(k, ns, layout, rng)
    sq[:k, :k, :ns] = seq.reshape(k, k, ns)
    if layout == "near_max":  # FF..FF 00 | FF FF FF FF ..: the bytes a too-wide compare would see
        near = (sq[:k, :k, :ns] == near_max_ns(ns)).all(axis=2)
        q0 = sq[:k, :k]
        q0[near, ns:ns + 4] = 0xFF
    return sq


def invert(sq, a, b, ns):
    """A copy with the namespace prefixes of two quadrant-0 cells (r, c) swapped, or,
    given two row numbers, those of two whole quadrant-0 rows."""
    out = sq.copy()
    k = sq.shape[0] // 2
    if isinstance(a, int):
        assert a < k and b < k
        out[a, :k, :ns], out[b, :k, :ns] = sq[b, :k, :ns], sq[a, :k, :ns]
    else:
        assert max(a) < k and max(b) < k
        assert sq[a][:ns].tobytes() != sq[b][:ns].tobytes(), "swapping equal namespaces inverts nothing"
        out[a][:ns], out[b][:ns] = sq[b][:ns], sq[a][:ns]
    return out


def plant_max(sq, cell, ns):
    """A copy whose quadrant-0 cell (r, c) carries 0xFF.. ahead of smaller namespaces.  With
    IgnoreMaxNamespace the cell's parent takes its max from the left sibling, so no
    sibling-order check further up sees this inversion: only the push-order check between
    the cell and the next leaf does."""
    out = sq.copy()
    assert max(cell) < sq.shape[0] // 2
    out[cell][:ns] = 0xFF
    return out


def plant_max_failing(sq, k, ns, r, c):
    """Trees that fail once (r, c) of a valid layout carries 0xFF..: row r unless nothing
    smaller follows in it, and column c likewise."""
    W = sq.shape[0]
    ff = b"\xff" * ns
    out = set()
    if c + 1 < k and _name(sq, (r, c + 1), ns) < ff:
        out.add(r)
    if r + 1 < k and _name(sq, (r + 1, c), ns) < ff:
        out.add(W + c)
    return out


def tree_leaves(sq, tree):
    W = sq.shape[0]
    return [sq[tree, p].tobytes() for p in range(W)] if tree < W else [sq[p, tree - W].tobytes() for p in range(W)]


def tree_root(sq, tree, k, ns, ignore_max=True):
    """The oracle's root of tree `tree` (rows 0..W-1, then columns), None where it raises."""
    W = sq.shape[0]
    try:
        return nmt.erasured_root(tree_leaves(sq, tree), tree % W, k, ns, ignore_max)
    except nmt.NmtError:
        return None


def expected(sq, k, ns, ignore_max=True):
    """(status uint32[2W], roots): one oracle tree at a time, status 1 and root None where
    erasured_root raises NmtError."""
    W = sq.shape[0]
    roots = [tree_root(sq, t, k, ns, ignore_max) for t in range(2 * W)]
    return np.array([r is None for r in roots], np.uint32), roots


def decreasing_status(sq, k, ns):
    """The status vector by the direct predicate: a tree fails iff two adjacent
    quadrant-0 cells of it decrease (past quadrant 0 every leaf carries 0xFF.., which no
    namespace exceeds).  Agrees with expected() (tests/test_nmt_layouts_cpu.py); the large
    GPU cases use it for the trees they do not run the oracle on."""
    W = sq.shape[0]
    q0 = sq[:k, :k, :ns].astype(np.int16)

    def less(b, a):  # b < a, bytewise from byte 0
        d = b - a
        first = np.argmax(d != 0, axis=-1)
        return np.take_along_axis(d, first[..., None], axis=-1)[..., 0] < 0

    st = np.zeros(2 * W, np.uint32)
    if k > 1:
        st[:k] = less(q0[:, 1:], q0[:, :-1]).any(axis=1)
        st[W:W + k] = less(q0[1:, :], q0[:-1, :]).any(axis=0)
    return st


def expected_sampled(sq, k, ns, ignore_max=True, others=16, seed=0):
    """For large squares: the predicate's status vector, and oracle roots for every
    failing tree (which must raise), the first and last tree of each half of both
    axes, and `others` seeded ones -- {tree: root or None}."""
    W = sq.shape[0]
    st = decreasing_status(sq, k, ns)
    rng = np.random.default_rng(seed)
    pick = set(int(t) for t in np.nonzero(st)[0])
    pick |= {0, k - 1, k, W - 1, W, W + k - 1, W + k, 2 * W - 1}
    pick |= set(int(t) for t in rng.choice(2 * W, size=min(others, 2 * W), replace=False))
    roots = {t: tree_root(sq, t, k, ns, ignore_max) for t in sorted(pick)}
    for t, r in roots.items():
        assert (r is None) == bool(st[t]), "oracle and predicate disagree on tree %d" % t
    return st, roots


def position_swaps(k):
    """Adjacent cells (r, c) <-> (r, c + 1) for c in {0, 1, 2, 3, 4, k - 2}, r in {0, k - 1}:
    the leaf pairs (2j, 2j+1), (2j+1, 2j+2), (4j+3, 4j+4) and the last quadrant-0 pair."""
    cols = sorted({c for c in (0, 1, 2, 3, 4, k - 2) if 0 <= c < k - 1})
    return [((r, c), (r, c + 1)) for r in sorted({0, k - 1}) for c in cols]


def transposed(swap):
    (r, c), (r2, c2) = swap
    return (c, r), (c2, r2)


def _name(sq, cell, ns):
    return sq[cell][:ns].tobytes()


def row_swap_failing(sq, k, ns, r, c):
    """Trees that fail once (r, c) <-> (r, c + 1) of a valid layout are swapped (the two
    must differ): row r alone.  Row-major order keeps both columns sorted: (r+1, c) comes
    after (r, c+1) and (r-1, c+1) before (r, c)."""
    assert _name(sq, (r, c), ns) < _name(sq, (r, c + 1), ns)
    return {r}


def col_swap_failing(sq, k, ns, r, c):
    """Trees that fail once (r, c) <-> (r + 1, c) are swapped: column c; row r when the
    larger namespace now stands before a smaller (r, c+1); row r + 1 when the smaller one
    now stands after a larger (r+1, c-1)."""
    W = sq.shape[0]
    a, b = _name(sq, (r, c), ns), _name(sq, (r + 1, c), ns)
    assert a < b
    out = {W + c}
    if c + 1 < k and _name(sq, (r, c + 1), ns) < b:
        out.add(r)
    if c >= 1 and _name(sq, (r + 1, c - 1), ns) > a:
        out.add(r + 1)
    return out


def first_step(sq, k, ns, fixed, lo, axis):
    """The first position p >= lo along row (axis 0) / column (axis 1) `fixed` of
    quadrant 0 whose namespace is below that of p + 1; None if there is none."""
    for p in range(lo, k - 1):
        a, b = ((fixed, p), (fixed, p + 1)) if axis == 0 else ((p, fixed), (p + 1, fixed))
        if _name(sq, a, ns) < _name(sq, b, ns):
            return p
    return None
