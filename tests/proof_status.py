"""TEST INFRASTRUCTURE ONLY -- what a proof verifier must answer, and the hostile
inputs it must answer it for.  Shared by tests/test_verify_cpu.py and
tests/test_gpu_verify.py.  Pure Python over hashlib and oracle/nmt.py (hash_leaf /
hash_node); nothing here calls the library under test.

Status words (include/rsmt2d_hip.h), the first condition that applies wins:
  0  the fold equals the root
  1  the record's n_nodes or right_mask differs from what (W, pos) dictates
  2  NMT: a fold step has right.min < left.max (oracle.nmt.hash_node raises)
  3  the fold completed but differs from the root
The node count and operand sides come from (W, pos) alone -- level l contributes when
((pos >> l) ^ 1) < ceil(W / 2^l), its sibling is the right operand when pos >> l is
even -- so the fold below never looks at a byte past the derived nodes."""
from collections import namedtuple

import numpy as np

from oracle import nmt
import proof_verify as V

OK, MALFORMED, ORDER, ROOT, OCCUPIED = 0, 1, 2, 3, 4

#: the tree of a test: ns = 0 is the DefaultTree, else the erasured NMT of square size k
Tree = namedtuple("Tree", "ns ignore_max k")
DEFAULT = Tree(0, 1, 0)


def tree_of(p):
    """Tree from None / a Tree / anything with rsm_nmt_params' fields."""
    if p is None:
        return DEFAULT
    if isinstance(p, Tree):
        return p
    return Tree(int(p.namespace_size), int(p.ignore_max_namespace), int(p.square_size))


def node_len(p) -> int:
    t = tree_of(p)
    return 2 * t.ns + 32 if t.ns else 32


def proof_shape(W: int, pos: int):
    """(n_nodes, right_mask) of the proof of leaf pos among W leaves."""
    n_nodes = mask = 0
    for l in range((W - 1).bit_length()):
        j = pos >> l
        if (j ^ 1) < -(-W // (1 << l)):
            if not j & 1:
                mask |= 1 << n_nodes
            n_nodes += 1
    return n_nodes, mask


def expected_status(root: bytes, share: bytes, record: bytes, pos: int, index: int, W: int, nmt_params) -> int:
    t = tree_of(nmt_params)
    nl = node_len(t)
    n_nodes, mask = proof_shape(W, pos)
    if int.from_bytes(record[0:4], "little") != n_nodes or int.from_bytes(record[4:8], "little") != mask:
        return MALFORMED
    nodes = [record[8 + i * nl: 8 + (i + 1) * nl] for i in range(n_nodes)]
    if not t.ns:
        acc = V.leaf_sum(share)
        for i, nd in enumerate(nodes):
            acc = V.node_sum(acc, nd) if (mask >> i) & 1 else V.node_sum(nd, acc)
        return OK if acc == root else ROOT
    acc = V.nmt_leaf(share, pos, index, t.k, t.ns)
    try:
        for i, nd in enumerate(nodes):
            acc = (nmt.hash_node(acc, nd, t.ns, bool(t.ignore_max)) if (mask >> i) & 1
                   else nmt.hash_node(nd, acc, t.ns, bool(t.ignore_max)))
    except nmt.NmtError:
        return ORDER
    return OK if acc == root else ROOT


# ---- valid proofs, built by levels (independent of the library's prover) -------------
def tree_levels(shares, index: int, p):
    """Every level of the tree over one vector's shares: level l node j covers leaves
    [j 2^l, min((j + 1) 2^l, W)), an unpaired last node is carried up unchanged."""
    t = tree_of(p)
    if t.ns:
        lv = [[V.nmt_leaf(s, i, index, t.k, t.ns) for i, s in enumerate(shares)]]
        join = lambda a, b: nmt.hash_node(a, b, t.ns, bool(t.ignore_max))
    else:
        lv = [[V.leaf_sum(s) for s in shares]]
        join = V.node_sum
    while len(lv[-1]) > 1:
        cur = lv[-1]
        nxt = [join(cur[2 * j], cur[2 * j + 1]) for j in range(len(cur) // 2)]
        if len(cur) & 1:
            nxt.append(cur[-1])
        lv.append(nxt)
    return lv


def record_of(levels, pos: int, p) -> bytes:
    W, nl = len(levels[0]), node_len(p)
    nodes, mask = [], 0
    for l in range((W - 1).bit_length()):
        j = pos >> l
        if (j ^ 1) < len(levels[l]):
            if not j & 1:
                mask |= 1 << len(nodes)
            nodes.append(levels[l][j ^ 1])
    body = len(nodes).to_bytes(4, "little") + mask.to_bytes(4, "little") + b"".join(nodes)
    return body + bytes(V.record_bytes(W, nl) - len(body))


# ---- mutations ------------------------------------------------------------------------
#: one thing handed to a verifier: sample = (square, axis, index, pos)
Item = namedtuple("Item", "label share record root sample")


def _flip(b: bytes, byte: int, bit: int = 0) -> bytes:
    a = bytearray(b)
    a[byte] ^= 1 << bit
    return bytes(a)


def _header(rec: bytes, n_nodes=None, mask=None) -> bytes:
    a = bytearray(rec)
    if n_nodes is not None:
        a[0:4] = (n_nodes & 0xFFFFFFFF).to_bytes(4, "little")
    if mask is not None:
        a[4:8] = (mask & 0xFFFFFFFF).to_bytes(4, "little")
    return bytes(a)


def mutations(share: bytes, record: bytes, root: bytes, sample, W: int, p, other_axis_root=None,
              other_square_root=None):
    """From one valid (share, record, root, sample): the hostile variants of the
    issue's list, each an Item.  The caller computes what each must answer with
    expected_status."""
    t = tree_of(p)
    nl = node_len(t)
    q, axis, index, pos = sample
    n_nodes, mask = proof_shape(W, pos)
    L = (W - 1).bit_length()
    yield Item("valid", share, record, root, sample)
    yield Item("share bit, first byte", _flip(share, 0, 3), record, root, sample)
    yield Item("share bit, last byte", _flip(share, len(share) - 1, 6), record, root, sample)
    for i in range(n_nodes):
        for at in sorted({0, t.ns, 2 * t.ns, nl - 1}):  # min, max, digest: first bytes; last byte
            yield Item("node %d byte %d" % (i, at), share, _flip(record, 8 + i * nl + at, (i + at) & 7), root, sample)
    yield Item("root bit, first byte", share, record, _flip(root, 0, 1), sample)
    yield Item("root bit, last byte", share, record, _flip(root, nl - 1, 7), sample)
    if t.ns:
        yield Item("root bit, max namespace", share, record, _flip(root, 2 * t.ns - 1, 2), sample)
    yield Item("n_nodes + 1", share, _header(record, n_nodes=n_nodes + 1), root, sample)
    yield Item("n_nodes - 1", share, _header(record, n_nodes=n_nodes - 1), root, sample)
    yield Item("n_nodes = 0xFFFFFFFF", share, _header(record, n_nodes=0xFFFFFFFF), root, sample)
    yield Item("right_mask bit", share, _header(record, mask=mask ^ (1 << (pos % max(n_nodes, 1)))), root, sample)
    yield Item("right_mask bit 31", share, _header(record, mask=mask ^ (1 << 31)), root, sample)
    for other in sorted({(pos + 1) % W, (pos + 2) % W, pos ^ 1 if (pos ^ 1) < W else pos} - {pos}):
        yield Item("as pos %d" % other, share, record, root, (q, axis, index, other))
    if other_axis_root is not None:
        yield Item("other axis' root", share, record, other_axis_root, sample)
    if other_square_root is not None:
        yield Item("another square's root", share, record, other_square_root, sample)
    if n_nodes < L:  # the zero tail is never read
        tail = 8 + n_nodes * nl
        yield Item("non-zero tail", share, record[:tail] + b"\xa5" * (len(record) - tail), root, sample)
    if t.ns and index < t.k and pos < t.k:
        for i in range(n_nodes):
            if (mask >> i) & 1:  # a right-hand sibling below the namespaces to its left
                a = bytearray(record)
                a[8 + i * nl: 8 + i * nl + t.ns] = bytes(t.ns)
                yield Item("node %d min namespace zeroed" % i, share, bytes(a), root, sample)
                break


def expect(items, W: int, p):
    return [expected_status(it.root, it.share, it.record, it.sample[3], it.sample[2], W, p) for it in items]


def assert_covers(statuses, p):
    """Every parametrisation must exercise every status the tree can give."""
    want = {OK, MALFORMED, ROOT} | ({ORDER} if tree_of(p).ns else set())
    assert want <= set(statuses), (want, set(statuses))


# ---- squares ---------------------------------------------------------------------------
def picked_samples(W: int, seed: int, count: int = 1, n: int = 256):
    """The four corners, both sides of the k boundary on both axes, n seeded samples
    over `count` squares: (square, axis, index, pos)."""
    k = W // 2
    s = {(0, a, i, p) for a in (0, 1) for i in (0, W - 1) for p in (0, W - 1)}
    s |= {(0, a, i, p) for a in (0, 1) for i in (k - 1, k) for p in (k - 1, k) if 0 <= i and 0 <= p}
    rng = np.random.default_rng(seed)
    s |= {(int(rng.integers(count)), int(rng.integers(2)), int(rng.integers(W)), int(rng.integers(W))) for _ in range(n)}
    return sorted(s)


class Squares:
    """`count` [W][W][S] squares with the levels of the trees the samples touch (built
    on demand, once)."""

    def __init__(self, batch: np.ndarray, p):
        self.batch, self.p = batch, p
        self.count, self.W, _, self.S = batch.shape
        self._levels = {}

    def levels(self, q, axis, index):
        key = (q, axis, index)
        if key not in self._levels:
            self._levels[key] = tree_levels(V.vector(self.batch[q], axis, index), index, self.p)
        return self._levels[key]

    def root(self, q, axis, index) -> bytes:
        return self.levels(q, axis, index)[-1][0]

    def share(self, sample) -> bytes:
        q, axis, index, pos = sample
        return (self.batch[q, index, pos] if axis == 0 else self.batch[q, pos, index]).tobytes()

    def record(self, sample) -> bytes:
        q, axis, index, pos = sample
        return record_of(self.levels(q, axis, index), pos, self.p)

    def items(self, samples):
        """Every mutation of every sample."""
        out = []
        for s in samples:
            q, axis, index, pos = s
            other_sq = self.root((q + 1) % self.count, axis, index) if self.count > 1 else None
            out.extend(mutations(self.share(s), self.record(s), self.root(q, axis, index), s, self.W, self.p,
                                 self.root(q, 1 - axis, index), other_sq))
        return out
