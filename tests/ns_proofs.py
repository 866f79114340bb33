"""TEST INFRASTRUCTURE ONLY -- namespace proofs (nmt's ProveNamespace / VerifyNamespace as
include/rsmt2d_hip.h "namespace proofs" states them) written the other way round: the
library derives a range proof's nodes level by level from (W, start, end); everything
here walks the RFC 6962 split recursively, in order.  hashlib and oracle.nmt's
hash_leaf / hash_node only; nothing here calls the library under test.

  Tree                 a vector's tree with every subtree root memoised
  prove_range          the nodes of the range proof of [start, end), in order
  prove_namespace      kind, start, end, nodes, leaf node
  record_of            the fixed-stride record
  expected_status      the verifier's five-step precedence
  derived_nodes        the level-picture derivation, asserted equal to the recursive walk
                       for every range of every W <= 33 when this module is imported
"""
from oracle import nmt

EMPTY, INCLUSION, ABSENCE, TREE = 0, 1, 2, 3
OK, MALFORMED, ORDER, ROOT, OCCUPIED, NAMESPACE, INCOMPLETE = 0, 1, 2, 3, 4, 5, 6


def levels(W):
    return (W - 1).bit_length()


def record_bytes(W, ns):
    return 16 + (2 * levels(W) + 1) * (2 * ns + 32)


def split(n):
    """The largest power of two below n (n >= 2)."""
    k = 1
    while k * 2 < n:
        k *= 2
    return k


def wrapper_ns(share, pos, index, k, ns):
    """The namespace the erasured wrapper pushes leaf `pos` of vector `index` with."""
    return bytes(share[:ns]) if (pos < k and index < k) else b"\xff" * ns


class Tree:
    """The erasured NMT over the shares of vector `index`; NmtError where it fails."""

    def __init__(self, shares, index, k, ns, ignore_max=True):
        self.ns, self.ignore_max, self.n = ns, ignore_max, len(shares)
        self.names = [wrapper_ns(sh, p, index, k, ns) for p, sh in enumerate(shares)]
        for a, b in zip(self.names, self.names[1:]):
            if b < a:
                raise nmt.NmtError("invalid push order")
        self.leaves = [nmt.hash_leaf(nm + bytes(sh), ns) for nm, sh in zip(self.names, shares)]
        self._memo = {}
        self.root = self.node(0, self.n)

    def node(self, lo, hi):
        if hi - lo == 1:
            return self.leaves[lo]
        if (lo, hi) not in self._memo:
            m = lo + split(hi - lo)
            self._memo[lo, hi] = nmt.hash_node(self.node(lo, m), self.node(m, hi), self.ns, self.ignore_max)
        return self._memo[lo, hi]


def range_shape(n, start, end):
    """The subtrees (lo, hi) a range proof of [start, end) of n leaves lists, in order."""
    out = []

    def walk(lo, hi):
        if hi <= start or lo >= end:
            out.append((lo, hi))
        elif not (start <= lo and hi <= end):
            m = lo + split(hi - lo)
            walk(lo, m)
            walk(m, hi)

    walk(0, n)
    return out


def prove_range(tree, start, end):
    return [tree.node(lo, hi) for lo, hi in range_shape(tree.n, start, end)]


def prove_namespace(tree, nid):
    """(kind, start, end, nodes, leaf node or None) of namespace `nid` in a tree that passed."""
    ns = tree.ns
    if nid < tree.root[:ns] or nid > tree.root[ns:2 * ns]:
        return EMPTY, 0, 0, [], None
    start = sum(1 for nm in tree.names if nm < nid)
    end = sum(1 for nm in tree.names if nm <= nid)
    if start < end:
        return INCLUSION, start, end, prove_range(tree, start, end), None
    return ABSENCE, start, start + 1, prove_range(tree, start, start + 1), tree.leaves[start]


def record_of(W, ns, kind, start, end, nodes, leaf):
    nl = 2 * ns + 32
    body = b"".join(nodes)
    assert len(nodes) <= 2 * levels(W)
    head = b"".join(v.to_bytes(4, "little") for v in (kind, start, end, len(nodes)))
    return head + body + bytes(2 * levels(W) * nl - len(body)) + (leaf if leaf is not None else bytes(nl))


def expected_status(W, ns, ignore_max, index, k, nid, shares, record, root):
    """The status word the verifier owes this (record, shares) for `nid` under `root`."""
    nl = 2 * ns + 32
    kind, start, end, n_nodes = (int.from_bytes(record[4 * i:4 * i + 4], "little") for i in range(4))
    covered = root[:ns] <= nid <= root[ns:2 * ns]
    if kind == EMPTY:
        if start or end or n_nodes or shares:
            return MALFORMED
        return INCOMPLETE if covered else OK
    if kind == INCLUSION:
        if not (start < end <= W) or len(shares) != end - start:
            return MALFORMED
    elif kind == ABSENCE:
        if not (end == start + 1 and end <= W) or shares:
            return MALFORMED
    else:
        return MALFORMED
    shape = range_shape(W, start, end)
    if n_nodes != len(shape):
        return MALFORMED
    nodes = [record[16 + i * nl:16 + (i + 1) * nl] for i in range(len(shape))]
    if kind == INCLUSION:
        names = [wrapper_ns(sh, start + i, index, k, ns) for i, sh in enumerate(shares)]
        if any(nm != nid for nm in names):
            return NAMESPACE
        leaves = [nmt.hash_leaf(nm + bytes(sh), ns) for nm, sh in zip(names, shares)]
    else:
        leaf = record[16 + 2 * levels(W) * nl:16 + (2 * levels(W) + 1) * nl]
        if leaf[:ns] != leaf[ns:2 * ns] or leaf[:ns] <= nid:
            return NAMESPACE
        leaves = [leaf]
    for (lo, hi), nd in zip(shape, nodes):
        if (hi <= start and nd[ns:2 * ns] >= nid) or (lo >= end and nd[:ns] <= nid):
            return INCOMPLETE
    it = iter(nodes)

    def fold(lo, hi):
        if hi <= start or lo >= end:
            return next(it)
        if hi - lo == 1:
            return leaves[lo - start]
        m = lo + split(hi - lo)
        left = fold(lo, m)
        return nmt.hash_node(left, fold(m, hi), ns, ignore_max)

    try:
        got = fold(0, W)
    except nmt.NmtError:
        return ORDER
    return OK if got == root else ROOT


def derived_nodes(W, start, end):
    """The library's derivation: (level, j) of the range proof's nodes in record order."""
    a, last, left, right = start, end - 1, [], []
    for l in range(levels(W)):
        if a & 1:
            left.append((l, a - 1))
        if not (last & 1) and last + 1 < (W + (1 << l) - 1) >> l:
            right.append((l, last + 1))
        a >>= 1
        last >>= 1
    return left[::-1] + right


def _check_derivation(max_w):
    for W in range(1, max_w + 1):
        for start in range(W):
            for end in range(start + 1, W + 1):
                want = range_shape(W, start, end)
                got = [(j << l, min((j + 1) << l, W)) for l, j in derived_nodes(W, start, end)]
                assert got == want, (W, start, end, got, want)
                assert len(want) <= max(levels(W), 2 * levels(W) - 2)  # the record keeps 2L slots


_check_derivation(33)


def _add(nid, d):
    v = int.from_bytes(nid, "big") + d
    return min(max(v, 0), (1 << (8 * len(nid))) - 1).to_bytes(len(nid), "big")


def query_namespaces(names, ns):
    """What a vector is asked: every distinct namespace present, each minus and plus one
    (clamped), all zeros, 0xFF.. and FF..FF 00."""
    out = []
    for nm in sorted(set(names)):
        out += [nm, _add(nm, -1), _add(nm, 1)]
    out += [bytes(ns), b"\xff" * ns, b"\xff" * (ns - 1) + b"\x00"]
    return sorted(set(out))


def vector_shares(sq, axis, index):
    W = sq.shape[0]
    return [sq[index, p].tobytes() if axis == 0 else sq[p, index].tobytes() for p in range(W)]


def vectors(k):
    """Both axes; indices inside quadrant 0 and at or past k (all-parity vectors)."""
    idx = sorted({0, k // 2, k - 1, k, 2 * k - 1})
    return [(axis, i) for axis in (0, 1) for i in idx]
