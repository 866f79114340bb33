"""TEST INFRASTRUCTURE ONLY -- range proofs (nmt's ProveRange / VerifyInclusion and, chained
to the data root, the rows of Celestia's ShareProof, as include/rsmt2d_hip.h "range proofs"
states them) written the other way round: the library derives a range proof's nodes level
by level and folds in the level picture; everything here walks the RFC 6962 split
recursively.  hashlib, oracle.nmt's hash_leaf / hash_node and the helpers of ns_proofs.py
and data_root.py only; nothing here calls the library under test.

ns == 0 stands for the DefaultTree (32-byte nodes) throughout.

  square               a [2k][2k][S] square whose quadrant-0 namespaces increase strictly
  tree_of              a vector's tree (ns_proofs.Tree, or DefaultTree here)
  prove                the record of [start, end)
  expected_status      what a verifier owes (query, record, shares, root)
  chained_status       the same under a data root, with a root record
  hostile              the hostile variants of one valid proof, each a Case
"""
from collections import namedtuple

import numpy as np

import data_root as D
import ns_proofs as H
from oracle import nmt

OK, MALFORMED, ORDER, ROOT = 0, 1, 2, 3
INCLUSION = 1


def node_len(ns):
    return 2 * ns + 32 if ns else 32


def record_bytes(W, ns):
    return 16 + (2 * H.levels(W) + 1) * node_len(ns)


def square(k, ns, S, seed):
    """Seeded random bytes; quadrant-0 cell (r, c) starts with the big-endian namespace
    r * k + c + 1 (ns >= 1), so every quadrant-0 row and column increases strictly."""
    g = np.random.default_rng([0x5250, k, ns, S, seed])
    sq = g.integers(0, 256, (2 * k, 2 * k, S), dtype=np.uint8)
    for r in range(k):
        for c in range(k):
            if ns:
                sq[r, c, :ns] = np.frombuffer(((r * k + c + 1) % (1 << (8 * ns))).to_bytes(ns, "big"), np.uint8)
    return sq


def vector(W, ns, S, k, seed):
    """W shares of one vector (any W >= 1, odd ones included): namespaces 1, 2, .. below k."""
    g = np.random.default_rng([0x5251, W, ns, S, seed])
    out = []
    for p in range(W):
        body = g.integers(0, 256, S, dtype=np.uint8).tobytes()
        out.append(((p + 1) % (1 << (8 * ns))).to_bytes(ns, "big") + body[ns:] if ns and p < k else body)
    return out


class DefaultTree:
    """RFC 6962 over the shares, with ns_proofs.Tree's surface."""

    def __init__(self, shares):
        self.t, self.n = D.RfcTree(shares), len(shares)
        self.leaves = [D.leaf_hash(bytes(sh)) for sh in shares]
        self.root = self.node(0, self.n)

    def node(self, lo, hi):
        return self.t.mth(lo, hi)


def tree_of(shares, index, k, ns, ig=True):
    return H.Tree(shares, index, k, ns, ig) if ns else DefaultTree([bytes(s) for s in shares])


def record_of(W, ns, kind, start, end, nodes, n_nodes=None):
    nl = node_len(ns)
    body = b"".join(nodes)
    head = b"".join(int(v).to_bytes(4, "little") for v in (kind, start, end, len(nodes) if n_nodes is None else n_nodes))
    return head + body + bytes((2 * H.levels(W) + 1) * nl - len(body))


def prove(tree, ns, start, end):
    return record_of(tree.n, ns, INCLUSION, start, end, H.prove_range(tree, start, end))


def _fold(W, ns, ig, index, k, start, end, shares, nodes):
    """The root the shares and nodes fold to by the recursive split; NmtError on unordered
    siblings."""
    if ns:
        leaves = [nmt.hash_leaf(H.wrapper_ns(sh, start + i, index, k, ns) + bytes(sh), ns) for i, sh in enumerate(shares)]
    else:
        leaves = [D.leaf_hash(bytes(sh)) for sh in shares]
    it = iter(nodes)

    def fold(lo, hi):
        if hi <= start or lo >= end:
            return next(it)
        if hi - lo == 1:
            return leaves[lo - start]
        m = lo + H.split(hi - lo)
        left = fold(lo, m)
        right = fold(m, hi)
        return nmt.hash_node(left, right, ns, ig) if ns else D.node_hash(left, right)

    return fold(0, W)


def _header_ok(W, start, end, n_shares, record):
    kind, rs, re_, n_nodes = (int.from_bytes(record[4 * i:4 * i + 4], "little") for i in range(4))
    return n_shares == end - start and kind == INCLUSION and rs == start and re_ == end and \
        n_nodes == len(H.range_shape(W, start, end))


def _nodes(W, ns, start, end, record):
    nl = node_len(ns)
    return [record[16 + i * nl:16 + (i + 1) * nl] for i in range(len(H.range_shape(W, start, end)))]


def expected_status(W, ns, ig, index, k, start, end, shares, record, root):
    """The status word owed to the question "are `shares` leaves [start, end) of vector
    `index`, by `record`, under `root`?" (0 <= start < end <= W)."""
    if not _header_ok(W, start, end, len(shares), record):
        return MALFORMED
    try:
        got = _fold(W, ns, ig, index, k, start, end, shares, _nodes(W, ns, start, end, record))
    except nmt.NmtError:
        return ORDER
    return OK if got == root else ROOT


def chained_status(W, ns, ig, axis, index, k, start, end, shares, record, root_record, data_root):
    """The same with no root: the fold's result is leaf axis * W + index under data_root."""
    if not _header_ok(W, start, end, len(shares), record):
        return MALFORMED
    m = axis * W + index
    n2, mask2 = D.shape(m, 2 * W)
    if int.from_bytes(root_record[0:4], "little") != n2 or int.from_bytes(root_record[4:8], "little") != mask2:
        return MALFORMED
    try:
        cand = _fold(W, ns, ig, index, k, start, end, shares, _nodes(W, ns, start, end, record))
    except nmt.NmtError:
        return ORDER
    aunts = [root_record[8 + 32 * i:40 + 32 * i] for i in range(n2)]
    return OK if D.root_from_path(D.leaf_hash(cand), m, 2 * W, aunts) == data_root else ROOT


#: one question put to a verifier: the query's (index, start, end), what is presented, the
#: root it is checked against and the status the model owes it
Case = namedtuple("Case", "name index start end record shares root must")


def _flip(b, byte, bit=0):
    b = bytearray(b)
    b[byte] ^= 1 << bit
    return bytes(b)


def _put(rec, field, v):
    return rec[:4 * field] + (v & 0xFFFFFFFF).to_bytes(4, "little") + rec[4 * field + 4:]


def hostile(tree, W, ns, ig, index, k, start, end, shares, next_root):
    """The valid proof of [start, end) of `tree` (vector `index`) and its hostile variants;
    next_root: the root of vector (index + 1) % W."""
    nl = node_len(ns)
    rec = prove(tree, ns, start, end)
    nodes = H.prove_range(tree, start, end)
    n_left = sum(1 for lo, hi in H.range_shape(W, start, end) if hi <= start)
    shares = [bytes(s) for s in shares]
    out = []

    def add(name, r=rec, sh=shares, root=tree.root, q=(index, start, end)):
        out.append(Case(name, q[0], q[1], q[2], r, sh, root,
                        expected_status(W, ns, ig, q[0], k, q[1], q[2], sh, r, root)))

    add("valid")
    add("share bit", sh=[_flip(shares[0], len(shares[0]) - 1, 3)] + shares[1:])
    add("last share bit", sh=shares[:-1] + [_flip(shares[-1], ns, 0)])
    for i in range(len(nodes)):
        add("node %d bit" % i, r=_flip(rec, 16 + i * nl + nl - 1, 6))
        if ns:
            add("node %d min bit" % i, r=_flip(rec, 16 + i * nl + ns - 1, 0))
    add("root bit", root=_flip(tree.root, len(tree.root) - 1, 1))
    for kind in (0, 2, 3):
        add("kind %d" % kind, r=_put(rec, 0, kind))
    add("n_nodes + 1", r=_put(rec, 3, len(nodes) + 1))
    add("n_nodes - 1", r=_put(rec, 3, len(nodes) - 1))
    add("record start + 1", r=_put(rec, 1, start + 1))
    add("record end - 1", r=_put(rec, 2, end - 1))
    add("record end + 1", r=_put(rec, 2, end + 1))
    if end < W:
        add("asked one further", q=(index, start + 1, end + 1))
    add("asked of the next vector", q=((index + 1) % W, start, end), root=next_root)
    add("one share too few", sh=shares[:-1])
    add("one share too many", sh=shares + [shares[-1]])
    add("0xA5 past the nodes", r=rec[:16 + len(nodes) * nl] + b"\xa5" * (len(rec) - 16 - len(nodes) * nl))
    if n_left:
        add("left node <- last leaf", r=rec[:16] + tree.leaves[end - 1] + rec[16 + nl:])
    if len(nodes) >= 2:
        sw = [nodes[-1]] + nodes[1:-1] + [nodes[0]]
        add("first and last node swapped", r=record_of(W, ns, INCLUSION, start, end, sw))
    return out


def named_musts(cases):
    """What the hostile set owes by construction, whatever the tree: asserted by the tests
    next to the model's word."""
    for c in cases:
        if c.name in ("valid", "0xA5 past the nodes"):
            assert c.must == OK, c.name
        elif c.name.startswith(("kind", "n_nodes", "record ", "one share", "asked one further")):
            assert c.must == MALFORMED, c.name
        else:
            assert c.must in (ORDER, ROOT), c.name


def all_ranges(W):
    return [(a, b) for a in range(W) for b in range(a + 1, W + 1)]


def share_range_rows(k, start, end):
    """ODS shares [start, end) in row-major order as (row, first column, end column)."""
    return [(r, max(start, r * k) - r * k, min(end, (r + 1) * k) - r * k) for r in range(start // k, (end - 1) // k + 1)]
