"""TEST INFRASTRUCTURE ONLY -- the data root (the RFC 6962 Merkle root over
rowRoots ++ colRoots), proofs of a root under it, and what a chained verifier (share ->
row / column root -> data root) must answer.  Shared by tests/test_data_root_cpu.py and
tests/test_gpu_data_root.py.  Pure Python over hashlib and oracle/nmt.py; nothing here
calls the library under test.

The tree is written in RFC 6962's recursive form -- MTH(D[n]) splits at the largest power
of two below n, PATH(m, D[n]) lists the other side's MTH on the way back up -- and NOT in
the level picture the library uses, so that the two are independent statements of one
tree.  test_data_root_cpu.py pins this module to the RFC's published vectors."""
import hashlib
from collections import namedtuple

from oracle import nmt
import proof_status as P
import proof_verify as V

OK, MALFORMED, ORDER, ROOT = P.OK, P.MALFORMED, P.ORDER, P.ROOT


def leaf_hash(data: bytes) -> bytes:
    return hashlib.sha256(b"\x00" + data).digest()


def node_hash(a: bytes, b: bytes) -> bytes:
    return hashlib.sha256(b"\x01" + a + b).digest()


def split(n: int) -> int:
    """The largest power of two below n (n >= 2)."""
    k = 1
    while k * 2 < n:
        k *= 2
    return k


class RfcTree:
    """RFC 6962 §2.1 over a fixed list of leaves: MTH(D[lo:hi]) by the recursive split,
    each range hashed once (many paths share their subtrees)."""

    def __init__(self, leaves):
        self.leaves = list(leaves)
        self._memo = {}

    def mth(self, lo: int, hi: int) -> bytes:
        if hi - lo == 0:
            return hashlib.sha256(b"").digest()
        if hi - lo == 1:
            return leaf_hash(self.leaves[lo])
        if (lo, hi) not in self._memo:
            k = split(hi - lo)
            self._memo[(lo, hi)] = node_hash(self.mth(lo, lo + k), self.mth(lo + k, hi))
        return self._memo[(lo, hi)]

    def root(self) -> bytes:
        return self.mth(0, len(self.leaves))

    def path(self, m: int, lo: int = 0, hi: int = None):
        """RFC 6962 §2.1.1 PATH(m, D[lo:hi]), m counted from lo: the aunts, bottom-up."""
        hi = len(self.leaves) if hi is None else hi
        if hi - lo == 1:
            return []
        k = split(hi - lo)
        if m < k:
            return self.path(m, lo, lo + k) + [self.mth(lo + k, hi)]
        return self.path(m - k, lo + k, hi) + [self.mth(lo, lo + k)]


def mth(leaves) -> bytes:
    """RFC 6962 §2.1 MTH; tendermint HashFromByteSlices."""
    return RfcTree(leaves).root()


def path(m: int, leaves):
    """RFC 6962 §2.1.1 PATH(m, D[n]): the aunts of leaf m, bottom-up."""
    return RfcTree(leaves).path(m)


def sides(m: int, n: int):
    """For each aunt of leaf m among n leaves, bottom-up: True where the aunt is the right
    operand of the hash it enters."""
    if n == 1:
        return []
    k = split(n)
    return sides(m, k) + [True] if m < k else sides(m - k, n - k) + [False]


def shape(m: int, n: int):
    """(n_nodes, right_mask) of the record of leaf m among n leaves."""
    s = sides(m, n)
    return len(s), sum(1 << i for i, right in enumerate(s) if right)


def root_from_path(leaf_digest: bytes, m: int, n: int, aunts) -> bytes:
    """The root a path folds to, top-down by the recursive split (tendermint's
    computeHashFromAunts); aunts bottom-up, exactly len(sides(m, n)) of them."""
    if n == 1:
        assert not aunts
        return leaf_digest
    k = split(n)
    if m < k:
        return node_hash(root_from_path(leaf_digest, m, k, aunts[:-1]), aunts[-1])
    return node_hash(aunts[-1], root_from_path(leaf_digest, m - k, n - k, aunts[:-1]))


def levels(n: int) -> int:
    return (n - 1).bit_length()


def record_bytes(width: int) -> int:
    return 8 + levels(2 * width) * 32


def record_of(roots, width: int, axis: int, index: int) -> bytes:
    """The root proof record of leaf axis * width + index over roots = rows + columns (a
    list, or an RfcTree of it when many records of one square are wanted)."""
    m = axis * width + index
    aunts = roots.path(m) if isinstance(roots, RfcTree) else path(m, roots)
    n_nodes, mask = shape(m, 2 * width)
    assert n_nodes == len(aunts)
    body = n_nodes.to_bytes(4, "little") + mask.to_bytes(4, "little") + b"".join(aunts)
    return body + bytes(record_bytes(width) - len(body))


def root_status(root_bytes: bytes, record: bytes, data_root: bytes, width: int, axis: int, index: int) -> int:
    """What a verifier of one root under a data root must answer."""
    m = axis * width + index
    n_nodes, mask = shape(m, 2 * width)
    if int.from_bytes(record[0:4], "little") != n_nodes or int.from_bytes(record[4:8], "little") != mask:
        return MALFORMED
    aunts = [record[8 + 32 * i: 40 + 32 * i] for i in range(n_nodes)]
    return OK if root_from_path(leaf_hash(root_bytes), m, 2 * width, aunts) == data_root else ROOT


def share_fold(share: bytes, record: bytes, pos: int, index: int, W: int, p):
    """(status, candidate root) of the share proof alone: MALFORMED / ORDER with no
    candidate, else OK with the bytes the fold ends in (DefaultTree: the digest; NMT:
    min || max || digest)."""
    t = P.tree_of(p)
    nl = P.node_len(t)
    n_nodes, mask = P.proof_shape(W, pos)
    if int.from_bytes(record[0:4], "little") != n_nodes or int.from_bytes(record[4:8], "little") != mask:
        return MALFORMED, None
    nodes = [record[8 + i * nl: 8 + (i + 1) * nl] for i in range(n_nodes)]
    if not t.ns:
        acc = V.leaf_sum(share)
        for i, nd in enumerate(nodes):
            acc = V.node_sum(acc, nd) if (mask >> i) & 1 else V.node_sum(nd, acc)
        return OK, acc
    acc = V.nmt_leaf(share, pos, index, t.k, t.ns)
    try:
        for i, nd in enumerate(nodes):
            acc = (nmt.hash_node(acc, nd, t.ns, bool(t.ignore_max)) if (mask >> i) & 1
                   else nmt.hash_node(nd, acc, t.ns, bool(t.ignore_max)))
    except nmt.NmtError:
        return ORDER, None
    return OK, acc


def chained_status(share: bytes, record: bytes, root_record: bytes, data_root: bytes, sample, W: int, p) -> int:
    """Status words of the chained verifier, the first that applies: MALFORMED (share
    record's header, then root record's header, both before any hashing), ORDER (NMT share
    fold), ROOT, OK."""
    _q, axis, index, pos = sample
    n1, m1 = P.proof_shape(W, pos)
    if int.from_bytes(record[0:4], "little") != n1 or int.from_bytes(record[4:8], "little") != m1:
        return MALFORMED
    n2, m2 = shape(axis * W + index, 2 * W)
    if int.from_bytes(root_record[0:4], "little") != n2 or int.from_bytes(root_record[4:8], "little") != m2:
        return MALFORMED
    st, cand = share_fold(share, record, pos, index, W, p)
    if st != OK:
        return st
    return root_status(cand, root_record, data_root, W, axis, index)


# ---- hostile inputs ---------------------------------------------------------------------
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


#: one root handed to a root verifier
RootItem = namedtuple("RootItem", "label root_bytes record data_root axis index")


def root_mutations(root_bytes: bytes, record: bytes, data_root: bytes, width: int, axis: int, index: int,
                   other_data_root: bytes):
    """From one valid (root, record, data root): a flipped node, the wrong index, the
    wrong axis, n_nodes +- 1, a changed mask, another data root, a non-zero tail."""
    n_nodes, mask = shape(axis * width + index, 2 * width)
    yield RootItem("valid", root_bytes, record, data_root, axis, index)
    yield RootItem("root byte", _flip(root_bytes, len(root_bytes) - 1, 2), record, data_root, axis, index)
    for i in range(n_nodes):
        yield RootItem("node %d" % i, root_bytes, _flip(record, 8 + 32 * i + (7 * i) % 32, i & 7), data_root, axis, index)
    if width > 1:
        yield RootItem("wrong index", root_bytes, record, data_root, axis, (index + 1) % width)
    yield RootItem("wrong axis", root_bytes, record, data_root, 1 - axis, index)
    yield RootItem("n_nodes + 1", root_bytes, _header(record, n_nodes=n_nodes + 1), data_root, axis, index)
    yield RootItem("n_nodes - 1", root_bytes, _header(record, n_nodes=n_nodes - 1), data_root, axis, index)
    yield RootItem("mask bit", root_bytes, _header(record, mask=mask ^ 1), data_root, axis, index)
    yield RootItem("mask bit 31", root_bytes, _header(record, mask=mask ^ (1 << 31)), data_root, axis, index)
    yield RootItem("another data root", root_bytes, record, other_data_root, axis, index)
    if n_nodes < levels(2 * width):  # never read: the status must not change
        tail = 8 + 32 * n_nodes
        yield RootItem("non-zero tail", root_bytes, record[:tail] + b"\x5a" * (len(record) - tail), data_root, axis, index)


#: one sample handed to a chained verifier: sample = (square, axis, index, pos)
ChainItem = namedtuple("ChainItem", "label share record root_record data_root sample")


def chain_mutations(share: bytes, record: bytes, root_record: bytes, data_root: bytes, sample, W: int, p,
                    other_data_root: bytes):
    """From one valid chained sample: the root-record variants of root_mutations, the
    same on the share record, a share bit flip, another data root, and the sample
    presented at another position, index and axis."""
    t = P.tree_of(p)
    nl = P.node_len(t)
    q, axis, index, pos = sample
    n1, m1 = P.proof_shape(W, pos)
    n2, m2 = shape(axis * W + index, 2 * W)
    mk = lambda label, **kw: ChainItem(label, **{**dict(share=share, record=record, root_record=root_record,
                                                        data_root=data_root, sample=sample), **kw})
    yield mk("valid")
    yield mk("share bit", share=_flip(share, len(share) - 1, 5))
    for i in range(n1):
        yield mk("share node %d" % i, record=_flip(record, 8 + i * nl + nl - 1 - (i % 32), i & 7))
    for i in range(n2):
        yield mk("root node %d" % i, root_record=_flip(root_record, 8 + 32 * i + (5 * i) % 32, (i + 3) & 7))
    if W > 1:
        yield mk("wrong index", sample=(q, axis, (index + 1) % W, pos))
        yield mk("wrong pos", sample=(q, axis, index, (pos + 1) % W))
    yield mk("row as column" if axis == 0 else "column as row", sample=(q, 1 - axis, index, pos))
    yield mk("share n_nodes + 1", record=_header(record, n_nodes=n1 + 1))
    yield mk("share n_nodes - 1", record=_header(record, n_nodes=n1 - 1))
    yield mk("share mask bit", record=_header(record, mask=m1 ^ 1))
    yield mk("root n_nodes + 1", root_record=_header(root_record, n_nodes=n2 + 1))
    yield mk("root n_nodes - 1", root_record=_header(root_record, n_nodes=n2 - 1))
    yield mk("root mask bit", root_record=_header(root_record, mask=m2 ^ 1))
    yield mk("root mask bit 31", root_record=_header(root_record, mask=m2 ^ (1 << 31)))
    yield mk("data root bit", data_root=_flip(data_root, 31, 7))
    yield mk("another square's data root", data_root=other_data_root)
    if n1 < levels(W):
        tail = 8 + n1 * nl
        yield mk("share record tail", record=record[:tail] + b"\xa5" * (len(record) - tail))
    if n2 < levels(2 * W):
        tail = 8 + 32 * n2
        yield mk("root record tail", root_record=root_record[:tail] + b"\x5a" * (len(root_record) - tail))
    if t.ns and index < t.k and pos < t.k:
        for i in range(n1):
            if (m1 >> i) & 1:  # a right-hand sibling below the namespaces to its left
                a = bytearray(record)
                a[8 + i * nl: 8 + i * nl + t.ns] = bytes(t.ns)
                yield mk("sibling order broken", record=bytes(a))
                break


class Chain:
    """A proof_status.Squares with its data roots and root records (built once)."""

    def __init__(self, squares: "P.Squares"):
        self.sq = squares
        self.W, self.p = squares.W, squares.p
        self.roots = [[squares.root(q, a, i) for a in (0, 1) for i in range(self.W)] for q in range(squares.count)]
        self.trees = [RfcTree(r) for r in self.roots]
        self.data_roots = [t.root() for t in self.trees]
        self._rrec = {}

    def root_record(self, q, axis, index) -> bytes:
        key = (q, axis, index)
        if key not in self._rrec:
            self._rrec[key] = record_of(self.trees[q], self.W, axis, index)
        return self._rrec[key]

    def valid(self, sample) -> ChainItem:
        q, axis, index, _pos = sample
        return ChainItem("valid", self.sq.share(sample), self.sq.record(sample), self.root_record(q, axis, index),
                         self.data_roots[q], sample)

    def items(self, samples):
        """Every mutation of every sample."""
        out = []
        for s in samples:
            v = self.valid(s)
            other = self.data_roots[(s[0] + 1) % self.sq.count]
            out.extend(chain_mutations(v.share, v.record, v.root_record, v.data_root, s, self.W, self.p, other))
        return out

    def expect(self, items):
        return [chained_status(it.share, it.record, it.root_record, it.data_root, it.sample, self.W, self.p) for it in items]
