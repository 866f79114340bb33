"""TEST INFRASTRUCTURE ONLY -- an independent verifier of share inclusion proofs and
the shared helpers of tests/test_proofs_cpu.py and tests/test_gpu_proofs.py.  Pure
Python over hashlib and oracle/nmt.py (hash_leaf / hash_node); nothing here calls the
library under test.

DefaultTree: NebulousLabs merkletree's VerifyProof, restated step by step (the
algorithm celestiaorg/merkletree, the reference's DefaultTree, inherits).
NMT: a bottom-up fold with the record's right_mask, and a recursive in-order verifier
for nodes in nmt's Proof.Nodes order."""
import hashlib

import numpy as np

from oracle import nmt


def leaf_sum(data: bytes) -> bytes:
    return hashlib.sha256(b"\x00" + data).digest()


def node_sum(a: bytes, b: bytes) -> bytes:
    return hashlib.sha256(b"\x01" + a + b).digest()


def verify_default(root: bytes, proof_set, index: int, num_leaves: int) -> bool:
    """merkletree.VerifyProof(h, root, proofSet, proofIndex, numLeaves)."""
    if index >= num_leaves or not proof_set:
        return False
    height = 0
    acc = leaf_sum(proof_set[height])
    height += 1
    stable_end = index
    while True:
        size = 1 << height
        start = (index // size) * size
        end = start + size - 1
        if end >= num_leaves:
            break
        stable_end = end
        if len(proof_set) <= height:
            return False
        if index - start < (1 << (height - 1)):
            acc = node_sum(acc, proof_set[height])
        else:
            acc = node_sum(proof_set[height], acc)
        height += 1
    if stable_end != num_leaves - 1:
        if len(proof_set) <= height:
            return False
        acc = node_sum(acc, proof_set[height])
        height += 1
    while height < len(proof_set):
        acc = node_sum(proof_set[height], acc)
        height += 1
    return acc == root


def level_count(n: int, pos: int) -> int:
    """Nodes of the proof of leaf pos by the level picture: level l has ceil(n / 2^l)
    nodes; the sibling (pos >> l) ^ 1 counts where it is below that."""
    levels = (n - 1).bit_length()
    return sum(1 for l in range(levels) if ((pos >> l) ^ 1) < -(-n // (1 << l)))


def parse_record(rec: bytes, node_len: int):
    """(nodes bottom-up, right_mask); the rest of the record must be zero."""
    n_nodes = int.from_bytes(rec[0:4], "little")
    mask = int.from_bytes(rec[4:8], "little")
    end = 8 + n_nodes * node_len
    assert end <= len(rec), "n_nodes past the record"
    assert rec[end:] == bytes(len(rec) - end), "record tail is not zero"
    assert mask >> n_nodes == 0, "right_mask bits past n_nodes"
    return [rec[8 + i * node_len: 8 + (i + 1) * node_len] for i in range(n_nodes)], mask


def record_bytes(n: int, node_len: int) -> int:
    return 8 + (n - 1).bit_length() * node_len


def nmt_leaf(share: bytes, pos: int, index: int, k: int, ns: int) -> bytes:
    """The leaf node as the erasured wrapper pushes it: quadrant 0 keeps the share's
    namespace, everything else gets the parity namespace."""
    nid = share[:ns] if (pos < k and index < k) else b"\xff" * ns
    return nmt.hash_leaf(nid + share, ns)


def verify_nmt(root: bytes, share: bytes, nodes, mask: int, pos: int, index: int, k: int, ns: int,
               ignore_max: bool = True) -> bool:
    acc = nmt_leaf(share, pos, index, k, ns)
    for i, nd in enumerate(nodes):
        acc = nmt.hash_node(acc, nd, ns, ignore_max) if (mask >> i) & 1 else nmt.hash_node(nd, acc, ns, ignore_max)
    return acc == root


def verify_nmt_inorder(root: bytes, leaf_node: bytes, nodes, pos: int, n: int, ns: int, ignore_max: bool = True) -> bool:
    """nmt's verification walk for the range [pos, pos + 1): recurse over the RFC 6962
    split of [0, n); a subtree outside the range takes the next node of the list."""
    it = iter(nodes)

    def walk(lo, hi):
        if hi <= pos or lo > pos:
            return next(it)
        if hi - lo == 1:
            return leaf_node
        k = 1
        while k * 2 < hi - lo:
            k *= 2
        left = walk(lo, lo + k)
        right = walk(lo + k, hi)
        return nmt.hash_node(left, right, ns, ignore_max)

    try:
        got = walk(0, n)
    except (StopIteration, nmt.NmtError):  # too few nodes / siblings out of namespace order
        return False
    return got == root and next(it, None) is None


def rand_square(W: int, S: int, seed: int) -> np.ndarray:
    """Seeded random [W][W][S] bytes (a tree test needs no valid extension)."""
    return np.random.default_rng(seed).integers(0, 256, (W, W, S), dtype=np.uint8)


def sorted_q0_square(k: int, S: int, ns: int, seed: int) -> np.ndarray:
    """A random [2k][2k][S] square whose quadrant 0 is sorted row-major by namespace
    (as genRandSortedDS does), so namespaces do not decrease along its rows and columns."""
    rng = np.random.default_rng(seed)
    sq = rng.integers(0, 256, (2 * k, 2 * k, S), dtype=np.uint8)
    q0 = sq[:k, :k].reshape(k * k, S)
    order = np.lexsort(q0[:, :ns][:, ::-1].T)  # the first namespace byte is the primary key
    sq[:k, :k] = q0[order].reshape(k, k, S)
    return sq


def vector(sq: np.ndarray, axis: int, index: int):
    W = sq.shape[0]
    return [sq[index, p].tobytes() if axis == 0 else sq[p, index].tobytes() for p in range(W)]
