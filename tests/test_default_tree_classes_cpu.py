"""CPU: the references of tests/default_tree_classes.py against each other, the pinned
width classes of the DefaultTree kernels, and the host restatements of the tree
(merkle.cpp rsm_default_tree_root, rsm_default_tree_prove, rsm_default_tree_verify) at the
widths tests/test_gpu_default_tree_classes.py runs the kernels at, up to 514: odd widths,
widths with a carried subtree at every height, both sides of every class boundary.  The
fallback paths and Repair's host checks rest on these functions; no expectation of the GPU
file comes from here."""
import ctypes

import numpy as np
import pytest

import data_root as D
import default_tree_classes as C
import proof_status as P
import proof_verify as V
import rsmt2d_amd as R
from oracle import crossword
from test_verify_cpu import host_status

S = C.S
WIDE = [254, 255, 256, 257, 258, 385, 386, 510, 511, 512, 513, 514, 1022, 1023, 1026, 2046, 2047, 2048]
#: every width of the GPU file up to 514
HOST_WIDTHS = [3, 5, 7, 9, 33, 126, 127, 129, 176, 177, 178, 254, 255, 257, 258, 384, 385, 386, 510, 514]


def vector(n, seed=0):
    g = np.random.default_rng([0xC1, n, seed])
    return [g.integers(0, 256, S, dtype=np.uint8).tobytes() for _ in range(n)]


def test_the_two_hashlib_statements_agree():
    """The stack fold and the recursive split, from shares and from digests, at every width
    1..300 and at the wide ones; a one-leaf tree is its leaf digest."""
    for n in list(range(1, 301)) + WIDE:
        leaves = vector(n)
        digests = [V.leaf_sum(x) for x in leaves]
        root = C.tree_root(leaves)
        assert root == C.fold_digests(digests) == C.split_digests(digests), n
        assert root == P.tree_levels(leaves, 0, None)[-1][0], n  # the level picture
    assert C.tree_root(vector(1)) == V.leaf_sum(vector(1)[0])


def test_the_statements_tell_trees_apart():
    """The references have teeth of their own: the last leaf, a leaf carried at height 0, and
    the order of the two top subtrees all change the root."""
    for n in (3, 5, 9, 177, 385):
        leaves = vector(n)
        root = C.tree_root(leaves)
        last = leaves[:-1] + [leaves[-1][:-1] + bytes([leaves[-1][-1] ^ 1])]
        assert C.tree_root(last) != root
        assert C.tree_root(leaves[:-1]) != root and C.tree_root(leaves + leaves[-1:]) != root
        k = D.split(n)
        assert C.tree_root(leaves[k:] + leaves[:k]) != root


def test_class_table(tmp_path):
    """The launcher's choices restated in tests/default_tree_classes.py against the constants
    read out of kernels_sha.hip and against the pinned literals."""
    C.check_classes()
    assert [C.trees_per_wave(W) for W in (176, 177, 178, 384, 385, 386, 2048)] == [4, 4, 2, 2, 2, 1, 1]
    assert C.root_form(2048, 1)[1] == 133120
    # the boundaries are where the class changes, and nowhere else
    change = [W for W in range(2, C.MAX_WIDTH) if C.trees_per_wave(W) != C.trees_per_wave(W + 1)]
    assert change == [177, 385]
    assert [W for W in range(2, C.MAX_WIDTH) if C.nodes_form(W)[2] != C.nodes_form(W + 1)[2]] == [512, 1024, 1536]
    assert [C.proof_trees_per_block(W) for W in (3, 16, 17, 255, 256, 257, 2047)] == [32, 32, 28, 2, 2, 1, 1]
    # a moved constant is noticed: the source with another budget, another workgroup
    with open(C.KERNELS_SHA) as f:
        src = f.read()
    for old, new, key, value in (("<= 52u * 1024u) return t;", "<= 48u * 1024u) return t;", "budget", 48 * 1024),
                                 ("kTreesPerBlock = 4;", "kTreesPerBlock = 8;", "trees_per_block", 8)):
        assert src.count(old) == 1
        path = tmp_path / ("%s.hip" % key)
        path.write_text(src.replace(old, new))
        assert C.source_constants(str(path)) == dict(C.SOURCE_WANT, **{key: value}) != C.SOURCE_WANT


def test_sampled_trees_cover_the_edges():
    for W, tpw in ((2047, 1), (2048, 1), (1026, 1), (385, 2), (177, 4)):
        t = C.sampled_trees(W, tpw)
        n = 4 * tpw
        assert set(range(n)) <= set(t) and set(range(2 * W - n, 2 * W)) <= set(t)
        assert {W - 2, W - 1, W, W + 1} <= set(t) and len(t) == 2 * n + 4 + 16
        assert all(0 <= x < 2 * W for x in t) and t == C.sampled_trees(W, tpw)


def test_square_roots_and_samples():
    """square_roots is every tree's root by the oracle functions; class_samples holds the
    carried leaf's position on several trees of every square."""
    for W in (1, 2, 3, 5, 9, 12):
        b = C.make_batch(W, 2)
        for sq in b:
            got = C.square_roots(sq)
            for t in range(2 * W):
                assert got[t].tobytes() == crossword.merkle_root(C.tree_leaves(sq, t)) == D.mth(C.tree_leaves(sq, t))
    for W in (3, 33, 257, 514):
        s = C.class_samples(W, 3)
        assert all(q < 3 and a < 2 and i < W and p < W for q, a, i, p in s)
        for q in range(3):
            assert len({(a, i) for (q_, a, i, p) in s if q_ == q and p == W - 1}) >= 4


def positions(n):
    if n <= 33:
        return list(range(n))
    top = D.split(n)
    g = np.random.default_rng([0xC2, n])
    return sorted({0, 1, top - 1, top, n - 2, n - 1} | {int(x) for x in g.integers(0, n, 10)})


@pytest.mark.parametrize("n", HOST_WIDTHS)
def test_host_tree_against_hashlib(lib, n):
    """Root, records and verification of one vector: the root by both statements, each record
    RFC 6962's PATH with the sides of the recursive split and the record built by levels,
    accepted by the NebulousLabs verifier; the host verifier status for status on every
    mutation of tests/proof_status.py."""
    leaves = vector(n, 1)
    want_root = C.tree_root(leaves)
    assert R._default_root(leaves) == want_root
    tree, lv = D.RfcTree(leaves), P.tree_levels(leaves, 0, None)
    keep, ptrs, _ = R._bufs(leaves)
    other = C.tree_root(vector(n, 2))
    seen = []
    for pos in positions(n):
        rec, root = ctypes.create_string_buffer(V.record_bytes(n, 32)), ctypes.create_string_buffer(32)
        assert lib.rsm_default_tree_prove(ptrs, n, S, pos, rec, root) == 0
        assert root.raw == want_root
        nodes, mask = V.parse_record(rec.raw, 32)
        assert nodes == tree.path(pos) and (len(nodes), mask) == D.shape(pos, n) == P.proof_shape(n, pos), (n, pos)
        assert rec.raw == P.record_of(lv, pos, None)
        assert V.verify_default(want_root, [leaves[pos]] + nodes, pos, n)
        items = list(P.mutations(leaves[pos], rec.raw, want_root, (0, 0, 0, pos), n, None, other, other[::-1]))
        want = P.expect(items, n, None)
        for it, w in zip(items, want):
            assert host_status(lib, None, 0, it.share, n, it.sample[3], it.record, it.root) == (0, w), (n, pos, it.label)
        seen += want
    if n & 1:  # the carried leaf's short proof: one node per perfect subtree to its left
        assert P.proof_shape(n, n - 1)[0] == bin(n - 1).count("1")
    P.assert_covers(seen, None)
