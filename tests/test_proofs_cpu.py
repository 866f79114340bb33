"""CPU: share inclusion proofs through the host restatements (merkle.cpp
rsm_default_tree_prove / rsm_nmt_tree_prove), the host path of rsm_eds_proofs and the
Python mirror, checked by the independent verifier of tests/proof_verify.py against
oracle roots (oracle.crossword.merkle_root, oracle.nmt.erasured_root)."""
import ctypes

import numpy as np
import pytest

import rsmt2d_amd as R
from oracle import crossword, nmt
import proof_verify as V

SIZES = [1, 2, 3, 5, 6, 7, 10, 11, 24, 70, 256]


def positions(n, seed):
    if n <= 24:
        return list(range(n))
    rng = np.random.default_rng(seed)
    return sorted({0, n - 1} | {int(x) for x in rng.integers(0, n, 32)})


def default_prove(lib, leaves, pos):
    keep, ptrs, _ = R._bufs(leaves)
    rec = ctypes.create_string_buffer(V.record_bytes(len(leaves), 32))
    root = ctypes.create_string_buffer(32)
    rc = lib.rsm_default_tree_prove(ptrs, len(leaves), len(leaves[0]), pos, rec, root)
    return rc, rec.raw, root.raw


def nmt_prove(lib, p, index, leaves, pos):
    keep, ptrs, _ = R._bufs(leaves)
    nl = 2 * p.namespace_size + 32
    rec = ctypes.create_string_buffer(V.record_bytes(len(leaves), nl))
    root = ctypes.create_string_buffer(nl)
    rc = lib.rsm_nmt_tree_prove(ctypes.byref(p), index, ptrs, len(leaves), len(leaves[0]), pos, rec, root)
    return rc, rec.raw, root.raw


@pytest.mark.parametrize("n", SIZES)
def test_default_tree_prove(lib, n):
    rng = np.random.default_rng(1000 + n)
    leaves = [rng.integers(0, 256, 64, dtype=np.uint8).tobytes() for _ in range(n)]
    want = crossword.merkle_root(leaves)
    assert lib.rsm_proof_record_bytes(n, None) == V.record_bytes(n, 32)
    for pos in positions(n, n):
        rc, rec, root = default_prove(lib, leaves, pos)
        assert rc == 0 and root == want
        nodes, mask = V.parse_record(rec, 32)
        assert len(nodes) == V.level_count(n, pos)
        assert V.verify_default(want, [leaves[pos]] + nodes, pos, n), (n, pos)
        assert R.Proof(leaves[pos], nodes, mask, pos, n).root == want
        if nodes:  # a wrong node must not verify
            bad = [leaves[pos]] + [bytes(32)] + nodes[1:]
            assert not V.verify_default(want, bad, pos, n)


@pytest.mark.parametrize("ns", [29, 8, 1, 32])
@pytest.mark.parametrize("n", SIZES)
def test_nmt_tree_prove(lib, n, ns):
    k = (n + 1) // 2  # the wrapper's square size: leaves past k take the parity namespace
    rng = np.random.default_rng(2000 + 37 * n + ns)
    leaves = sorted((rng.integers(0, 256, 64, dtype=np.uint8).tobytes() for _ in range(n)), key=lambda s: s[:ns])
    nl = 2 * ns + 32
    p = R.NmtParams(ns, 1, k)
    assert lib.rsm_proof_record_bytes(n, ctypes.byref(p)) == V.record_bytes(n, nl)
    for index in (0, k):  # a quadrant-0 vector and an all-parity one
        if index + 1 > 2 * k:
            continue
        want = nmt.erasured_root(leaves, index, k, ns)
        for pos in positions(n, n + ns):
            rc, rec, root = nmt_prove(lib, p, index, leaves, pos)
            assert rc == 0 and root == want, (n, ns, index, pos)
            nodes, mask = V.parse_record(rec, nl)
            assert len(nodes) == V.level_count(n, pos)
            assert V.verify_nmt(want, leaves[pos], nodes, mask, pos, index, k, ns)
            assert R.Proof(leaves[pos], nodes, mask, pos, n, p, index).root == want


def test_default_tree_proofs_reference_case(lib):
    """TestDefaultTreeProofs (datasquare_test.go:282-301): leaves {3,4},{5,6}, pos 1."""
    leaves = [bytes([3, 4]), bytes([5, 6])]
    rc, rec, root = default_prove(lib, leaves, 1)
    assert rc == 0
    nodes, mask = V.parse_record(rec, 32)
    pr = R.Proof(leaves[1], nodes, mask, 1, 2)
    assert len(pr.proofSet()) == 2 and pr.index == 1 and pr.numLeaves == 2
    assert pr.proofSet()[0] == leaves[1] and pr.proofSet()[1] == V.leaf_sum(leaves[0]) and mask == 0
    assert root == crossword.merkle_root(leaves) == pr.root
    assert V.verify_default(root, pr.proofSet(), 1, 2)


def test_prove_argument_errors(lib):
    leaves = [bytes(64)] * 4
    assert default_prove(lib, leaves, 4)[0] == R.RSM_EINVAL
    p = R.NmtParams(8, 1, 1)  # 4 leaves past a square of 2
    assert nmt_prove(lib, p, 0, leaves, 0)[0] == R.RSM_ETREE
    p = R.NmtParams(8, 1, 2)
    unordered = [bytes([9]) * 64, bytes([1]) * 64, bytes([2]) * 64, bytes([3]) * 64]
    assert nmt_prove(lib, p, 0, unordered, 2)[0] == R.RSM_ETREE
    assert nmt_prove(lib, p, 2, unordered, 2)[0] == 0  # all parity namespaces past the square size


def _square(k, S, ns, seed):
    sq = V.sorted_q0_square(k, S, ns, seed)
    W = 2 * k
    return sq, [sq[r, c].tobytes() for r in range(W) for c in range(W)]


def _proofs_raw(lib, eds, fn, user, samples, rb):
    arr = (R.Sample * len(samples))(*[R.Sample(*s) for s in samples])
    rec = ctypes.create_string_buffer(len(samples) * rb)
    sh = ctypes.create_string_buffer(len(samples) * eds.shareSize)
    return lib.rsm_eds_proofs(eds._h, fn, user, arr, len(samples), rec, sh), rec.raw, sh.raw


def test_eds_proofs_host_path(lib):
    """A context-free imported square: every proof through the host restatement."""
    k, S, ns = 3, 64, 8
    sq, flat = _square(k, S, ns, 7)
    W = 2 * k
    for tree_fn in (R.NewDefaultTree, R.newErasuredNamespacedMerkleTreeConstructor(k, ns)):
        eds = R.ImportExtendedDataSquare(flat, R.NewLeoRSCodec(), tree_fn)
        for r in range(W):
            for c in range(W):
                rp, cp = eds.RowProof(r, c), eds.ColProof(r, c)
                assert rp.share == cp.share == flat[r * W + c]
                assert (rp.index, cp.index, rp.numLeaves) == (c, r, W)
                if tree_fn is R.NewDefaultTree:
                    assert V.verify_default(crossword.merkle_root(V.vector(sq, 0, r)), rp.proofSet(), c, W)
                    assert V.verify_default(crossword.merkle_root(V.vector(sq, 1, c)), cp.proofSet(), r, W)
                else:
                    assert V.verify_nmt(nmt.erasured_root(V.vector(sq, 0, r), r, k, ns), rp.share, rp.nodes,
                                        rp.right_mask, c, r, k, ns)
                    assert V.verify_nmt(nmt.erasured_root(V.vector(sq, 1, c), c, k, ns), cp.share, cp.nodes,
                                        cp.right_mask, r, c, k, ns)


def test_eds_proofs_errors(lib):
    k, S, ns = 2, 64, 8
    sq, flat = _square(k, S, ns, 11)
    W = 2 * k
    rb = V.record_bytes(W, 32)
    missing = list(flat)
    missing[1 * W + 2] = None
    eds = R.ImportExtendedDataSquare(missing, R.NewLeoRSCodec(), R.NewDefaultTree)
    # a sample in an incomplete vector; complete vectors of the same square still prove
    assert _proofs_raw(lib, eds, None, None, [(0, 0, 1, 0)], rb)[0] == R.RSM_ETREE
    assert _proofs_raw(lib, eds, None, None, [(0, 1, 2, 3)], rb)[0] == R.RSM_ETREE
    rc, rec, sh = _proofs_raw(lib, eds, None, None, [(0, 0, 0, 3), (0, 1, 0, 2)], rb)
    assert rc == 0 and sh == flat[3] + flat[2 * W]
    nodes, _ = V.parse_record(rec[:rb], 32)
    assert V.verify_default(crossword.merkle_root(V.vector(sq, 0, 0)), [flat[3]] + nodes, 3, W)
    with pytest.raises(R.RSMError) as ei:
        eds.RowProof(1, 0)
    assert ei.value.code == R.RSM_ETREE
    # bad samples: square, axis, index, pos
    for s in [(1, 0, 0, 0), (0, 2, 0, 0), (0, 0, W, 0), (0, 1, 0, W)]:
        assert _proofs_raw(lib, eds, None, None, [(0, 0, 0, 0), s], rb)[0] == R.RSM_EINVAL
    assert b"sample 1" in lib.rsm_last_error()
    # a custom plugin
    keep, fn, user = R._tree_callback(lambda axis, index: None)
    assert _proofs_raw(lib, eds, fn, user, [(0, 0, 0, 0)], rb)[0] == R.RSM_EUNSUPPORTED
    custom = R.ImportExtendedDataSquare(flat, R.NewLeoRSCodec(), lambda axis, index: None)
    with pytest.raises(R.RSMError) as ei:
        custom.RowProof(0, 0)
    assert ei.value.code == R.RSM_EUNSUPPORTED
    # an NMT row out of namespace order
    bad = list(flat)
    bad[0], bad[1] = bytes([0xEE]) * S, bytes([0x01]) * S
    ctor = R.newErasuredNamespacedMerkleTreeConstructor(k, ns)
    e2 = R.ImportExtendedDataSquare(bad, R.NewLeoRSCodec(), ctor)
    with pytest.raises(R.RSMError) as ei:
        e2.RowProof(0, 3)
    assert ei.value.code == R.RSM_ETREE
    pr = e2.RowProof(1, 0)  # other rows are unaffected
    assert V.verify_nmt(nmt.erasured_root(V.vector(sq, 0, 1), 1, k, ns), pr.share, pr.nodes, pr.right_mask, 0, 1, k, ns)


@pytest.mark.parametrize("n", [6, 7, 10])
def test_nmt_nodes_in_order(lib, n):
    ns, k = 8, (n + 1) // 2
    rng = np.random.default_rng(300 + n)
    leaves = sorted((rng.integers(0, 256, 64, dtype=np.uint8).tobytes() for _ in range(n)), key=lambda s: s[:ns])
    p = R.NmtParams(ns, 1, k)
    want = nmt.erasured_root(leaves, 0, k, ns)
    for pos in range(n):
        rc, rec, _root = nmt_prove(lib, p, 0, leaves, pos)
        assert rc == 0
        nodes, mask = V.parse_record(rec, 2 * ns + 32)
        pr = R.Proof(leaves[pos], nodes, mask, pos, n, p, 0)
        assert sorted(pr.nmt_nodes()) == sorted(nodes)
        assert V.verify_nmt_inorder(want, V.nmt_leaf(leaves[pos], pos, 0, k, ns), pr.nmt_nodes(), pos, n, ns)
        if len(nodes) > 1 and pr.nmt_nodes() != nodes:
            assert not V.verify_nmt_inorder(want, V.nmt_leaf(leaves[pos], pos, 0, k, ns), nodes, pos, n, ns)
