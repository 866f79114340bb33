"""CPU: the host restatements of the range proofs (rsm_default_tree_range_prove / _verify,
rsm_nmt_tree_range_prove / _verify), rsm_share_range_queries and rsm_eds_range_proofs on the
host path, against the recursive hashlib model of tests/range_proofs.py."""
import ctypes

import pytest

import ns_proofs as H
import range_proofs as M
import rsmt2d_amd as R
from range_calls import host_prove, host_status, params

S = 64
TREES = [(0, True), (1, True), (1, False), (8, True), (8, False), (29, True), (29, False)]  # (ns, ignore_max); 0: DefaultTree


def indices(W, k):
    """Vector indices inside quadrant 0 and at or past k."""
    return sorted({0, max(k - 1, 0), min(k, W - 1), W - 1})


@pytest.mark.parametrize("ns,ig", TREES)
@pytest.mark.parametrize("W", range(1, 10))
def test_host_prover_and_verifier_match_the_model(lib, W, ns, ig):
    k = (W + 1) // 2
    p = params(k, ns, ig)
    for index in indices(W, k):
        leaves = M.vector(W, ns, S, k if index < k else 0, 11 * W + index)
        tree = M.tree_of(leaves, index, k, ns, ig)
        for start, end in M.all_ranges(W):
            rc, rec, root = host_prove(lib, p, index, leaves, start, end)
            assert rc == 0 and root == tree.root
            assert rec == M.prove(tree, ns, start, end), (W, index, start, end)
            case = M.Case("valid", index, start, end, rec, leaves[start:end], tree.root, M.OK)
            assert M.expected_status(W, ns, ig, index, k, start, end, case.shares, rec, tree.root) == M.OK
            assert host_status(lib, p, W, case, S) == M.OK, (W, index, start, end)
            if end < W:  # positions are bound: the same proof never answers the range one further
                moved = case._replace(start=start + 1, end=end + 1)
                assert host_status(lib, p, W, moved, S) == M.MALFORMED


def hostile_cases(k, ns, ig, seed=3):
    """The hostile set over quadrant-0 rows (0, k - 1) and all-parity rows (k, W - 1) of a
    square with increasing namespaces: a third of each row's ranges and four picked ones."""
    W = 2 * k
    sq = M.square(k, ns, S, seed)
    out = []
    for index in (0, k - 1, k, W - 1):
        leaves = [sq[index, p].tobytes() for p in range(W)]
        nxt = (index + 1) % W
        tree = M.tree_of(leaves, index, k, ns, ig)
        next_root = M.tree_of([sq[nxt, p].tobytes() for p in range(W)], nxt, k, ns, ig).root
        for start, end in M.all_ranges(W):
            if (start + end + index) % 3 and (start, end) not in ((1, 2), (1, W - 1), (k - 1, k + 1), (3, 4)):
                continue
            out += M.hostile(tree, W, ns, ig, index, k, start, end, leaves[start:end], next_root)
    return out


@pytest.mark.parametrize("ns,ig", TREES)
def test_hostile_set(lib, ns, ig):
    k = 4
    p, W = params(k, ns, ig), 2 * k
    cases = hostile_cases(k, ns, ig)
    M.named_musts(cases)
    for c in cases:
        assert host_status(lib, p, W, c, S) == c.must, (c.name, c.index, c.start, c.end)
    seen = {c.must for c in cases}
    assert seen == ({M.OK, M.MALFORMED, M.ORDER, M.ROOT} if ns else {M.OK, M.MALFORMED, M.ROOT})


def test_swapped_nodes_are_order_in_quadrant_0_and_root_in_parity():
    """The two node replacements of the hostile set: ORDER as well as ROOT on quadrant-0
    vectors with increasing namespaces, only ROOT on all-parity vectors (k = 4, ns = 8)."""
    k, ns = 4, 8
    by_vector = {True: set(), False: set()}
    for c in hostile_cases(k, ns, True):
        if c.name in ("left node <- last leaf", "first and last node swapped"):
            by_vector[c.index < k].add(c.must)
    assert by_vector[True] == {M.ORDER, M.ROOT} and by_vector[False] == {M.ROOT}


def test_record_bytes_and_node_bound(lib):
    for W in (1, 2, 3, 8, 131, 1024, 2048):
        assert lib.rsm_range_record_bytes(W, None) == M.record_bytes(W, 0)
        for ns in (1, 29, 32):
            assert lib.rsm_range_record_bytes(W, ctypes.byref(R.NmtParams(ns, 1, 1))) == M.record_bytes(W, ns)
    assert lib.rsm_range_record_bytes(0, None) == 0
    assert lib.rsm_range_record_bytes(8, ctypes.byref(R.NmtParams(0, 1, 4))) == 0
    for W in range(1, 70):
        for start, end in M.all_ranges(W):
            assert len(H.range_shape(W, start, end)) <= 2 * H.levels(W)


def test_host_argument_errors(lib):
    leaves = M.vector(4, 8, S, 2, 1)
    p = params(2, 8)
    for start, end in ((2, 2), (3, 2), (0, 5), (4, 5)):
        assert host_prove(lib, None, 0, leaves, start, end)[0] == R.RSM_EINVAL
        assert host_prove(lib, p, 0, leaves, start, end)[0] == R.RSM_EINVAL
        st = ctypes.c_uint32(0)
        rec = bytes(M.record_bytes(4, 8))
        assert lib.rsm_default_tree_range_verify(start, end, leaves[0], 1, S, 4, rec, bytes(32), ctypes.byref(st)) == R.RSM_EINVAL
        assert lib.rsm_nmt_tree_range_verify(ctypes.byref(p), 0, start, end, leaves[0], 1, S, 4, rec, bytes(48),
                                             ctypes.byref(st)) == R.RSM_EINVAL
    st = ctypes.c_uint32(0)  # shares shorter than the namespace
    assert lib.rsm_nmt_tree_range_verify(ctypes.byref(p), 0, 0, 1, b"abc", 1, 3, 4, bytes(M.record_bytes(4, 8)), bytes(48),
                                         ctypes.byref(st)) == R.RSM_ETREE
    unsorted = [leaves[1], leaves[0]] + leaves[2:]  # the prover's tree fails as rsm_nmt_tree_prove's
    assert host_prove(lib, p, 0, unsorted, 0, 1)[0] == R.RSM_ETREE


@pytest.mark.parametrize("start,end", [(1, 3), (5, 8), (2, 11), (0, 16), (15, 16), (0, 1)])
def test_share_range_queries(lib, start, end):
    """Within one row, ending at a row's end, three rows (a partial first, a whole middle and
    a partial last one), the whole square and its corners, at k = 4."""
    k = 4
    got = R.share_range_queries(k, start, end, square=2)
    assert got == [(2, 0, r, a, b) for r, a, b in M.share_range_rows(k, start, end)]
    cells = [(q[2], c) for q in got for c in range(q[3], q[4])]
    assert cells == [(i // k, i % k) for i in range(start, end)] and all(c < k for _, c in cells)


def test_share_range_queries_errors(lib):
    out, n = (R.RangeQuery * 4)(), ctypes.c_uint32(0)
    f = lib.rsm_share_range_queries
    for k, start, end in ((4, 3, 3), (4, 5, 4), (4, 0, 17), (0, 0, 1), (32769, 0, 1)):
        assert f(k, 0, start, end, out, ctypes.byref(n)) == R.RSM_EINVAL
    assert f(4, 0, 0, 1, None, ctypes.byref(n)) == R.RSM_EINVAL
    assert f(4, 0, 0, 1, out, None) == R.RSM_EINVAL
    assert f(4, 0, 2, 11, out, ctypes.byref(n)) == 0 and n.value == 3
    big = (R.RangeQuery * 2)()  # the largest k: no overflow in k * k
    assert f(32768, 0, 32768 * 32768 - 2, 32768 * 32768, big, ctypes.byref(n)) == 0
    assert n.value == 1 and (big[0].index, big[0].start, big[0].end) == (32767, 32766, 32768)


@pytest.mark.parametrize("ns", [0, 8])
def test_eds_range_proofs_host_path(lib, ns):
    """An imported square has no device context: rsm_eds_range_proofs runs the host
    restatement per query; RangeProof.verify and ShareProof.Validate(device=None) agree."""
    k, W = 4, 8
    sq = M.square(k, ns, S, 21)
    ctor = R.newErasuredNamespacedMerkleTreeConstructor(k, ns) if ns else R.NewDefaultTree
    flat = [sq[r, c].tobytes() for r in range(W) for c in range(W)]
    eds = R.ImportExtendedDataSquare(flat, R.NewLeoRSCodec(), ctor)
    queries = [(a, i, s, e) for a in (0, 1) for i in (0, k, W - 1) for (s, e) in ((0, 1), (1, 6), (3, 8), (0, 8))]
    proofs = eds.RangeProofs(queries)
    roots = [eds.RowRoots(), eds.ColRoots()]
    for (a, i, s, e), pr in zip(queries, proofs):
        leaves = [(sq[i, p] if a == 0 else sq[p, i]).tobytes() for p in range(W)]
        tree = M.tree_of(leaves, i, k, ns)
        assert pr.record() == M.prove(tree, ns, s, e) and pr.shares == leaves[s:e], (a, i, s, e)
        assert roots[a][i] == tree.root and pr.verify(tree.root) == M.OK
        assert pr.verify(roots[a][(i + 1) % W]) in (M.ROOT, M.ORDER)
    sp = eds.ShareProof(2, 11)
    assert [(pr.tree_index, pr.start, pr.end) for pr in sp.rows] == [(0, 2, 4), (1, 0, 4), (2, 0, 3)]
    assert sp.shares() == [sq[i // k, i % k].tobytes() for i in range(2, 11)]
    dr = eds.DataRoot()
    assert sp.Validate(dr, device=None)
    sp.rows[1].shares[2] = bytes([sp.rows[1].shares[2][0] ^ 1]) + sp.rows[1].shares[2][1:]
    assert not sp.Validate(dr, device=None)


def test_eds_range_proofs_errors(lib):
    k, W = 2, 4
    sq = M.square(k, 0, S, 5)
    flat = [sq[r, c].tobytes() for r in range(W) for c in range(W)]
    eds = R.ImportExtendedDataSquare(flat, R.NewLeoRSCodec(), R.NewDefaultTree)
    for q in ((0, 4, 0, 1), (2, 0, 0, 1), (0, 0, 1, 1), (0, 0, 0, 5)):
        with pytest.raises(R.RSMError) as e:
            eds.RangeProofs([q])
        assert e.value.code == R.RSM_EINVAL
    flat[5] = None
    hole = R.ImportExtendedDataSquare(flat, R.NewLeoRSCodec(), R.NewDefaultTree)
    with pytest.raises(R.RSMError) as e:
        hole.RangeProofs([(0, 1, 0, 2)])
    assert e.value.code == R.RSM_ETREE
    assert len(hole.RangeProofs([(0, 0, 0, 2)])) == 1  # a complete row of an incomplete square
