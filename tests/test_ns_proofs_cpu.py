"""CPU: namespace proofs through the host restatements (merkle.cpp
rsm_nmt_namespace_prove / rsm_nmt_namespace_verify), the host path of
rsm_eds_namespace_proofs and the Python mirror, against the recursive helper of
tests/ns_proofs.py over the structured squares of tests/nmt_layouts.py.  Every
comparison is byte-exact.

Two demands of the feature's specification cannot hold and are asserted the other way
round.  An ABSENCE proof never has its leaf at position 0: leaf 0's namespace is the
root's min, so a namespace below it is EMPTY by the rule that applies first.  And no
namespace proof verifies to status 4 (RSM_PROOF_OCCUPIED): that word belongs to
rsm_eds_import_samples alone."""
import ctypes
import functools

import numpy as np
import pytest

import nmt_layouts as NL
import ns_proofs as H
import rsmt2d_amd as R
from oracle import nmt

S = 64
KS = [1, 2, 3, 4, 6, 8]
NSS = [1, 8, 29]


def c_prove(lib, p, index, shares, nid):
    keep, ptrs, _ = R._bufs(shares)
    nl = 2 * p.namespace_size + 32
    rec = ctypes.create_string_buffer(H.record_bytes(len(shares), p.namespace_size))
    root = ctypes.create_string_buffer(nl)
    rc = lib.rsm_nmt_namespace_prove(ctypes.byref(p), index, ptrs, len(shares), len(shares[0]), nid, rec, root)
    return rc, rec.raw, root.raw


def c_verify(lib, p, index, nid, shares, W, record, root):
    st = ctypes.c_uint32(99)
    size = len(shares[0]) if shares else S
    rc = lib.rsm_nmt_namespace_verify(ctypes.byref(p), index, nid, b"".join(shares), len(shares), size, W,
                                      record, root, ctypes.byref(st))
    assert rc == 0
    return st.value


def flip(b, i, bit=0):
    return b[:i] + bytes([b[i] ^ (1 << bit)]) + b[i + 1:]


def header(rec, **kw):
    f = [int.from_bytes(rec[4 * i:4 * i + 4], "little") for i in range(4)]
    for name, v in kw.items():
        f[("kind", "start", "end", "n_nodes").index(name)] = v & 0xFFFFFFFF
    return b"".join(v.to_bytes(4, "little") for v in f) + rec[16:]


def hostile(tree, W, ns, index, k, nid, proof, shares, other_root):
    """(name, record, shares, root, the status it must have or None = the helper's)."""
    kind, start, end, nodes, leaf = proof
    nl, L = 2 * ns + 32, H.levels(W)
    rec = H.record_of(W, ns, kind, start, end, nodes, leaf)
    root = tree.root
    out = [("other root", rec, shares, other_root, None)]
    for f, v in (("kind", kind + 1), ("kind", 3), ("kind", 7), ("start", start + 1), ("start", start - 1),
                 ("end", end + 1), ("end", end - 1), ("end", W + 1), ("n_nodes", len(nodes) + 1),
                 ("n_nodes", len(nodes) - 1)):
        out.append(("header " + f, header(rec, **{f: v}), shares, root, None))
    for i in range(len(nodes)):
        for at, bit in ((0, 7), (ns - 1, 0), (ns, 7), (2 * ns - 1, 0), (2 * ns + 5, 3)):
            out.append(("node %d byte %d" % (i, at), flip(rec, 16 + i * nl + at, bit), shares, root, None))
    if kind == H.ABSENCE:
        for at, bit in ((0, 7), (ns - 1, 0), (2 * ns - 1, 0), (2 * ns + 31, 0)):
            out.append(("leaf node byte %d" % at, flip(rec, 16 + 2 * L * nl + at, bit), shares, root, None))
    # bytes the verifier must not read: past the derived nodes (and not the absence leaf)
    tail = bytearray(rec)
    for i in range(16 + len(nodes) * nl, 16 + (2 * L + (kind != H.ABSENCE)) * nl):
        tail[i] ^= 0xA5
    out.append(("non-zero tail", bytes(tail), shares, root, H.OK))
    if kind == H.INCLUSION:
        out.append(("share bit", rec, [flip(shares[0], S - 1)] + shares[1:], root, None))
        alien = bytes([shares[-1][0] ^ 1]) + shares[-1][1:]
        out.append(("alien share", rec, shares[:-1] + [alien], root,
                    H.NAMESPACE if index < k and end - 1 < k else None))
        if end - start >= 2:  # shares left out at either end
            for s2, e2 in ((start + 1, end), (start, end - 1)):
                r2 = H.record_of(W, ns, kind, s2, e2, H.prove_range(tree, s2, e2), None)
                out.append(("narrowed", r2, shares[s2 - start:e2 - start], root, H.INCOMPLETE))
        for p in (start, end):  # an absence proof for a namespace that is present
            if p < W:
                r2 = H.record_of(W, ns, H.ABSENCE, p, p + 1, H.prove_range(tree, p, p + 1), tree.leaves[p])
                out.append(("false absence", r2, [], root, H.NAMESPACE if p == start else H.INCOMPLETE))
    if kind != H.EMPTY:
        out.append(("false empty", bytes(H.record_bytes(W, ns)), [], root, H.INCOMPLETE))
    return out


@functools.lru_cache(maxsize=None)
def run_case(k, ns, ig):
    """Every layout of one (k, ns, ignore_max): (kinds, absence leaf positions, statuses)."""
    lib = R.library()
    W = 2 * k
    p = R.NmtParams(ns, int(ig), k)
    kinds, absent_at, statuses = set(), set(), set()
    for li, layout in enumerate(NL.all_layouts(ns)):
        sq = NL.square(k, ns, S, layout, 7)
        for axis, index in H.vectors(k):
            leaves = H.vector_shares(sq, axis, index)
            tree = H.Tree(leaves, index, k, ns, ig)
            other = H.Tree(H.vector_shares(sq, axis, (index + 1) % W), (index + 1) % W, k, ns, ig).root
            for qi, nid in enumerate(H.query_namespaces(tree.names, ns)):
                want = H.prove_namespace(tree, nid)
                kind, start, end, nodes, leaf = want
                rc, rec, root = c_prove(lib, p, index, leaves, nid)
                assert rc == 0 and root == tree.root, (layout, axis, index, nid.hex())
                assert rec == H.record_of(W, ns, *want), (layout, axis, index, nid.hex(), kind, start, end)
                shares = leaves[start:end] if kind == H.INCLUSION else []
                assert H.expected_status(W, ns, ig, index, k, nid, shares, rec, tree.root) == H.OK
                assert c_verify(lib, p, index, nid, shares, W, rec, tree.root) == H.OK
                pr = R.NamespaceProof(kind, start, end, nodes, leaf, shares, W, p, index)
                assert pr.record() == rec and pr.verify(tree.root, nid) == H.OK
                kinds.add(kind)
                if kind == H.ABSENCE:
                    absent_at.add("k" if start == k else ("0" if start == 0 else "mid"))
                if (li + qi + index) % 3:  # the hostile variants of a third of the queries
                    continue
                for name, r2, sh2, root2, must in hostile(tree, W, ns, index, k, nid, want, shares, other):
                    exp = H.expected_status(W, ns, ig, index, k, nid, sh2, r2, root2)
                    got = c_verify(lib, p, index, nid, sh2, W, r2, root2)
                    assert got == exp, (layout, axis, index, nid.hex(), name, got, exp)
                    if must is not None:
                        assert got == must, (layout, axis, index, nid.hex(), name, got, must)
                    statuses.add(got)
    return kinds, absent_at, statuses


@pytest.mark.parametrize("ig", [True, False])
@pytest.mark.parametrize("ns", NSS)
@pytest.mark.parametrize("k", KS)
def test_prove_and_verify(lib, k, ns, ig):
    kinds, absent_at, statuses = run_case(k, ns, ig)
    assert H.TREE not in kinds and "0" not in absent_at and H.OCCUPIED not in statuses
    if k >= 2:
        assert kinds == {H.EMPTY, H.INCLUSION, H.ABSENCE}


def test_every_kind_and_status_occurs(lib):
    kinds, absent_at, statuses = set(), set(), set()
    for ig in (True, False):
        a, b, c = run_case(6, 8, ig)
        kinds |= a
        absent_at |= b
        statuses |= c
    assert kinds == {H.EMPTY, H.INCLUSION, H.ABSENCE}
    # the first parity leaf proves absence only when the root's max is 0xFF.. (ignore_max off)
    assert absent_at == {"mid", "k"}
    assert statuses == {H.OK, H.MALFORMED, H.ORDER, H.ROOT, H.NAMESPACE, H.INCOMPLETE}


def test_failing_tree_and_arguments(lib):
    k, ns = 4, 8
    p = R.NmtParams(ns, 1, k)
    sq = NL.square(k, ns, S, "ladder:7", 3)
    bad = NL.invert(sq, (0, 1), (0, 2), ns)
    leaves = H.vector_shares(bad, 0, 0)
    with pytest.raises(nmt.NmtError):
        H.Tree(leaves, 0, k, ns)
    assert c_prove(lib, p, 0, leaves, leaves[0][:ns])[0] == R.RSM_ETREE
    assert c_prove(lib, p, 2 * k, leaves, leaves[0][:ns])[0] == R.RSM_ETREE  # a vector past the square
    assert c_prove(lib, p, 1, H.vector_shares(bad, 0, 1), leaves[0][:ns])[0] == 0
    assert lib.rsm_ns_record_bytes(2 * k, ctypes.byref(p)) == H.record_bytes(2 * k, ns)
    assert lib.rsm_ns_record_bytes(2 * k, None) == 0 and lib.rsm_ns_record_bytes(0, ctypes.byref(p)) == 0
    st = ctypes.c_uint32(0)
    rec = bytes(H.record_bytes(2 * k, ns))
    assert lib.rsm_nmt_namespace_verify(ctypes.byref(p), 0, None, None, 0, S, 2 * k, rec, bytes(48),
                                        ctypes.byref(st)) == R.RSM_EINVAL
    assert lib.rsm_nmt_namespace_verify(ctypes.byref(p), 0, bytes(ns), bytes(4), 1, 4, 2 * k, rec, bytes(48),
                                        ctypes.byref(st)) == R.RSM_ETREE


@pytest.mark.parametrize("n", [1, 5, 7, 11, 33])
def test_any_leaf_count(lib, n):
    """The restatements take any n_leaves >= 1, not only the even widths of a square."""
    ns, k = 8, (n + 1) // 2
    p = R.NmtParams(ns, 0, k)
    rng = np.random.default_rng(n)
    leaves = sorted((bytes([0, 0, 0, 0, 0, 0, 0, int(x)]) + bytes(rng.integers(0, 256, S - ns, dtype=np.uint8))
                     for x in rng.integers(1, 6, n)), key=lambda s: s[:ns])
    tree = H.Tree(leaves, 0, k, ns, False)
    for nid in H.query_namespaces(tree.names, ns):
        want = H.prove_namespace(tree, nid)
        rc, rec, root = c_prove(lib, p, 0, leaves, nid)
        assert rc == 0 and root == tree.root and rec == H.record_of(n, ns, *want), (n, nid.hex())
        shares = leaves[want[1]:want[2]] if want[0] == H.INCLUSION else []
        assert c_verify(lib, p, 0, nid, shares, n, rec, root) == H.OK


def _square(k, ns, layout):
    sq = NL.square(k, ns, S, layout, 11)
    W = 2 * k
    return sq, R.ImportExtendedDataSquare([sq[r, c].tobytes() for r in range(W) for c in range(W)],
                                          R.NewLeoRSCodec(), R.newErasuredNamespacedMerkleTreeConstructor(k, ns))


def test_square_host_path(lib):
    """rsm_eds_namespace_proofs without a context: the host restatement per vector."""
    k, ns = 4, 8
    W = 2 * k
    sq, eds = _square(k, ns, "runs")
    roots = {0: eds.RowRoots(), 1: eds.ColRoots()}
    for axis in (0, 1):
        names = sorted({sq[r, c, :ns].tobytes() for r in range(k) for c in range(k)})
        for nid in names + [b"\xff" * ns, bytes(ns)]:
            proofs = eds.NamespaceProofs(nid, axis)
            assert len(proofs) == W
            for index, pr in enumerate(proofs):
                tree = H.Tree(H.vector_shares(sq, axis, index), index, k, ns)
                kind, start, end, nodes, leaf = H.prove_namespace(tree, nid)
                assert (pr.kind, pr.start, pr.end, pr.nodes, pr.leaf_node) == (kind, start, end, nodes, leaf)
                assert pr.shares == (H.vector_shares(sq, axis, index)[start:end] if kind == H.INCLUSION else [])
                assert roots[axis][index] == tree.root and pr.verify(tree.root, nid) == H.OK
    nid = sq[0, 0, :ns].tobytes()
    data = eds.NamespaceData(nid)
    assert [r for r, _ in data] == [r for r, pr in enumerate(eds.NamespaceProofs(nid)) if pr.kind != H.EMPTY]
    assert data and all(pr.verify(roots[0][r], nid) == H.OK for r, pr in data)
    assert eds.NamespaceProofs(nid, 0, [3, 0, 3])[1].shares == eds.NamespaceProofs(nid, 0, [0])[0].shares
    with pytest.raises(R.RSMError) as e:
        eds.NamespaceProofs(nid, 0, [W])
    assert e.value.code == R.RSM_EINVAL
    eds.setCell(1, 1, None)  # an incomplete vector
    with pytest.raises(R.RSMError) as e:
        eds.NamespaceProofs(nid, 0, [1])
    assert e.value.code == R.RSM_ETREE
    assert eds.NamespaceProofs(nid, 0, [0])[0].kind == H.INCLUSION


def test_square_failing_tree_and_plugins(lib):
    k, ns = 4, 8
    W = 2 * k
    sq = NL.invert(NL.square(k, ns, S, "ladder:7", 5), (2, 0), (2, 3), ns)
    eds = R.ImportExtendedDataSquare([sq[r, c].tobytes() for r in range(W) for c in range(W)], R.NewLeoRSCodec(),
                                     R.newErasuredNamespacedMerkleTreeConstructor(k, ns))
    with pytest.raises(R.RSMError) as e:
        eds.NamespaceProofs(bytes(ns), 0, [2])
    assert e.value.code == R.RSM_ETREE
    assert len(eds.NamespaceProofs(bytes(ns), 0, [1])) == 1
    plain = R.ImportExtendedDataSquare([sq[r, c].tobytes() for r in range(W) for c in range(W)], R.NewLeoRSCodec(),
                                       R.NewDefaultTree)
    with pytest.raises(R.RSMError) as e:
        plain.NamespaceProofs(bytes(ns))
    assert e.value.code == R.RSM_EUNSUPPORTED


def test_shares_cap_host(lib):
    """shares_cap below the total: the full total in offsets[n], exactly the vectors that fit."""
    k, ns = 4, 8
    W = 2 * k
    sq, eds = _square(k, ns, "single")
    nid = sq[0, 0, :ns].tobytes()
    p = eds._tree_fn.params
    keep, fn, user = R._tree_callback(eds._tree_fn)
    rb = H.record_bytes(W, ns)
    idx = (ctypes.c_uint32 * W)(*range(W))
    for cap in (0, k, 2 * k + 1, k * k):
        rec = ctypes.create_string_buffer(W * rb)
        offs = (ctypes.c_uint32 * (W + 1))()
        sh = ctypes.create_string_buffer(b"\xa5" * (k * k * S + S), k * k * S + S)
        R._check(lib.rsm_eds_namespace_proofs(eds._h, fn, user, 0, idx, W, nid, rec, offs, sh, cap))
        assert list(offs) == [min(i, k) * k for i in range(W + 1)]
        fit = cap // k  # rows 0 .. fit-1 end at or below the capacity
        want = b"".join(sq[r, c].tobytes() for r in range(min(fit, k)) for c in range(k))
        assert sh.raw[:len(want)] == want and set(sh.raw[len(want):]) == {0xA5}
