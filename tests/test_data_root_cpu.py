"""CPU: the data root through the host restatements (merkle.cpp rsm_data_root /
rsm_data_root_prove / rsm_data_root_verify / rsm_sample_verify_data_root) and the
context-free path of rsm_eds_data_root, against tests/data_root.py -- RFC 6962's recursive
split in hashlib, itself pinned here to the RFC's published vectors."""
import ctypes

import numpy as np
import pytest

import rsmt2d_amd as R
import data_root as DR
import proof_status as P
import proof_verify as V

WIDTHS = [1, 2, 3, 6, 17, 34, 130]
# 1 + root_len message bytes: 55 is the last that fits one block; 57 and 63 need a second
# block of padding only; 65 and more put data into the second block
ROOT_LENS = [32, 34, 54, 56, 62, 64, 90, 96]


def test_helper_reproduces_the_rfc6962_vectors():
    """The test vectors published for RFC 6962 §2.1 (certificate-transparency's
    merkle tree tests): roots over the first n of eight fixed leaves."""
    leaves = [bytes.fromhex(x) for x in ("", "00", "10", "2021", "3031", "40414243", "5051525354555657",
                                         "606162636465666768696a6b6c6d6e6f")]
    want = {1: "6e340b9cffb37a989ca544e6bb780a2c78901d3fb33738768511a30617afa01d",
            2: "fac54203e7cc696cf0dfcb42c92a1d9dbaf70ad9e621f4bd8d98662f00e3c125",
            3: "aeb6bcfe274b70a14fb067a5e5578264db0fa9b51af5e0ba159158f329e06e77",
            5: "4e3bbb1f7b478dcfe71fb631631519a3bca12c9aefca1612bfce4c13a86264d4",
            7: "ddb89be403809e325750d3d263cd78929c2942b7942a34b77e122c9594a74c8c",
            8: "5dc9da79a70659a9ad559cb701ded9a2ab9d823aad2f4960cfe370eff4604328"}
    for n, root in want.items():
        assert DR.mth(leaves[:n]).hex() == root, n
        for m in range(n):  # every path folds back to the root, with the sides the split gives
            aunts = DR.path(m, leaves[:n])
            assert len(aunts) == DR.shape(m, n)[0]
            assert DR.root_from_path(DR.leaf_hash(leaves[m]), m, n, aunts).hex() == root, (n, m)


def test_helper_shape_is_the_level_picture():
    """The recursive split and the level picture give one record header, for every leaf of
    every leaf count the tests use (an even count: 2 * width) and the odd ones between."""
    for n in list(range(1, 70)) + [260]:
        for m in range(n):
            assert DR.shape(m, n) == P.proof_shape(n, m), (n, m)


def rand_roots(width, root_len, seed):
    g = np.random.default_rng([0xDA7A, width, root_len, seed])
    return [g.integers(0, 256, root_len, dtype=np.uint8).tobytes() for _ in range(2 * width)]


def host_data_root(lib, roots, width):
    out = ctypes.create_string_buffer(32)
    assert lib.rsm_data_root(b"".join(roots), width, len(roots[0]), out) == 0
    return out.raw


def host_root_record(lib, roots, width, axis, index):
    rec = ctypes.create_string_buffer(int(lib.rsm_data_root_record_bytes(width)))
    assert lib.rsm_data_root_prove(b"".join(roots), width, len(roots[0]), axis, index, rec) == 0
    return rec.raw


def host_root_status(lib, it, width):
    st = ctypes.c_uint32(0xDEAD)
    rc = lib.rsm_data_root_verify(it.root_bytes, len(it.root_bytes), width, it.axis, it.index, it.record, it.data_root,
                                  ctypes.byref(st))
    return rc, st.value


@pytest.mark.parametrize("width", WIDTHS)
def test_host_data_root_and_proofs(lib, width):
    assert int(lib.rsm_data_root_record_bytes(width)) == DR.record_bytes(width)
    for root_len in ROOT_LENS:
        roots = rand_roots(width, root_len, 1)
        want = DR.mth(roots)
        assert host_data_root(lib, roots, width) == want, root_len
        for axis in (0, 1):
            for index in range(width):
                rec = host_root_record(lib, roots, width, axis, index)
                assert rec == DR.record_of(roots, width, axis, index), (root_len, axis, index)
                it = DR.RootItem("valid", roots[axis * width + index], rec, want, axis, index)
                assert host_root_status(lib, it, width) == (0, DR.OK), (root_len, axis, index)


@pytest.mark.parametrize("width", WIDTHS)
def test_host_root_verify_hostile_variants(lib, width):
    seen = set()
    for root_len in (32, 90):
        roots, other = rand_roots(width, root_len, 2), DR.mth(rand_roots(width, root_len, 3))
        dr = DR.mth(roots)
        picks = sorted({(a, i) for a in (0, 1) for i in (0, width // 2, width - 1)})
        for axis, index in picks:
            rec = DR.record_of(roots, width, axis, index)
            base = None
            for it in DR.root_mutations(roots[axis * width + index], rec, dr, width, axis, index, other):
                want = DR.root_status(it.root_bytes, it.record, it.data_root, width, it.axis, it.index)
                assert host_root_status(lib, it, width) == (0, want), (root_len, axis, index, it.label)
                if it.label == "valid":
                    base = want
                if it.label == "non-zero tail":
                    assert want == base == DR.OK
                seen.add(want)
    assert seen == {DR.OK, DR.MALFORMED, DR.ROOT}


def test_argument_errors(lib):
    roots = b"".join(rand_roots(2, 32, 4))
    out = ctypes.create_string_buffer(32)
    rec = ctypes.create_string_buffer(DR.record_bytes(2))
    st = ctypes.c_uint32(0)
    assert int(lib.rsm_data_root_record_bytes(0)) == 0
    assert lib.rsm_data_root(roots, 0, 32, out) == R.RSM_EINVAL
    assert lib.rsm_data_root(roots, 2, 0, out) == R.RSM_EINVAL
    assert lib.rsm_data_root(roots, 2, 97, out) == R.RSM_EINVAL
    assert lib.rsm_data_root_prove(roots, 2, 32, 2, 0, rec) == R.RSM_EINVAL
    assert lib.rsm_data_root_prove(roots, 2, 32, 0, 2, rec) == R.RSM_EINVAL
    assert lib.rsm_data_root_verify(roots, 32, 2, 0, 2, rec, out, ctypes.byref(st)) == R.RSM_EINVAL
    # the device calls check their arguments before they touch a device
    assert int(lib.rsm_data_root_nodes_bytes(2049, 1)) == 0 and int(lib.rsm_data_root_nodes_bytes(0, 1)) == 0
    assert int(lib.rsm_data_root_nodes_bytes(1, 3)) == 3 * (2 + 1) * 32
    assert int(lib.rsm_data_root_nodes_bytes(3, 1)) == (6 + 3 + 2 + 1) * 32


TREES = [("default", 0), ("nmt", 29), ("nmt", 12)]


def squares_for(k, tree, ns, seed, count=2, S=64):
    p = R.NmtParams(ns, 1, k) if tree == "nmt" else None
    batch = np.stack([V.sorted_q0_square(k, S, max(ns, 8), seed + q) for q in range(count)])
    assert ns == 0 or batch[:, :k, :k, :ns].any(axis=-1).all()  # non-zero quadrant-0 namespaces
    return p, DR.Chain(P.Squares(batch, p))


def host_chain_status(lib, p, W, it):
    st = ctypes.c_uint32(0xDEAD)
    sm = R.Sample(*it.sample)
    rc = lib.rsm_sample_verify_data_root(ctypes.byref(p) if p is not None else None, W, ctypes.byref(sm), it.share,
                                         len(it.share), it.record, it.root_record, it.data_root, ctypes.byref(st))
    return rc, st.value


@pytest.mark.parametrize("tree,ns", TREES)
@pytest.mark.parametrize("k", [2, 3])
def test_host_chained_verifier(lib, k, tree, ns):
    p, ch = squares_for(k, tree, ns, 100 * k + ns)
    W = 2 * k
    samples = [(q, a, i, pos) for q in range(2) for a in (0, 1) for i in range(W) for pos in range(W)]
    for s in samples:  # the data roots the chain was built under are the library's
        assert host_chain_status(lib, p, W, ch.valid(s)) == (0, DR.OK), s
    for q in range(2):
        assert host_data_root(lib, ch.roots[q], W) == ch.data_roots[q]
    items = ch.items(samples)
    want = ch.expect(items)
    assert {DR.OK, DR.MALFORMED, DR.ROOT} | ({DR.ORDER} if ns else set()) == set(want)
    for it, w in zip(items, want):
        assert host_chain_status(lib, p, W, it) == (0, w), (it.sample, it.label, w)


@pytest.mark.parametrize("tree,ns", TREES)
def test_eds_data_root_without_a_context(lib, tree, ns):
    """An imported square has no context: the host trees, then the host data root.  (A
    seeded complete square with a namespace-sorted quadrant 0: a tree test needs no valid
    extension.)"""
    k, S = 3, 64
    ctor = R.NewDefaultTree if tree == "default" else R.newErasuredNamespacedMerkleTreeConstructor(k, ns)
    cells = [c.tobytes() for row in V.sorted_q0_square(k, S, max(ns, 8), 78 + ns) for c in row]
    eds = R.ImportExtendedDataSquare(cells, R.NewLeoRSCodec(), ctor)
    roots = eds.RowRoots() + eds.ColRoots()
    assert len(roots[0]) == (32 if tree == "default" else 2 * ns + 32)
    assert eds.DataRoot() == DR.mth(roots)
    for axis in (0, 1):
        for index in range(2 * k):
            pr = eds.RootProof(axis, index)
            assert pr.record() == DR.record_of(roots, 2 * k, axis, index)
            assert pr.verify(roots[axis * 2 * k + index], eds.DataRoot()) == DR.OK
            assert pr.verify(roots[axis * 2 * k + index], bytes(32)) == DR.ROOT
