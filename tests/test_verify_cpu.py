"""CPU: proof verification through the host restatements (merkle.cpp
rsm_default_tree_verify / rsm_nmt_tree_verify) and the context-free path of
rsm_eds_import_samples, against tests/proof_status.py: valid proofs built by levels in
Python and every hostile variant of them, status word for status word."""
import ctypes

import numpy as np
import pytest

import rsmt2d_amd as R
from oracle import crossword, nmt
import proof_status as P
import proof_verify as V

S = 64
TREES = [("default", 0, 1), ("nmt", 8, 0), ("nmt", 8, 1), ("nmt", 29, 0), ("nmt", 29, 1)]


def params(tree, ns, ig, k):
    return R.NmtParams(ns, ig, k) if tree == "nmt" else None


def host_status(lib, p, index, share, W, pos, record, root):
    st = ctypes.c_uint32(0xDEAD)
    if p is None:
        rc = lib.rsm_default_tree_verify(share, len(share), W, pos, record, root, ctypes.byref(st))
    else:
        rc = lib.rsm_nmt_tree_verify(ctypes.byref(p), index, share, len(share), W, pos, record, root, ctypes.byref(st))
    return rc, st.value


def vector_of(n, ns, seed):
    """n shares whose first (n + 1) // 2 -- the quadrant-0 part -- are in namespace order
    and have non-zero namespaces."""
    rng = np.random.default_rng(seed)
    sh = [rng.integers(0, 256, S, dtype=np.uint8).tobytes() for _ in range(n)]
    k = (n + 1) // 2
    head = sorted(sh[:k], key=lambda s: s[:max(ns, 1)])
    assert ns == 0 or all(any(s[:ns]) for s in head)
    return head + sh[k:]


@pytest.mark.parametrize("tree,ns,ig", TREES)
def test_host_verify_every_leaf_and_mutation(lib, tree, ns, ig):
    items, Ws, ps = [], [], []
    for n in range(1, 34):
        k = (n + 1) // 2
        p = params(tree, ns, ig, k)
        for index in ((0, k) if p is not None else (0,)):
            vecs = [vector_of(n, ns, 1000 * n + 7 * ns + v) for v in range(3)]
            lv = [P.tree_levels(v, index, p) for v in vecs]
            root = lv[0][-1][0]
            want = (crossword.merkle_root(vecs[0]) if p is None else
                    nmt.erasured_root(vecs[0], index, k, ns, bool(ig)))
            assert root == want  # the level picture is the reference's tree
            for pos in range(n):
                rec = P.record_of(lv[0], pos, p)
                for it in P.mutations(vecs[0][pos], rec, root, (0, 0, index, pos), n, p, lv[1][-1][0], lv[2][-1][0]):
                    items.append(it)
                    Ws.append(n)
                    ps.append(p)
    want = [P.expected_status(it.root, it.share, it.record, it.sample[3], it.sample[2], W, p)
            for it, W, p in zip(items, Ws, ps)]
    P.assert_covers(want, ps[-1])
    for it, W, p, w in zip(items, Ws, ps, want):
        rc, got = host_status(lib, p, it.sample[2], it.share, W, it.sample[3], it.record, it.root)
        assert rc == 0 and got == w, (W, it.sample, it.label, got, w)


@pytest.mark.parametrize("tree,ns,ig", TREES)
def test_prover_records_verify(lib, tree, ns, ig):
    """Records of rsm_default_tree_prove / rsm_nmt_tree_prove verify against the root
    those calls return, and are the records the Python levels give."""
    for n in (1, 2, 3, 7, 16, 33):
        k = (n + 1) // 2
        p = params(tree, ns, ig, k)
        leaves = vector_of(n, ns, 50 + n)
        keep, ptrs, _ = R._bufs(leaves)
        nl = P.node_len(p)
        lv = P.tree_levels(leaves, 0, p)
        for pos in range(n):
            rec = ctypes.create_string_buffer(V.record_bytes(n, nl))
            root = ctypes.create_string_buffer(nl)
            if p is None:
                rc = lib.rsm_default_tree_prove(ptrs, n, S, pos, rec, root)
            else:
                rc = lib.rsm_nmt_tree_prove(ctypes.byref(p), 0, ptrs, n, S, pos, rec, root)
            assert rc == 0 and rec.raw == P.record_of(lv, pos, p) and root.raw == lv[-1][0]
            assert host_status(lib, p, 0, leaves[pos], n, pos, rec.raw, root.raw) == (0, P.OK)
            if n > 1:  # the position is bound
                assert host_status(lib, p, 0, leaves[pos], n, (pos + 1) % n, rec.raw, root.raw)[1] != P.OK


def test_host_verify_argument_errors(lib):
    share, rec, root = bytes(S), bytes(8 + 2 * 32), bytes(32)
    st = ctypes.c_uint32()
    assert lib.rsm_default_tree_verify(share, S, 4, 4, rec, root, ctypes.byref(st)) == R.RSM_EINVAL
    assert lib.rsm_default_tree_verify(share, S, 0, 0, rec, root, ctypes.byref(st)) == R.RSM_EINVAL
    assert lib.rsm_default_tree_verify(share, S, 4, 0, rec, root, None) == R.RSM_EINVAL
    p = R.NmtParams(8, 1, 2)
    nrec, nroot = bytes(8 + 2 * 48), bytes(48)
    assert lib.rsm_nmt_tree_verify(ctypes.byref(p), 0, share, S, 4, 4, nrec, nroot, ctypes.byref(st)) == R.RSM_EINVAL
    assert lib.rsm_nmt_tree_verify(None, 0, share, S, 4, 0, nrec, nroot, ctypes.byref(st)) == R.RSM_EINVAL
    assert lib.rsm_nmt_tree_verify(ctypes.byref(p), 0, share, 4, 4, 0, nrec, nroot, ctypes.byref(st)) == R.RSM_ETREE
    zero = R.NmtParams(0, 1, 2)
    assert lib.rsm_nmt_tree_verify(ctypes.byref(zero), 0, share, S, 4, 0, nrec, nroot, ctypes.byref(st)) == R.RSM_EINVAL


def import_samples(lib, eds, tree_fn, row_roots, col_roots, items):
    """rsm_eds_import_samples over Items (sample square 0): (rc, statuses, accepted)."""
    n = len(items)
    keep, fn, user = R._tree_callback(tree_fn)
    arr = (R.Sample * max(n, 1))(*[R.Sample(*it.sample) for it in items])
    status = (ctypes.c_uint32 * max(n, 1))(*([0xDEAD] * max(n, 1)))
    acc = ctypes.c_uint32(0xDEAD)
    rc = lib.rsm_eds_import_samples(eds._h, b"".join(row_roots), b"".join(col_roots), len(row_roots[0]), fn, user, arr,
                                    n, b"".join(it.share for it in items), b"".join(it.record for it in items), status,
                                    ctypes.byref(acc))
    return rc, [int(status[i]) for i in range(n)], acc.value


def import_case(tree, seed):
    """A k = 4 square, its roots, and a batch of samples to import: every cell of
    quadrant 0 by row proofs and a diagonal by column proofs, hostile variants of some,
    duplicates; cell (1, 2) is set beforehand."""
    k, ns = 4, 8
    W = 2 * k
    p = R.NmtParams(ns, 1, k) if tree == "nmt" else None
    sq = P.Squares(V.sorted_q0_square(k, S, ns, seed)[None], p)
    rr = [sq.root(0, 0, i) for i in range(W)]
    cr = [sq.root(0, 1, i) for i in range(W)]
    items = []
    for s in [(0, 0, r, c) for r in range(k) for c in range(k)] + [(0, 1, i, i) for i in range(W)] + [(0, 0, 6, 7)]:
        muts = list(P.mutations(sq.share(s), sq.record(s), sq.root(*s[:3]), s, W, p))
        root_ok = [m for m in muts if m.root == sq.root(*m.sample[:3])]  # the call takes the committed roots
        # hostile variants first, so that none of them may claim the cell
        items += [m for m in root_ok if m.label != "valid"][(s[2] + s[3]) % 3::3]
        items.append(root_ok[0])
    items += [it for it in items if it.label == "valid"][::5]  # duplicates of cells set earlier in the batch
    return k, ns, W, p, sq, rr, cr, items


def apply_in_order(items, want, W, preset):
    """The statuses and cells rsm_eds_import_samples must leave: verified samples are
    applied in order, a verified sample of a non-nil cell reports OCCUPIED."""
    cells, out = dict(preset), []
    for it, w in zip(items, want):
        _q, axis, index, pos = it.sample
        rc = (index, pos) if axis == 0 else (pos, index)
        if w == P.OK:
            if rc in cells:
                w = P.OCCUPIED
            else:
                cells[rc] = it.share
        out.append(w)
    return out, cells


@pytest.mark.parametrize("tree", ["default", "nmt"])
def test_import_samples_context_free(lib, tree):
    k, ns, W, p, sq, rr, cr, items = import_case(tree, 31)
    tree_fn = R.NewDefaultTree if p is None else R.newErasuredNamespacedMerkleTreeConstructor(k, ns)
    eds = R.NewExtendedDataSquare(R.NewLeoRSCodec(), tree_fn, W, S)  # no context: the host restatement
    preset = {(1, 2): sq.share((0, 0, 1, 2))}
    eds.SetCell(1, 2, preset[(1, 2)])
    want, cells = apply_in_order(items, P.expect(items, W, p), W, preset)
    P.assert_covers(want, p)
    assert P.OCCUPIED in want and want.count(P.OCCUPIED) >= 2  # the preset cell and the duplicates
    rc, got, accepted = import_samples(lib, eds, tree_fn, rr, cr, items)
    assert rc == 0 and got == want
    assert accepted == want.count(P.OK) == len(cells) - 1
    flat = eds.Flattened()
    assert flat == [cells.get((r, c)) for r in range(W) for c in range(W)]  # rejected cells stay nil
    # the Python mirror on a fresh square gives the same
    eds2 = R.NewExtendedDataSquare(R.NewLeoRSCodec(), tree_fn, W, S)
    eds2.SetCell(1, 2, preset[(1, 2)])
    valid = [it for it in items if it.label == "valid"]
    prs = []
    for it in valid:
        nodes, mask = V.parse_record(it.record, P.node_len(p))
        pr = R.Proof(it.share, nodes, mask, it.sample[3], W, p, it.sample[2])
        assert pr.record() == it.record  # the inverse of _parse_records
        prs.append((it.sample[1], it.sample[2], it.sample[3], pr))
    st2 = eds2.SetCellsVerified(rr, cr, prs, device=False)
    want2, cells2 = apply_in_order(valid, [P.OK] * len(valid), W, preset)
    assert st2 == want2 and eds2.Flattened() == [cells2.get((r, c)) for r in range(W) for c in range(W)]


def test_import_samples_errors(lib):
    k, ns, W, p, sq, rr, cr, items = import_case("default", 5)
    eds = R.NewExtendedDataSquare(R.NewLeoRSCodec(), R.NewDefaultTree, W, S)
    it = items[0]
    for s in [(1, 0, 0, 0), (0, 2, 0, 0), (0, 0, W, 0), (0, 1, 0, W)]:  # square must be 0
        rc, _, _ = import_samples(lib, eds, R.NewDefaultTree, rr, cr, [it, it._replace(sample=s)])
        assert rc == R.RSM_EINVAL and b"sample 1" in lib.rsm_last_error()
    assert eds.Flattened() == [None] * (W * W)  # nothing was written
    rc, _, _ = import_samples(lib, eds, lambda axis, index: None, rr, cr, [it])
    assert rc == R.RSM_EUNSUPPORTED
    rc, _, _ = import_samples(lib, eds, R.NewDefaultTree, [r + b"\0" for r in rr], [c + b"\0" for c in cr], [it])
    assert rc == R.RSM_EINVAL  # roots of another tree's length
    rc, got, acc = import_samples(lib, eds, R.NewDefaultTree, rr, cr, [])
    assert rc == 0 and acc == 0
