"""GPU: range proofs on the device -- rsm_range_proofs_dev (the prover out of a node store),
rsm_range_proofs_verify_dev and rsm_range_proofs_verify_data_root_dev (one wave per query:
nmt_range_verify_kernel in kernels_nmt.hip, range_verify_kernel in kernels_sha.hip).  Every
record, offset, share and status word is compared with the recursive hashlib model of
tests/range_proofs.py and with the host restatements; every operand sits between guard
bands and only the outputs may change.  ns == 0 stands for the DefaultTree."""
import functools

import numpy as np
import pytest

import data_root as D
import ns_proofs as H
import range_proofs as M
import rsmt2d_amd as R
from device_calls import Guarded, device_proofs
from range_calls import data_root_tree, device_prove, device_statuses, host_prove, host_status, params, pref, square_roots
from test_range_proofs_cpu import TREES, hostile_cases

pytestmark = pytest.mark.gpu
S = 64


def batch_of(k, ns, S=S, count=3):
    return np.stack([M.square(k, ns, S, 100 + s) for s in range(count)])


@functools.lru_cache(maxsize=None)
def every_range(k, ns):
    """Every range of every vector of a batch of three squares: (batch, queries, the model's
    records, share lists, trees by (square, axis, index))."""
    W, batch = 2 * k, batch_of(k, ns)
    queries, records, shares, trees = [], [], [], {}
    for s in range(3):
        rows, cols = square_roots(batch[s], k, ns)
        for axis, ts in ((0, rows), (1, cols)):
            for index, tree in enumerate(ts):
                trees[s, axis, index] = tree
                leaves = H.vector_shares(batch[s], axis, index)
                for start, end in M.all_ranges(W):
                    queries.append((s, axis, index, start, end))
                    records.append(M.prove(tree, ns, start, end))
                    shares.append(leaves[start:end])
    return batch, queries, records, shares, trees


# ---- 1. the prover --------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [0, 1, 8, 29])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_prover_parity(lib, k, ns):
    batch, queries, records, shares, trees = every_range(k, ns)
    rec, offs, sh, roots = device_prove(lib, params(k, ns), batch, S, queries)
    rb = M.record_bytes(2 * k, ns)
    assert list(offs) == list(np.cumsum([0] + [len(x) for x in shares]))
    for i, want in enumerate(records):
        assert rec[i * rb:(i + 1) * rb] == want, queries[i]
    assert sh == b"".join(b"".join(x) for x in shares)
    for (s, a, i), tree in trees.items():
        assert roots[s, a, i].tobytes() == tree.root


@pytest.mark.parametrize("ns", [1, 8, 29])
def test_a_namespaces_range_gives_the_namespace_proofs_record(lib, ns):
    """For a range that is exactly a namespace's range the record is byte-identical to the
    one rsm_ns_proofs_dev writes."""
    k, ig = 4, False  # ignore_max off: 0xFF.. of a quadrant-0 row is a namespace like another
    W, batch = 2 * k, batch_of(k, ns, count=1)
    asked = []  # (query, nid, start, end)
    for axis in (0, 1):
        for index in (0, k - 1, k, W - 1):
            names = [H.wrapper_ns(sh, p, index, k, ns) for p, sh in enumerate(H.vector_shares(batch[0], axis, index))]
            for nid in sorted(set(names)):
                asked.append(((0, axis, index), nid, names.index(nid), W - names[::-1].index(nid)))
    nrec, noffs, _, _, _ = device_proofs(lib, batch, k, ns, ig, S, [a[0] for a in asked], [a[1] for a in asked],
                                        total=sum(a[3] - a[2] for a in asked))
    rrec, roffs, _, _ = device_prove(lib, R.NmtParams(ns, int(ig), k), batch, S, [a[0] + (a[2], a[3]) for a in asked])
    assert nrec == rrec and list(noffs) == list(roffs)
    assert {a[3] - a[2] for a in asked} >= {1, k, W}


def test_prover_share_capacity(lib):
    """Shares are written only where d_offsets[i + 1] <= shares_cap; nothing lands past it."""
    k, ns = 2, 8
    batch = batch_of(k, ns, count=1)
    queries = [(0, 0, 0, 0, 3), (0, 1, 2, 1, 4), (0, 0, 3, 0, 4)]
    rec, offs, sh, _ = device_prove(lib, params(k, ns), batch, S, queries, cap=6)
    assert list(offs) == [0, 3, 6, 10]
    want = b"".join(H.vector_shares(batch[0], 0, 0)[0:3] + H.vector_shares(batch[0], 1, 2)[1:4])
    assert sh[:6 * S] == want


# ---- 2. the verifiers -----------------------------------------------------------------------
def check(lib, p, W, S, cases, **kw):
    """Device == host == model, status for status."""
    got = device_statuses(lib, p, W, S, cases, **kw)
    for c, g in zip(cases, got):
        assert g == c.must, (c.name, c.index, c.start, c.end, g, c.must)
        assert host_status(lib, p, W, c, S) == c.must, c.name
    return set(got)


@pytest.mark.parametrize("ns,ig", TREES)
def test_verifier_parity_and_hostile_set(lib, ns, ig):
    k = 4
    W, p = 2 * k, params(k, ns, ig)
    cases = hostile_cases(k, ns, ig)
    M.named_musts(cases)
    # the device prover's and the host prover's records of every valid one
    sq = M.square(k, ns, S, 3)
    valid = [c for c in cases if c.name == "valid"]
    rec, offs, sh, _ = device_prove(lib, p, sq[None], S, [(0, 0, c.index, c.start, c.end) for c in valid])
    rb = M.record_bytes(W, ns)
    for i, c in enumerate(valid):
        dev_sh = [sh[j * S:(j + 1) * S] for j in range(int(offs[i]), int(offs[i + 1]))]
        cases.append(c._replace(name="device prover", record=rec[i * rb:(i + 1) * rb], shares=dev_sh))
        rc, hrec, _ = host_prove(lib, p, c.index, H.vector_shares(sq, 0, c.index), c.start, c.end)
        assert rc == 0
        cases.append(c._replace(name="host prover", record=hrec))
    seen = check(lib, p, W, S, cases)
    assert seen == ({M.OK, M.MALFORMED, M.ORDER, M.ROOT} if ns else {M.OK, M.MALFORMED, M.ROOT})


def vector_cases(W, ns, ig, k, index, ranges, S=S, seed=0, hostile=True):
    leaves = M.vector(W, ns, S, k if index < k else 0, seed)
    tree = M.tree_of(leaves, index, k, ns, ig)
    nxt = (index + 1) % W
    next_root = M.tree_of(M.vector(W, ns, S, k if nxt < k else 0, seed + 1), nxt, k, ns, ig).root
    out = []
    for start, end in ranges:
        if hostile and W > 1:
            out += M.hostile(tree, W, ns, ig, index, k, start, end, leaves[start:end], next_root)
        else:
            out.append(M.Case("valid", index, start, end, M.prove(tree, ns, start, end), leaves[start:end], tree.root, M.OK))
    return out


@pytest.mark.parametrize("ns,ig", [(0, True), (8, True), (29, True), (29, False)])
@pytest.mark.parametrize("W", [1, 3, 5, 7, 33, 131])
def test_verify_only_widths(lib, W, ns, ig):
    """Odd widths, which the prover's node store cannot hold: host-proved records.  W = 131:
    ranges of 1, 63, 64, 65 and 129 shares (three leaf passes of a wave), one of them
    crossing square_size in a quadrant-0 vector."""
    k = (W + 1) // 2
    if W <= 7:
        ranges = M.all_ranges(W)
    elif W == 33:
        ranges = [(0, 1), (32, 33), (0, 33), (5, 30), (16, 17), (15, 18), (1, 32)]
    else:
        ranges = [(77, 78), (130, 131), (3, 66), (64, 128), (31, 96), (1, 130), (k - 2, k + 3)]
        assert sorted(e - s for s, e in ranges)[:6] == [1, 1, 5, 63, 64, 65] and (1, 130) in ranges
    cases = []
    for index in (0, W - 1):
        cases += vector_cases(W, ns, ig, k, index, ranges, seed=W + index, hostile=W <= 7 or index == 0)
    M.named_musts(cases)
    p = params(k, ns, ig)
    for c in cases:
        if c.name == "valid":
            assert host_prove(lib, p, c.index, M.vector(W, ns, S, k if c.index < k else 0, W + c.index), c.start, c.end)[1] == c.record
    assert M.OK in check(lib, p, W, S, cases)


@pytest.mark.parametrize("ns", [0, 29, 8])
@pytest.mark.parametrize("share", [128, 512])
def test_share_sizes(lib, share, ns):
    k, W = 4, 8
    cases = vector_cases(W, ns, True, k, 1, [(1, 7), (3, 4)], S=share, seed=share)
    assert check(lib, params(k, ns), W, share, cases) >= {M.OK, M.MALFORMED, M.ROOT}


@pytest.mark.parametrize("ns,W", [(32, 1024), (0, 2048)])
def test_width_limits(lib, ns, W):
    """The LDS limits: the full range, a one-leaf range at both ends and a middle range."""
    k = W // 2
    ranges = [(0, W), (0, 1), (W - 1, W), (W // 3, W // 3 + 200)]
    cases = vector_cases(W, ns, True, k, 0, ranges, seed=9, hostile=False)
    cases += vector_cases(W, ns, True, k, W - 1, ranges[:2], seed=10, hostile=False)
    sh0 = cases[3].shares[0]
    flipped = cases[3]._replace(name="share bit", shares=[sh0[:-1] + bytes([sh0[-1] ^ 1])] + cases[3].shares[1:], must=M.ROOT)
    cases.append(flipped)
    p = params(k, ns)
    got = device_statuses(lib, p, W, S, cases)
    assert got == [c.must for c in cases]
    ctx = R.device_context(0)
    q = (R.RangeQuery * 1)(R.RangeQuery(0, 0, 0, 0, 1))
    for call, ops in ((lib.rsm_range_proofs_verify_dev, [4096]), (lib.rsm_range_proofs_verify_data_root_dev, [4096, 4096])):
        assert call(ctx, 4096, 4096, 4096, 1, *ops, W + 1, S, 1, pref(p), q, 1, 4096, None) == R.RSM_EUNSUPPORTED


def test_offsets_rule(lib):
    """Decreasing offsets and offsets past shares_total are MALFORMED before anything else
    of the query is read; the neighbours keep their own status."""
    k, W, ns = 4, 8, 8
    cases = vector_cases(W, ns, True, k, 0, [(0, 2), (1, 4), (2, 7)], hostile=False)
    p = params(k, ns)
    assert device_statuses(lib, p, W, S, cases) == [M.OK] * 3
    assert device_statuses(lib, p, W, S, cases, offsets=[0, 2, 1, 10]) == [M.OK, M.MALFORMED, M.MALFORMED]
    assert device_statuses(lib, p, W, S, cases, shares_total=9) == [M.OK, M.OK, M.MALFORMED]
    assert device_statuses(lib, p, W, S, cases, offsets=[0, 2, 5, 0xFFFFFFF0]) == [M.OK, M.OK, M.MALFORMED]
    plain = vector_cases(W, 0, True, k, 0, [(0, 2), (1, 4), (2, 7)], hostile=False)
    assert device_statuses(lib, None, W, S, plain, offsets=[7, 2, 5, 10]) == [M.MALFORMED, M.OK, M.OK]


# ---- 3. composition on the device -----------------------------------------------------------
@pytest.mark.parametrize("ns", [0, 29])
def test_prove_then_verify_on_device_buffers(lib, ns):
    """rsm_proof_nodes_dev -> rsm_range_proofs_dev -> rsm_range_proofs_verify_dev, and
    rsm_data_roots_dev -> rsm_root_proofs_dev -> rsm_range_proofs_verify_data_root_dev with
    no root table, with nothing between them but the stream.  2,500 queries take the offset
    scan (chunks of 1024 with a running carry) past its first chunk twice."""
    k, n = 4, 2500
    W, p = 2 * k, params(k, ns)
    batch, base_q, base_r, base_s, trees = every_range(k, ns)
    pick = [(7 * j) % len(base_q) for j in range(n)]
    queries, records, shares = [base_q[j] for j in pick], [base_r[j] for j in pick], [base_s[j] for j in pick]
    lens = [len(x) for x in shares]
    cap, count = sum(lens), batch.shape[0]
    ctx, rb, nl, rrb = R.device_context(0), M.record_bytes(W, ns), M.node_len(ns), D.record_bytes(W)
    plain = [R.DeviceBuffer(batch.size), R.DeviceBuffer(int(lib.rsm_proof_nodes_bytes(W, pref(p), count))),
             R.DeviceBuffer(count * 2 * W * nl), R.DeviceBuffer(int(lib.rsm_data_root_nodes_bytes(W, count)))]
    d, nodes, roots, dr_nodes = plain
    recs, offs, shs = Guarded(n * rb, 3, 61), Guarded((n + 1) * 4, 4, 62), Guarded(cap * S, 0, 63)
    st, st2, rrecs, drs = Guarded(n * 4, 4, 64), Guarded(n * 4, 4, 65), Guarded(n * rrb, 5, 66), Guarded(count * 32, 7, 67)
    try:
        d.upload(batch.reshape(-1))
        arr = (R.RangeQuery * n)(*[R.RangeQuery(*q) for q in queries])
        refs = (R.RootRef * n)(*[R.RootRef(*q[:3]) for q in queries])
        R._check(lib.rsm_proof_nodes_dev(ctx, d.ptr, W, S, count, pref(p), nodes.ptr, roots.ptr, None, None))
        R._check(lib.rsm_range_proofs_dev(ctx, nodes.ptr, d.ptr, W, S, count, pref(p), arr, n, recs.ptr, offs.ptr, shs.ptr, cap,
                                          None))
        R._check(lib.rsm_range_proofs_verify_dev(ctx, recs.ptr, offs.ptr, shs.ptr, cap, roots.ptr, W, S, count, pref(p), arr, n,
                                                 st.ptr, None))
        R._check(lib.rsm_data_roots_dev(ctx, roots.ptr, W, nl, count, drs.ptr, dr_nodes.ptr, None))
        R._check(lib.rsm_root_proofs_dev(ctx, dr_nodes.ptr, W, count, refs, n, rrecs.ptr, None))
        R._check(lib.rsm_range_proofs_verify_data_root_dev(ctx, recs.ptr, offs.ptr, shs.ptr, cap, rrecs.ptr, drs.ptr, W, S,
                                                           count, pref(p), arr, n, st2.ptr, None))
        R._check(lib.rsm_sync(ctx))
        assert list(offs.result().view(np.uint32)) == list(np.cumsum([0] + lens))
        assert recs.result().tobytes() == b"".join(records)
        assert shs.result().tobytes() == b"".join(b"".join(x) for x in shares)
        want_dr = b"".join(data_root_tree([trees[s, 0, i] for i in range(W)], [trees[s, 1, i] for i in range(W)]).root()
                           for s in range(count))
        assert drs.result().tobytes() == want_dr
        assert list(st.result().view(np.uint32)) == [M.OK] * n
        assert list(st2.result().view(np.uint32)) == [M.OK] * n
    finally:
        for b in plain + [recs, offs, shs, st, st2, rrecs, drs]:
            b.free()


# ---- 4. chained to the data root ------------------------------------------------------------
def chained_cases(k, ns, ig=True):
    """Valid and hostile range proofs of rows of one square, each with the row's root record,
    and some also with a root record whose node, whose header or whose index is wrong:
    (cases, root records, what is wrong with each root record, the model's chained statuses,
    the data root)."""
    W = 2 * k
    sq = M.square(k, ns, S, 3)
    rows, cols = square_roots(sq, k, ns, ig)
    drt = data_root_tree(rows, cols)
    dr = drt.root()
    cases, rrecs, wrong, musts = [], [], [], []
    for index in (0, k - 1, k, W - 1):
        leaves = H.vector_shares(sq, 0, index)
        good = D.record_of(drt, W, 0, index)
        variants = {"": good, "node": good[:8] + bytes([good[8] ^ 4]) + good[9:],
                    "header": (int.from_bytes(good[:4], "little") ^ 1).to_bytes(4, "little") + good[4:],
                    "index": D.record_of(drt, W, 0, (index + 1) % W)}
        for start, end in ((0, W), (1, 3), (k - 1, k + 1), (W - 1, W)):
            for c in M.hostile(rows[index], W, ns, ig, index, k, start, end, leaves[start:end], rows[(index + 1) % W].root):
                if c.name in ("asked of the next vector", "root bit"):
                    continue  # they change the root table's entry, which the chained form does not have
                with_bad = c.name in ("valid", "kind 2", "share bit", "first and last node swapped", "left node <- last leaf")
                for what, rrec in variants.items():
                    if what and not with_bad:
                        continue
                    cases.append(c)
                    rrecs.append(rrec)
                    wrong.append(what)
                    musts.append(M.chained_status(W, ns, ig, 0, c.index, k, c.start, c.end, c.shares, c.record, rrec, dr))
    return cases, rrecs, wrong, musts, dr


@pytest.mark.parametrize("ns,ig", [(0, True), (8, True), (8, False), (29, True)])
def test_chained_parity_and_precedence(lib, ns, ig):
    """A bad share-record header wins over a bad root-record header, which wins over
    ORDER / ROOT; a root record of another index is MALFORMED."""
    k = 4
    W = 2 * k
    cases, rrecs, wrong, musts, dr = chained_cases(k, ns, ig)
    got = device_statuses(lib, params(k, ns, ig), W, S, cases, chained=(b"".join(rrecs), dr * len(cases)))
    assert got == musts
    for c, what, g in zip(cases, wrong, got):
        if c.must == M.MALFORMED or what in ("header", "index"):
            assert g == M.MALFORMED, (c.name, what)
        elif c.must == M.ORDER:
            assert g == M.ORDER, (c.name, what)  # the range fold's, whatever the root record's nodes
        elif what == "node" or c.must == M.ROOT:
            assert g == M.ROOT, (c.name, what)
        else:
            assert g == M.OK, (c.name, what)
    assert {"valid", "kind 2"} <= {c.name for c, what in zip(cases, wrong) if what == "header"}
    assert set(got) == ({M.OK, M.MALFORMED, M.ORDER, M.ROOT} if ns else {M.OK, M.MALFORMED, M.ROOT})


@pytest.mark.parametrize("ns", [0, 29])
def test_share_proof_validates_against_the_data_root(lib, ns):
    """ShareProof(start, end).Validate(DataRoot()) for a three-row range at k = 4 -- a partial
    first row, a whole middle row, a partial last row -- and after one bit of one share, one
    node or one root-record node is flipped."""
    k, W, S2 = 4, 8, 64
    sq = M.square(k, ns, S2, 77)
    ods = [sq[r, c].tobytes() for r in range(k) for c in range(k)]
    ctor = R.newErasuredNamespacedMerkleTreeConstructor(k, ns) if ns else R.NewDefaultTree
    eds = R.ComputeExtendedDataSquare(ods, R.NewLeoRSCodec(), ctor)
    dr = eds.DataRoot()
    sp = eds.ShareProof(2, 11)
    assert [(pr.tree_index, pr.start, pr.end) for pr in sp.rows] == [(0, 2, 4), (1, 0, 4), (2, 0, 3)]
    assert sp.shares() == ods[2:11]
    for pr, root in zip(sp.rows, sp.row_roots):  # the device path's records are the model's
        tree = M.tree_of([eds.GetCell(pr.tree_index, c) for c in range(W)], pr.tree_index, k, ns)
        assert pr.record() == M.prove(tree, ns, pr.start, pr.end) and root == tree.root
    assert sp.Validate(dr) and sp.Validate(dr, device=None)
    assert sp.statuses(dr) == [M.OK] * 3

    def flipped(b, at=5):
        return b[:at] + bytes([b[at] ^ 0x10]) + b[at + 1:]

    def both(want):
        assert sp.statuses(dr) == want and sp.statuses(dr, device=None) == want and not sp.Validate(dr)

    keep = sp.rows[1].shares[3]
    sp.rows[1].shares[3] = flipped(keep, S2 - 1)
    both([M.OK, M.ROOT, M.OK])
    sp.rows[1].shares[3] = keep
    keep = sp.rows[2].nodes[0]
    sp.rows[2].nodes[0] = flipped(keep, len(keep) - 1)
    both([M.OK, M.OK, M.ROOT])
    sp.rows[2].nodes[0] = keep
    keep = sp.root_proofs[0].nodes[1]
    sp.root_proofs[0].nodes[1] = flipped(keep)
    both([M.ROOT, M.OK, M.OK])
    sp.root_proofs[0].nodes[1] = keep
    assert sp.Validate(dr)
    assert not sp.Validate(flipped(dr))


@pytest.mark.parametrize("ns", [0, 8])
def test_python_device_calls(lib, ns):
    """prove_ranges_dev / verify_ranges_dev / verify_ranges_data_root_dev over one square."""
    k, W = 2, 4
    sq = M.square(k, ns, S, 8)
    p = params(k, ns)
    queries = [(0, a, i, s, e) for a in (0, 1) for i in range(W) for s, e in ((0, 1), (1, 4), (0, 4))]
    rows, cols = square_roots(sq, k, ns)
    drt = data_root_tree(rows, cols)
    d = R.DeviceBuffer(sq.size)
    try:
        d.upload(sq.reshape(-1))
        proofs = R.prove_ranges_dev(d, W, S, queries, nmt=p)
    finally:
        d.free()
    trees = {0: rows, 1: cols}
    for q, pr in zip(queries, proofs):
        assert pr.record() == M.prove(trees[q[1]][q[2]], ns, q[3], q[4]) and pr.verify(trees[q[1]][q[2]].root) == M.OK
    recs = b"".join(pr.record() for pr in proofs)
    packed = b"".join(b"".join(pr.shares) for pr in proofs)
    offs = np.cumsum([0] + [len(pr.shares) for pr in proofs]).astype(np.uint32)
    roots = b"".join(t.root for t in rows + cols)
    rrecs = b"".join(D.record_of(drt, W, q[1], q[2]) for q in queries)
    bufs = [R.DeviceBuffer(len(x)) for x in (recs, offs.tobytes(), packed, roots, rrecs, bytes(32))]
    try:
        for b, x in zip(bufs, (recs, offs.tobytes(), packed, roots, rrecs, drt.root())):
            b.upload(np.frombuffer(x, np.uint8))
        total = len(packed) // S
        assert list(R.verify_ranges_dev(bufs[0], bufs[1], bufs[2], total, bufs[3], W, S, queries, nmt=p)) == [M.OK] * len(queries)
        assert list(R.verify_ranges_data_root_dev(bufs[0], bufs[1], bufs[2], total, bufs[4], bufs[5], W, S, queries,
                                                  nmt=p)) == [M.OK] * len(queries)
        moved = [(0, a, (i + 1) % W, s, e) for (_, a, i, s, e) in queries]
        assert M.OK not in set(R.verify_ranges_dev(bufs[0], bufs[1], bufs[2], total, bufs[3], W, S, moved, nmt=p))
    finally:
        for b in bufs:
            b.free()
