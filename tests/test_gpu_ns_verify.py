"""GPU: namespace proofs verified on the device (rsm_ns_proofs_verify_dev,
nmt_ns_verify_kernel in kernels_nmt.hip): one wave per query hashes the range's shares,
folds the range proof in its LDS and applies the completeness checks.  Every status word
is compared with the hashlib helper of tests/ns_proofs.py (expected_status) and with the
host verifier rsm_nmt_namespace_verify; every call's operands sit between guard bands and
only the status words may change."""
import ctypes
import functools

import numpy as np
import pytest

import nmt_classes as NC
import nmt_layouts as NL
import ns_proofs as H
import rsmt2d_amd as R
from device_calls import Guarded, device_proofs, expect
from ns_verify_calls import (S, Item, answers, compare, device_ns_statuses, host_status, namespace_data_cases, proved,
                             roots_table, with_variants)
from test_ns_proofs_cpu import header, hostile

pytestmark = pytest.mark.gpu


def layouts(ns):
    return ["runs", "carry", "max_tail", "near_max", "ladder:0"] + (["ladder:%d" % (ns - 1)] if ns > 1 else [])


# ---- 1. oracle parity ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def parity(k, ns, ig):
    """Every layout's square in one batch: the device prover's records and shares, the host
    prover's, and the hostile variants of every third query, in ONE verification call."""
    lib = R.library()
    W, p, names = 2 * k, R.NmtParams(ns, int(ig), k), layouts(ns)
    nsq, rb = len(names), H.record_bytes(2 * k, ns)
    batch = np.stack([NL.square(k, ns, S, name, 7) for name in names])
    queries, nids, records, shares = expect(lib, batch, k, ns, ig, H.vectors(k))
    rec, offs, sh, _, _ = device_proofs(lib, batch, k, ns, ig, S, queries, nids, total=sum(len(x) for x in shares))
    trees, items, musts = {}, [], []
    for i, (q, nid) in enumerate(zip(queries, nids)):
        s, axis, index = q
        if q not in trees:
            nxt = (index + 1) % W
            trees[q] = (H.Tree(H.vector_shares(batch[s], axis, index), index, k, ns, ig),
                        H.Tree(H.vector_shares(batch[s], axis, nxt), nxt, k, ns, ig).root)
        tree, other = trees[q]
        dev_sh = [sh[j * S:(j + 1) * S].tobytes() for j in range(int(offs[i]), int(offs[i + 1]))]
        items += [Item("device prover", q, nid, rec[i * rb:(i + 1) * rb], dev_sh, tree.root),
                  Item("host prover", q, nid, records[i], shares[i], tree.root)]
        musts += [H.OK, H.OK]
        if i % 3:
            continue
        for name, r2, sh2, root2, must in hostile(tree, W, ns, index, k, nid, H.prove_namespace(tree, nid), shares[i], other):
            # a root that is not the committed one comes from a second pseudo-square of the table
            items.append(Item(name, q if root2 == tree.root else (s + nsq, axis, index), nid, r2, sh2, root2))
            musts.append(must)
    got = compare(lib, items, musts, W, p, 2 * nsq)
    return {int.from_bytes(it.record[:4], "little") for it in items}, set(got)


@pytest.mark.parametrize("ig", [True, False])
@pytest.mark.parametrize("ns", [1, 8, 29])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 8])
def test_oracle_parity(lib, k, ns, ig):
    kinds, statuses = parity(k, ns, ig)
    assert H.OK in statuses and H.OCCUPIED not in statuses


def test_every_status_and_kind_occurs(lib):
    kinds, statuses = set(), set()
    for ig in (True, False):
        a, b = parity(4, 8, ig)
        kinds |= a
        statuses |= b
    assert {H.EMPTY, H.INCLUSION, H.ABSENCE} <= kinds
    assert statuses == {H.OK, H.MALFORMED, H.ORDER, H.ROOT, H.NAMESPACE, H.INCOMPLETE}


# ---- 2. composition on the device ---------------------------------------------------------
def test_prove_then_verify_on_device_buffers(lib):
    """rsm_proof_nodes_dev -> rsm_ns_proofs_dev -> rsm_ns_proofs_verify_dev with nothing
    between them but the stream: the prover's records, offsets and shares and the store
    build's roots are verified where they lie.  2,500 queries take the prover's offset scan
    (chunks of 1024 with a running carry) past its first chunk twice."""
    k, ns, ig, n = 4, 29, True, 2500
    W = 2 * k
    batch = NC.batch_of_three(k, ns)
    count = batch.shape[0]
    base = expect(lib, batch, k, ns, ig, [(a, i) for a in (0, 1) for i in range(W)])
    pick = [j % len(base[0]) for j in range(n)]
    queries, nids, records, shares = ([col[j] for j in pick] for col in base)
    lens = [len(x) for x in shares]
    cap = sum(lens)
    p = R.NmtParams(ns, int(ig), k)
    pp, ctx, rb, nl = ctypes.byref(p), R.device_context(0), H.record_bytes(W, ns), 2 * ns + 32
    d, nodes = R.DeviceBuffer(batch.size), R.DeviceBuffer(int(lib.rsm_proof_nodes_bytes(W, pp, count)))
    roots, tstat = R.DeviceBuffer(count * 2 * W * nl), R.DeviceBuffer(count * 2 * W * 4)
    recs, offs, shs, st = Guarded(n * rb, 3, 31), Guarded((n + 1) * 4, 4, 32), Guarded(cap * S, 0, 33), Guarded(n * 4, 4, 34)
    try:
        d.upload(batch.reshape(-1))
        arr = (R.NsQuery * n)(*[R.NsQuery(*q) for q in queries])
        flat = b"".join(nids)
        R._check(lib.rsm_proof_nodes_dev(ctx, d.ptr, W, S, count, pp, nodes.ptr, roots.ptr, tstat.ptr, None))
        R._check(lib.rsm_ns_proofs_dev(ctx, nodes.ptr, tstat.ptr, d.ptr, W, S, count, pp, arr, flat, n, recs.ptr, offs.ptr,
                                       shs.ptr, cap, None))
        R._check(lib.rsm_ns_proofs_verify_dev(ctx, recs.ptr, offs.ptr, shs.ptr, cap, roots.ptr, W, S, count, pp, arr, flat, n,
                                              st.ptr, None))
        R._check(lib.rsm_sync(ctx))
        got = st.result().view(np.uint32)
        assert list(offs.result().view(np.uint32)) == list(np.cumsum([0] + lens))
        assert recs.result().tobytes() == b"".join(records)
        assert shs.result().tobytes() == b"".join(b"".join(x) for x in shares)
    finally:
        for b in (d, nodes, roots, tstat, recs, offs, shs, st):
            b.free()
    failing = np.array([q in NC.FAILING for q in queries])
    assert failing.any() and list(got) == [H.MALFORMED if f else H.OK for f in failing]


# ---- 3. ranges longer than a wave, carried nodes ------------------------------------------
def sorted_vector(W, ns, bounds, seed):
    """W shares whose namespaces 00..01, 00..02, .. change at the positions `bounds`."""
    rng = np.random.default_rng([seed, W, ns])
    out, v = [], 1
    for pos in range(W):
        v += pos in bounds
        out.append(bytes(ns - 1) + bytes([v]) + rng.integers(0, 256, S - ns, dtype=np.uint8).tobytes())
    return out


@pytest.mark.parametrize("k", [35, 67])
def test_ranges_longer_than_a_wave(lib, k):
    ns, W = 29, 2 * k
    # (a) rows of a square, ignore_max off: a parity row asked for 0xFF.. (all W leaves, no
    # proof node), a quadrant-0 row of one namespace ([0, k): right nodes only), and the
    # namespace just above it (ABSENCE at position k, the first parity leaf)
    p = R.NmtParams(ns, 0, k)
    sq = NL.square(k, ns, S, "single", 50 + k)
    one = sq[0, 0, :ns].tobytes()
    cases = [proved(lib, p, "parity row", (0, 0, k + 1), H.vector_shares(sq, 0, k + 1), b"\xff" * ns),
             proved(lib, p, "single row", (0, 0, 2), H.vector_shares(sq, 0, 2), one),
             proved(lib, p, "absence at k", (0, 0, 3), H.vector_shares(sq, 0, 3), H._add(one, 1))]
    heads = [tuple(int.from_bytes(it.record[4 * i:4 * i + 4], "little") for i in range(4)) for it in cases]
    assert heads[0] == (H.INCLUSION, 0, W, 0) and heads[1][:3] == (H.INCLUSION, 0, k) and heads[2][:3] == (H.ABSENCE, k, k + 1)
    pairs = [v for it in cases for v in with_variants(lib, p, it, H.vector_shares(sq, 0, it.q[2]), W)]
    compare(lib, [it for it, _ in pairs], [m for _, m in pairs], W, p, 1)
    # (b) vectors whose every leaf carries its own namespace (square_size = W): ranges that
    # start or end at 63, 64 and 65
    p = R.NmtParams(ns, 1, W)
    pairs, ranges = [], set()
    for index, bounds in enumerate([(1, 63, 64, 65), (64,), (65,), (2, 63, 65)]):
        leaves = sorted_vector(W, ns, bounds, index)
        for v in range(1, len(bounds) + 2):
            it = proved(lib, p, "bounds %r" % (bounds,), (0, 1, index), leaves, bytes(ns - 1) + bytes([v]))
            ranges.add(tuple(int.from_bytes(it.record[4 * i:4 * i + 4], "little") for i in (1, 2)))
            pairs += with_variants(lib, p, it, leaves, W)
    assert {(1, 63), (63, 64), (64, 65), (65, W), (0, 64), (64, W), (0, 65), (63, 65), (2, 63)} <= ranges
    got = compare(lib, [it for it, _ in pairs], [m for _, m in pairs], W, p, 1)
    assert set(got) == {H.OK, H.ROOT, H.INCOMPLETE}


# ---- 4. any width -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 7, 11, 33])
def test_any_leaf_count(lib, n):
    """No tree is built, so the width need not be a square's: odd widths, and 1."""
    ns, k = 8, (n + 1) // 2
    p = R.NmtParams(ns, 0, k)
    rng = np.random.default_rng(n)
    leaves = sorted((bytes([0, 0, 0, 0, 0, 0, 0, int(x)]) + bytes(rng.integers(0, 256, S - ns, dtype=np.uint8))
                     for x in rng.integers(1, 6, n)), key=lambda s: s[:ns])
    tree = H.Tree(leaves, 0, k, ns, False)
    pairs = []
    for nid in H.query_namespaces(tree.names, ns):
        it = proved(lib, p, "n = %d" % n, (0, 0, 0), leaves, nid)
        assert it.root == tree.root and it.record == H.record_of(n, ns, *H.prove_namespace(tree, nid))
        pairs += with_variants(lib, p, it, leaves, n)
    got = compare(lib, [it for it, _ in pairs], [m for _, m in pairs], n, p, 1)
    assert H.OK in got and (n == 1 or H.ROOT in got)


# ---- 5. framing ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small():
    """k = 4, ns = 8 (W = 8): an inclusion of two shares, an absence and an empty proof."""
    lib = R.library()
    k, ns = 4, 8
    p = R.NmtParams(ns, 1, k)
    sq = NL.square(k, ns, S, "runs", 11)
    leaves = H.vector_shares(sq, 0, 0)
    assert [sh[ns - 1] for sh in leaves[:k]] == [1, 2, 2, 4]
    inc, absent, empty = (proved(lib, p, name, (0, 0, 0), leaves, bytes(ns - 1) + bytes([v]))
                          for name, v in (("inclusion", 2), ("absence", 3), ("empty", 0)))
    assert [int.from_bytes(it.record[:4], "little") for it in (inc, absent, empty)] == [H.INCLUSION, H.ABSENCE, H.EMPTY]
    return p, H.Tree(leaves, 0, k, ns, True), inc, absent, empty


def test_headers_tails_and_odd_record_addresses(lib):
    p, tree, inc, absent, empty = small()
    W, ns = 8, 8
    items, musts = [inc, absent, empty], [H.OK, H.OK, H.OK]
    for it in (inc, absent):
        for f in ("start", "end", "n_nodes"):
            items.append(it._replace(name=it.name + ", %s = 0xFFFFFFFF" % f, record=header(it.record, **{f: 0xFFFFFFFF})))
            musts.append(H.MALFORMED)
    for it in (inc, absent, empty):
        proof = H.prove_namespace(tree, it.nid)
        tail = [v for v in hostile(tree, W, ns, 0, 4, it.nid, proof, it.shares, tree.root) if v[0] == "non-zero tail"]
        assert len(tail) == 1 and tail[0][1] != it.record
        items.append(it._replace(name=it.name + ", non-zero tail", record=tail[0][1]))
        musts.append(H.OK)
    for skew in (2, 1):  # records at ptr + 2 and ptr + 1 of a 64-byte boundary
        compare(lib, items, musts, W, p, 1, rec_skew=skew)


def test_offsets_are_bounded(lib):
    p, tree, inc, absent, empty = small()
    roots = roots_table([inc], 1, 8, 48)
    # decreasing offsets: MALFORMED, and the neighbour with an empty range of its own is served
    got, _ = device_ns_statuses(lib, [empty, empty], 8, p, roots, offsets=[5, 3, 3], shares_total=8)
    assert list(got) == [H.MALFORMED, H.OK]
    # offsets past shares_total: the first query's two shares are all the buffer holds
    got, _ = device_ns_statuses(lib, [inc, inc], 8, p, roots, shares_total=3)
    assert list(got) == [H.OK, H.MALFORMED]
    got, _ = device_ns_statuses(lib, [inc, inc], 8, p, roots, shares_total=4)
    assert list(got) == [H.OK, H.OK]
    # a share count that is not the record's: MALFORMED as on the host
    got, _ = device_ns_statuses(lib, [inc, absent], 8, p, roots, offsets=[0, 1, 2], shares_total=2)
    assert list(got) == [H.MALFORMED, H.MALFORMED]
    assert host_status(lib, absent._replace(shares=inc.shares[:1]), 8, p) == H.MALFORMED


def test_nothing_is_written_for_no_queries(lib):
    p, tree, inc, absent, empty = small()
    roots = roots_table([inc], 1, 8, 48)
    for kw in ({"n": 0}, {"count": 0}):
        got, st = device_ns_statuses(lib, [inc, absent], 8, p, roots, **kw)
        assert np.array_equal(got.view(np.uint8), st.untouched(0, 8))


# ---- 6. arguments -------------------------------------------------------------------------
def test_arguments(lib):
    ctx = R.device_context(0)
    p = R.NmtParams(8, 1, 2)
    pp = ctypes.byref(p)
    buf = R.DeviceBuffer(1 << 16)
    q = (R.NsQuery * 1)(R.NsQuery(0, 0, 0))
    try:
        def call(nmt=pp, query=q, n=1, count=1, width=4, size=64, recs=buf.ptr, offs=buf.ptr, shs=buf.ptr, roots=buf.ptr,
                 st=buf.ptr, nids=bytes(8), c=ctx):
            return lib.rsm_ns_proofs_verify_dev(c, recs, offs, shs, 4, roots, width, size, count, nmt, query, nids, n, st, None)
        assert call(n=0) == 0 and call(count=0) == 0  # nothing launched
        for kw in ({"c": None}, {"recs": None}, {"offs": None}, {"shs": None}, {"roots": None}, {"st": None},
                   {"query": None}, {"nids": None}, {"width": 0}):
            assert call(**kw) == R.RSM_EINVAL, kw
        assert call(st=None, n=0) == 0
        assert call(shs=buf.ptr + 8) == R.RSM_EINVAL and call(offs=buf.ptr + 2) == R.RSM_EINVAL
        assert call(st=buf.ptr + 2) == R.RSM_EINVAL
        assert call(n=(1 << 20) + 1) == R.RSM_EINVAL
        for bad_ns in (0, 33):
            assert call(nmt=ctypes.byref(R.NmtParams(bad_ns, 1, 2))) == R.RSM_EINVAL
        for bad in (R.NsQuery(1, 0, 0), R.NsQuery(0, 2, 0), R.NsQuery(0, 0, 4)):
            assert call(query=(R.NsQuery * 1)(bad)) == R.RSM_EINVAL
        two = (R.NsQuery * 2)(R.NsQuery(0, 0, 0), R.NsQuery(0, 0, 9))
        assert call(query=two, n=2, nids=bytes(16)) == R.RSM_EINVAL
        assert b"query 1 " in lib.rsm_last_error()
        assert call(nmt=None) == R.RSM_EUNSUPPORTED
        assert call(width=1025) == R.RSM_EUNSUPPORTED
        assert call(nmt=ctypes.byref(R.NmtParams(32, 1, 2)), size=0) == R.RSM_ETREE
        assert call(size=96) == R.RSM_ESHARESIZE
    finally:
        buf.free()


# ---- verify_namespace_data ----------------------------------------------------------------
@pytest.mark.parametrize("ns", [8, 29])
def test_verify_namespace_data_paths_agree(lib, ns):
    """The client side of NamespaceData: one device call gives what NamespaceProof.verify
    gives row by row, for the honest answer and the dishonest ones."""
    seen = set()
    for case in namespace_data_cases(4, ns):
        for name, data, want in answers(case):
            dev = R.verify_namespace_data(case.roots, case.nid, data, case.p, 8)
            host = R.verify_namespace_data(case.roots, case.nid, data, case.p, 8, device=None)
            assert dev == host == want, (ns, case.what, name, dev, host, want)
            seen |= set(dev)
    assert seen == {H.OK, H.NAMESPACE, H.INCOMPLETE}
