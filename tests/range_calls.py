"""TEST INFRASTRUCTURE ONLY -- the library calls the range proof tests share: the host
restatements (rsm_*_tree_range_prove / _verify) and the three device entry points with
their operands between guard bands (device_calls.Guarded).  ns == 0 is the DefaultTree, as
in tests/range_proofs.py.  Importing this module touches no GPU."""
import ctypes

import numpy as np

import data_root as D
import range_proofs as M
import rsmt2d_amd as R
from device_calls import Guarded


def params(k, ns, ig=True):
    return R.NmtParams(ns, int(ig), k) if ns else None


def pref(p):
    return ctypes.byref(p) if p is not None else None


def host_prove(lib, p, index, leaves, start, end):
    """(rc, record, root) of the host prover over the vector `leaves`."""
    keep, ptrs, _ = R._bufs(leaves)
    ns = p.namespace_size if p is not None else 0
    rec = ctypes.create_string_buffer(M.record_bytes(len(leaves), ns))
    root = ctypes.create_string_buffer(M.node_len(ns))
    if p is None:
        rc = lib.rsm_default_tree_range_prove(ptrs, len(leaves), len(leaves[0]), start, end, rec, root)
    else:
        rc = lib.rsm_nmt_tree_range_prove(ctypes.byref(p), index, ptrs, len(leaves), len(leaves[0]), start, end, rec, root)
    return rc, rec.raw, root.raw


def host_status(lib, p, W, case, S):
    """The host verifier's status word for a range_proofs.Case."""
    st = ctypes.c_uint32(99)
    flat = b"".join(case.shares)
    if p is None:
        rc = lib.rsm_default_tree_range_verify(case.start, case.end, flat, len(case.shares), S, W, case.record, case.root,
                                               ctypes.byref(st))
    else:
        rc = lib.rsm_nmt_tree_range_verify(ctypes.byref(p), case.index, case.start, case.end, flat, len(case.shares), S, W,
                                           case.record, case.root, ctypes.byref(st))
    assert rc == 0, (case.name, rc)
    return int(st.value)


def fill(g, data):
    """Puts `data` into the operand of a Guarded buffer."""
    a = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else np.asarray(data).view(np.uint8).reshape(-1)
    assert len(a) <= g.n
    g.sent[g.front:g.front + len(a)] = a
    g.buf.upload(g.sent)


def device_statuses(lib, p, W, S, cases, axis=0, offsets=None, shares_total=None, chained=None):
    """One verify call over `cases` (query i = square i's vector (axis, case.index), so every
    case has a root slot of its own); chained: (root records, data roots [n][32]) for
    rsm_range_proofs_verify_data_root_dev.  Every operand sits between guard bands; only
    the status words may change."""
    ctx, n = R.device_context(0), len(cases)
    ns = p.namespace_size if p is not None else 0
    nl, rb = M.node_len(ns), M.record_bytes(W, ns)
    packed = b"".join(b"".join(c.shares) for c in cases)
    offs = np.cumsum([0] + [len(c.shares) for c in cases]).astype(np.uint32) if offsets is None else \
        np.asarray(offsets, np.uint32)
    total = len(packed) // S if shares_total is None else shares_total
    roots = np.zeros((n, 2, W, nl), np.uint8)
    for i, c in enumerate(cases):
        roots[i, axis, c.index] = np.frombuffer(c.root, np.uint8)
    queries = [(i, axis, c.index, c.start, c.end) for i, c in enumerate(cases)]
    recs, og, shs = Guarded(n * rb, 3, 41), Guarded((n + 1) * 4, 4, 42), Guarded(max(len(packed), 16), 0, 43)
    st = Guarded(n * 4, 4, 44)
    against = [Guarded(roots.nbytes, 1, 45)] if chained is None else \
        [Guarded(len(chained[0]), 5, 46), Guarded(len(chained[1]), 7, 47)]
    bufs = [recs, og, shs, st] + against
    try:
        fill(recs, b"".join(c.record for c in cases))
        fill(og, offs)
        fill(shs, packed)
        if chained is None:
            fill(against[0], roots)
            call = lib.rsm_range_proofs_verify_dev
        else:
            fill(against[0], chained[0])
            fill(against[1], chained[1])
            call = lib.rsm_range_proofs_verify_data_root_dev
        arr = (R.RangeQuery * n)(*[R.RangeQuery(*q) for q in queries])
        R._check(call(ctx, recs.ptr, og.ptr, shs.ptr, total, *[g.ptr for g in against], W, S, n, pref(p), arr, n, st.ptr, None))
        del arr  # copied before the call returned
        R._check(lib.rsm_sync(ctx))
        for g in bufs[:3] + against:
            assert np.array_equal(g.result(), g.untouched(0, g.n)), "a verifier wrote into an input"
        return [int(x) for x in st.result().view(np.uint32)]
    finally:
        for g in bufs:
            g.free()


def device_prove(lib, p, batch, S, queries, cap=None):
    """One node-store build (with its roots) and one rsm_range_proofs_dev over `batch`
    ([count][W][W][S]): (records, offsets, packed shares, roots [count][2][W][nl])."""
    ctx = R.device_context(0)
    count, W = batch.shape[0], batch.shape[1]
    ns = p.namespace_size if p is not None else 0
    n, rb, nl = len(queries), M.record_bytes(W, ns), M.node_len(ns)
    total = sum(q[4] - q[3] for q in queries)
    cap = total if cap is None else cap
    d = R.DeviceBuffer(batch.size)
    nodes = R.DeviceBuffer(int(lib.rsm_proof_nodes_bytes(W, pref(p), count)))
    roots, status = R.DeviceBuffer(count * 2 * W * nl), R.DeviceBuffer(count * 2 * W * 4)
    recs, offs, shs = Guarded(n * rb, 3, 51), Guarded((n + 1) * 4, 4, 52), Guarded(max(cap, 1) * S, 0, 53)
    try:
        d.upload(batch.reshape(-1))
        arr = (R.RangeQuery * n)(*[R.RangeQuery(*q) for q in queries])
        R._check(lib.rsm_proof_nodes_dev(ctx, d.ptr, W, S, count, pref(p), nodes.ptr, roots.ptr, status.ptr, None))
        R._check(lib.rsm_range_proofs_dev(ctx, nodes.ptr, d.ptr, W, S, count, pref(p), arr, n, recs.ptr, offs.ptr, shs.ptr, cap,
                                          None))
        del arr
        R._check(lib.rsm_sync(ctx))
        return (recs.result().tobytes(), offs.result().view(np.uint32).copy(), shs.result().tobytes(),
                roots.download(count * 2 * W * nl).reshape(count, 2, W, nl).copy())
    finally:
        for b in (d, nodes, roots, status, recs, offs, shs):
            b.free()


def square_roots(sq, k, ns, ig=True):
    """(trees of the rows, trees of the columns) of a complete square by the model."""
    W = sq.shape[0]
    rows = [M.tree_of([sq[i, p].tobytes() for p in range(W)], i, k, ns, ig) for i in range(W)]
    cols = [M.tree_of([sq[p, i].tobytes() for p in range(W)], i, k, ns, ig) for i in range(W)]
    return rows, cols


def data_root_tree(rows, cols):
    return D.RfcTree([t.root for t in rows] + [t.root for t in cols])
