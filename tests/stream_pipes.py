"""TEST INFRASTRUCTURE ONLY -- the device pipelines tests/test_gpu_share_sizes.py and
tests/test_gpu_streams.py share, written as generators: each allocates its buffers, then
yields after every call it enqueues on its stream (NULL: the context stream), and only after
its last yield waits for the stream (rsm_stream_check) and downloads what the calls wrote.
`run` advances several of them in turn, so their calls alternate on their streams and no
pipeline synchronises before every pipeline has enqueued all of its calls.  Outputs lie
between guard bands (device_calls.Guarded), which must come back intact.  Importing this
module touches no GPU."""
import ctypes

import numpy as np

import data_root as DR
import ns_proofs as H
import range_calls as RG
import range_proofs as M
import rsmt2d_amd as R
from device_calls import Guarded


def run(*pipes):
    """Advances the generators round-robin until all have finished; their return values."""
    out, live = [None] * len(pipes), list(enumerate(pipes))
    while live:
        nxt = []
        for i, g in live:
            try:
                next(g)
                nxt.append((i, g))
            except StopIteration as e:
                out[i] = e.value
        live = nxt
    return out


def _free(bufs):
    for b in bufs:
        b.free()


def share_pipe(lib, stream, square, p, samples, start, pres0):
    """rsm_proof_nodes_dev -> rsm_proofs_dev -> rsm_proofs_verify_dev -> rsm_samples_scatter_dev:
    the serving side holds `square` ([W][W][S]), the receiving side starts from `start` with
    the presence map `pres0`.  Returns a dict of everything the calls wrote."""
    ctx = R.device_context(0)
    W, _, S = square.shape
    k, n = W // 2, len(samples)
    pp = ctypes.byref(p) if p is not None else None
    nl = 32 if p is None else 2 * p.namespace_size + 32
    rb = int(lib.rsm_proof_record_bytes(W, pp))
    plain = [R.DeviceBuffer(square.nbytes), R.DeviceBuffer(int(lib.rsm_proof_nodes_bytes(W, pp, 1)))]
    src, nodes = plain
    roots, recs, shs, status = Guarded(2 * W * nl, 0, 71), Guarded(n * rb, 0, 72), Guarded(n * S, 0, 73), Guarded(n * 4, 4, 74)
    dst, dpres = Guarded(square.nbytes, 0, 75), Guarded(W * W, 0, 76)
    try:
        src.upload(square.reshape(-1))
        dst.buf.upload(start.reshape(-1), dst.front)
        dpres.buf.upload(np.asarray(pres0, np.uint8).reshape(-1), dpres.front)
        arr = (R.Sample * n)(*[R.Sample(*s) for s in samples])
        R._check(lib.rsm_proof_nodes_dev(ctx, src.ptr, W, S, 1, pp, nodes.ptr, roots.ptr, None, stream))
        yield
        R._check(lib.rsm_proofs_dev(ctx, nodes.ptr, src.ptr, W, S, 1, pp, arr, n, recs.ptr, shs.ptr, stream))
        yield
        R._check(lib.rsm_proofs_verify_dev(ctx, shs.ptr, recs.ptr, roots.ptr, W, S, 1, pp, arr, n, status.ptr, stream))
        yield
        R._check(lib.rsm_samples_scatter_dev(ctx, dst.ptr, dpres.ptr, k, S, 1, arr, n, shs.ptr, status.ptr, stream))
        yield
        R._check(lib.rsm_stream_check(ctx, stream))
        return dict(roots=roots.result().tobytes(), records=recs.result().tobytes(), shares=shs.result().tobytes(),
                    status=[int(x) for x in status.result().view(np.uint32)],
                    square=dst.result().reshape(W, W, S).copy(), presence=dpres.result().reshape(W, W).copy())
    finally:
        _free(plain + [roots, recs, shs, status, dst, dpres])


def ns_pipe(lib, stream, batch, k, ns, ig, S, queries, nids):
    """rsm_proof_nodes_dev -> rsm_ns_proofs_dev -> rsm_ns_proofs_verify_dev on the prover's own
    device buffers: (records, offsets, packed shares, status words)."""
    ctx = R.device_context(0)
    count, W, n = batch.shape[0], 2 * k, len(queries)
    p = R.NmtParams(ns, int(ig), k)
    pp, rb, nl = ctypes.byref(p), H.record_bytes(W, ns), 2 * ns + 32
    trees, cap = {}, 0  # the share capacity: what the model says the proofs carry
    for q, nid in zip(queries, nids):
        if q not in trees:
            trees[q] = H.Tree(H.vector_shares(batch[q[0]], q[1], q[2]), q[2], k, ns, ig)
        kind, start, end = H.prove_namespace(trees[q], nid)[:3]
        cap += end - start if kind == H.INCLUSION else 0
    plain = [R.DeviceBuffer(batch.size), R.DeviceBuffer(int(lib.rsm_proof_nodes_bytes(W, pp, count))),
             R.DeviceBuffer(count * 2 * W * nl), R.DeviceBuffer(count * 2 * W * 4)]
    d, nodes, roots, tstat = plain
    recs, offs, shs, st = Guarded(n * rb, 3, 31), Guarded((n + 1) * 4, 4, 32), Guarded(max(cap, 1) * S, 0, 33), Guarded(n * 4, 4, 34)
    try:
        d.upload(batch.reshape(-1))
        arr = (R.NsQuery * n)(*[R.NsQuery(*q) for q in queries])
        flat = b"".join(nids)
        R._check(lib.rsm_proof_nodes_dev(ctx, d.ptr, W, S, count, pp, nodes.ptr, roots.ptr, tstat.ptr, stream))
        yield
        R._check(lib.rsm_ns_proofs_dev(ctx, nodes.ptr, tstat.ptr, d.ptr, W, S, count, pp, arr, flat, n, recs.ptr, offs.ptr,
                                       shs.ptr, cap, stream))
        yield
        R._check(lib.rsm_ns_proofs_verify_dev(ctx, recs.ptr, offs.ptr, shs.ptr, cap, roots.ptr, W, S, count, pp, arr, flat, n,
                                              st.ptr, stream))
        yield
        R._check(lib.rsm_stream_check(ctx, stream))
        return (recs.result().tobytes(), [int(x) for x in offs.result().view(np.uint32)], shs.result()[:cap * S].tobytes(),
                [int(x) for x in st.result().view(np.uint32)])
    finally:
        _free(plain + [recs, offs, shs, st])


def range_pipe(lib, stream, k, ns, S, batch, queries):
    """rsm_proof_nodes_dev -> rsm_range_proofs_dev -> rsm_range_proofs_verify_dev, then
    rsm_data_roots_dev -> rsm_root_proofs_dev -> rsm_range_proofs_verify_data_root_dev:
    (records, offsets, packed shares, roots, data roots, root records, status words,
    chained status words).  ns == 0: the DefaultTree."""
    ctx = R.device_context(0)
    count, W, n, p = batch.shape[0], 2 * k, len(queries), RG.params(k, ns)
    cap = sum(q[4] - q[3] for q in queries)
    rb, nl, rrb = M.record_bytes(W, ns), M.node_len(ns), DR.record_bytes(W)
    plain = [R.DeviceBuffer(batch.size), R.DeviceBuffer(int(lib.rsm_proof_nodes_bytes(W, RG.pref(p), count))),
             R.DeviceBuffer(int(lib.rsm_data_root_nodes_bytes(W, count)))]
    d, nodes, dr_nodes = plain
    roots = Guarded(count * 2 * W * nl, 0, 60)
    recs, offs, shs = Guarded(n * rb, 3, 61), Guarded((n + 1) * 4, 4, 62), Guarded(cap * S, 0, 63)
    st, st2, rrecs, drs = Guarded(n * 4, 4, 64), Guarded(n * 4, 4, 65), Guarded(n * rrb, 5, 66), Guarded(count * 32, 7, 67)
    try:
        d.upload(batch.reshape(-1))
        arr = (R.RangeQuery * n)(*[R.RangeQuery(*q) for q in queries])
        refs = (R.RootRef * n)(*[R.RootRef(*q[:3]) for q in queries])
        R._check(lib.rsm_proof_nodes_dev(ctx, d.ptr, W, S, count, RG.pref(p), nodes.ptr, roots.ptr, None, stream))
        yield
        R._check(lib.rsm_range_proofs_dev(ctx, nodes.ptr, d.ptr, W, S, count, RG.pref(p), arr, n, recs.ptr, offs.ptr, shs.ptr, cap,
                                          stream))
        yield
        R._check(lib.rsm_range_proofs_verify_dev(ctx, recs.ptr, offs.ptr, shs.ptr, cap, roots.ptr, W, S, count, RG.pref(p), arr, n,
                                                 st.ptr, stream))
        yield
        R._check(lib.rsm_data_roots_dev(ctx, roots.ptr, W, nl, count, drs.ptr, dr_nodes.ptr, stream))
        yield
        R._check(lib.rsm_root_proofs_dev(ctx, dr_nodes.ptr, W, count, refs, n, rrecs.ptr, stream))
        yield
        R._check(lib.rsm_range_proofs_verify_data_root_dev(ctx, recs.ptr, offs.ptr, shs.ptr, cap, rrecs.ptr, drs.ptr, W, S,
                                                           count, RG.pref(p), arr, n, st2.ptr, stream))
        yield
        R._check(lib.rsm_stream_check(ctx, stream))
        return (recs.result().tobytes(), [int(x) for x in offs.result().view(np.uint32)], shs.result().tobytes(),
                roots.result().tobytes(), drs.result().tobytes(), rrecs.result().tobytes(),
                [int(x) for x in st.result().view(np.uint32)], [int(x) for x in st2.result().view(np.uint32)])
    finally:
        _free(plain + [roots, recs, offs, shs, st, st2, rrecs, drs])
