#!/usr/bin/env python3
"""Timing of namespace-proof verification on the device (DESIGN.md §4 Roots, "Namespace
proofs"): the workload of scripts/diag/ns_proof_bench.py -- 512 squares of k = 128
(W = 256) with 512-byte shares and 29-byte namespaces laid out in runs, one query per
quadrant-0 row, 65,536 queries -- proved on the device (rsm_proof_nodes_dev,
rsm_ns_proofs_dev) and then verified where the prover left it:

  * rsm_ns_proofs_verify_dev of all 65,536 queries and of n = 256 (another part of the set
    each call), the query upload included; every status of the first call must be 0,
  * in the same process, as SHA-256 blocks per second: rsm_nmt_roots_squares_dev of 32
    squares and rsm_proofs_verify_dev of 65,536 single-share samples (the yardsticks),
  * the wall time of the host loop of rsm_nmt_namespace_verify over the same records.

SHA blocks of a query: shares * (S/64 + 1) leaf blocks and joins * 3 (90-byte nodes), the
joins counted from the record's shape: shares + n_nodes - 1 (ABSENCE: n_nodes).  A sample
of rsm_proofs_verify_dev: S/64 + 1 leaf blocks and 8 fold steps of 3; a square: W * W
leaves and 2 W trees of W - 1 nodes.

Protocol as scripts/diag/verify_bench.py: every call is timed on its own with rsm_event_*
on the context stream, after warm-up calls; the figure is the median of --reps (>= 20)
calls; a 384 MiB buffer is rewritten before every timed call, so no call finds its input
in the 256 MiB Infinity Cache.  One JSON line.

    python scripts/diag/ns_verify_bench.py [--reps 24] > profiles/ns_verify_bench.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import rsmt2d_amd as R  # noqa: E402
from ns_proof_bench import K, NS, S, SQUARES, W, runs_square  # noqa: E402

BATCH, LEVELS, SMALL = 32, 8, 256
FLUSH = 384 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--squares", type=int, default=SQUARES)
    ap.add_argument("--host-queries", type=int, default=None, help="queries of the host loop (default: all)")
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    L, ctx, count = R.library(), R.device_context(0), a.squares
    if count < BATCH:
        raise SystemExit("--squares must be at least %d" % BATCH)
    rng = np.random.default_rng(1)
    sq = runs_square(rng)
    sq_bytes = W * W * S
    buf = R.DeviceBuffer(count * sq_bytes)
    for i in range(count):
        buf.upload(sq.reshape(-1), i * sq_bytes)
    p = R.NmtParams(NS, 1, K)
    pp = ctypes.byref(p)
    nl, leaf_blocks, node_blocks = 2 * NS + 32, S // 64 + 1, 3
    n = count * K
    cols = rng.integers(0, K, n)  # the cell of its row each query takes its namespace from
    queries = [(s, 0, r) for s in range(count) for r in range(K)]
    nid_rows = np.stack([sq[r, int(cols[i]), :NS] for i, (_s, _a, r) in enumerate(queries)])
    nids = nid_rows.tobytes()
    arr = (R.NsQuery * n)(*[R.NsQuery(*q) for q in queries])
    rb = int(L.rsm_ns_record_bytes(W, pp))
    nodes = R.DeviceBuffer(int(L.rsm_proof_nodes_bytes(W, pp, count)))
    tstat, roots = R.DeviceBuffer(count * 2 * W * 4), R.DeviceBuffer(count * 2 * W * nl)
    recs, offs, status = R.DeviceBuffer(n * rb), R.DeviceBuffer((n + 1) * 4), R.DeviceBuffer(n * 4)
    R._check(L.rsm_proof_nodes_dev(ctx, buf.ptr, W, S, count, pp, nodes.ptr, roots.ptr, tstat.ptr, None))
    R._check(L.rsm_ns_proofs_dev(ctx, nodes.ptr, tstat.ptr, buf.ptr, W, S, count, pp, arr, nids, n, recs.ptr, offs.ptr,
                                 None, 0, None))
    R._check(L.rsm_sync(ctx))
    offsets = offs.download((n + 1) * 4).view(np.uint32).copy()
    total = int(offsets[n])
    shs = R.DeviceBuffer(max(total, 1) * S)
    R._check(L.rsm_ns_proofs_dev(ctx, nodes.ptr, tstat.ptr, buf.ptr, W, S, count, pp, arr, nids, n, recs.ptr, offs.ptr,
                                 shs.ptr, total, None))
    R._check(L.rsm_sync(ctx))
    nodes.free()
    flush = R.DeviceBuffer(FLUSH)
    ev = []
    for _ in range(2):
        e = ctypes.c_void_p()
        R._check(L.rsm_event_create(ctx, ctypes.byref(e)))
        ev.append(e)

    def timed(call):
        """Median device milliseconds of call(i), i counting every call made."""
        out = []
        for i in range(a.warmup + a.reps):
            R._check(L.rsm_dev_fill_random(ctx, flush.ptr, FLUSH, i))
            R._check(L.rsm_event_record(ctx, ev[0], None))
            call(i)
            R._check(L.rsm_event_record(ctx, ev[1], None))
            ms = ctypes.c_float()
            R._check(L.rsm_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)))
            if i >= a.warmup:
                out.append(ms.value)
        return statistics.median(out)

    # the shapes: shares and joins of every query
    records = np.frombuffer(recs.download(n * rb).tobytes(), np.uint8).reshape(n, rb)
    head = records[:, :16].copy().view("<u4")
    kind, n_nodes = head[:, 0], head[:, 3].astype(np.int64)
    lens = np.diff(offsets.astype(np.int64))
    joins = np.where(kind == R.NS_EMPTY, 0, np.where(kind == R.NS_ABSENCE, n_nodes, lens + n_nodes - 1))
    csum_blocks = np.concatenate([[0], np.cumsum(lens * leaf_blocks + joins * node_blocks)])
    res = {"squares": count, "k": K, "share_size": S, "namespace_size": NS, "queries": n, "shares": total,
           "joins": int(joins.sum()), "record_bytes": rb, "reps": a.reps, "inclusion": int((kind == R.NS_INCLUSION).sum()),
           "absence": int((kind == R.NS_ABSENCE).sum()), "mean_shares_per_query": total / n,
           "max_shares_per_query": int(lens.max())}

    def verify(first, m):
        q = ctypes.c_void_p(ctypes.addressof(arr) + first * ctypes.sizeof(R.NsQuery))
        R._check(L.rsm_ns_proofs_verify_dev(ctx, recs.ptr + first * rb, offs.ptr + first * 4, shs.ptr, total, roots.ptr, W, S,
                                            count, pp, q, nids[first * NS:(first + m) * NS], m, status.ptr, None))

    for m in (n, SMALL):
        steps = max((n - m) // SMALL, 1)
        call = lambda i, m=m, steps=steps: verify(((i * 7919) % steps) * SMALL if m < n else 0, m)  # noqa: E731
        call(1)
        R._check(L.rsm_sync(ctx))
        if status.download(m * 4).any():
            raise SystemExit("a valid namespace proof did not verify")
        ms = timed(call)
        blocks = int(csum_blocks[n]) if m == n else int(csum_blocks[n]) * m / n  # (the small calls: the set's mean)
        res["verify_%d_ms" % m] = ms
        res["verify_%d_queries_per_s" % m] = m / (ms * 1e-3)
        res["verify_%d_shares_per_s" % m] = total * (m / n) / (ms * 1e-3)
        res["verify_%d_blocks_per_s" % m] = blocks / (ms * 1e-3)
    res["sha_blocks"] = int(csum_blocks[n])

    # the yardsticks, in this process: NMT roots of 32 squares, single-share verification
    pool = 2 * 65536
    samples = np.stack([rng.integers(BATCH, size=pool), rng.integers(2, size=pool), rng.integers(W, size=pool),
                        rng.integers(W, size=pool)], axis=1).astype(np.uint32)
    prb = int(L.rsm_proof_record_bytes(W, pp))
    store = R.DeviceBuffer(int(L.rsm_proof_nodes_bytes(W, pp, BATCH)))
    roots32, tstat32 = R.DeviceBuffer(BATCH * 2 * W * nl), R.DeviceBuffer(BATCH * 2 * W * 4)
    precs, pshs = R.DeviceBuffer(pool * prb), R.DeviceBuffer(pool * S)
    R._check(L.rsm_proof_nodes_dev(ctx, buf.ptr, W, S, BATCH, pp, store.ptr, roots32.ptr, tstat32.ptr, None))
    R._check(L.rsm_proofs_dev(ctx, store.ptr, buf.ptr, W, S, BATCH, pp, samples.ctypes.data, pool, precs.ptr, pshs.ptr, None))
    R._check(L.rsm_sync(ctx))
    store.free()
    ms = timed(lambda i: R._check(L.rsm_nmt_roots_squares_dev(ctx, buf.ptr + (i % 2) * BATCH * sq_bytes, W, S, BATCH, pp,
                                                              roots32.ptr, tstat32.ptr, None)))
    res["roots_32_ms"] = ms
    res["roots_32_blocks_per_s"] = BATCH * (W * W * leaf_blocks + 2 * W * (W - 1) * node_blocks) / (ms * 1e-3)

    def sample_verify(i):
        first = (i % 2) * 65536
        R._check(L.rsm_proofs_verify_dev(ctx, pshs.ptr + first * S, precs.ptr + first * prb, roots32.ptr, W, S, BATCH, pp,
                                         samples[first:].ctypes.data, 65536, status.ptr, None))

    sample_verify(1)
    R._check(L.rsm_sync(ctx))
    if status.download(65536 * 4).any():
        raise SystemExit("a valid sample did not verify")
    ms = timed(sample_verify)
    res["proofs_verify_65536_ms"] = ms
    res["proofs_verify_65536_blocks_per_s"] = 65536 * (leaf_blocks + LEVELS * node_blocks) / (ms * 1e-3)
    res["ns_verify_to_proofs_verify_block_rate"] = res["verify_%d_blocks_per_s" % n] / res["proofs_verify_65536_blocks_per_s"]
    res["ns_verify_to_roots_block_rate"] = res["verify_%d_blocks_per_s" % n] / res["roots_32_blocks_per_s"]

    # the host loop over the same records
    hq = n if a.host_queries is None else min(a.host_queries, n)
    hshares = np.frombuffer(shs.download(int(offsets[hq]) * S).tobytes(), np.uint8) if offsets[hq] else np.zeros(1, np.uint8)
    hroots = np.frombuffer(roots.download(count * 2 * W * nl).tobytes(), np.uint8).reshape(count, 2, W, nl)
    st = ctypes.c_uint32(0)
    bad = 0
    t0 = time.perf_counter()
    for i in range(hq):
        s, _a, r = queries[i]
        L.rsm_nmt_namespace_verify(pp, r, nid_rows[i].ctypes.data, hshares.ctypes.data + int(offsets[i]) * S, int(lens[i]), S,
                                   W, records[i].ctypes.data, hroots[s, 0, r].ctypes.data, ctypes.byref(st))
        bad += st.value != 0
    host_s = time.perf_counter() - t0
    if bad:
        raise SystemExit("the host verifier rejects %d of the device's proofs" % bad)
    res["host_loop_queries"] = hq
    res["host_loop_s"] = host_s
    res["host_loop_queries_per_s"] = hq / host_s
    res["device_to_host_speedup"] = (hq / host_s) and res["verify_%d_queries_per_s" % n] / (hq / host_s)
    print(json.dumps({k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in res.items()}), flush=True)
    for e in ev:
        L.rsm_event_destroy(e)
    for b in (buf, tstat, roots, recs, offs, status, shs, flush, roots32, tstat32, precs, pshs):
        b.free()


if __name__ == "__main__":
    main()
