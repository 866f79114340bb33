#!/usr/bin/env python3
"""Timing of range proofs on the device (DESIGN.md §4 Roots, "Range proofs"): the workload of
scripts/diag/ns_proof_bench.py -- 512 squares of k = 128 (W = 256) with 512-byte shares and
29-byte namespaces laid out in runs, one query per quadrant-0 row, 65,536 queries -- whose
ranges are the namespaces' runs (taken from rsm_ns_proofs_dev's records), so the range
records are byte for byte the namespace records:

  * rsm_range_proofs_dev (records, offsets and shares out of the node store),
  * rsm_range_proofs_verify_dev, rsm_range_proofs_verify_data_root_dev (root records of
    rsm_root_proofs_dev, no root table) and the DefaultTree verifier on the same ranges,
  * in the same process, two yardsticks: rsm_ns_proofs_verify_dev on the same records and
    rsm_proofs_verify_dev on the same shares as single-share samples.

Every status must be 0.  SHA-256 blocks are counted from the record shapes: a query hashes
shares * (S/64 + 1) leaf blocks and joins = shares + n_nodes - 1 nodes of 3 blocks (90-byte
NMT nodes) or 2 (DefaultTree); the chained form adds 2 blocks for the root as a leaf and 2
per level of the data-root tree (9 for 2W = 512); a single-share sample hashes S/64 + 1
blocks and 8 fold steps of 3.

Protocol as scripts/diag/ns_verify_bench.py: every call is timed on its own with rsm_event_*
on the context stream, after warm-up calls; the figure is the median of --reps (>= 20)
calls, with the reps' minimum and maximum next to it; a 384 MiB buffer is rewritten before
every timed call, so no call finds its input in the 256 MiB Infinity Cache.  One JSON line.

    python scripts/diag/range_proof_bench.py [--reps 24] > profiles/range_proof_bench.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import rsmt2d_amd as R  # noqa: E402
from ns_proof_bench import K, NS, S, SQUARES, W, runs_square  # noqa: E402

LEVELS, ROOT_LEVELS = 8, 9
FLUSH = 384 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--squares", type=int, default=SQUARES)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    L, ctx, count = R.library(), R.device_context(0), a.squares
    rng = np.random.default_rng(1)
    sq = runs_square(rng)
    sq_bytes = W * W * S
    buf = R.DeviceBuffer(count * sq_bytes)
    for i in range(count):
        buf.upload(sq.reshape(-1), i * sq_bytes)
    p = R.NmtParams(NS, 1, K)
    pp = ctypes.byref(p)
    nl, leaf_blocks = 2 * NS + 32, S // 64 + 1
    n = count * K
    cols = rng.integers(0, K, n)  # the cell of its row each query takes its namespace from
    refs = [(s, 0, r) for s in range(count) for r in range(K)]
    nids = np.stack([sq[r, int(cols[i]), :NS] for i, (_s, _a, r) in enumerate(refs)]).tobytes()
    ns_arr = (R.NsQuery * n)(*[R.NsQuery(*q) for q in refs])
    rb = int(L.rsm_ns_record_bytes(W, pp))
    assert rb == int(L.rsm_range_record_bytes(W, pp))
    nodes = R.DeviceBuffer(int(L.rsm_proof_nodes_bytes(W, pp, count)))
    tstat, roots = R.DeviceBuffer(count * 2 * W * 4), R.DeviceBuffer(count * 2 * W * nl)
    ns_recs, recs, offs, status = R.DeviceBuffer(n * rb), R.DeviceBuffer(n * rb), R.DeviceBuffer((n + 1) * 4), R.DeviceBuffer(n * 4)
    R._check(L.rsm_proof_nodes_dev(ctx, buf.ptr, W, S, count, pp, nodes.ptr, roots.ptr, tstat.ptr, None))
    R._check(L.rsm_ns_proofs_dev(ctx, nodes.ptr, tstat.ptr, buf.ptr, W, S, count, pp, ns_arr, nids, n, ns_recs.ptr, offs.ptr,
                                 None, 0, None))
    R._check(L.rsm_sync(ctx))
    ns_records = ns_recs.download(n * rb).tobytes()
    head = np.frombuffer(ns_records, np.uint8).reshape(n, rb)[:, :16].copy().view("<u4")
    if (head[:, 0] != R.NS_INCLUSION).any():
        raise SystemExit("a namespace taken from a cell is not an inclusion")
    start, end, n_nodes = head[:, 1].astype(np.int64), head[:, 2].astype(np.int64), head[:, 3].astype(np.int64)
    lens = end - start
    total = int(lens.sum())
    queries = np.stack([np.array(refs, np.uint32).T[0], np.zeros(n, np.uint32), np.array(refs, np.uint32).T[2],
                        start.astype(np.uint32), end.astype(np.uint32)], axis=1).copy()
    qptr = queries.ctypes.data
    shs = R.DeviceBuffer(total * S)
    flush = R.DeviceBuffer(FLUSH)
    ev = []
    for _ in range(2):
        e = ctypes.c_void_p()
        R._check(L.rsm_event_create(ctx, ctypes.byref(e)))
        ev.append(e)

    def timed(call):
        """(median, minimum, maximum) device milliseconds of call()."""
        out = []
        for i in range(a.warmup + a.reps):
            R._check(L.rsm_dev_fill_random(ctx, flush.ptr, FLUSH, i))
            R._check(L.rsm_event_record(ctx, ev[0], None))
            call()
            R._check(L.rsm_event_record(ctx, ev[1], None))
            ms = ctypes.c_float()
            R._check(L.rsm_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)))
            if i >= a.warmup:
                out.append(ms.value)
        return statistics.median(out), min(out), max(out)

    joins = lens + n_nodes - 1
    blocks = {"nmt": int((lens * leaf_blocks + joins * 3).sum()), "default": int((lens * leaf_blocks + joins * 2).sum())}
    blocks["chained"] = blocks["nmt"] + n * (2 + 2 * ROOT_LEVELS)
    blocks["single"] = total * (leaf_blocks + LEVELS * 3)
    res = {"squares": count, "k": K, "share_size": S, "namespace_size": NS, "queries": n, "shares": total,
           "joins": int(joins.sum()), "record_bytes": rb, "reps": a.reps, "mean_shares_per_query": total / n,
           "max_shares_per_query": int(lens.max()), "sha_blocks": blocks}

    def report(name, call, nblocks, per=None):
        call()
        R._check(L.rsm_sync(ctx))
        if per is not None and status.download(per * 4).any():
            raise SystemExit("%s: a valid proof did not verify" % name)
        ms, lo, hi = timed(call)
        res[name + "_ms"], res[name + "_ms_min"], res[name + "_ms_max"] = ms, lo, hi
        res[name + "_shares_per_s"] = total / (ms * 1e-3)
        if nblocks:
            res[name + "_blocks_per_s"] = nblocks / (ms * 1e-3)

    # prove: the records must be the namespace prover's
    report("prove", lambda: R._check(L.rsm_range_proofs_dev(ctx, nodes.ptr, buf.ptr, W, S, count, pp, qptr, n, recs.ptr,
                                                            offs.ptr, shs.ptr, total, None)), 0)
    if recs.download(n * rb).tobytes() != ns_records:
        raise SystemExit("the range records differ from the namespace records")
    report("verify", lambda: R._check(L.rsm_range_proofs_verify_dev(ctx, recs.ptr, offs.ptr, shs.ptr, total, roots.ptr, W, S,
                                                                    count, pp, qptr, n, status.ptr, None)), blocks["nmt"], n)
    report("ns_verify", lambda: R._check(L.rsm_ns_proofs_verify_dev(ctx, recs.ptr, offs.ptr, shs.ptr, total, roots.ptr, W, S,
                                                                    count, pp, ns_arr, nids, n, status.ptr, None)),
           blocks["nmt"], n)
    # chained: the data roots and the root records
    drs, dr_nodes = R.DeviceBuffer(count * 32), R.DeviceBuffer(int(L.rsm_data_root_nodes_bytes(W, count)))
    rrb = int(L.rsm_data_root_record_bytes(W))
    rrecs = R.DeviceBuffer(n * rrb)
    ref_arr = (R.RootRef * n)(*[R.RootRef(*q) for q in refs])
    R._check(L.rsm_data_roots_dev(ctx, roots.ptr, W, nl, count, drs.ptr, dr_nodes.ptr, None))
    R._check(L.rsm_root_proofs_dev(ctx, dr_nodes.ptr, W, count, ref_arr, n, rrecs.ptr, None))
    report("verify_data_root", lambda: R._check(L.rsm_range_proofs_verify_data_root_dev(
        ctx, recs.ptr, offs.ptr, shs.ptr, total, rrecs.ptr, drs.ptr, W, S, count, pp, qptr, n, status.ptr, None)),
        blocks["chained"], n)
    # single-share samples over the same shares (the records out of the same store)
    samples = np.empty((total, 4), np.uint32)
    at = np.concatenate([[0], np.cumsum(lens)])
    for i in range(n):
        samples[at[i]:at[i + 1]] = (queries[i, 0], 0, queries[i, 2], 0)
        samples[at[i]:at[i + 1], 3] = np.arange(start[i], end[i])
    prb = int(L.rsm_proof_record_bytes(W, pp))
    precs, pstatus = R.DeviceBuffer(total * prb), R.DeviceBuffer(total * 4)
    R._check(L.rsm_proofs_dev(ctx, nodes.ptr, None, W, S, count, pp, samples.ctypes.data, total, precs.ptr, None, None))
    R._check(L.rsm_sync(ctx))
    nodes.free()

    def single():
        R._check(L.rsm_proofs_verify_dev(ctx, shs.ptr, precs.ptr, roots.ptr, W, S, count, pp, samples.ctypes.data, total,
                                         pstatus.ptr, None))

    report("proofs_verify", single, blocks["single"])
    if pstatus.download(total * 4).any():
        raise SystemExit("a valid sample did not verify")
    precs.free()
    # the DefaultTree verifier on the same ranges
    dnodes = R.DeviceBuffer(int(L.rsm_proof_nodes_bytes(W, None, count)))
    droots, drb = R.DeviceBuffer(count * 2 * W * 32), int(L.rsm_range_record_bytes(W, None))
    drecs = R.DeviceBuffer(n * drb)
    R._check(L.rsm_proof_nodes_dev(ctx, buf.ptr, W, S, count, None, dnodes.ptr, droots.ptr, None, None))
    R._check(L.rsm_range_proofs_dev(ctx, dnodes.ptr, buf.ptr, W, S, count, None, qptr, n, drecs.ptr, offs.ptr, shs.ptr, total,
                                    None))
    R._check(L.rsm_sync(ctx))
    dnodes.free()
    report("default_verify", lambda: R._check(L.rsm_range_proofs_verify_dev(
        ctx, drecs.ptr, offs.ptr, shs.ptr, total, droots.ptr, W, S, count, None, qptr, n, status.ptr, None)),
        blocks["default"], n)
    res["verify_to_ns_verify_time"] = res["verify_ms"] / res["ns_verify_ms"]
    res["verify_to_proofs_verify_time_per_share"] = res["verify_ms"] / res["proofs_verify_ms"]
    res["single_to_range_blocks"] = blocks["single"] / blocks["nmt"]
    print(json.dumps({k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in res.items()}), flush=True)
    for e in ev:
        L.rsm_event_destroy(e)
    for b in (buf, tstat, roots, ns_recs, recs, offs, status, shs, flush, drs, dr_nodes, rrecs, pstatus, droots, drecs):
        b.free()


if __name__ == "__main__":
    main()
