#!/usr/bin/env python3
"""Timing of blob share commitments on the device (DESIGN.md §4 Roots, "Commitments"): the
squares of scripts/diag/ns_proof_bench.py -- k = 128 (W = 256), 512-byte shares, 29-byte
namespaces in runs -- filled with blobs whose lengths are spread from 1 share to the whole
ODS (square 0 is one blob of 16,384 shares; the others are packed with lengths cycling
through LENGTHS at aligned starts), threshold 64:

  * rsm_blob_commitments_dev on the blobs' shares, packed (shares path), beside the host
    restatement rsm_blob_commitment looped over the same blobs (one host thread),
  * rsm_commitments_dev on the squares' node store (store path; the store's build,
    rsm_proof_nodes_dev, is timed on its own),
  * in the same process, the yardstick: rsm_nmt_roots_squares_dev over the same squares.

Both paths must give the host's commitments.  SHA-256 blocks are counted from the shapes: a
share's leaf is S/64 + 1 blocks; a subtree of z leaves has z - 1 joins of 3 blocks (90-byte
NMT nodes); the fold hashes each root as a leaf (2 blocks) and has roots - 1 joins of 2
blocks per blob.  The store path runs the fold's blocks only.  A square's roots are W * W
leaves and 2 W (W - 1) joins.

Protocol as scripts/diag/range_proof_bench.py: every call is timed on its own with
rsm_event_* on the context stream, after warm-up calls; the figure is the median of --reps
(>= 20) calls with the reps' minimum and maximum; a 384 MiB buffer is rewritten before every
timed call.  One JSON line.

    python scripts/diag/commitment_bench.py [--reps 24] > profiles/commitment_bench.json
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
from ns_proof_bench import K, NS, S, W, runs_square  # noqa: E402

FLUSH = 384 << 20
THRESHOLD = 64
LENGTHS = [1, 3, 10, 33, 64, 65, 129, 400, 1000, 3000]


def layout(square):
    """(start, len) of the blobs of one square, starts aligned to each blob's width."""
    if square == 0:
        return [(0, K * K)]
    out, at, i = [], 0, square
    while at < K * K:
        n = min(LENGTHS[i % len(LENGTHS)], K * K - at)
        w = R.SubTreeWidth(n, THRESHOLD)
        at = -(-at // w) * w
        if at + n > K * K:
            break
        out.append((at, n))
        at += n
        i += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--squares", type=int, default=16)
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
    blobs = [(s, st, n) for s in range(count) for st, n in layout(s)]
    n = len(blobs)
    lens = np.array([b[2] for b in blobs], np.int64)
    roots_of = np.array([len(R.MerkleMountainRangeSizes(int(x), R.SubTreeWidth(int(x), THRESHOLD))) for x in lens], np.int64)
    total, total_roots = int(lens.sum()), int(roots_of.sum())
    ods = np.ascontiguousarray(sq[:K, :K]).reshape(K * K, S)
    packed = np.concatenate([ods[st:st + ln] for _s, st, ln in blobs])
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    shs = R.DeviceBuffer(total * S)
    shs.upload(packed.reshape(-1))
    work = R.DeviceBuffer(int(L.rsm_commit_work_bytes(total, total_roots, pp)))
    com, status = R.DeviceBuffer(n * 32), R.DeviceBuffer(n * 4)
    nodes = R.DeviceBuffer(int(L.rsm_proof_nodes_bytes(W, pp, count)))
    tstat, roots = R.DeviceBuffer(count * 2 * W * 4), R.DeviceBuffer(count * 2 * W * nl)
    flush = R.DeviceBuffer(FLUSH)
    refs = (R.BlobRef * n)(*[R.BlobRef(*b) for b in blobs])
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

    # the host restatement, one blob after another (also the expected commitments)
    want = np.zeros((n, 32), np.uint8)
    st_word = ctypes.c_uint32(0)
    t0 = time.perf_counter()
    for i in range(n):
        lo = int(offsets[i])
        R._check(L.rsm_blob_commitment(pp, packed[lo:].ctypes.data, int(lens[i]), S, THRESHOLD, want[i].ctypes.data,
                                       ctypes.byref(st_word)))
        if st_word.value:
            raise SystemExit("host: blob %d fails" % i)
    host_ms = (time.perf_counter() - t0) * 1e3

    fold_blocks = int((roots_of * 2 + (roots_of - 1) * 2).sum())
    blocks = {"shares_path": int(total * leaf_blocks + (total - total_roots) * 3) + fold_blocks, "store_path": fold_blocks,
              "nmt_roots": count * (W * W * leaf_blocks + 2 * W * (W - 1) * 3)}
    res = {"squares": count, "k": K, "share_size": S, "namespace_size": NS, "threshold": THRESHOLD, "blobs": n,
           "shares": total, "subtree_roots": total_roots, "min_len": int(lens.min()), "max_len": int(lens.max()),
           "reps": a.reps, "sha_blocks": blocks, "host_ms": host_ms}

    def report(name, call, nblocks, check=True):
        call()
        R._check(L.rsm_sync(ctx))
        if check:
            if status.download(n * 4).any() or not np.array_equal(com.download(n * 32).reshape(n, 32), want):
                raise SystemExit("%s: the commitments differ from the host's" % name)
        ms, lo, hi = timed(call)
        res[name + "_ms"], res[name + "_ms_min"], res[name + "_ms_max"] = ms, lo, hi
        res[name + "_blocks_per_s"] = nblocks / (ms * 1e-3)

    optr = offsets.ctypes.data
    report("shares_path", lambda: R._check(L.rsm_blob_commitments_dev(ctx, shs.ptr, S, pp, THRESHOLD, optr, n, work.ptr, com.ptr,
                                                                     status.ptr, None)), blocks["shares_path"])
    report("store_build", lambda: R._check(L.rsm_proof_nodes_dev(ctx, buf.ptr, W, S, count, pp, nodes.ptr, None, tstat.ptr,
                                                                 None)), blocks["nmt_roots"], check=False)
    R._check(L.rsm_memcpy(ctx, com.ptr, np.zeros(n * 32, np.uint8).ctypes.data, n * 32, 0))
    report("store_path", lambda: R._check(L.rsm_commitments_dev(ctx, nodes.ptr, tstat.ptr, W, count, pp, THRESHOLD, refs, n, None,
                                                                None, com.ptr, status.ptr, None)), blocks["store_path"])
    report("nmt_roots", lambda: R._check(L.rsm_nmt_roots_squares_dev(ctx, buf.ptr, W, S, count, pp, roots.ptr, tstat.ptr, None)),
           blocks["nmt_roots"], check=False)
    res["host_to_shares_path_time"] = host_ms / res["shares_path_ms"]
    res["shares_path_to_store_path_time"] = res["shares_path_ms"] / res["store_path_ms"]
    res["shares_path_to_store_path_blocks"] = blocks["shares_path"] / blocks["store_path"]
    res["shares_path_to_nmt_roots_block_rate"] = res["shares_path_blocks_per_s"] / res["nmt_roots_blocks_per_s"]
    print(json.dumps({k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in res.items()}), flush=True)
    for e in ev:
        L.rsm_event_destroy(e)
    for b in (buf, shs, work, com, status, nodes, tstat, roots, flush):
        b.free()


if __name__ == "__main__":
    main()
