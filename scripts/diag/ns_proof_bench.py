#!/usr/bin/env python3
"""Timing of the namespace-proof path (DESIGN.md §4 Roots, "Namespace proofs"):
512 squares of k = 128 (W = 256) with 512-byte shares and 29-byte namespaces laid out
in runs (Celestia-shaped: reserved namespaces, then user namespaces in runs of irregular
length that cross row ends), one query per quadrant-0 row -- 65,536 queries a call --
each for a namespace drawn from its row.

Protocol as scripts/diag/proof_bench.py: every rsm_ns_proofs_dev call (query upload,
locate, scan, node gather, share copy) is timed on its own with rsm_event_* on the
context stream, after warm-up calls; the figure is the median of --reps (>= 20) calls.
The 512 squares (16 GiB) and their node store (8.5 GB) exceed the 256 MiB Infinity
Cache many times over and every call reads all of them, so no call finds its input in
the cache from the previous one.  One square's bytes fill every slot; the queried
namespace differs per (square, row).  One JSON line.

    python scripts/diag/ns_proof_bench.py [--reps 24] > profiles/ns_proof_bench.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import rsmt2d_amd as R  # noqa: E402

K, S, NS, SQUARES = 128, 512, 29, 512
W = 2 * K


def runs_square(rng):
    """uint8[W][W][S]: random bytes, quadrant 0's namespaces non-decreasing in runs."""
    sq = rng.integers(0, 256, (W, W, S), dtype=np.uint8)
    lens = []
    while sum(lens) < K * K - 4:
        lens.append(int(rng.integers(1, 40)))
    tails = rng.integers(0, 256, (len(lens), 10), dtype=np.uint8)
    tails[:, 0] = 5 + tails[:, 0] % 250  # above the reserved namespaces, below 0xFF..
    tails = tails[np.lexsort(tails[:, ::-1].T)]
    names = np.zeros((K * K, NS), np.uint8)
    names[:4, NS - 1] = [1, 2, 2, 4]
    names[4:, NS - 10:] = np.repeat(tails, lens, axis=0)[:K * K - 4]
    sq[:K, :K, :NS] = names.reshape(K, K, NS)
    return sq


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
    n = count * K
    cols = rng.integers(0, K, n)  # the cell of its row each query takes its namespace from
    queries = [(s, 0, r) for s in range(count) for r in range(K)]
    nids = b"".join(sq[r, int(cols[i]), :NS].tobytes() for i, (_s, _a, r) in enumerate(queries))
    arr = (R.NsQuery * n)(*[R.NsQuery(*q) for q in queries])
    rb = int(L.rsm_ns_record_bytes(W, pp))
    nodes = R.DeviceBuffer(int(L.rsm_proof_nodes_bytes(W, pp, count)))
    status, recs, offs = R.DeviceBuffer(count * 2 * W * 4), R.DeviceBuffer(n * rb), R.DeviceBuffer((n + 1) * 4)
    R._check(L.rsm_proof_nodes_dev(ctx, buf.ptr, W, S, count, pp, nodes.ptr, None, status.ptr, None))
    # the share total first (no share buffer), then the timed calls with one of that size
    R._check(L.rsm_ns_proofs_dev(ctx, nodes.ptr, status.ptr, buf.ptr, W, S, count, pp, arr, nids, n, recs.ptr, offs.ptr,
                                 None, 0, None))
    R._check(L.rsm_sync(ctx))
    total = int(offs.download((n + 1) * 4).view(np.uint32)[n])
    shs = R.DeviceBuffer(max(total, 1) * S)
    ev = []
    for _ in range(2):
        e = ctypes.c_void_p()
        R._check(L.rsm_event_create(ctx, ctypes.byref(e)))
        ev.append(e)

    def timed(shares):
        out = []
        for i in range(a.warmup + a.reps):
            R._check(L.rsm_event_record(ctx, ev[0], None))
            R._check(L.rsm_ns_proofs_dev(ctx, nodes.ptr, status.ptr, buf.ptr, W, S, count, pp, arr, nids, n, recs.ptr,
                                         offs.ptr, shs.ptr if shares else None, total, None))
            R._check(L.rsm_event_record(ctx, ev[1], None))
            ms = ctypes.c_float()
            R._check(L.rsm_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)))
            if i >= a.warmup:
                out.append(ms.value)
        return statistics.median(out)

    with_ms, without_ms = timed(True), timed(False)
    kinds = np.frombuffer(recs.download(n * rb).tobytes(), np.uint8).reshape(n, rb)[:, 0]
    res = {"squares": count, "k": K, "share_size": S, "namespace_size": NS, "queries": n, "shares": total,
           "record_bytes": rb, "reps": a.reps, "inclusion": int((kinds == R.NS_INCLUSION).sum()),
           "call_ms": with_ms, "records_only_ms": without_ms,
           "queries_per_s": n / (with_ms * 1e-3), "shares_per_s": total / (with_ms * 1e-3),
           "share_bytes_per_s": total * S / (with_ms * 1e-3)}
    print(json.dumps({k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in res.items()}), flush=True)
    for e in ev:
        L.rsm_event_destroy(e)
    for b in (buf, nodes, status, recs, offs, shs):
        b.free()


if __name__ == "__main__":
    main()
