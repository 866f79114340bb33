#!/usr/bin/env python3
"""Timing of proof verification (DESIGN.md §4 "Verification") at W = 256, S = 512, for
the DefaultTree and the NMT (29-byte namespaces):

  * rsm_proofs_verify_dev of n = 256 (one fraud-proof vector), 4,096 and 65,536 valid
    samples, the sample upload included,
  * rsm_roots_squares_dev / rsm_nmt_roots_squares_dev of 32 squares in the same process:
    the yardstick, as SHA-256 blocks per second.

SHA blocks: a sample is S/64 + 1 leaf blocks and L = 8 fold steps of 2 (DefaultTree) or
3 (NMT, 90-byte nodes) blocks; a square is W * W leaves of S/64 + 1 blocks and 2 W trees
of W - 1 nodes.

Protocol: every call is timed on its own with rsm_event_* on the context stream, after
warm-up calls; the figure is the median of --reps (>= 20) calls.  The shares and records
of a call come from a pool of 6 * 65,536 proofs (rsm_proofs_dev over 32 squares), a
different part each call, and a 384 MiB buffer is rewritten before every timed call, so
no call finds its input in the 256 MiB Infinity Cache.  The first call of each size is
checked: every status must be 0.  One JSON line per tree.

    python scripts/diag/verify_bench.py [--reps 24] > profiles/verify_bench.json
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

W, S, NS, BATCH, NBATCH = 256, 512, 29, 32, 2
SIZES, SETS = (256, 4096, 65536), 6
LEVELS = 8
FLUSH = 384 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    L, ctx = R.library(), R.device_context(0)
    k, sq_bytes, slots = W // 2, W * W * S, BATCH * NBATCH
    rng = np.random.default_rng(1)
    sq = rng.integers(0, 256, (W, W, S), dtype=np.uint8)
    q0 = sq[:k, :k].reshape(k * k, S)
    sq[:k, :k] = q0[np.lexsort(q0[:, :NS][:, ::-1].T)].reshape(k, k, S)
    buf = R.DeviceBuffer(slots * sq_bytes)
    for i in range(slots):
        buf.upload(sq.reshape(-1), i * sq_bytes)
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

    pool = SETS * SIZES[-1]
    samples = np.stack([rng.integers(BATCH, size=pool), rng.integers(2, size=pool), rng.integers(W, size=pool),
                        rng.integers(W, size=pool)], axis=1).astype(np.uint32)
    leaf_blocks = S // 64 + 1
    for name, p, node_blocks in (("DefaultTree", None, 2), ("NMT", R.NmtParams(NS, 1, k), 3)):
        pp = ctypes.byref(p) if p is not None else None
        nl = 32 if p is None else 2 * NS + 32
        rb = int(L.rsm_proof_record_bytes(W, pp))
        store = R.DeviceBuffer(int(L.rsm_proof_nodes_bytes(W, pp, BATCH)))
        roots, tstat = R.DeviceBuffer(BATCH * 2 * W * nl), R.DeviceBuffer(BATCH * 2 * W * 4)
        recs, shs, status = R.DeviceBuffer(pool * rb), R.DeviceBuffer(pool * S), R.DeviceBuffer(SIZES[-1] * 4)
        R._check(L.rsm_proof_nodes_dev(ctx, buf.ptr, W, S, BATCH, pp, store.ptr, roots.ptr, tstat.ptr, None))
        R._check(L.rsm_proofs_dev(ctx, store.ptr, buf.ptr, W, S, BATCH, pp, samples.ctypes.data, pool, recs.ptr, shs.ptr,
                                  None))
        R._check(L.rsm_sync(ctx))
        store.free()
        res = {"tree": name, "width": W, "share_size": S, "reps": a.reps, "record_bytes": rb}

        def roots_call(i):
            src = buf.ptr + (i % NBATCH) * BATCH * sq_bytes
            if p is None:
                R._check(L.rsm_roots_squares_dev(ctx, src, W, S, BATCH, roots.ptr, None))
            else:
                R._check(L.rsm_nmt_roots_squares_dev(ctx, src, W, S, BATCH, pp, roots.ptr, tstat.ptr, None))

        ms = timed(roots_call)
        blocks = BATCH * (W * W * leaf_blocks + 2 * W * (W - 1) * node_blocks)
        res["roots_32_ms"] = ms
        res["roots_32_blocks_per_s"] = blocks / (ms * 1e-3)
        for n in SIZES:
            def verify(i, n=n):
                first = (i * SIZES[-1] + (i // SETS) * n) % (pool - n + 1)  # another part of the pool each call
                R._check(L.rsm_proofs_verify_dev(ctx, shs.ptr + first * S, recs.ptr + first * rb, roots.ptr, W, S, BATCH,
                                                 pp, samples[first:].ctypes.data, n, status.ptr, None))

            verify(1)
            R._check(L.rsm_sync(ctx))
            if status.download(n * 4).any():
                raise SystemExit("%s: a valid sample did not verify" % name)
            ms = timed(verify)
            blocks = n * (leaf_blocks + LEVELS * node_blocks)
            res["verify_%d_us" % n] = ms * 1e3
            res["verify_%d_samples_per_s" % n] = n / (ms * 1e-3)
            res["verify_%d_blocks_per_s" % n] = blocks / (ms * 1e-3)
        res["verify_65536_to_roots_block_rate"] = res["verify_65536_blocks_per_s"] / res["roots_32_blocks_per_s"]
        R._check(L.rsm_sync(ctx))
        print(json.dumps({k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in res.items()}), flush=True)
        for b in (roots, tstat, recs, shs, status):
            b.free()
    for e in ev:
        L.rsm_event_destroy(e)
    flush.free()
    buf.free()


if __name__ == "__main__":
    main()
