#!/usr/bin/env python3
"""Timing of the share-inclusion-proof path (DESIGN.md §4 Roots, "Proofs") at
W = 256, S = 512, for the DefaultTree and the NMT (29-byte namespaces):

  * the node-store build (rsm_proof_nodes_dev) of 1 square and of 32 squares,
  * rsm_roots_squares_dev / rsm_nmt_roots_squares_dev of the same buffers, same run,
  * the gather of 4,096 random samples with their shares (rsm_proofs_dev).

Protocol: every call is timed on its own with rsm_event_* on the context stream,
after warm-up calls; the figure is the median of --reps (>= 20) calls.  Calls rotate
over squares / batches whose bytes exceed the 256 MiB Infinity Cache, so no call finds
its input there from the previous one.  One JSON line per tree.

    python scripts/diag/proof_bench.py [--reps 24] > profiles/proof_bench.json
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

W, S, NS, BATCH, NBATCH, NSAMPLES = 256, 512, 29, 32, 2, 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    L, ctx = R.library(), R.device_context(0)
    k, sq_bytes, slots = W // 2, W * W * S, BATCH * NBATCH
    # one square with a namespace-ordered quadrant 0 (a valid NMT input), in every slot
    rng = np.random.default_rng(1)
    sq = rng.integers(0, 256, (W, W, S), dtype=np.uint8)
    q0 = sq[:k, :k].reshape(k * k, S)
    sq[:k, :k] = q0[np.lexsort(q0[:, :NS][:, ::-1].T)].reshape(k, k, S)
    buf = R.DeviceBuffer(slots * sq_bytes)
    for i in range(slots):
        buf.upload(sq.reshape(-1), i * sq_bytes)
    ev = []
    for _ in range(2):
        e = ctypes.c_void_p()
        R._check(L.rsm_event_create(ctx, ctypes.byref(e)))
        ev.append(e)

    def timed(call):
        """Median device milliseconds of call(i), i counting every call made."""
        out = []
        for i in range(a.warmup + a.reps):
            R._check(L.rsm_event_record(ctx, ev[0], None))
            call(i)
            R._check(L.rsm_event_record(ctx, ev[1], None))
            ms = ctypes.c_float()
            R._check(L.rsm_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)))
            if i >= a.warmup:
                out.append(ms.value)
        return statistics.median(out)

    samples = [(int(rng.integers(BATCH)), int(rng.integers(2)), int(rng.integers(W)), int(rng.integers(W)))
               for _ in range(NSAMPLES)]
    arr = (R.Sample * NSAMPLES)(*[R.Sample(*s) for s in samples])
    for name, p in (("DefaultTree", None), ("NMT", R.NmtParams(NS, 1, k))):
        pp = ctypes.byref(p) if p is not None else None
        nl = 32 if p is None else 2 * NS + 32
        one, many = int(L.rsm_proof_nodes_bytes(W, pp, 1)), int(L.rsm_proof_nodes_bytes(W, pp, BATCH))
        nstores = 16  # single-square stores rotated: 16 of them exceed the cache as well
        store1, storeb = R.DeviceBuffer(nstores * one), R.DeviceBuffer(many)
        roots, status = R.DeviceBuffer(BATCH * 2 * W * nl), R.DeviceBuffer(BATCH * 2 * W * 4)
        rb = int(L.rsm_proof_record_bytes(W, pp))
        recs, shs = R.DeviceBuffer(NSAMPLES * rb), R.DeviceBuffer(NSAMPLES * S)

        def build(count, store_of):
            def call(i):
                src = buf.ptr + ((i % slots) * sq_bytes if count == 1 else (i % NBATCH) * BATCH * sq_bytes)
                R._check(L.rsm_proof_nodes_dev(ctx, src, W, S, count, pp, store_of(i), roots.ptr, status.ptr, None))
            return call

        def roots_only(count):
            def call(i):
                src = buf.ptr + ((i % slots) * sq_bytes if count == 1 else (i % NBATCH) * BATCH * sq_bytes)
                if p is None:
                    R._check(L.rsm_roots_squares_dev(ctx, src, W, S, count, roots.ptr, None))
                else:
                    R._check(L.rsm_nmt_roots_squares_dev(ctx, src, W, S, count, pp, roots.ptr, status.ptr, None))
            return call

        res = {"tree": name, "width": W, "share_size": S, "reps": a.reps,
               "store_bytes_per_square": one, "record_bytes": rb}
        res["build_1_ms"] = timed(build(1, lambda i: store1.ptr + (i % nstores) * one))
        res["roots_1_ms"] = timed(roots_only(1))
        res["build_32_ms"] = timed(build(BATCH, lambda i: storeb.ptr))
        res["roots_32_ms"] = timed(roots_only(BATCH))
        res["build_to_roots_1"] = res["build_1_ms"] / res["roots_1_ms"]
        res["build_to_roots_32"] = res["build_32_ms"] / res["roots_32_ms"]
        # the store of batch 0 for the gather (the last timed build may have been batch 1)
        R._check(L.rsm_proof_nodes_dev(ctx, buf.ptr, W, S, BATCH, pp, storeb.ptr, None, None, None))
        res["gather_4096_ms"] = timed(lambda i: R._check(L.rsm_proofs_dev(
            ctx, storeb.ptr, buf.ptr, W, S, BATCH, pp, arr, NSAMPLES, recs.ptr, shs.ptr, None)))
        res["samples_per_s"] = NSAMPLES / (res["gather_4096_ms"] * 1e-3)
        R._check(L.rsm_sync(ctx))
        print(json.dumps({k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in res.items()}), flush=True)
        for b in (store1, storeb, roots, status, recs, shs):
            b.free()
    for e in ev:
        L.rsm_event_destroy(e)
    buf.free()


if __name__ == "__main__":
    main()
