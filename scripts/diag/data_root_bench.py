#!/usr/bin/env python3
"""Timing of the data root (DESIGN.md §4 "Data root") at W = 256, S = 512:

  (a) rsm_data_roots_dev over the NMT roots (29-byte namespaces, 90-byte roots) of 512
      squares and of one square, each beside the rsm_nmt_roots_squares_dev launch of the
      same batch -- existing code, the yardstick -- in the same run;
  (b) rsm_proofs_verify_data_root_dev of n = 65,536 and n = 256 valid samples beside
      rsm_proofs_verify_dev on the same samples, for the DefaultTree and the NMT, the
      sample upload included in both.

SHA-256 blocks, from the code: a data root hashes 2W leaves of 2 blocks (91 bytes; 1 for
a 33-byte DefaultTree leaf) and 2W - 1 nodes of 2; the roots launch W * W leaves of
S/64 + 1 blocks and 2W trees of W - 1 nodes of 3 (NMT).  A sample of the plain verifier is
S/64 + 1 leaf blocks and L = 8 fold steps of 2 (DefaultTree) or 3 (NMT) blocks; the chain
adds the candidate's leaf (1 or 2 blocks) and L2 = 9 fold steps of 2.

Protocol: every call is timed on its own with rsm_event_* on the context stream, after
warm-up calls; the figure is the median of --reps (>= 20) calls.  The two calls of a
comparison alternate within one loop.  A 384 MiB buffer is rewritten before every timed
call, so no call finds its input in the 256 MiB Infinity Cache; the verifier's shares and
records come from a pool of 6 * 65,536 proofs, a different part each call; the 512-square
batch (16 GiB) is its own rotation.  The first call of each size is checked: the data
roots of the batch against the host restatement, every status 0.  One JSON line per
comparison.

    python scripts/diag/data_root_bench.py [--reps 24] > profiles/data_root_bench.json
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

W, S, NS, SQUARES, BATCH = 256, 512, 29, 512, 32
SIZES, SETS = (256, 65536), 6
LEVELS, LEVELS2 = 8, 9
FLUSH = 384 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--squares", type=int, default=SQUARES, help="squares of comparison (a) (rehearsals: fewer)")
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    L, ctx = R.library(), R.device_context(0)
    k, sq_bytes, nsq = W // 2, W * W * S, max(a.squares, BATCH)
    rng = np.random.default_rng(1)
    sq = rng.integers(0, 256, (W, W, S), dtype=np.uint8)
    q0 = sq[:k, :k].reshape(k * k, S)
    sq[:k, :k] = q0[np.lexsort(q0[:, :NS][:, ::-1].T)].reshape(k, k, S)
    buf = R.DeviceBuffer(nsq * sq_bytes)
    buf.upload(sq.reshape(-1), 0)
    have = 1
    while have < nsq:  # the same square in every slot, copied on the device
        n = min(have, nsq - have)
        R._check(L.rsm_memcpy(ctx, buf.ptr + have * sq_bytes, buf.ptr, n * sq_bytes, 2))
        have += n
    flush = R.DeviceBuffer(FLUSH)
    ev = []
    for _ in range(2):
        e = ctypes.c_void_p()
        R._check(L.rsm_event_create(ctx, ctypes.byref(e)))
        ev.append(e)

    def timed_pair(first, second):
        """Median device milliseconds of first(i) and of second(i), alternating."""
        out = ([], [])
        for i in range(a.warmup + a.reps):
            for which, call in enumerate((first, second)):
                R._check(L.rsm_dev_fill_random(ctx, flush.ptr, FLUSH, 2 * i + which))
                R._check(L.rsm_event_record(ctx, ev[0], None))
                call(i)
                R._check(L.rsm_event_record(ctx, ev[1], None))
                ms = ctypes.c_float()
                R._check(L.rsm_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)))
                if i >= a.warmup:
                    out[which].append(ms.value)
        return statistics.median(out[0]), statistics.median(out[1])

    p = R.NmtParams(NS, 1, k)
    pp = ctypes.byref(p)
    leaf_blocks = S // 64 + 1

    # ---- (a) the data root beside the roots launch of the same batch ----
    RL = 2 * NS + 32
    want = None
    for count in (a.squares, 1):
        roots, tstat, dr = R.DeviceBuffer(count * 2 * W * RL), R.DeviceBuffer(count * 2 * W * 4), R.DeviceBuffer(count * 32)

        def roots_call(i):
            R._check(L.rsm_nmt_roots_squares_dev(ctx, buf.ptr, W, S, count, pp, roots.ptr, tstat.ptr, None))

        def data_roots_call(i):
            R._check(L.rsm_data_roots_dev(ctx, roots.ptr, W, RL, count, dr.ptr, None, None))

        roots_call(0)
        data_roots_call(0)
        R._check(L.rsm_sync(ctx))
        if tstat.download(count * 2 * W * 4).any():
            raise SystemExit("a tree of the batch failed")
        if want is None:
            out = ctypes.create_string_buffer(32)
            R._check(L.rsm_data_root(roots.download(2 * W * RL).tobytes(), W, RL, out))
            want = out.raw
        if dr.download(count * 32).tobytes() != want * count:
            raise SystemExit("a device data root differs from the host restatement")
        roots_ms, dr_ms = timed_pair(roots_call, data_roots_call)
        roots_blocks = count * (W * W * leaf_blocks + 2 * W * (W - 1) * 3)
        dr_blocks = count * (2 * W * 2 + (2 * W - 1) * 2)
        res = {"comparison": "a", "tree": "NMT", "width": W, "share_size": S, "squares": count, "reps": a.reps,
               "nmt_roots_squares_ms": roots_ms, "data_roots_ms": dr_ms, "data_roots_to_roots_time": dr_ms / roots_ms,
               "data_roots_to_roots_sha_blocks": dr_blocks / roots_blocks}
        print(json.dumps({k_: (round(v, 6) if isinstance(v, float) else v) for k_, v in res.items()}), flush=True)
        for b in (roots, tstat, dr):
            b.free()

    # ---- (b) the chained verifier beside the plain one, on the same samples ----
    pool = SETS * SIZES[-1]
    samples = np.stack([rng.integers(BATCH, size=pool), rng.integers(2, size=pool), rng.integers(W, size=pool),
                        rng.integers(W, size=pool)], axis=1).astype(np.uint32)
    refs = np.ascontiguousarray(samples[:, :3])
    rrb = int(L.rsm_data_root_record_bytes(W))
    for name, p, node_blocks, cand_blocks in (("DefaultTree", None, 2, 1), ("NMT", R.NmtParams(NS, 1, k), 3, 2)):
        pp = ctypes.byref(p) if p is not None else None
        nl = 32 if p is None else 2 * NS + 32
        rb = int(L.rsm_proof_record_bytes(W, pp))
        store = R.DeviceBuffer(int(L.rsm_proof_nodes_bytes(W, pp, BATCH)))
        rstore = R.DeviceBuffer(int(L.rsm_data_root_nodes_bytes(W, BATCH)))
        roots, tstat, dr = R.DeviceBuffer(BATCH * 2 * W * nl), R.DeviceBuffer(BATCH * 2 * W * 4), R.DeviceBuffer(BATCH * 32)
        recs, shs, status = R.DeviceBuffer(pool * rb), R.DeviceBuffer(pool * S), R.DeviceBuffer(SIZES[-1] * 4)
        rrecs = R.DeviceBuffer(pool * rrb)
        R._check(L.rsm_proof_nodes_dev(ctx, buf.ptr, W, S, BATCH, pp, store.ptr, roots.ptr, tstat.ptr, None))
        R._check(L.rsm_proofs_dev(ctx, store.ptr, buf.ptr, W, S, BATCH, pp, samples.ctypes.data, pool, recs.ptr, shs.ptr,
                                  None))
        R._check(L.rsm_data_roots_dev(ctx, roots.ptr, W, nl, BATCH, dr.ptr, rstore.ptr, None))
        R._check(L.rsm_root_proofs_dev(ctx, rstore.ptr, W, BATCH, refs.ctypes.data, pool, rrecs.ptr, None))
        R._check(L.rsm_sync(ctx))
        store.free()
        rstore.free()
        plain_blocks = leaf_blocks + LEVELS * node_blocks
        chain_blocks = plain_blocks + cand_blocks + LEVELS2 * 2
        for n in SIZES:
            def first_of(i, n=n):
                return (i * SIZES[-1] + (i // SETS) * n) % (pool - n + 1)  # another part of the pool each call

            def plain(i, n=n):
                f = first_of(i)
                R._check(L.rsm_proofs_verify_dev(ctx, shs.ptr + f * S, recs.ptr + f * rb, roots.ptr, W, S, BATCH, pp,
                                                 samples[f:].ctypes.data, n, status.ptr, None))

            def chained(i, n=n):
                f = first_of(i)
                R._check(L.rsm_proofs_verify_data_root_dev(ctx, shs.ptr + f * S, recs.ptr + f * rb, rrecs.ptr + f * rrb,
                                                           dr.ptr, W, S, BATCH, pp, samples[f:].ctypes.data, n, status.ptr,
                                                           None))

            for call in (plain, chained):
                R._check(L.rsm_dev_fill_random(ctx, status.ptr, n * 4, 9))
                call(1)
                R._check(L.rsm_sync(ctx))
                if status.download(n * 4).any():
                    raise SystemExit("%s: a valid sample did not verify (%s)" % (name, call.__name__))
            plain_ms, chain_ms = timed_pair(plain, chained)
            res = {"comparison": "b", "tree": name, "width": W, "share_size": S, "samples": n, "reps": a.reps,
                   "verify_us": plain_ms * 1e3, "verify_data_root_us": chain_ms * 1e3,
                   "data_root_to_plain_time": chain_ms / plain_ms, "sha_blocks_per_sample": plain_blocks,
                   "sha_blocks_per_sample_data_root": chain_blocks, "data_root_to_plain_sha_blocks": chain_blocks / plain_blocks}
            print(json.dumps({k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in res.items()}), flush=True)
        R._check(L.rsm_sync(ctx))
        for b in (roots, tstat, dr, recs, shs, status, rrecs):
            b.free()
    for e in ev:
        L.rsm_event_destroy(e)
    flush.free()
    buf.free()


if __name__ == "__main__":
    main()
