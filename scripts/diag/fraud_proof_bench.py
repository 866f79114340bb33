#!/usr/bin/env python3
"""Timing of bad-encoding fraud-proof validation (DESIGN.md §5 "Fraud proofs") at k = 128,
S = 512, for the DefaultTree and the NMT (29-byte namespaces), n = 1, 64 and 512 proofs, in
one run:

  new       rsm_fraud_proofs_verify_dev over the n packed vectors (k of every vector's 2k
            slots present) with their 2k share proofs each;
  assembled the path it replaces, from existing calls: rsm_proofs_verify_dev of the same
            n * 2k samples (the statuses are downloaded), then per vector, from host memory
            as bench.py's bench_fraud_proof does, rsm_decode, the host tree root of the
            rebuilt vector (compared with the committed one), rsm_encode of its first half
            and the parity compare.

The operands are made on the device the way a node makes them: one valid square, its roots
and node store, rsm_proofs_dev over rsm_fraud_proof_samples of every ref, and
rsm_vectors_gather_dev under a checkerboard presence map (every row and column keeps k
cells).  Both paths must find every proof CONSISTENT.  Every call is synchronous, so it is
timed by the host clock; the figure is the median of --reps (>= 20) calls after warm-up.

    python scripts/diag/fraud_proof_bench.py [--reps 24] [--out profiles/fraud_proof_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import rsmt2d_amd as R  # noqa: E402

K, S, NS = 128, 512, 29
W = 2 * K
SIZES = (1, 64, 512)


def square(ctx, L, nmt, rng):
    """One valid [W][W][S] square on the device (NMT: quadrant 0 sorted by namespace)."""
    host = np.zeros((W, W, S), np.uint8)
    ods = rng.integers(0, 256, (K * K, S), dtype=np.uint8)
    if nmt is not None:
        ods = ods[np.lexsort(ods[:, :NS].T[::-1])]
    host[:K, :K] = ods.reshape(K, K, S)
    buf = R.DeviceBuffer(host.nbytes)
    buf.upload(host.reshape(-1))
    R._check(L.rsm_extend_squares_dev(ctx, buf.ptr, K, S, 1, None))
    R._check(L.rsm_sync(ctx))
    return buf


def median_ms(call, reps, warmup):
    t = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        call()
        if i >= warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def run(L, ctx, nmt, reps, warmup):
    rng = np.random.default_rng(0xF4A)
    pp = ctypes.byref(nmt) if nmt is not None else None
    nl = 32 if nmt is None else 2 * NS + 32
    rb = int(L.rsm_proof_record_bytes(W, pp))
    eds = square(ctx, L, nmt, rng)
    roots, status = R.DeviceBuffer(2 * W * nl), R.DeviceBuffer(2 * W * 4)
    nodes = R.DeviceBuffer(int(L.rsm_proof_nodes_bytes(W, pp, 1)))
    R._check(L.rsm_proof_nodes_dev(ctx, eds.ptr, W, S, 1, pp, nodes.ptr, roots.ptr, status.ptr, None))
    R._check(L.rsm_sync(ctx))
    table = roots.download().reshape(2, W, nl)
    pres = R.DeviceBuffer(W * W)
    pres.upload(((np.add.outer(np.arange(W), np.arange(W)) & 1) == 0).astype(np.uint8).reshape(-1))
    out = {}
    for n in SIZES:
        refs = [(0, i & 1, (i * 37 + (i >> 1)) % W) for i in range(n)]
        samples = [s for r in refs for s in R.fraud_proof_samples(r[1], r[2], K, r[0])]
        arr_s, arr_r = R._records(R.Sample, samples), R._records(R.RootRef, refs)
        recs, spare = R.DeviceBuffer(n * W * rb), R.DeviceBuffer(n * W * S)
        shares, present, st = R.DeviceBuffer(n * W * S), R.DeviceBuffer(max(n * W, 16)), R.DeviceBuffer(n * W * 4)
        work = R.DeviceBuffer(int(L.rsm_fraud_work_bytes(K, S, n, pp)))
        R._check(L.rsm_proofs_dev(ctx, nodes.ptr, eds.ptr, W, S, 1, pp, arr_s, n * W, recs.ptr, spare.ptr, None))
        R._check(L.rsm_vectors_gather_dev(ctx, eds.ptr, pres.ptr, K, S, 1, arr_r, n, shares.ptr, present.ptr, None))
        R._check(L.rsm_sync(ctx))
        h_sh = shares.download().reshape(n, W, S)
        h_pr = present.download()[:n * W].reshape(n, W).copy()
        verdicts = (R.FraudVerdict * n)()

        def new():
            R._check(L.rsm_fraud_proofs_verify_dev(ctx, shares.ptr, present.ptr, recs.ptr, roots.ptr, K, S, 1, pp, arr_r, n,
                                                   work.ptr, verdicts, None))
            if any((v.verdict, v.present) != (R.FRAUD_CONSISTENT, K) for v in verdicts):
                raise SystemExit("the new call found a proof that is not CONSISTENT")

        vec = np.empty((W, S), np.uint8)
        par = np.empty((K, S), np.uint8)
        vp = (ctypes.c_void_p * W)(*[vec.ctypes.data + i * S for i in range(W)])
        ppar = (ctypes.c_void_p * K)(*[par.ctypes.data + i * S for i in range(K)])
        root, rlen = ctypes.create_string_buffer(128), ctypes.c_uint32()
        split = {}

        def assembled():
            t0 = time.perf_counter()
            R._check(L.rsm_proofs_verify_dev(ctx, shares.ptr, recs.ptr, roots.ptr, W, S, 1, pp, arr_s, n * W, st.ptr, None))
            R._check(L.rsm_sync(ctx))
            words = st.download().view(np.uint32).reshape(n, W)
            if (words[h_pr != 0] != 0).any():
                raise SystemExit("a present share failed rsm_proofs_verify_dev")
            t1 = time.perf_counter()
            for i, (_, axis, index) in enumerate(refs):
                vec[:] = h_sh[i] * (h_pr[i] != 0)[:, None]
                R._check(L.rsm_decode(ctx, vp, h_pr[i].ctypes.data, W, S))
                rlen.value = 128
                if nmt is None:
                    R._check(L.rsm_default_tree_root(None, axis, index, vp, W, S, root, ctypes.byref(rlen)))
                else:
                    R._check(L.rsm_nmt_tree_root(pp, axis, index, vp, W, S, root, ctypes.byref(rlen)))
                R._check(L.rsm_encode(ctx, vp, K, S, ppar))
                if root.raw[:nl] != table[axis, index].tobytes() or not np.array_equal(par, vec[K:]):
                    raise SystemExit("the assembled path found a proof that is not consistent")
            split.setdefault("verify", []).append((t1 - t0) * 1e3)

        r = reps if n < 512 else max(20, reps // 2)
        new_ms = median_ms(new, r, warmup)
        old_ms = median_ms(assembled, r, warmup)
        out[str(n)] = {"new_ms": round(new_ms, 4), "assembled_ms": round(old_ms, 4),
                       "assembled_share_verify_ms": round(statistics.median(split["verify"]), 4),
                       "ratio_assembled_over_new": round(old_ms / new_ms, 2),
                       "new_us_per_proof": round(new_ms * 1e3 / n, 2), "reps": r}
        for b in (recs, spare, shares, present, st, work):
            b.free()
    for b in (eds, roots, status, nodes, pres):
        b.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fraud_proof_bench.json"))
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    L, ctx = R.library(), R.device_context(0)
    res = {"k": K, "share_size": S, "present_per_vector": K, "clock": "host, synchronous calls, median",
           "default_tree": run(L, ctx, None, a.reps, a.warmup),
           "nmt_ns29": run(L, ctx, R.NmtParams(NS, 1, K), a.reps, a.warmup)}
    text = json.dumps(res, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
