#!/usr/bin/env python3
"""Timing of Repair on device-resident squares (DESIGN.md §5 "Device-resident Repair"):

  single    one half-erased k = 128, S = 512 square (BenchmarkRepair's shape: k of every
            row's 2k cells erased) through rsm_repair_squares_dev, beside rsm_eds_repair
            of the same cells on a host square (its zero-copy fast path) in the same run;
  batch     64 such squares in one call against 64 calls of one square each;
  sweeps    an avalanche map at k = 128 (every cell erased independently, the first seed
            the peeling model completes in >= 6 sweeps): time per sweep.

Every call is synchronous, so it is timed as a whole with rsm_event_* on the context
stream (the second event is recorded after the call has returned) and, beside it, with
the host clock; the figure is the median of --reps (>= 20) calls after warm-up calls.
Between calls, outside the timed window, the presence map is restored from a device
copy (the erased cells keep whatever the last call rebuilt: no decoder reads a cell
whose presence byte is 0) and the host square is imported afresh.  One JSON line.

    python scripts/diag/repair_dev_bench.py [--reps 24] > profiles/repair_dev_bench.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import rsmt2d_amd as R  # noqa: E402

K, S, BATCH = 128, 512, 64
W = 2 * K
AVALANCHE_T = 148  # a cell is erased iff its byte is below T (tests/repair_patterns.py's value at k = 128)


def model(pres):
    """The schedule's peeling model: (sweeps, decoded vectors, complete)."""
    p = pres.copy()
    sweeps = vectors = 0
    while True:
        progress = False
        for axis in (0, 1):
            have = p.sum(axis=1 - axis)
            todo = np.flatnonzero((have >= K) & (have < W))
            if todo.size == 0:
                continue
            if axis == 0:
                p[todo, :] = True
            else:
                p[:, todo] = True
            sweeps, vectors, progress = sweeps + 1, vectors + int(todo.size), True
        if not progress:
            return sweeps, vectors, bool(p.all())


def half_erased(rng):
    pres = np.ones((W, W), bool)
    for r in range(W):
        pres[r, rng.choice(W, size=K, replace=False)] = False
    return pres


def avalanche():
    for seed in range(256):
        pres = np.random.default_rng([0xA7A1, seed]).integers(0, 256, (W, W)) >= AVALANCHE_T
        sweeps, vectors, done = model(pres)
        if done and sweeps >= 6:
            return pres, sweeps, vectors
    raise SystemExit("no avalanche seed below 256")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    L, ctx = R.library(), R.device_context(0)
    rng = np.random.default_rng(1)
    sq_bytes, cells = W * W * S, W * W

    # BATCH copies of one valid square, its committed roots
    buf = R.DeviceBuffer(BATCH * sq_bytes)
    host = np.zeros((W, W, S), np.uint8)
    host[:K, :K] = rng.integers(0, 256, (K, K, S), dtype=np.uint8)
    buf.upload(host.reshape(-1))
    R._check(L.rsm_extend_squares_dev(ctx, buf.ptr, K, S, 1, None))
    R._check(L.rsm_sync(ctx))
    valid = buf.download(sq_bytes)
    for i in range(1, BATCH):
        buf.upload(valid, i * sq_bytes)
    roots = R.DeviceBuffer(BATCH * 2 * W * 32)
    R._check(L.rsm_roots_squares_dev(ctx, buf.ptr, W, S, BATCH, roots.ptr, None))
    R._check(L.rsm_sync(ctx))
    root_bytes = roots.download(2 * W * 32).tobytes()
    rr, cr = root_bytes[:W * 32], root_bytes[W * 32:]

    pres_half = half_erased(rng)
    pres_av, av_sweeps, av_vectors = avalanche()
    keep = R.DeviceBuffer(BATCH * cells)  # pristine presence maps
    pres = R.DeviceBuffer(BATCH * cells)
    work = R.DeviceBuffer(int(L.rsm_repair_work_bytes(K, S, BATCH, None)))
    res = (R.RepairResult * BATCH)()
    ev = []
    for _ in range(2):
        e = ctypes.c_void_p()
        R._check(L.rsm_event_create(ctx, ctypes.byref(e)))
        ev.append(e)

    def timed(prepare, call):
        """(median event ms, median host-clock ms) of call() after prepare(), per rep."""
        dev, wall = [], []
        for i in range(a.warmup + a.reps):
            prepare()
            R._check(L.rsm_sync(ctx))
            R._check(L.rsm_event_record(ctx, ev[0], None))
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            R._check(L.rsm_event_record(ctx, ev[1], None))
            ms = ctypes.c_float()
            R._check(L.rsm_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)))
            if i >= a.warmup:
                dev.append(ms.value)
                wall.append((t1 - t0) * 1e3)
        return statistics.median(dev), statistics.median(wall)

    def set_maps(m):
        for i in range(BATCH):
            keep.upload(m.astype(np.uint8).reshape(-1), i * cells)

    def restore(count):
        R._check(L.rsm_memcpy(ctx, pres.ptr, keep.ptr, count * cells, 2))

    def repair(first, count, want):
        R._check(L.rsm_repair_squares_dev(ctx, buf.ptr + first * sq_bytes, pres.ptr + first * cells, K, S, count, None,
                                          roots.ptr + first * 2 * W * 32, work.ptr, res, None))
        for s in range(count):
            got = (res[s].status, res[s].sweeps, res[s].decoded_vectors, res[s].missing)
            if got != want:
                raise SystemExit("square %d: %r, expected %r" % (first + s, got, want))

    # ---- single: the device form beside the host form of the same cells ----
    set_maps(pres_half)
    one = (R.REPAIR_OK, 1, W, 0)
    single_dev = timed(lambda: restore(1), lambda: repair(0, 1, one))
    vcells = np.ascontiguousarray(valid).reshape(cells, S)
    ptrs = np.arange(cells, dtype=np.uint64) * np.uint64(S) + np.uint64(vcells.ctypes.data)
    ptrs[~pres_half.reshape(-1)] = 0
    lens = np.full(cells, S, np.uint32)
    handle = [None]

    def import_host():
        if handle[0] is not None:
            L.rsm_eds_free(handle[0])
        h = ctypes.c_void_p()
        R._check(L.rsm_eds_import(ctx, ptrs.ctypes.data, lens.ctypes.data, cells, ctypes.byref(h)))
        handle[0] = h.value

    def repair_host():
        R._check(L.rsm_eds_repair(handle[0], rr, cr, 32, None, None, None))

    single_host = timed(import_host, repair_host)
    st = R.RepairStats()
    R._check(L.rsm_eds_repair_stats(handle[0], ctypes.byref(st)))
    L.rsm_eds_free(handle[0])

    # ---- batch: one call of BATCH squares against BATCH calls of one ----
    batch = timed(lambda: restore(BATCH), lambda: repair(0, BATCH, one))

    def singles():
        for i in range(BATCH):
            repair(i, 1, one)

    singles_ms = timed(lambda: restore(BATCH), singles)

    # ---- sweeps: time per sweep of a many-sweep map ----
    set_maps(pres_av)
    av = (R.REPAIR_OK, av_sweeps, av_vectors, 0)
    av_one = timed(lambda: restore(1), lambda: repair(0, 1, av))
    av_batch = timed(lambda: restore(BATCH), lambda: repair(0, BATCH, av))

    out = {"k": K, "share_size": S, "reps": a.reps, "batch": BATCH,
           "single_dev_ms": single_dev[0], "single_dev_host_clock_ms": single_dev[1],
           "single_host_ms": single_host[0], "single_host_host_clock_ms": single_host[1],
           "single_host_fast_path": int(st.fast_path),
           "batch_call_ms": batch[0], "batch_per_square_ms": batch[0] / BATCH,
           "batch_as_single_calls_ms": singles_ms[0], "batch_as_single_calls_per_square_ms": singles_ms[0] / BATCH,
           "avalanche_sweeps": av_sweeps, "avalanche_vectors": av_vectors,
           "avalanche_ms": av_one[0], "avalanche_per_sweep_ms": av_one[0] / av_sweeps,
           "avalanche_batch_ms": av_batch[0], "avalanche_batch_per_sweep_per_square_ms": av_batch[0] / av_sweeps / BATCH}
    print(json.dumps({k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in out.items()}), flush=True)
    for e in ev:
        L.rsm_event_destroy(e)
    for b in (buf, roots, keep, pres, work):
        b.free()


if __name__ == "__main__":
    main()
