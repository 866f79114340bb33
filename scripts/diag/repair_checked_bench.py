#!/usr/bin/env python3
"""Timing of Repair with attribution on device-resident squares (DESIGN.md §5 "Checked
Repair"), beside rsm_repair_squares_dev and rsm_eds_repair of the same cells in the same
run.  k = 128, S = 512; four workloads:

  single     one half-erased square (k of every row's 2k cells erased): one sweep;
  batch      64 of them in one call (rsm_eds_repair: one square, 64 times is 64 of these);
  avalanche  every cell erased independently, the first seed the peeling model completes
             in >= 6 sweeps;
  a_row_k    the attribution case: a minimum-weight row codeword XOR-ed into row k of a
             valid square, the roots committed to the altered square, half-erased.  Every
             row is a codeword, k + 1 columns are not: the checked call names column 0 in
             round 1, the unchecked call says ENCODING, rsm_eds_repair falls back to its
             exact sequential solver and names a column.

Calls are timed as in repair_dev_bench.py: rsm_event_* around the synchronous call and the
host clock beside it, medians of --reps (>= 20) calls after warm-up; presence maps are
restored and host squares imported afresh outside the timed window.  One JSON line.

    python scripts/diag/repair_checked_bench.py [--reps 24] > profiles/repair_checked_bench.json
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
from repair_dev_bench import BATCH, K, S, W, avalanche, half_erased  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated workloads (default: all four)")
    ap.add_argument("--forms", default="checked,plain,eds_repair_one_square",
                    help="comma-separated forms to time (a kernel trace of one form: --only single --forms checked)")
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    L, ctx = R.library(), R.device_context(0)
    rng = np.random.default_rng(1)
    sq_bytes, cells = W * W * S, W * W

    # BATCH copies of one valid square and their roots; then the altered square and its roots
    buf = R.DeviceBuffer((BATCH + 1) * sq_bytes)
    host = np.zeros((W, W, S), np.uint8)
    host[:K, :K] = rng.integers(0, 256, (K, K, S), dtype=np.uint8)
    buf.upload(host.reshape(-1))
    R._check(L.rsm_extend_squares_dev(ctx, buf.ptr, K, S, 1, None))
    R._check(L.rsm_sync(ctx))
    valid = buf.download(sq_bytes)
    for i in range(1, BATCH):
        buf.upload(valid, i * sq_bytes)
    data = [bytes([0x5A]) + bytes(S - 1)] + [bytes(S)] * (K - 1)
    delta = np.frombuffer(b"".join(data + list(R.NewLeoRSCodec().Encode(data))), np.uint8).reshape(W, S)
    altered = valid.reshape(W, W, S).copy()
    altered[K] ^= delta
    buf.upload(altered.reshape(-1), BATCH * sq_bytes)
    roots = R.DeviceBuffer((BATCH + 1) * 2 * W * 32)
    R._check(L.rsm_roots_squares_dev(ctx, buf.ptr, W, S, BATCH + 1, roots.ptr, None))
    R._check(L.rsm_sync(ctx))
    root_bytes = roots.download().tobytes()

    pres_half = half_erased(rng)
    pres_av, av_sweeps, av_vectors = avalanche()
    keep = R.DeviceBuffer(BATCH * cells)  # pristine presence maps
    pres = R.DeviceBuffer(BATCH * cells)
    work = R.DeviceBuffer(max(int(L.rsm_repair_work_bytes(K, S, BATCH, None)),
                              int(L.rsm_repair_checked_work_bytes(K, S, BATCH, None))))
    res, chk = (R.RepairResult * BATCH)(), (R.RepairCheck * BATCH)()
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
        return round(statistics.median(dev), 4), round(statistics.median(wall), 4)

    def set_maps(m):
        for i in range(BATCH):
            keep.upload(m.astype(np.uint8).reshape(-1), i * cells)

    def restore(count):
        R._check(L.rsm_memcpy(ctx, pres.ptr, keep.ptr, count * cells, 2))

    def device(first, count, want, checked):
        args = (ctx, buf.ptr + first * sq_bytes, pres.ptr, K, S, count, None, roots.ptr + first * 2 * W * 32, work.ptr)
        if checked:
            R._check(L.rsm_repair_squares_checked_dev(*args, res, chk, None))
        else:
            R._check(L.rsm_repair_squares_dev(*args, res, None))
        for s in range(count):
            got = (res[s].status, res[s].sweeps, res[s].decoded_vectors, res[s].missing)
            if got != want:
                raise SystemExit("square %d (%s): %r, expected %r" % (first + s, "checked" if checked else "plain", got, want))

    handle = [None]
    lens = np.full(cells, S, np.uint32)

    def host_form(square, m, rr, cr, want_rc):
        """(import, repair) closures of rsm_eds_repair on the given cells of `square`."""
        vcells = np.ascontiguousarray(square).reshape(cells, S)
        ptrs = np.arange(cells, dtype=np.uint64) * np.uint64(S) + np.uint64(vcells.ctypes.data)
        ptrs[~m.reshape(-1)] = 0

        def imp():
            if handle[0] is not None:
                L.rsm_eds_free(handle[0])
            h = ctypes.c_void_p()
            R._check(L.rsm_eds_import(ctx, ptrs.ctypes.data, lens.ctypes.data, cells, ctypes.byref(h)))
            handle[0] = h.value

        def rep():
            rc = L.rsm_eds_repair(handle[0], rr, cr, 32, None, None, None)
            if rc != want_rc:
                raise SystemExit("rsm_eds_repair returned %d, expected %d" % (rc, want_rc))

        return (imp, rep), vcells

    def three(first, count, m, want_checked, want_plain, square, want_rc):
        """The three forms on one workload: {form: (event ms, host-clock ms)}."""
        set_maps(m)
        rr = root_bytes[first * 2 * W * 32:][:W * 32]
        cr = root_bytes[first * 2 * W * 32 + W * 32:][:W * 32]
        (imp, rep), keepalive = host_form(square, m, rr, cr, want_rc)
        forms = {"checked": lambda: timed(lambda: restore(count), lambda: device(first, count, want_checked, True)),
                 "plain": lambda: timed(lambda: restore(count), lambda: device(first, count, want_plain, False)),
                 "eds_repair_one_square": lambda: timed(imp, rep)}
        out = {f: forms[f]() for f in a.forms.split(",")}
        del keepalive
        return out

    one = (R.REPAIR_OK, 1, W, 0)
    av = (R.REPAIR_OK, av_sweeps, av_vectors, 0)
    vsq = valid.reshape(W, W, S)
    loads = {"single": lambda: three(0, 1, pres_half, one, one, vsq, R.RSM_OK),
             "batch64": lambda: three(0, BATCH, pres_half, one, one, vsq, R.RSM_OK),
             "avalanche": lambda: three(0, 1, pres_av, av, av, vsq, R.RSM_OK),
             "a_row_k": lambda: three(BATCH, 1, pres_half, (R.REPAIR_BYZANTINE, 1, W, 0), (R.REPAIR_ENCODING, 1, W, 0),
                                      altered, R.RSM_EBYZANTINE)}
    out = {"k": K, "share_size": S, "reps": a.reps, "batch": BATCH, "avalanche_sweeps": av_sweeps,
           "avalanche_vectors": av_vectors}
    for name in (a.only.split(",") if a.only else list(loads)):
        out[name] = loads[name]()
    if "a_row_k" in out and "checked" in out["a_row_k"]:
        out["a_row_k_named"] = [int(chk[0].axis), int(chk[0].index), int(chk[0].round), int(chk[0].reason)]
    print(json.dumps(out), flush=True)
    if handle[0] is not None:
        L.rsm_eds_free(handle[0])
    for e in ev:
        L.rsm_event_destroy(e)
    for b in (buf, roots, keep, pres, work):
        b.free()


if __name__ == "__main__":
    main()
