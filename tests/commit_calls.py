"""TEST INFRASTRUCTURE ONLY -- the device calls the share commitment tests share
(rsm_blob_commitments_dev, rsm_proof_nodes_dev + rsm_commitments_dev), every output between
guard bands (device_calls.Guarded).  Importing this module touches no GPU."""
import ctypes

import numpy as np

import commitments as C
import rsmt2d_amd as R
from device_calls import Guarded
from range_calls import fill


def total_roots(lens, t):
    return sum(len(C.sizes(n, C.width(n, t))) for n in lens)


def shares_path(lib, p, S, blobs, t, lead=0):
    """One rsm_blob_commitments_dev over `blobs` (each a list of shares, or an [n][S] array),
    packed behind `lead` shares that belong to no blob: (rc, commitments [n] bytes, status
    words).  The shares and the offsets are inputs: the call must leave the shares alone."""
    ctx, n = R.device_context(0), len(blobs)
    parts = [np.frombuffer(b"".join(b), np.uint8) if isinstance(b, list) else np.ascontiguousarray(b).reshape(-1) for b in blobs]
    lens = [len(x) // S for x in parts]
    packed = np.concatenate([np.full(lead * S, 0xA5, np.uint8)] + parts)
    offs = np.cumsum([lead] + lens).astype(np.uint32)
    wb = int(lib.rsm_commit_work_bytes(sum(lens), total_roots(lens, t), ctypes.byref(p)))
    shs, work = Guarded(len(packed), 0, 61), Guarded(max(wb, 16), 0, 62)
    com, st = Guarded(n * 32, 3, 63), Guarded(n * 4, 4, 64)
    try:
        fill(shs, packed)
        arr = (ctypes.c_uint32 * (n + 1))(*[int(o) for o in offs])
        rc = lib.rsm_blob_commitments_dev(ctx, shs.ptr, S, ctypes.byref(p), t, arr, n, work.ptr, com.ptr, st.ptr, None)
        R._check(lib.rsm_sync(ctx))
        assert np.array_equal(shs.result(), packed), "the call wrote into the shares"
        work.result()
        c = com.result().tobytes()
        return rc, [c[i * 32:(i + 1) * 32] for i in range(n)], [int(x) for x in st.result().view(np.uint32)]
    finally:
        for g in (shs, work, com, st):
            g.free()


class Store:
    """The NMT node store, roots and tree status words of a [count][W][W][S] batch."""

    def __init__(self, lib, batch, p):
        self.lib, self.p = lib, p
        self.count, self.W, _, self.S = batch.shape
        self.nl = 2 * p.namespace_size + 32
        ctx, pp = R.device_context(0), ctypes.byref(p)
        nbytes = int(lib.rsm_proof_nodes_bytes(self.W, pp, self.count))
        assert nbytes > 0
        self.nodes, self.status = R.DeviceBuffer(nbytes), R.DeviceBuffer(self.count * 2 * self.W * 4)
        roots = R.DeviceBuffer(self.count * 2 * self.W * self.nl)
        d = R.DeviceBuffer(batch.nbytes)
        try:
            d.upload(batch.reshape(-1))
            R._check(lib.rsm_proof_nodes_dev(ctx, d.ptr, self.W, self.S, self.count, pp, self.nodes.ptr, roots.ptr,
                                             self.status.ptr, None))
            R._check(lib.rsm_sync(ctx))
            self.roots = roots.download().reshape(self.count, 2, self.W, self.nl).copy()
            self.tree_status = self.status.download().view(np.uint32).reshape(self.count, 2 * self.W).copy()
        finally:
            d.free()
            roots.free()

    def commitments(self, blobs, t, want_roots=True):
        """One rsm_commitments_dev over (square, start, len) blobs: (rc, commitments, status
        words, per-blob lists of subtree roots or None).  On an error return nothing may
        have been written."""
        lib, ctx, n = self.lib, R.device_context(0), len(blobs)
        counts = [len(C.sizes(b[2], C.width(b[2], t))) if b[2] else 0 for b in blobs]
        com, st = Guarded(max(n * 32, 1), 3, 71), Guarded(max(n * 4, 4), 4, 72)
        ro, offs = Guarded(max(sum(counts) * self.nl, 1), 1, 73), Guarded((n + 1) * 4, 4, 74)
        try:
            arr = (R.BlobRef * max(n, 1))(*[R.BlobRef(*b) for b in blobs])
            rc = lib.rsm_commitments_dev(ctx, self.nodes.ptr, self.status.ptr, self.W, self.count, ctypes.byref(self.p), t, arr,
                                         n, ro.ptr if want_roots else None, offs.ptr if want_roots else None, com.ptr,
                                         st.ptr, None)
            R._check(lib.rsm_sync(ctx))
            got = [g.result() for g in (com, st, ro, offs)]
            if rc or not want_roots:
                for g, x in list(zip((com, st, ro, offs), got))[0 if rc else 2:]:
                    assert np.array_equal(x, g.untouched(0, g.n)), "an output that the call does not own was written"
            if rc:
                return rc, None, None, None
            c = got[0].tobytes()
            coms = [c[i * 32:(i + 1) * 32] for i in range(n)]
            status = [int(x) for x in got[1].view(np.uint32)[:n]]
            roots = None
            if want_roots:
                o = got[3].view(np.uint32)
                assert list(o) == list(np.cumsum([0] + counts)), "root offsets"
                raw = got[2].tobytes()
                roots = [[raw[j * self.nl:(j + 1) * self.nl] for j in range(int(o[i]), int(o[i + 1]))] for i in range(n)]
            return rc, coms, status, roots
        finally:
            for g in (com, st, ro, offs):
                g.free()

    def free(self):
        self.nodes.free()
        self.status.free()


def make_blob(n, S, ns, seed, distinct=7):
    """[n][S] shares whose namespaces are non-decreasing."""
    g = np.random.default_rng([0xB10B, seed, n, S, ns])
    sh = g.integers(0, 256, (n, S), dtype=np.uint8)
    pool = np.sort(g.integers(0, 255, (distinct, ns), dtype=np.uint8).view([("", np.uint8)] * ns), axis=0)
    sh[:, :ns] = pool.view(np.uint8).reshape(distinct, ns)[np.sort(g.integers(0, distinct, n))]
    return sh
