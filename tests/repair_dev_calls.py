"""TEST INFRASTRUCTURE ONLY -- the calls tests/test_gpu_repair_dev.py and
tests/test_gpu_scatter_dev.py share: one place that lays a batch of squares, presence
maps and committed roots out in device memory between guard bands, calls
rsm_repair_squares_dev and downloads what it wrote.  Importing this module touches no
GPU; every function that does takes `lib`."""
import ctypes

import numpy as np

import rsmt2d_amd as R
from device_calls import Guarded

FILL = 0xA5  # what absent cells hold before a call: a decoder that reads them is caught

# RC case family -> the statuses a device repair may give (tests/test_repair_dev_cpu.py
# pins them to RC.expected)
RC_STATUS = {
    "D_control": {R.REPAIR_OK},
    "A_row_k": {R.REPAIR_ENCODING}, "A_row_last": {R.REPAIR_ENCODING}, "A_row_0": {R.REPAIR_ENCODING},
    "B_col_kept": {R.REPAIR_ENCODING},
    "C_row_root_0": {R.REPAIR_ROOTS}, "C_col_root_last": {R.REPAIR_ROOTS}, "C_row_root_last": {R.REPAIR_ROOTS},
    "B_row_kept": {R.REPAIR_ENCODING, R.REPAIR_ROOTS}, "E_overdetermined_row": {R.REPAIR_ENCODING, R.REPAIR_ROOTS},
}


def nmt_params(k, ns):
    return R.NmtParams(ns, 1, k)


def given(full, pres):
    """The [W][W][S] square a call starts from: `full` where pres, FILL elsewhere."""
    sq = np.full(full.shape, FILL, np.uint8)
    sq[pres] = full[pres]
    return sq


def case_square(flat, W, S):
    """(square with FILL in the erased cells, presence) of an RC.case cell list."""
    pres = np.array([x is not None for x in flat], bool).reshape(W, W)
    sq = np.full((W, W, S), FILL, np.uint8)
    for i, x in enumerate(flat):
        if x is not None:
            sq[i // W, i % W] = np.frombuffer(x, np.uint8)
    return sq, pres


def roots_table(roots):
    """[count][2][W][root_len] bytes from [(row roots, column roots)] per square."""
    return np.frombuffer(b"".join(b"".join(rr) + b"".join(cr) for rr, cr in roots), np.uint8)


class Result:
    def __init__(self, res, squares, presence):
        self.status, self.sweeps, self.vectors, self.missing = res.status, res.sweeps, res.decoded_vectors, res.missing
        self.square, self.presence = squares, presence

    def stats(self):
        return self.status, self.sweeps, self.vectors, self.missing


def repair(lib, squares, presences, roots, k, S, nmt=None, ctx=None, stream=None):
    """One rsm_repair_squares_dev over the batch: squares [W][W][S] uint8 (as given()),
    presences [W][W] bool, roots [(rr, cr)].  d_eds, d_presence and d_work lie between
    guard bands, which must come back intact, and every given cell byte-identical.  `stream`:
    the caller stream the call runs on (NULL: the context stream).
    Returns one Result per square."""
    ctx = R.device_context(0) if ctx is None else ctx
    count, W = len(squares), 2 * k
    pp = ctypes.byref(nmt) if nmt is not None else None
    batch = np.ascontiguousarray(np.stack(squares))
    pres = np.ascontiguousarray(np.stack(presences)).astype(np.uint8)
    assert batch.shape == (count, W, W, S) and pres.shape == (count, W, W)
    nwork = int(lib.rsm_repair_work_bytes(k, S, count, pp))
    assert nwork > 0
    table = roots_table(roots)
    assert table.size == count * 2 * W * (32 if nmt is None else 2 * nmt.namespace_size + 32)
    d_eds, d_pres, d_work = Guarded(batch.nbytes, 0, 11), Guarded(pres.nbytes, 0, 12), Guarded(nwork, 0, 13)
    d_roots = R.DeviceBuffer(table.size)
    try:
        d_eds.buf.upload(batch.reshape(-1), d_eds.front)
        d_pres.buf.upload(pres.reshape(-1), d_pres.front)
        d_roots.upload(table)
        res = (R.RepairResult * count)()
        R._check(lib.rsm_repair_squares_dev(ctx, d_eds.ptr, d_pres.ptr, k, S, count, pp, d_roots.ptr, d_work.ptr, res, stream))
        got = d_eds.result().reshape(count, W, W, S).copy()
        got_pres = d_pres.result().reshape(count, W, W).copy()
        d_work.result()
    finally:
        for b in (d_eds, d_pres, d_work, d_roots):
            b.free()
    for s in range(count):
        m = presences[s]
        assert np.array_equal(got[s][m], batch[s][m]), "a given cell of square %d was written" % s
        assert got_pres[s][m].all(), "a given cell of square %d lost its presence byte" % s
    return [Result(res[s], got[s], got_pres[s]) for s in range(count)]


def import_host(lib, valid, pres, tree_fn):
    """rsm_eds_import of a square's present cells (NULL pointers elsewhere)."""
    W, S = valid.shape[0], valid.shape[2]
    cells = np.ascontiguousarray(valid).reshape(W * W, S)
    ptrs = np.arange(W * W, dtype=np.uint64) * np.uint64(S) + np.uint64(cells.ctypes.data)
    ptrs[~np.asarray(pres, bool).reshape(-1)] = 0
    lens = np.full(W * W, S, np.uint32)
    h = ctypes.c_void_p()
    R._check(lib.rsm_eds_import(None, ptrs.ctypes.data, lens.ctypes.data, W * W, ctypes.byref(h)))
    return R.ExtendedDataSquare(h.value, R.NewLeoRSCodec(), tree_fn)


def flattened_host(lib, eds, W, S):
    got = np.empty((W, W, S), np.uint8)
    pres = np.empty((W, W), np.uint8)
    R._check(lib.rsm_eds_flattened(eds._h, got.ctypes.data, pres.ctypes.data))
    return got, pres.astype(bool)
