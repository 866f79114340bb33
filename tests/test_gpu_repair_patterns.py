"""GPU: Repair on multi-sweep, uneven and stuck erasure patterns (tests/repair_patterns.py)
at the sizes of every decoder class.  BenchmarkRepair's erasures -- k of every row's 2k
cells, no row complete -- are finished by one row sweep; these patterns run what that
shape never reaches in rsm_eds_repair:

  the sweep loop of fast_repair: column sweeps, todo lists on both sides of the split
  decoder's 64-task threshold, the presence map re-uploaded between sweeps (a later sweep
  decodes from cells an earlier one rebuilt), vectors with more than k and fewer than 2k
  cells, and the FALLBACK_STUCK exit;

  fast_repair_rows_zero_copy on squares with complete rows (rows_uneven: runs of complete
  rows at the top, across the middle and at the bottom, single ones between todo rows)
  and with rows of more than k cells.  The complete rows are in the device square
  only because the pre-repair check uploaded the whole square; a row missing there
  cannot produce a wrong square -- the encoding compare rejects the sweep and the exact
  solver repairs the square -- so the cases assert repair_stats(): for rows_uneven and
  q1_q2 at 65 <= k <= 512 with a device tree, fast_path = 1 means the zero-copy path
  accepted the square (rows_uneven runs on a square of its own, so that the device
  buffers hold another square's bytes before it);

  the host-plugin tail of fast_repair (a tree constructor the library does not know)
  after several sweeps;

  unrepairable squares: the cells left behind are exactly the peeling closure.

  k = 8       byte tables                      k = 129   dec16f (m = 256)
  k = 33      byte tables, M = 64              k = 257   dec16h (m = 512)
  k = 65, 128 split bit-sliced                 k = 64, 200 on lowered limits: the wide forms

Every repairable case asserts the square bit for bit against the valid square (the
answer is unique) and repair_stats() == (fast_path 1, fallback_reason 0, sweeps, decoded
vectors) of the peeling model, which tests/test_repair_patterns_cpu.py pins to the
oracle crossword.  Squares are imported through the C ABI from numpy pointer arrays.
"""
import ctypes

import numpy as np
import pytest

import repair_patterns as RP
import rsmt2d_amd as R

pytestmark = pytest.mark.gpu
S = 64


def _import(lib, valid, pres, tree_fn):
    """rsm_eds_import of the valid square's present cells (NULL pointers elsewhere)."""
    W = valid.shape[0]
    cells = valid.reshape(W * W, S)
    ptrs = np.arange(W * W, dtype=np.uint64) * np.uint64(S) + np.uint64(cells.ctypes.data)
    ptrs[~pres.reshape(-1)] = 0
    lens = np.full(W * W, S, np.uint32)
    h = ctypes.c_void_p()
    R._check(lib.rsm_eds_import(None, ptrs.ctypes.data, lens.ctypes.data, W * W, ctypes.byref(h)))
    return R.ExtendedDataSquare(h.value, R.NewLeoRSCodec(), tree_fn)


def _flattened(lib, eds, W):
    got = np.empty((W, W, S), np.uint8)
    pres = np.empty((W, W), np.uint8)
    R._check(lib.rsm_eds_flattened(eds._h, got.ctypes.data, pres.ctypes.data))
    return got, pres.astype(bool)


def _stats(eds):
    st = eds.repair_stats()
    return st.fast_path, st.fallback_reason, st.sweeps, st.decoded_vectors


def _tree(tree, k):
    if tree == "default":
        return R.NewDefaultTree
    if tree == "nmt":
        return R.newErasuredNamespacedMerkleTreeConstructor(k, RP.NS)
    c = R.ErasuredNamespacedMerkleTreeConstructor(k, RP.NS)  # "nmt_host": the same tree behind a
    return lambda axis, idx: c(axis, idx)  # callback the library does not recognise as a device tree


def _repair(lib, family, k, tree="default"):
    """Import the family's cells, Repair, and check square and counters.  Returns (eds, rr, cr)."""
    valid, rr, cr = RP.square_for(family, k, S, "default" if tree == "default" else "nmt")
    eds = _import(lib, valid, RP.presence(family, k), _tree(tree, k))
    eds.Repair(list(rr), list(cr))
    got, pres = _flattened(lib, eds, 2 * k)
    sweeps, vectors, per, _ = RP.expected_stats(family, k)
    assert pres.all(), per
    assert np.array_equal(got, valid), per
    assert _stats(eds) == (1, R.FALLBACK_NONE, sweeps, vectors), per
    return eds, rr, cr


@pytest.mark.parametrize("k", [8, 33, 65, 128, 129, 257])
@pytest.mark.parametrize("family", RP.REPAIRABLE)
def test_repairable_default_tree(lib, family, k):
    """Every repairable family at every decoder class, DefaultTree roots on the device.
    rows_uneven and q1_q2 at k >= 65: the zero-copy path accepted a square with complete
    rows between its todo rows (rows_uneven) / rows of parity only and of data only."""
    _repair(lib, family, k)


@pytest.mark.parametrize("family", ["chain3", "avalanche", "rows_uneven"])
def test_repairable_nmt_device_trees(lib, family):
    """The erasured NMT (29-byte namespaces), roots on the device; rows_uneven through
    the zero-copy path."""
    _repair(lib, family, 65, "nmt")


@pytest.mark.parametrize("k", [8, 65])
@pytest.mark.parametrize("family", ["chain3", "avalanche", "rows_uneven"])
def test_repairable_nmt_host_plugin(lib, family, k):
    """The same tree through a constructor the library does not recognise: the sweeps of
    the general loop, then the tail that downloads the square, takes the roots through
    the host plugin and swaps buffers."""
    _repair(lib, family, k, "nmt_host")


@pytest.fixture
def pctx(lib):
    """A private context (its limits are lowered; the shared one keeps the defaults)."""
    h = ctypes.c_void_p()
    R._check(lib.rsm_ctx_create(0, ctypes.byref(h)))
    yield h.value
    lib.rsm_ctx_destroy(h.value)


@pytest.mark.parametrize("k", [64, 200])
@pytest.mark.parametrize("family", ["chain3_t", "chain3_cf", "avalanche"])
def test_repairable_wide_forms(lib, pctx, monkeypatch, family, k):
    """Offset limit 1 on a private context: every decode of the sweeps runs on the wide
    forms (k = 64: decode_gf8_wide_kernel; k = 200: the multi-pass GF(2^16) form)."""
    monkeypatch.setattr(R, "device_context", lambda device=0: pctx)  # Repair attaches this context
    R._check(lib.rsm_ctx_set_limits(pctx, 1, 0))
    try:
        _repair(lib, family, k)
    finally:
        R._check(lib.rsm_ctx_set_limits(pctx, 0, 0))


def _stuck(lib, family, k):
    valid, rr, cr = RP.square_for(family, k, S)
    pres0 = RP.presence(family, k)
    sweeps, vectors, per, closure = RP.expected_stats(family, k)
    assert not closure.all()
    eds = _import(lib, valid, pres0, R.NewDefaultTree)
    with pytest.raises(R.RSMError) as ei:
        eds.Repair(list(rr), list(cr))
    assert ei.value is R.ErrUnrepairableDataSquare
    got, pres = _flattened(lib, eds, 2 * k)
    # solved cells stay, nothing else appears
    assert np.array_equal(pres, closure), (int((pres & ~closure).sum()), int((closure & ~pres).sum()))
    assert np.array_equal(got[closure], valid[closure])
    assert eds.Flattened() == [valid[r, c].tobytes() if closure[r, c] else None
                               for r in range(2 * k) for c in range(2 * k)]
    # the sweeps the fast path ran before it gave up are counted
    assert _stats(eds) == (0, R.FALLBACK_STUCK, sweeps, vectors), per


@pytest.mark.parametrize("k", [8, 65, 128, 129])
@pytest.mark.parametrize("family", ["core", "core_edge"])
def test_stuck(lib, family, k):
    """Legitimately unrepairable squares: ErrUnrepairableDataSquare, and the square keeps
    exactly the cells the peeling closure solves (the reference leaves them in place)."""
    _stuck(lib, family, k)


@pytest.mark.parametrize("k", [16, 65])
def test_stuck_avalanche(lib, k):
    _stuck(lib, "avalanche_stuck", k)


@pytest.mark.parametrize("family,k", [("avalanche", 8), ("chain3", 33), ("rows_uneven", 65), ("chain3_cf", 128),
                                      ("rows_uneven", 129), ("avalanche", 257)])
def test_repaired_handle(lib, family, k):
    """One case per decoder class: the repaired square's own roots are the committed
    ones, and a second Repair is a no-op with zeroed counters."""
    eds, rr, cr = _repair(lib, family, k)
    assert eds.RowRoots() == list(rr) and eds.ColRoots() == list(cr)
    eds.Repair(list(rr), list(cr))
    assert _stats(eds) == (0, R.FALLBACK_NONE, 0, 0)
    got, pres = _flattened(lib, eds, 2 * k)
    assert pres.all() and np.array_equal(got, RP.square_for(family, k, S)[0])
