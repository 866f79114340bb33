"""CPU: what rsm_repair_squares_checked_dev and rsm_vectors_gather_dev decide before any
device use (symbols, record size, scratch size, argument errors), and the model of the
checked schedule (tests/repair_checked.py) pinned to repair_patterns.model, to the oracle
crossword and to the schedule-independent validity predicate.
tests/test_gpu_repair_checked.py holds the device to that model."""
import ctypes

import numpy as np
import pytest

import repair_cases as RC
import repair_checked as C
import repair_dev_calls as D
import repair_patterns as RP
import rsmt2d_amd as R

S = 64


def _nmt(ns, k):
    return ctypes.byref(R.NmtParams(ns, 1, k))


# ---- ABI -----------------------------------------------------------------------------
def test_symbols_and_records(lib):
    for name in ("rsm_repair_checked_work_bytes", "rsm_repair_squares_checked_dev", "rsm_vectors_gather_dev"):
        assert hasattr(lib, name), name
        assert name in R.SIGNATURES and getattr(lib, name).argtypes == R.SIGNATURES[name][1], name
    assert ctypes.sizeof(R.RepairCheck) == 24
    assert [f[0] for f in R.RepairCheck._fields_] == ["axis", "index", "round", "reason", "checked_vectors",
                                                      "hashed_cells"]
    assert R.REPAIR_BYZANTINE == 4
    assert (R.BYZ_ROOT, R.BYZ_ENCODING, R.BYZ_TREE) == (1, 2, 3)
    assert (C.OK, C.STUCK, C.BYZANTINE) == (R.REPAIR_OK, R.REPAIR_STUCK, R.REPAIR_BYZANTINE)
    assert (C.ROOT, C.ENCODING, C.TREE) == (R.BYZ_ROOT, R.BYZ_ENCODING, R.BYZ_TREE)


def test_checked_work_bytes(lib):
    """0 exactly where rsm_repair_work_bytes is; elsewhere at least the leaf records and
    the per-vector checked bytes."""
    wb, cwb = lib.rsm_repair_work_bytes, lib.rsm_repair_checked_work_bytes
    shapes = [(1, 64, 1, None), (8, 64, 4, None), (8, 64, 0, None), (65, 64, 1, None), (128, 512, 64, None),
              (1024, 64, 1, None), (1025, 64, 1, None), (0, 64, 1, None), (8, 96, 1, None), (1024, 64, 1024, None),
              (8, 64, 65536, None)]
    for k in (8, 65, 512, 513):
        for ns in (0, 1, 29, 32, 33):
            shapes.append((k, 64, 2, (ns, k)))
    for k, s, count, p in shapes:
        a = wb(k, s, count, _nmt(*p) if p else None)
        b = cwb(k, s, count, _nmt(*p) if p else None)
        assert (a == 0) == (b == 0), (k, s, count, p)
        if b:
            W = 2 * k
            assert b >= count * W * W * (64 if p else 32) + count * 4 * k, (k, s, count, p)


def test_argument_errors_before_any_device_use(lib):
    """As rsm_repair_squares_dev's: `ctx` is the address of a zeroed buffer, no rsm_ctx."""
    fake = ctypes.create_string_buffer(4096)
    ctx = ctypes.addressof(fake)
    res, chk = (R.RepairResult * 1)(), (R.RepairCheck * 1)()
    rep, ga = lib.rsm_repair_squares_checked_dev, lib.rsm_vectors_gather_dev
    assert rep(None, None, None, 8, 64, 1, None, None, None, res, chk, None) == R.RSM_EINVAL
    assert rep(ctx, None, None, 0, 64, 1, None, None, None, res, chk, None) == R.RSM_EINVAL
    assert rep(ctx, None, None, 8, 96, 1, None, None, None, res, chk, None) == R.RSM_ESHARESIZE
    assert b"multiple of 64" in lib.rsm_last_error()
    assert rep(ctx, None, None, 1025, 64, 1, None, None, None, res, chk, None) == R.RSM_EUNSUPPORTED
    assert rep(ctx, None, None, 8, 64, 1, _nmt(33, 8), None, None, res, chk, None) == R.RSM_EUNSUPPORTED
    assert rep(ctx, None, None, 8, 64, 1, None, None, None, res, chk, None) == R.RSM_EINVAL  # NULL operands
    assert rep(ctx, None, None, 8, 64, 0, None, None, None, None, None, None) == R.RSM_OK    # nothing to do
    # every operand there but `checks`: 16-byte aligned addresses that are never touched
    a = 4096
    assert rep(ctx, a, a, 8, 64, 1, None, a, a, res, None, None) == R.RSM_EINVAL
    assert b"rsm_repair_squares_checked_dev" in lib.rsm_last_error()
    assert rep(ctx, a + 8, a, 8, 64, 1, None, a, a, res, chk, None) == R.RSM_EINVAL
    assert b"16-byte aligned" in lib.rsm_last_error()
    ref = (R.RootRef * 1)(R.RootRef(0, 0, 0))
    assert ga(None, None, None, 8, 64, 1, ref, 1, None, None, None) == R.RSM_EINVAL
    assert ga(ctx, None, None, 0, 64, 1, ref, 1, None, None, None) == R.RSM_EINVAL
    assert ga(ctx, None, None, 8, 96, 1, ref, 1, None, None, None) == R.RSM_ESHARESIZE
    assert ga(ctx, None, None, 8, 64, 1, ref, 1, None, None, None) == R.RSM_EINVAL       # NULL operands
    assert ga(ctx, None, None, 8, 64, 1, ref, 0, None, None, None) == R.RSM_OK           # nothing to do
    assert ga(ctx, a, a, 8, 64, 1, ref, 1, a + 4, a, None) == R.RSM_EINVAL               # misaligned d_shares
    for bad in (R.RootRef(1, 0, 0), R.RootRef(0, 2, 0), R.RootRef(0, 1, 16)):
        assert ga(ctx, a, a, 8, 64, 1, (R.RootRef * 1)(bad), 1, a, a, None) == R.RSM_EINVAL
        assert b"out of range" in lib.rsm_last_error()


# ---- the model -----------------------------------------------------------------------
def _family(family, k, tree="default"):
    valid, rr, cr = RP.square_for(family, k, S, tree)
    pres = RP.presence(family, k)
    return C.model(D.given(valid, pres), pres, rr, cr, k, tree), valid


@pytest.mark.parametrize("k", [8, 16])
@pytest.mark.parametrize("family", RP.FAMILIES)
def test_model_on_valid_squares_is_the_peeling_model(family, k):
    """Status, sweeps, decoded vectors, missing and closure of repair_patterns.model; every
    vector of a repaired square checked once, every cell hashed once."""
    out, valid = _family(family, k)
    sweeps, vectors, _, closure = RP.expected_stats(family, k)
    missing = int((~closure).sum())
    assert out.stats() == (C.STUCK if missing else C.OK, sweeps, vectors, missing)
    assert np.array_equal(out.presence, closure)
    assert out.check()[:4] == (0, 0, 0, 0)
    if not missing:
        assert (out.checked_vectors, out.hashed_cells) == (4 * k, 4 * k * k)
        assert len(out.passed) == 4 * k
    assert out.hashed_cells <= int(closure.sum())


def _rc_model(name, k, tree="default"):
    flat, rr, cr, note = RC.case(name, k, S, tree)
    sq, pres = D.case_square(flat, 2 * k, S)
    return C.model(sq, pres, rr, cr, k, tree), (rr, cr), note


@pytest.mark.parametrize("tree", ["default", "nmt"])
@pytest.mark.parametrize("k", [8, 16])
@pytest.mark.parametrize("name", RC.CASES)
def test_model_on_the_verification_cases(name, k, tree):
    out, roots, note = _rc_model(name, k, tree)
    outcome, _ = RC.expected(name, k, S, tree)
    if outcome == "ok":
        assert out.stats() == (C.OK, 1, 2 * k, 0)
        return
    assert out.status == C.BYZANTINE
    assert C.is_byzantine(out.shares, out.axis, out.index, roots[out.axis][out.index], k, tree)
    if name in ("B_col_kept", "B_row_kept"):  # the oracle crossword's pre-repair answer
        assert (out.axis, out.index, out.shares) == (outcome[0], outcome[1], list(outcome[2]))
        assert out.round == 0 and out.sweeps == 0
    if name.startswith("A_row"):  # rows valid: the row pass decodes them all, the columns fail
        assert (out.axis, out.round, out.reason) == (C.Col, 1, C.ENCODING)
        assert out.index == min(note["bad"][RC.Col])
    if name.startswith("C_"):
        (axis, index), = [(a, i) for a in (C.Row, C.Col) for i in note["touched"][a]]
        assert (out.axis, out.index, out.reason) == (axis, index, C.ROOT)


def test_validity_predicate_rejects_good_vectors():
    """The predicate is no rubber stamp: a valid row is not byzantine, with all its shares
    or with k of them; with a flipped root, or one altered share among k + 1, it is."""
    k = 8
    valid, rr, cr = RP.square(k, S)
    row = [valid[3, c].tobytes() for c in range(2 * k)]
    half = [x if c % 2 else None for c, x in enumerate(row)]
    assert not C.is_byzantine(row, C.Row, 3, rr[3], k)
    assert not C.is_byzantine(half, C.Row, 3, rr[3], k)
    assert not C.is_byzantine([None] * (k + 1) + row[k + 1:], C.Row, 3, rr[3], k)  # k - 1 shares
    assert C.is_byzantine(half, C.Row, 3, RC.flip_byte(rr[3]), k)
    bad = list(row)
    bad[5] = bytes([bad[5][0] ^ 1]) + bad[5][1:]
    assert C.is_byzantine(bad, C.Row, 3, rr[3], k)
    col = [valid[r, 2].tobytes() for r in range(2 * k)]
    assert not C.is_byzantine(col, C.Col, 2, cr[2], k)


@pytest.mark.parametrize("tree", ["default", "nmt"])
@pytest.mark.parametrize("k", [8, 16])
def test_late_culprit(k, tree):
    """One altered given cell in an avalanche map, found no earlier than round 3: the named
    vector satisfies the predicate, and nothing present descends from an unchecked vector."""
    sq, pres, rr, cr, out = C.late_culprit(k, tree)
    assert out.status == C.BYZANTINE and out.round >= 3
    assert C.is_byzantine(out.shares, out.axis, out.index, (rr, cr)[out.axis][out.index], k, tree)
    allowed = np.array(pres, bool)
    for a, i in out.passed:
        if a == C.Row:
            allowed[i, :] = True
        else:
            allowed[:, i] = True
    assert not (out.presence & ~allowed).any()


@pytest.mark.parametrize("k", [8, 16])
def test_stage_order_square(k):
    """The decoded row W - 1 fails its root in stage 1, while the same pass completes
    lower-indexed columns that hold its wrong cells: the row is named, stage 2 never runs."""
    sq, pres, rr, cr = C.stage_order(k)
    valid = RP.square(k, S)[0]
    W = 2 * k
    assert not RC.complete_vectors(pres)  # nothing for round 0
    out = C.model(sq, pres, rr, cr, k)
    assert (out.status, out.axis, out.index, out.round, out.reason) == (C.BYZANTINE, C.Row, W - 1, 1, C.ROOT)
    assert out.checked_vectors == W  # the W decoded rows; stage 2 did not run
    assert C.is_byzantine(out.shares, C.Row, W - 1, rr[W - 1], k)
    # the pass leaves a wrong cell in a column below W - 1, which it also completes
    dec = C.oracle.decode([sq[W - 1, c].tobytes() if pres[W - 1, c] else None for c in range(W)])
    j = int(np.flatnonzero(~pres[W - 1])[0])
    assert j < W - 1 and dec[j] != valid[W - 1, j].tobytes()
