"""GPU: rsm_repair_squares_checked_dev and rsm_vectors_gather_dev -- device-resident Repair
that names the byzantine row or column (include/rsmt2d_hip.h "Repair of device-resident
squares with attribution").

Every call runs through repair_checked.repair_checked: squares between guard bands, absent
cells 0xA5, given cells byte-identical afterwards.  Valid squares are held to
rsm_repair_squares_dev on the same input; bad squares to the model of the schedule
(tests/repair_checked.py, pinned on the CPU by tests/test_repair_checked_cpu.py) and to the
schedule-independent validity predicate.

  k = 8    byte tables            k = 33, 65   split bit-sliced, W no power of two
  k = 129  GF(2^16)               k = 300      W = 600: past the wave-per-tree NMT form
  k = 1024 / 512 (NMT)            the widest squares the trees take
avalanche_stuck exists in repair_patterns only at k = 8, 16 and 65.
"""
import ctypes

import numpy as np
import pytest

import repair_cases as RC
import repair_checked as C
import repair_dev_calls as D
import repair_patterns as RP
import rsmt2d_amd as R

pytestmark = pytest.mark.gpu
S = 64


def _nmt(k, tree):
    return D.nmt_params(k, RP.NS) if tree == "nmt" else None


# ---- valid squares: the unchecked call's results, and every vector checked once ------------
def _families(k):
    return [f for f in RP.FAMILIES if f != "avalanche_stuck" or k in RP.AVALANCHE_STUCK_T]


VALID = [(k, "default") for k in (8, 33, 65, 129)] + [(k, "nmt") for k in (8, 33)]


@pytest.mark.parametrize("k,tree", VALID)
def test_valid_squares_equal_the_unchecked_call(lib, k, tree):
    """Every REPAIRABLE and STUCK family in one batch per call: status, square bytes,
    presence, sweeps, decoded vectors and missing of rsm_repair_squares_dev on the same
    input; OK squares have all 4k vectors checked and all 4k^2 cells hashed, and no square
    hashes more cells than are present at the end."""
    fams = _families(k)
    items = []
    for f in fams:
        valid, rr, cr = RP.square_for(f, k, S, tree)
        pres = RP.presence(f, k)
        items.append((D.given(valid, pres), pres, (rr, cr)))
    squares, presences, roots = (list(x) for x in zip(*items))
    plain = D.repair(lib, squares, presences, roots, k, S, _nmt(k, tree))
    got = C.repair_checked(lib, squares, presences, roots, k, S, _nmt(k, tree))
    for f, a, b in zip(fams, plain, got):
        assert b.stats() == a.stats(), f
        assert np.array_equal(b.presence, a.presence), f
        m = a.presence != 0
        assert np.array_equal(b.square[m], a.square[m]), f
        assert (b.axis, b.index, b.round, b.reason) == (0, 0, 0, 0), f
        assert b.status == (R.REPAIR_OK if f in RP.REPAIRABLE else R.REPAIR_STUCK), f
        if b.status == R.REPAIR_OK:
            assert (b.checked_vectors, b.hashed_cells) == (4 * k, 4 * k * k), f
            assert np.array_equal(b.square, RP.square_for(f, k, S, tree)[0]), f
        assert b.hashed_cells <= int(m.sum()), f


# ---- the verification cases ------------------------------------------------------------
def _rc(name, k, tree):
    flat, rr, cr, note = RC.case(name, k, S, tree)
    sq, pres = D.case_square(flat, 2 * k, S)
    return sq, pres, (rr, cr), note


def _check_named(got, roots, k, tree):
    assert got.status == R.REPAIR_BYZANTINE
    assert C.is_byzantine(got.shares, got.axis, got.index, roots[got.axis][got.index], k, tree)


@pytest.mark.parametrize("k,tree", [(8, "default"), (8, "nmt"), (65, "default"), (129, "default")])
def test_verification_cases_equal_the_model(lib, k, tree):
    """All of RC's cases in one batch: status, check record, final presence and gathered
    shares of the model; the named vector passes the validity predicate; the unchecked call
    on the same input is not OK either; B_*: the vector rsm_eds_repair names, with
    rsm_eds_byzantine_shares' shares."""
    items = [_rc(name, k, tree) for name in RC.CASES]
    squares, presences, roots = [i[0] for i in items], [i[1] for i in items], [i[2] for i in items]
    got = C.repair_checked(lib, squares, presences, roots, k, S, _nmt(k, tree))
    plain = D.repair(lib, squares, presences, roots, k, S, _nmt(k, tree))
    for name, it, g, u in zip(RC.CASES, items, got, plain):
        want = C.model(it[0], it[1], it[2][0], it[2][1], k, tree)
        C.assert_equals_model(g, want, name)
        if name == "D_control":
            assert g.status == R.REPAIR_OK and u.status == R.REPAIR_OK
            assert np.array_equal(g.square, it[3]["valid"])
            continue
        _check_named(g, it[2], k, tree)
        assert u.status != R.REPAIR_OK, name
        if name.startswith("B_"):
            tree_fn = R.NewDefaultTree if tree == "default" else \
                R.newErasuredNamespacedMerkleTreeConstructor(k, RP.NS)
            eds = D.import_host(lib, it[3]["full"], it[1], tree_fn)
            with pytest.raises(R.ErrByzantineData) as err:
                eds.Repair(list(it[2][0]), list(it[2][1]))
            assert (g.axis, g.index, g.shares) == (err.value.Axis, err.value.Index, err.value.Shares), name
            assert g.round == 0


# ---- late culprit, stage order -----------------------------------------------------------
@pytest.mark.parametrize("k,tree", [(8, "default"), (8, "nmt"), (16, "default"), (65, "default")])
def test_late_culprit(lib, k, tree):
    """One altered given cell in an avalanche map, found in round >= 3: the model's
    outcome, and every present cell was given or lies in a vector that passed."""
    sq, pres, rr, cr, want = C.late_culprit(k, tree)
    assert want.round >= 3
    (got,) = C.repair_checked(lib, [sq], [pres], [(rr, cr)], k, S, _nmt(k, tree))
    C.assert_equals_model(got, want)
    _check_named(got, (rr, cr), k, tree)
    allowed = np.array(pres, bool)
    for a, i in want.passed:
        if a == C.Row:
            allowed[i, :] = True
        else:
            allowed[:, i] = True
    assert not ((got.presence != 0) & ~allowed).any()


@pytest.mark.parametrize("k", [8, 65])
def test_stage_order(lib, k):
    """A decoded row fails its root while lower-indexed columns completed by the same pass
    hold its wrong cells: the row is named, the columns are never checked."""
    sq, pres, rr, cr = C.stage_order(k)
    (got,) = C.repair_checked(lib, [sq], [pres], [(rr, cr)], k, S)
    W = 2 * k
    assert (got.status, got.axis, got.index, got.round, got.reason) == (R.REPAIR_BYZANTINE, C.Row, W - 1, 1, R.BYZ_ROOT)
    assert got.checked_vectors == W
    C.assert_equals_model(got, C.model(sq, pres, rr, cr, k))
    assert np.array_equal(got.presence != 0, pres)  # the failing pass's rows are not marked


# ---- width classes of the list-driven trees ----------------------------------------------
@pytest.mark.parametrize("tree", ["default", "nmt"])
def test_generic_width(lib, tree):
    """k = 300 (W = 600): one kept bad column (round 0) and A_row_k (round 1).  The
    expectations are what the model gives for these cases at k = 8 and 16
    (tests/test_repair_checked_cpu.py), written out: the kept column alone is checked on
    entry; A_row_k's row pass decodes 2k valid rows, which pass, and completes every column,
    of which the lowest non-codeword is named with all its cells present."""
    k = 300
    W = 2 * k
    items = [_rc(name, k, tree) for name in ("B_col_kept", "A_row_k")]
    b, a = C.repair_checked(lib, [i[0] for i in items], [i[1] for i in items], [i[2] for i in items], k, S, _nmt(k, tree))
    kept = k + k // 2
    assert b.stats() == (R.REPAIR_BYZANTINE, 0, 0, int((~items[0][1]).sum()))
    assert b.check() == (C.Col, kept, 0, R.BYZ_ENCODING, 1, W)
    assert np.array_equal(b.presence != 0, items[0][1])
    assert b.shares == [items[0][3]["full"][r, kept].tobytes() for r in range(W)]
    first = min(items[1][3]["bad"][RC.Col])
    assert a.stats() == (R.REPAIR_BYZANTINE, 1, W, 0)
    assert a.check() == (C.Col, first, 1, R.BYZ_ENCODING, 2 * W, W * W)
    assert (a.presence != 0).all()
    assert a.shares == [items[1][3]["full"][r, first].tobytes() for r in range(W)]
    for it, g in zip(items, (b, a)):
        _check_named(g, it[2], k, tree)


@pytest.mark.parametrize("k,tree", [(1024, "default"), (512, "nmt")])
def test_widest_squares(lib, k, tree):
    """The widest squares the trees take, k of every row's cells erased: the control
    repairs with every vector checked; with one committed column root flipped the row pass
    passes its own checks and that column is named in round 1.  The committed roots are the
    device's own (rsm_roots_squares_dev / rsm_nmt_roots_squares_dev, tested elsewhere)."""
    W = 2 * k
    valid = RC.valid_square(k, S, 0xB16 + k, tree)
    pres = RC.erase(W, k, 0xE2A5E + k)
    ctx = R.device_context(0)
    rl = 32 if tree == "default" else 2 * RP.NS + 32
    d, out, st = R.DeviceBuffer(valid.nbytes), R.DeviceBuffer(2 * W * rl), R.DeviceBuffer(2 * W * 4)
    try:
        d.upload(valid.reshape(-1))
        if tree == "default":
            R._check(lib.rsm_roots_squares_dev(ctx, d.ptr, W, S, 1, out.ptr, None))
        else:
            R._check(lib.rsm_nmt_roots_squares_dev(ctx, d.ptr, W, S, 1, ctypes.byref(_nmt(k, tree)), out.ptr, st.ptr, None))
        R._check(lib.rsm_sync(ctx))
        table = out.download().copy()
    finally:
        for b in (d, out, st):
            b.free()
    col = W - 3
    flipped = table.copy()
    flipped[(W + col) * rl + rl - 1] ^= 1
    sq = D.given(valid, pres)
    (good,) = C.repair_checked(lib, [sq], [pres], None, k, S, _nmt(k, tree), table=table)
    assert good.stats() == (R.REPAIR_OK, 1, W, 0)
    assert (good.checked_vectors, good.hashed_cells) == (2 * W, W * W)
    assert np.array_equal(good.square, valid)
    (bad,) = C.repair_checked(lib, [sq], [pres], None, k, S, _nmt(k, tree), table=flipped)
    assert bad.stats() == (R.REPAIR_BYZANTINE, 1, W, 0)
    assert bad.check() == (C.Col, col, 1, R.BYZ_ROOT, 2 * W, W * W)
    assert bad.shares == [valid[r, col].tobytes() for r in range(W)]


# ---- a mixed batch -----------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 65])
def test_mixed_batch_equals_single_runs(lib, k):
    """OK, STUCK, round-0, round-1 and late-culprit squares in one batch of 8: each result is
    what the square gives alone, so a square that drops out does not disturb the others."""
    items = []
    for f in ("avalanche", "core", "chain3_cf"):
        valid, rr, cr = RP.square_for(f, k, S)
        pres = RP.presence(f, k)
        items.append((D.given(valid, pres), pres, (rr, cr)))
    for name in ("B_row_kept", "A_row_last", "C_col_root_last"):
        items.append(_rc(name, k, "default")[:3])
    sq, pres, rr, cr, _ = C.late_culprit(k, "default")
    items.append((sq, pres, (rr, cr)))
    sq, pres, rr, cr = C.stage_order(k)
    items.append((sq, pres, (rr, cr)))
    batch = C.repair_checked(lib, [i[0] for i in items], [i[1] for i in items], [i[2] for i in items], k, S)
    assert [b.status for b in batch] == [R.REPAIR_OK, R.REPAIR_STUCK, R.REPAIR_OK] + [R.REPAIR_BYZANTINE] * 5
    assert [b.round for b in batch[3:6]] == [0, 1, 1]
    for i, it in enumerate(items):
        (alone,) = C.repair_checked(lib, [it[0]], [it[1]], [it[2]], k, S)
        assert alone.stats() == batch[i].stats() and alone.check() == batch[i].check(), i
        assert np.array_equal(alone.presence, batch[i].presence), i
        assert alone.shares == batch[i].shares, i
        m = alone.presence != 0
        assert np.array_equal(alone.square[m], batch[i].square[m]), i


# ---- rsm_vectors_gather_dev --------------------------------------------------------------
def test_vectors_gather(lib):
    """Rows and columns, first and last index, several squares, against numpy slicing; the
    presence bytes are copied as they are."""
    k, count = 8, 3
    W = 2 * k
    rng = np.random.default_rng(0x6A7)
    batch = rng.integers(0, 256, (count, W, W, S), dtype=np.uint8)
    pres = rng.integers(0, 3, (count, W, W), dtype=np.uint8) * 7
    refs = [(0, 0, 0), (0, 1, 0), (2, 0, W - 1), (2, 1, W - 1), (1, 1, 5), (1, 0, 5), (2, 1, 0)]
    d_eds, d_pres = R.DeviceBuffer(batch.nbytes), R.DeviceBuffer(pres.nbytes)
    try:
        d_eds.upload(batch.reshape(-1))
        d_pres.upload(pres.reshape(-1))
        shares, present = R.gather_vectors_dev(d_eds, d_pres, k, S, refs, count)
        ctx = R.device_context(0)
        ref = (R.RootRef * 1)(R.RootRef(count, 0, 0))
        assert lib.rsm_vectors_gather_dev(ctx, d_eds.ptr, d_pres.ptr, k, S, count, ref, 1, d_eds.ptr, d_pres.ptr,
                                          None) == R.RSM_EINVAL
        ref = (R.RootRef * 1)(R.RootRef(0, 1, W))
        assert lib.rsm_vectors_gather_dev(ctx, d_eds.ptr, d_pres.ptr, k, S, count, ref, 1, d_eds.ptr, d_pres.ptr,
                                          None) == R.RSM_EINVAL
        ref = (R.RootRef * 1)(R.RootRef(0, 1, 0))
        assert lib.rsm_vectors_gather_dev(ctx, d_eds.ptr, d_pres.ptr, k, S, count, ref, 1, d_eds.ptr + 4, d_pres.ptr,
                                          None) == R.RSM_EINVAL
        assert lib.rsm_vectors_gather_dev(ctx, d_eds.ptr, d_pres.ptr, k, S, count, ref, 1, None, d_pres.ptr,
                                          None) == R.RSM_EINVAL
    finally:
        d_eds.free()
        d_pres.free()
    for j, (s, axis, i) in enumerate(refs):
        assert np.array_equal(shares[j], batch[s, i] if axis == 0 else batch[s, :, i]), refs[j]
        assert np.array_equal(present[j], pres[s, i] if axis == 0 else pres[s, :, i]), refs[j]


def test_byzantine_data_dev(lib):
    """The Python flow: repair_squares_checked_dev, then byzantine_data_dev -- the oracle
    crossword's ErrByzantineData for B_col_kept, None for the control."""
    k = 8
    items = [_rc(name, k, "default") for name in ("D_control", "B_col_kept")]
    W = 2 * k
    batch = np.stack([i[0] for i in items])
    pres = np.stack([i[1] for i in items]).astype(np.uint8)
    d_eds, d_pres, d_roots = R.DeviceBuffer(batch.nbytes), R.DeviceBuffer(pres.nbytes), R.DeviceBuffer(2 * 2 * W * 32)
    try:
        d_eds.upload(batch.reshape(-1))
        d_pres.upload(pres.reshape(-1))
        d_roots.upload(D.roots_table([i[2] for i in items]))
        outcome = R.repair_squares_checked_dev(d_eds, d_pres, k, S, d_roots, 2)
        errs = R.byzantine_data_dev(d_eds, d_pres, k, S, outcome, 2)
    finally:
        for b in (d_eds, d_pres, d_roots):
            b.free()
    assert [o[0].status for o in outcome] == [R.REPAIR_OK, R.REPAIR_BYZANTINE]
    want, _ = RC.expected("B_col_kept", k, S, "default")
    assert errs[0] is None
    assert (errs[1].Axis, errs[1].Index, errs[1].Shares) == (want[0], want[1], list(want[2]))
