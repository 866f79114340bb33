"""GPU: rsm_repair_squares_dev -- Repair of squares that stay in device memory, a batch per
call (include/rsmt2d_hip.h "Repair of device-resident squares").

The erasure maps are those of tests/repair_patterns.py (RP) and the verification cases
those of tests/repair_cases.py (RC); the expected sweeps, vectors and closures come from
RP's peeling model, which tests/test_repair_patterns_cpu.py pins to the oracle crossword.
Every call runs through repair_dev_calls.repair: absent cells hold 0xA5 before the call,
d_eds, d_presence and d_work lie between guard bands that must stay intact, and every
given cell must come back byte-identical.

  k = 8     byte tables                k = 65    split bit-sliced
  k = 129   GF(2^16), dec16f           k = 64    on a lowered offset limit: the wide forms
"""
import ctypes

import numpy as np
import pytest

import repair_cases as RC
import repair_dev_calls as D
import repair_patterns as RP
import rsmt2d_amd as R

pytestmark = pytest.mark.gpu
S = 64


def _family(lib, family, k, tree="default", ctx=None):
    valid, rr, cr = RP.square_for(family, k, S, tree)
    pres = RP.presence(family, k)
    nmt = D.nmt_params(k, RP.NS) if tree == "nmt" else None
    (r,) = D.repair(lib, [D.given(valid, pres)], [pres], [(rr, cr)], k, S, nmt, ctx)
    return r, valid


def _check_repaired(r, valid, family, k):
    sweeps, vectors, per, _ = RP.expected_stats(family, k)
    assert r.stats() == (R.REPAIR_OK, sweeps, vectors, 0), per
    assert r.presence.all(), per
    assert np.array_equal(r.square, valid), per


def _check_stuck(r, valid, family, k):
    sweeps, vectors, per, closure = RP.expected_stats(family, k)
    assert not closure.all()
    assert r.stats() == (R.REPAIR_STUCK, sweeps, vectors, int((~closure).sum())), per
    assert np.array_equal(r.presence != 0, closure), (int(((r.presence != 0) & ~closure).sum()),
                                                      int((closure & (r.presence == 0)).sum()))
    assert np.array_equal(r.square[closure], valid[closure])


@pytest.mark.parametrize("k", [8, 65, 129])
@pytest.mark.parametrize("family", RP.REPAIRABLE)
def test_repairable_families(lib, family, k):
    """Status OK, the square bit for bit, (sweeps, decoded vectors) of the peeling model,
    nothing missing, presence all ones."""
    r, valid = _family(lib, family, k)
    _check_repaired(r, valid, family, k)


@pytest.mark.parametrize("k", [8, 65])
@pytest.mark.parametrize("family", RP.STUCK)
def test_stuck_families(lib, family, k):
    """Status STUCK; the returned presence is the model's closure, `missing` its zero
    count, closure cells equal the valid square."""
    r, valid = _family(lib, family, k)
    _check_stuck(r, valid, family, k)


def _rc(name, k, tree="default"):
    flat, rr, cr, _ = RC.case(name, k, S, tree)
    sq, pres = D.case_square(flat, 2 * k, S)
    return sq, pres, (rr, cr)


def test_mixed_batch(lib):
    """avalanche (many sweeps), core (stuck at once), a square with one committed root
    flipped and one whose last word breaks the encoding under roots committed to it, in
    one call: every result is what the square gives alone, so a square that has finished
    does not disturb the others."""
    k = 8
    items = []
    for family in ("avalanche", "core"):
        valid, rr, cr = RP.square_for(family, k, S)
        pres = RP.presence(family, k)
        items.append((D.given(valid, pres), pres, (rr, cr)))
    items.append(_rc("C_col_root_last", k))
    items.append(_rc("A_row_last", k))
    squares, presences, roots = (list(x) for x in zip(*items))
    batch = D.repair(lib, squares, presences, roots, k, S)
    assert [r.status for r in batch] == [R.REPAIR_OK, R.REPAIR_STUCK, R.REPAIR_ROOTS, R.REPAIR_ENCODING]
    _check_repaired(batch[0], RP.square_for("avalanche", k, S)[0], "avalanche", k)
    _check_stuck(batch[1], RP.square_for("core", k, S)[0], "core", k)
    for i, it in enumerate(items):
        (alone,) = D.repair(lib, [it[0]], [it[1]], [it[2]], k, S)
        assert alone.stats() == batch[i].stats(), i
        assert np.array_equal(alone.presence, batch[i].presence), i
        if alone.status != R.REPAIR_STUCK:
            assert np.array_equal(alone.square, batch[i].square), i
        else:
            m = alone.presence != 0
            assert np.array_equal(alone.square[m], batch[i].square[m]), i


@pytest.mark.parametrize("tree", ["default", "nmt"])
@pytest.mark.parametrize("k", [8, 65])
@pytest.mark.parametrize("name", RC.CASES)
def test_verification_cases(lib, name, k, tree):
    """RC's squares, each of which leaves one verification step between a bad square and
    OK: D_control OK; A_* and B_col_kept ENCODING (the roots are committed to the altered
    square); C_* ROOTS; B_row_kept and E_overdetermined_row are decoded from inconsistent
    input, so only the rejection is asserted."""
    sq, pres, roots = _rc(name, k, tree)
    nmt = D.nmt_params(k, RC.NS) if tree == "nmt" else None
    (r,) = D.repair(lib, [sq], [pres], [roots], k, S, nmt)
    assert r.missing == 0 and r.presence.all() and r.sweeps >= 1
    assert r.status in D.RC_STATUS[name], r.stats()
    note = RC.case(name, k, S, tree)[3]
    if name == "D_control" or name.startswith("C_"):
        assert np.array_equal(r.square, note["valid"])
    elif name.startswith("A_") or name == "B_col_kept":
        assert np.array_equal(r.square, note["full"])  # rows decoded from valid row codewords


@pytest.mark.parametrize("family", ["chain3", "avalanche"])
def test_nmt_device_trees(lib, family):
    """The erasured NMT with 29-byte namespaces at k = 65: roots and tree statuses on the
    device."""
    r, valid = _family(lib, family, 65, "nmt")
    _check_repaired(r, valid, family, 65)


@pytest.fixture
def pctx(lib):
    """A private context (its limits are lowered; the shared one keeps the defaults)."""
    h = ctypes.c_void_p()
    R._check(lib.rsm_ctx_create(0, ctypes.byref(h)))
    yield h.value
    lib.rsm_ctx_destroy(h.value)


@pytest.mark.parametrize("family", ["chain3_cf", "avalanche"])
def test_wide_forms(lib, pctx, family):
    """Offset limit 1 on a private context: every decode of the sweeps and the
    re-extension run on the wide forms (k = 64: decode_gf8_wide_kernel)."""
    R._check(lib.rsm_ctx_set_limits(pctx, 1, 0))
    try:
        r, valid = _family(lib, family, 64, ctx=pctx)
    finally:
        R._check(lib.rsm_ctx_set_limits(pctx, 0, 0))
    _check_repaired(r, valid, family, 64)


def test_agrees_with_host_repair(lib):
    """chain3 at k = 65: rsm_eds_repair on the same cells gives the same square and the
    same sweep and vector counts."""
    k, family = 65, "chain3"
    r, valid = _family(lib, family, k)
    _, rr, cr = RP.square_for(family, k, S)
    eds = D.import_host(lib, valid, RP.presence(family, k), R.NewDefaultTree)
    eds.Repair(list(rr), list(cr))
    got, pres = D.flattened_host(lib, eds, 2 * k, S)
    st = eds.repair_stats()
    assert pres.all() and r.status == R.REPAIR_OK
    assert np.array_equal(got, r.square)
    assert (st.sweeps, st.decoded_vectors) == (r.sweeps, r.vectors)


def test_complete_square_and_empty_batch(lib):
    """A square with nothing missing is verified without a sweep; count = 0 launches
    nothing and touches no operand."""
    k = 8
    valid, rr, cr = RP.square(k, S)
    pres = np.ones((2 * k, 2 * k), bool)
    (r,) = D.repair(lib, [np.array(valid)], [pres], [(rr, cr)], k, S)
    assert r.stats() == (R.REPAIR_OK, 0, 0, 0)
    bad = np.array(valid)
    bad[2 * k - 1, 2 * k - 1, S - 1] ^= 1
    (r,) = D.repair(lib, [bad], [pres], [(rr, cr)], k, S)
    assert r.stats() == (R.REPAIR_ENCODING, 0, 0, 0)
    R._check(lib.rsm_repair_squares_dev(R.device_context(0), None, None, k, S, 0, None, None, None, None, None))
