"""CPU: the squares of tests/repair_cases.py are what they claim to be, and the oracle
crossword gives each family's outcome class.  The expected (axis, index, shares) of the
GPU tests comes from the same oracle run; nothing here is hard-coded."""
import numpy as np
import pytest

import repair_cases as RC
from oracle import crossword

Row, Col = RC.Row, RC.Col

# every case at k = 8 (GF(2^8), byte tables) and k = 65 (m = 128); family A also at
# k = 129 (GF(2^16): the delta has a partner byte)
PARAMS = ([(name, k, 64, "default") for k in (8, 65) for name in RC.CASES] +
          [(name, 129, 64, "default") for name in RC.FAMILY_A] +
          [("A_row_last", 65, 128, "default")] +
          [(name, 65, 64, "nmt") for name in ("A_row_last", "A_row_0", "C_row_root_0", "C_col_root_last", "D_control")])
IDS = ["%s-k%d-S%d-%s" % p for p in PARAMS]


def _codeword_vectors(sq, axis):
    W = sq.shape[0]
    return [i for i in range(W) if crossword.verify_encoding(
        [(sq[i, p] if axis == Row else sq[p, i]).tobytes() for p in range(W)])]


@pytest.mark.parametrize("k,S", [(8, 64), (65, 128), (129, 64)])
def test_delta_is_a_minimum_weight_codeword(k, S):
    for j, b in ((0, 0), (k - 1, S - 1), (k // 2, 17)):
        d = RC.delta(k, S, j, b)
        assert crossword.verify_encoding([x.tobytes() for x in d])
        assert np.flatnonzero(d.any(axis=1)).tolist() == [j] + list(range(k, 2 * k))
        assert set(np.flatnonzero(d.any(axis=0)).tolist()) == RC.delta_offsets(k, S, b)
    assert RC.delta_offsets(129, 64, 63) == {31, 63} and RC.delta_offsets(65, 128, 127) == {127}


@pytest.mark.parametrize("name,k,S,tree", PARAMS, ids=IDS)
def test_case_properties(name, k, S, tree):
    flat, rr, cr, note = RC.case(name, k, S, tree)
    W, valid, full, pres = 2 * k, note["valid"], note["full"], note["present"]
    assert len(flat) == W * W and len(rr) == len(cr) == W
    # the valid square is a 2D codeword; the committed square fails in exactly the named vectors
    everything = list(range(W))
    assert _codeword_vectors(valid, Row) == everything and _codeword_vectors(valid, Col) == everything
    for axis in (Row, Col):
        assert _codeword_vectors(full, axis) == [i for i in everything if i not in note["bad"][axis]], axis
    if name in ("A_row_k", "A_row_last", "A_row_0", "B_col_kept"):
        assert note["bad"][Row] == [] and len(note["bad"][Col]) == k + 1
    if name == "B_row_kept":
        assert note["bad"][Col] == [] and len(note["bad"][Row]) == k + 1
    if note["family"] in "CD":
        assert np.array_equal(full, valid) and note["bad"] == {Row: [], Col: []}
    # differing cells and byte offsets
    diff = full != valid
    assert set(np.flatnonzero(diff.any(axis=(0, 1))).tolist()) == set(note["offsets"])
    if tree == "nmt":
        assert all(o >= RC.NS for o in note["offsets"])
        assert np.array_equal(full[:, :, :RC.NS], valid[:, :, :RC.NS])
    assert np.flatnonzero(diff.any(axis=(1, 2))).tolist() == sorted(
        note["touched"][Row] if note["family"] in "ABE" else [])
    assert np.flatnonzero(diff.any(axis=(0, 2))).tolist() == sorted(
        note["touched"][Col] if note["family"] in "ABE" else [])
    if name == "A_row_k":  # the first 16-byte word of the bottom half
        assert diff[k, 0, 0 if tree == "default" else RC.NS]
    if name == "A_row_last":  # the last byte of the square
        assert diff[W - 1, W - 1, S - 1]
    # presence: BenchmarkRepair's k of 2k per row; which vectors are complete
    assert [x is not None for x in flat] == pres.reshape(-1).tolist()
    assert all(a == b for a, b in zip(flat, RC.cells(full)) if a is not None)
    assert RC.complete_vectors(pres) == note["complete"]
    if name == "B_col_kept":
        assert note["complete"] == [(Col, k + k // 2)] and k + k // 2 in note["bad"][Col]
        assert (pres.sum(axis=1) == k).all()
    elif name == "B_row_kept":
        assert note["complete"] == [(Row, k + k // 2)] and k + k // 2 in note["bad"][Row]
        assert (pres.sum(axis=0) == k).all()
    elif name == "E_overdetermined_row":
        assert note["complete"] == []
        assert pres.sum(axis=1).tolist() == [k, k + 3] + [k] * (W - 2)
        (r,), (c,) = note["bad"][Row], note["bad"][Col]
        assert r == 1 and pres[r, c]
    else:
        assert note["complete"] == [] and (pres.sum(axis=1) == k).all()
    # committed roots differ from the valid square's in exactly the touched vectors
    rr_v, cr_v = RC.default_roots(valid)
    rr_d, cr_d = note["default_roots"]
    assert [i for i in everything if rr_d[i] != rr_v[i]] == sorted(note["touched"][Row])
    assert [i for i in everything if cr_d[i] != cr_v[i]] == sorted(note["touched"][Col])
    if tree == "default":
        assert (rr, cr) == (rr_d, cr_d)
    else:
        from oracle import nmt
        rr_n, cr_n = nmt.eds_roots(valid, k, RC.NS)
        assert [i for i in everything if rr[i] != rr_n[i]] == sorted(note["touched"][Row])
        assert [i for i in everything if cr[i] != cr_n[i]] == sorted(note["touched"][Col])
        assert all(len(x) == 2 * RC.NS + 32 for x in rr + cr)
    if note["family"] == "C":  # one byte of one root
        (axis, idx), = [(a, i) for a in (Row, Col) for i in note["touched"][a]]
        got, was = ((rr, rr_v) if axis == Row else (cr, cr_v)) if tree == "default" else (
            (rr, rr_n) if axis == Row else (cr, cr_n))
        assert sum(x != y for x, y in zip(got[idx], was[idx])) == 1


@pytest.mark.parametrize("name,k,S,tree", PARAMS, ids=IDS)
def test_oracle_outcome(name, k, S, tree):
    """A: Byzantine(Col, .) from the solver; B: Byzantine on the complete vector with no
    nil among its shares; C: Byzantine on the altered root's vector; D: ok; E: whatever
    the oracle says, which is not ok."""
    flat, _, _, note = RC.case(name, k, S, tree)
    want, after = RC.expected(name, k, S, tree)
    family = note["family"]
    # present cells are never changed; the oracle fills nil cells only with verified rows / columns
    assert all(a == b for a, b in zip(flat, after) if a is not None)
    if family == "D":
        assert want == "ok" and after == RC.cells(note["valid"])
        return
    assert isinstance(want, tuple), want
    axis, index, shares = want
    W = 2 * k
    # the vector as the solver left it: cells it had verified and inserted stay
    assert shares == [after[index * W + p] if axis == Row else after[p * W + index] for p in range(W)]
    if family == "A":
        assert axis == Col and index in note["bad"][Col]
        assert any(s is None for s in shares)
    elif family == "B":
        assert [(axis, index)] == note["complete"] and all(s is not None for s in shares)
        assert after == list(flat)  # found before any sweep
    elif family == "C":
        assert [(axis, index)] == [(a, i) for a in (Row, Col) for i in note["touched"][a]]
    else:
        assert index in note["bad"][axis]
