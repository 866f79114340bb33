"""GPU: Repair's device verification on squares committed to bad encodings
(tests/repair_cases.py): each case leaves exactly one of the three checks -- the
pre-repair check (DevSquare::verify_encoding), the fast paths' encoding compare, the
root compare -- between a bad square and RSM_OK, at sizes where the device fast paths
run:

  k = 8, 16   generic fast_repair, byte-table kernels
  k = 65      zero-copy sweep (decode_gf8_split_zc_kernel), bit-sliced column re-encode;
              once with 128-byte shares, so the delta byte is not in a cell's only
              64-byte block
  k = 128     the same at the workload's k (family A only)
  k = 129     zero-copy GF(2^16), m = 256

k = 257 (m = 512) is left out: the Python oracle needs 17 s for one family-A case
there (0.3 s at k = 65, 1.9 s at k = 129), and the verification code after the sweep is
the same as at k = 129.

Every case asserts the outcome (ok / ErrUnrepairableDataSquare / ErrByzantineData with
Axis, Index, Shares) and the cells left behind against the oracle crossword on the
same cells, and repair_stats() against the family's expectation: fallback_reason names
the check that rejected the fast path.

NMT cases: the oracle crossword only knows the DefaultTree.  The solver's control flow
(extendeddatacrossword.go) depends on the tree only through root equality -- every
use of a root is a comparison with the committed one -- and the namespaces of these
squares are sorted and untouched (delta offsets >= 29), so no tree of theirs fails.  A
computed root equals the committed one exactly when the vector's shares equal the
committed square's, for either tree (up to hash collisions).  So the expected (Axis,
Index, Shares) is the DefaultTree oracle's outcome on the same cells with the
DefaultTree roots of the same altered square (and the same root flipped).
"""
import ctypes

import pytest

import repair_cases as RC
import rsmt2d_amd as R

pytestmark = pytest.mark.gpu

# family -> (fast_path, fallback_reason); E: any non-zero reason
STATS = {"A": (0, R.FALLBACK_ENCODING), "B": (0, R.FALLBACK_NONE), "C": (0, R.FALLBACK_ROOTS),
         "D": (1, R.FALLBACK_NONE)}


def _outcome(eds, rr, cr):
    try:
        eds.Repair(list(rr), list(cr))
        return "ok"
    except R.ErrByzantineData as b:
        return (b.Axis, b.Index, b.Shares)
    except R.RSMError as e:
        assert e is R.ErrUnrepairableDataSquare, e
        return "unrepairable"


def _check_case(name, k, S=64, tree="default"):
    flat, rr, cr, note = RC.case(name, k, S, tree)
    want, after = RC.expected(name, k, S, tree)
    ctor = R.NewDefaultTree if tree == "default" else R.newErasuredNamespacedMerkleTreeConstructor(k, RC.NS)
    eds = R.ImportExtendedDataSquare(list(flat), R.NewLeoRSCodec(), ctor)
    got = _outcome(eds, rr, cr)
    st = eds.repair_stats()
    stats = dict(fast_path=st.fast_path, sweeps=st.sweeps, decoded_vectors=st.decoded_vectors,
                 fallback_reason=st.fallback_reason)
    kind = lambda o: o if isinstance(o, str) else ("byzantine",) + tuple(o[:2])
    assert kind(got) == kind(want), stats
    assert got == want, stats  # and the byzantine vector's shares, nil where missing
    left = eds.Flattened()
    # present cells unchanged; nil cells nil unless the oracle's solver filled them (the
    # zero-copy sweep's rebuilt bytes in nil cells must not show)
    assert all(a == b for a, b in zip(flat, left) if a is not None), stats
    assert [x is None for x in left] == [x is None for x in after], stats
    assert left == after, stats
    family = note["family"]
    if family == "E":
        assert st.fast_path == 0 and st.fallback_reason != R.FALLBACK_NONE, stats
    else:
        assert (st.fast_path, st.fallback_reason) == STATS[family], stats
    if family == "A":  # the encoding compare alone found it: roots and statuses were consistent
        assert st.sweeps >= 1, stats
    if family == "B":  # the pre-repair check found it
        assert st.sweeps == 0 and st.decoded_vectors == 0, stats
    if family == "D":
        assert st.sweeps >= 1 and left == RC.cells(note["valid"]), stats
    return st


@pytest.mark.parametrize("k", [8, 16, 65, 129])
@pytest.mark.parametrize("name", RC.CASES)
def test_case_matches_oracle(lib, name, k):
    _check_case(name, k)


@pytest.mark.parametrize("name", RC.FAMILY_A)
def test_family_a_at_workload_k(lib, name):
    _check_case(name, 128)


def test_family_a_two_block_shares(lib):
    _check_case("A_row_last", 65, S=128)


@pytest.mark.parametrize("name", ["A_row_last", "A_row_0", "C_row_root_0", "C_col_root_last", "D_control"])
def test_case_matches_oracle_nmt(lib, name):
    _check_case(name, 65, tree="nmt")


@pytest.fixture
def pctx(lib):
    """A private context (its limits are lowered; the shared one keeps the defaults)."""
    h = ctypes.c_void_p()
    R._check(lib.rsm_ctx_create(0, ctypes.byref(h)))
    yield h.value
    lib.rsm_ctx_destroy(h.value)


def test_declined_zero_copy_rejects_with_encoding(lib, pctx, monkeypatch):
    """k = 128, S = 64 on a context whose offset limit sends the column codewords to the
    wide forms: the zero-copy Repair declines (as test_gpu_large.py's "columns" case
    makes it) and the generic fast_repair must reject the square itself."""
    k, S = 128, 64
    R._check(lib.rsm_ctx_set_limits(pctx, (k + 1) * S + S, 0))
    monkeypatch.setattr(R, "device_context", lambda device=0: pctx)  # Repair attaches this context
    st = _check_case("A_row_k", k, S)
    assert st.sweeps >= 1
