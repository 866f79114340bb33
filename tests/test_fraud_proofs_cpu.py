"""CPU: the model of rsm_fraud_proofs_verify_dev (tests/fraud_proofs.py) on the reference's
own fraud-proof scenario and on the verification cases of tests/repair_cases.py, and what the
new calls decide before any device use: rsm_fraud_proof_samples, rsm_fraud_work_bytes and
the argument errors of rsm_fraud_proofs_verify_dev, with a fake context as in
tests/test_dev_entry_errors_cpu.py.  tests/test_gpu_fraud_proofs.py holds the device to the model."""
import ctypes

import numpy as np
import pytest

import fraud_proofs as F
import oracle
import proof_status as PS
import repair_cases as RC
import repair_checked as C
import repair_dev_calls as D
import rsmt2d_amd as R
from oracle import crossword

S = 64


def _nmt(ns, k):
    return ctypes.byref(R.NmtParams(ns, 1, k))


# ---- ABI -----------------------------------------------------------------------------
def test_symbols_and_records(lib):
    for name in ("rsm_fraud_work_bytes", "rsm_fraud_proof_samples", "rsm_fraud_proofs_verify_dev"):
        assert hasattr(lib, name), name
        assert name in R.SIGNATURES and getattr(lib, name).argtypes == R.SIGNATURES[name][1], name
    assert ctypes.sizeof(R.FraudVerdict) == 16
    assert [f[0] for f in R.FraudVerdict._fields_] == ["verdict", "reason", "pos", "present"]
    assert (R.FRAUD_VALID, R.FRAUD_TOOFEW, R.FRAUD_SHARE, R.FRAUD_CONSISTENT) == (0, 1, 2, 3)
    assert (F.VALID, F.TOOFEW, F.SHARE, F.CONSISTENT) == (0, 1, 2, 3)
    assert (F.ROOT, F.ENCODING, F.TREE) == (R.BYZ_ROOT, R.BYZ_ENCODING, R.BYZ_TREE)


# ---- the model -----------------------------------------------------------------------
def test_model_on_the_reference_scenario():
    """extendeddatacrossword_test.go:116-163: the k = 2 square of constant shares with cell
    (0, 0) = 66..., roots committed to it; the shares the crossword's ErrByzantineData
    carries, each with its proof in the orthogonal tree, are a valid fraud proof."""
    k, size = 2, 512
    ods = np.array([[np.full(size, v, np.uint8) for v in row] for row in ((1, 2), (3, 4))])
    sq = np.array(oracle.extend_square(np.ascontiguousarray(ods), nthreads=1))
    sq[0, 0] = 66
    rr, cr = RC.default_roots(sq)
    with pytest.raises(crossword.Byzantine) as ei:
        crossword.repair(RC.cells(sq), list(rr), list(cr))
    byz = ei.value
    squares = PS.Squares(sq[None], None)
    table = F.table_of(squares)
    assert table[0, 0].tobytes() == b"".join(rr) and table[0, 1].tobytes() == b"".join(cr)
    proof = F.honest(squares, (0, byz.axis, byz.index), [x is not None for x in byz.shares])
    assert [s.tobytes() for s, x in zip(proof.shares, byz.shares) if x is not None] == [x for x in byz.shares if x is not None]
    want, full = proof.expect(table, k, None)
    assert want[0] == F.VALID and want[1] in (F.ROOT, F.ENCODING) and want[3] == sum(x is not None for x in byz.shares)
    assert len(full) == 2 * k


def _case_proof(name, k, tree, ref=None, present=None):
    """(proof, table, params, note): the vector the checked model names in an RC case (or
    `ref`), as its holder proves it: the cells of the square the roots are committed to, under
    the case's presence (or `present`)."""
    flat, rr, cr, note = RC.case(name, k, S, tree)
    p = D.nmt_params(k, RC.NS) if tree == "nmt" else None
    squares = PS.Squares(np.array(note["full"])[None], p)
    nl = PS.node_len(p)
    table = np.frombuffer(b"".join(rr) + b"".join(cr), np.uint8).reshape(1, 2, 2 * k, nl)
    if ref is None:
        sq, pres = D.case_square(flat, 2 * k, S)
        out = C.model(sq, pres, rr, cr, k, tree)
        assert out.status == C.BYZANTINE
        ref, present = (0, out.axis, out.index), [x is not None for x in out.shares]
    return F.honest(squares, ref, present), table, p, note


@pytest.mark.parametrize("tree", ["default", "nmt"])
@pytest.mark.parametrize("name,reason", [("B_col_kept", F.ENCODING), ("B_row_kept", F.ENCODING),
                                         ("C_row_root_0", F.ROOT), ("C_col_root_last", F.ROOT),
                                         ("C_row_root_last", F.ROOT), ("E_overdetermined_row", None)])
def test_model_on_the_verification_cases(name, reason, tree):
    """The vector checked Repair names is a valid fraud proof: B cases by their encoding (the
    kept vector is complete and its root committed), C cases by the flipped root, the
    overdetermined row by either."""
    k = 8
    proof, table, p, note = _case_proof(name, k, tree)
    if name.startswith("C_"):  # only that root differs: every share proof verifies
        (axis, index), = [(a, i) for a in (0, 1) for i in note["touched"][a]]
        assert proof.ref == (0, axis, index)
    want, full = proof.expect(table, k, p)
    assert want[0] == F.VALID and want[2] == 0 and want[3] == int(proof.present.sum())
    if reason is not None:
        assert want[1] == reason
    q, axis, index = proof.ref
    shares = [s.tobytes() if on else None for s, on in zip(proof.shares, proof.present)]
    assert C.is_byzantine(shares, axis, index, table[0, axis, index].tobytes(), k, tree)
    assert want[1] == C.vector_reason(full, axis, index, table[0, axis, index].tobytes(), k, tree)


@pytest.mark.parametrize("tree", ["default", "nmt"])
def test_model_finds_no_fraud_in_the_control(tree):
    k = 8
    pres = np.array(RC.case("D_control", k, S, tree)[3]["present"], bool)
    for axis in (0, 1):
        for index in (0, k - 1, k, 2 * k - 1):
            on = pres[index] if axis == 0 else pres[:, index]
            for present in (on, None):
                proof, table, p, _ = _case_proof("D_control", k, tree, (0, axis, index), present)
                want, full = proof.expect(table, k, p)
                have = 2 * k if present is None else int(on.sum())  # a column may keep fewer than k
                assert want == (F.CONSISTENT if have >= k else F.TOOFEW, 0, 0, have)
                assert have < k or [x.tobytes() for x in proof.shares] == list(full)


def test_model_rules_in_order():
    """TOOFEW before SHARE before the vector's check; the lowest failing slot is named."""
    k = 8
    proof, table, p, _ = _case_proof("B_col_kept", k, "default")
    assert proof.expect(table, k, p)[0][:2] == (F.VALID, F.ENCODING)
    bad = proof.copy()
    bad.shares[5, 7] ^= 1
    bad.shares[11, 0] ^= 0x80
    assert bad.expect(table, k, p)[0] == (F.SHARE, PS.ROOT, 5, 2 * k)
    bad.records[3] = b"\xff" + bad.records[3][1:]
    assert bad.expect(table, k, p)[0] == (F.SHARE, PS.MALFORMED, 3, 2 * k)
    bad.present[:] = F.pattern("short", k)
    assert bad.expect(table, k, p)[0] == (F.TOOFEW, 0, 0, k - 1)


# ---- rsm_fraud_proof_samples ----------------------------------------------------------
def test_proof_samples(lib):
    for k in (1, 2, 3, 8, 129):
        for axis in (0, 1):
            for index in (0, 2 * k - 1):
                for square in (0, 7):
                    got = R.fraud_proof_samples(axis, index, k, square)
                    assert got == [(square, axis ^ 1, j, index) for j in range(2 * k)]
    out = (R.Sample * 4)()
    ref = R.RootRef(0, 0, 0)
    f = lib.rsm_fraud_proof_samples
    assert f(None, 2, out) == R.RSM_EINVAL and f(ctypes.byref(ref), 2, None) == R.RSM_EINVAL
    assert f(ctypes.byref(ref), 0, out) == R.RSM_EINVAL and f(ctypes.byref(ref), 32769, out) == R.RSM_EINVAL
    for bad in (R.RootRef(0, 2, 0), R.RootRef(0, 1, 4)):
        assert f(ctypes.byref(bad), 2, out) == R.RSM_EINVAL
        assert b"out of range" in lib.rsm_last_error()


# ---- rsm_fraud_work_bytes -------------------------------------------------------------
def test_work_bytes_zero_exactly_beyond_the_limits(lib):
    """The limits of the device trees (those rsm_repair_checked_work_bytes has for one
    square), share sizes a multiple of 64, n <= 65535 and n * 2k <= 2^24."""
    wb, tree_ok = lib.rsm_fraud_work_bytes, lib.rsm_repair_checked_work_bytes
    shapes = [(k, 64, n, None) for k in (1, 2, 3, 8, 128, 129, 1024, 1025, 0) for n in (0, 1, 5, 4097, 65535, 65536)]
    shapes += [(128, 64, 65535, None), (128, 64, 65536, None), (129, 64, 65535, None)]  # 2^24 - 256, n, 2^24 + ...
    shapes += [(8, 96, 1, None), (8, 0, 1, None), (8, 512, 64, None), (1024, 64, 8192, None), (1024, 64, 8193, None)]
    for k in (4, 8, 512, 513):
        for ns in (0, 1, 29, 32, 33):
            shapes += [(k, 64, n, (ns, k)) for n in (1, 2 * k + 3)]
    shapes += [(8, 64, 1, (29, 4)), (8, 64, 1, (29, 7)), (8, 64, 1, (29, 0)), (8, 64, 1, (29, 100))]
    seen = set()
    for k, s, n, p in shapes:
        got = wb(k, s, n, _nmt(*p) if p else None)
        want = tree_ok(k, s, 1, _nmt(*p) if p else None) != 0 and n <= 65535 and n * 2 * k <= 1 << 24
        assert (got != 0) == want, (k, s, n, p)
        seen.add(want)
        if got:
            W = 2 * k
            assert got >= n * W * (16 + 4 + (64 if p else 32)) + min(n, W) * W * s, (k, s, n, p)
    assert seen == {True, False}
    assert wb(128, 64, 65535, None) != 0 and wb(129, 64, 65535, None) == 0 and wb(1024, 64, 8193, None) == 0


# ---- argument errors -------------------------------------------------------------------
A, A8 = 4096, 4096 + 8
_FAKE = ctypes.create_string_buffer(4096)
CTX = ctypes.addressof(_FAKE)
_OUT = (R.FraudVerdict * 3)()
NAMES = ["ctx", "d_shares", "d_present", "d_records", "d_roots", "k", "S", "count", "nmt", "refs", "n", "d_work", "verdicts",
         "stream"]
GOOD = dict(ctx=CTX, d_shares=A, d_present=A + 1, d_records=A + 3, d_roots=A + 5, k=8, S=64, count=1, nmt=None,
            refs=[(0, 1, 15)], d_work=A, verdicts=_OUT, stream=None)
OPERANDS = ["d_shares", "d_present", "d_records", "d_roots", "refs", "d_work", "verdicts"]
BAD_ARGS, EMPTY, ALIGNED, RANGE = b"bad arguments", b"empty shares", b"16-byte aligned", b"out of range"
UNSUP = b"not supported"

CASES = {
    "null_ctx": (dict(ctx=None), R.RSM_EINVAL, BAD_ARGS),
    "k_0": (dict(k=0), R.RSM_EINVAL, BAD_ARGS),
    "S_96": (dict(S=96), R.RSM_ESHARESIZE, b"multiple of 64"),
    "S_0": (dict(S=0), R.RSM_EINVAL, EMPTY),
    "k_1025": (dict(k=1025), R.RSM_EUNSUPPORTED, UNSUP),
    "ns_33": (dict(nmt=(33, 1, 8)), R.RSM_EUNSUPPORTED, UNSUP),
    "ns_0": (dict(nmt=(0, 1, 8)), R.RSM_EUNSUPPORTED, UNSUP),
    "nmt_past_its_square": (dict(nmt=(8, 1, 4)), R.RSM_EUNSUPPORTED, UNSUP),
    "nmt_width_1026": (dict(k=513, nmt=(8, 1, 513)), R.RSM_EUNSUPPORTED, UNSUP),
    "n_65536": (dict(n=65536), R.RSM_EUNSUPPORTED, UNSUP),
    "cells_past_2_24": (dict(k=1024, n=8193), R.RSM_EUNSUPPORTED, UNSUP),
    "n_0": (dict(n=0), R.RSM_OK, b""),
    "count_0": (dict(count=0), R.RSM_OK, b""),
    "shares_misaligned": (dict(d_shares=A8), R.RSM_EINVAL, ALIGNED),
    "work_misaligned": (dict(d_work=A8), R.RSM_EINVAL, ALIGNED),
    "bad_square_at_0": (dict(refs=[(1, 1, 15), (0, 1, 15), (0, 1, 15)]), R.RSM_EINVAL, b"ref 0 (square 1, axis 1, index 15)"),
    "bad_axis_at_2": (dict(refs=[(0, 1, 15), (0, 1, 15), (0, 2, 15)]), R.RSM_EINVAL, b"ref 2 (square 0, axis 2, index 15)"),
    "bad_index_at_2": (dict(refs=[(0, 1, 15), (0, 1, 15), (0, 0, 16)]), R.RSM_EINVAL, b"ref 2 (square 0, axis 0, index 16)"),
    # two checks fire: the earlier one answers
    "order_k_S": (dict(k=0, S=96), R.RSM_EINVAL, BAD_ARGS),
    "order_S_shape": (dict(S=96, k=1025), R.RSM_ESHARESIZE, b"multiple of 64"),
    "order_empty_shape": (dict(S=0, k=1025), R.RSM_EINVAL, EMPTY),
    "order_shape_n_0": (dict(k=1025, n=0), R.RSM_EUNSUPPORTED, UNSUP),
    "order_shape_count_0": (dict(k=1025, count=0), R.RSM_EUNSUPPORTED, UNSUP),
    "order_n_0_nulls": (dict({x: None for x in OPERANDS}, n=0), R.RSM_OK, b""),
    "order_count_0_nulls": (dict({x: None for x in OPERANDS if x != "refs"}, count=0), R.RSM_OK, b""),
    "order_count_0_range": (dict(count=0, refs=[(0, 2, 0)]), R.RSM_OK, b""),
    "order_null_misaligned": (dict(d_roots=None, d_shares=A8), R.RSM_EINVAL, BAD_ARGS),
    "order_misaligned_range": (dict(d_work=A8, refs=[(1, 0, 0)]), R.RSM_EINVAL, ALIGNED),
}
CASES.update({f"null_{x}": (dict({x: None}), R.RSM_EINVAL, BAD_ARGS) for x in OPERANDS})


def _call(lib, overrides):
    v = dict(GOOD, **overrides)
    keep, args = [], []
    for name in NAMES:
        x = v.get(name)
        if name == "n" and "n" not in v:
            x = len(v["refs"]) if v.get("refs") else 1  # a NULL array of one element
        elif name == "refs" and x is not None:
            x = (R.RootRef * len(x))(*[R.RootRef(*e) for e in x])
        elif name == "nmt" and x is not None:
            keep.append(R.NmtParams(*x))
            x = ctypes.byref(keep[-1])
        args.append(x)
    rc = lib.rsm_fraud_proofs_verify_dev(*args)
    return int(rc), (lib.rsm_last_error() or b"") if rc else b""


@pytest.mark.parametrize("label", sorted(CASES))
def test_argument_errors_before_any_device_use(lib, label):
    """`ctx` is the address of a zeroed buffer (no rsm_ctx) and the device pointers are small
    integers that are never dereferenced: every case returns before use_device."""
    overrides, want_rc, text = CASES[label]
    rc, msg = _call(lib, overrides)
    assert rc != R.RSM_EDEVICE
    assert rc == want_rc, (label, rc, msg)
    if rc:
        assert text in msg, (label, msg)
        if rc != R.RSM_ESHARESIZE:  # the share-size text is the codec's, shared by every call
            assert b"rsm_fraud_proofs_verify_dev" in msg, (label, msg)
