"""GPU: rsm_fraud_proofs_verify_dev -- bad-encoding fraud proofs validated in batches on the
device (include/rsmt2d_hip.h "bad-encoding fraud proofs").

Every call runs through fraud_proofs.run: shares, presence bytes, records and scratch between
guard bands, absent slots 0xA5, every present slot byte-identical afterwards.  The device is
held to the model of tests/fraud_proofs.py (pinned on the CPU by
tests/test_fraud_proofs_cpu.py) verdict record for verdict record, and the rebuilt slots to
the oracle codec.

  k = 2 (S = 512)  the reference's case      k = 3    width 6: unpaired nodes, odd encode
  k = 8            byte tables               k = 66   the 65..128 decoders, W = 132
  k = 129          GF(2^16), four proofs     NMT: k = 8 (ns 29), k = 4 (ns 1 and 32)
"""
import ctypes
import functools

import numpy as np
import pytest

import fraud_proofs as F
import oracle
import proof_status as PS
import proof_verify as V
import repair_cases as RC
import repair_dev_calls as D
import rsmt2d_amd as R

pytestmark = pytest.mark.gpu

Row, Col = 0, 1


def _params(k, ns):
    return R.NmtParams(ns, 1, k) if ns else None


def _valid(k, S, ns, seed):
    if ns:
        ods = V.sorted_q0_square(k, S, ns, seed)[:k, :k]
    else:
        ods = np.random.default_rng(seed).integers(0, 256, (k, k, S), dtype=np.uint8)
    return np.array(oracle.extend_square(np.ascontiguousarray(ods), nthreads=8))


@functools.lru_cache(maxsize=None)
def world(k, S, ns):
    """(Squares, table): three squares and the roots committed to them.
    0: valid.  1: a minimum-weight row codeword XOR-ed into row k, so every row is a codeword
    and columns 0 and k .. 2k - 1 are not.  2, NMT: valid but for row 0 of quadrant 0, which
    is out of namespace order (its tree fails, no root exists); 2, DefaultTree: valid, with
    the committed root of row 0 flipped."""
    W = 2 * k
    a = _valid(k, S, ns, 0xF4A0 + k)
    b = _valid(k, S, ns, 0xF4A1 + k)
    b[k] ^= RC.delta(k, S, 0, ns)
    broken = ()
    if ns:
        seed = 0xF4A2 + k
        while True:
            try:
                c = np.array(F.unordered_q0(k, S, ns, seed))
                break
            except AssertionError:  # (0, 1) and (1, 0) drew the same namespace
                seed += 0x100
        broken = ((2, Row, 0),)
    else:
        c = _valid(k, S, ns, 0xF4A2 + k)
    sq = PS.Squares(np.stack([a, b, c]), _params(k, ns))
    table = F.table_of(sq, broken)
    if not ns:
        table[2, Row, 0, -1] ^= 1
    table.setflags(write=False)
    return sq, table


def _flip(proof, slot, byte=None, label=None):
    out = proof.copy(label)
    out.shares[slot, out.shares.shape[1] - 1 if byte is None else byte] ^= 0x10
    return out


def mixed_batch(k, S, ns, n):
    """n proofs over the three squares of world(); the first seven hold every verdict, every
    reason the tree can give and both axes."""
    sq, _ = world(k, S, ns)
    W = 2 * k
    specs = [((1, Col, 0), "all", "ENCODING: a non-codeword column, complete"),
             ((1, Col, 0), "first", "ROOT: the same column rebuilt from its first half"),
             ((2, Row, 0), "mixed", "TREE (NMT) / ROOT: the bad row of square 2"),
             ((0, Row, 1), "mixed", "CONSISTENT row below k"),
             ((0, Row, 0), "short", "TOOFEW"),
             ((0, Row, W - 1), "all", "SHARE"),
             ((0, Col, W - 1), "second", "CONSISTENT column past k"),
             ((1, Col, k), "all", "ENCODING: column k"),
             ((2, Row, 0), "all", "TREE (NMT) / ROOT, complete"),
             ((0, Row, k), "none", "TOOFEW: nothing"),
             ((1, Row, k), "all", "CONSISTENT: the altered row is a codeword"),
             ((1, Col, 1), "first", "CONSISTENT column below k"),
             ((1, Col, W - 1), "mixed", "ROOT: last column from k shares"),
             ((0, Col, 0), "mixed", "CONSISTENT column 0")]
    out = []
    for i in range(n):
        ref, kind, label = specs[i % len(specs)]
        f = F.honest(sq, ref, F.pattern(kind, k, i), label)
        if label == "SHARE":
            f = _flip(f, (3 + i) % W)
        out.append(f)
    return out


DEFAULT = [(2, 512), (3, 64), (8, 64), (66, 64)]
NMT = [(8, 64, 29), (4, 64, 1), (4, 64, 32)]
SHAPES = [(k, S, 0) for k, S in DEFAULT] + NMT


@pytest.mark.parametrize("k,S,ns", SHAPES)
def test_mixed_batch_equals_the_model(lib, k, S, ns):
    """count = 3 squares, n = 2k + 3 proofs -- more than the width, so the batch spans two
    chunks of the decoders' square view."""
    _, table = world(k, S, ns)
    proofs = mixed_batch(k, S, ns, 2 * k + 3)
    got = F.check(lib, proofs, table, k, S, _params(k, ns))
    verdicts = {g[0] for g in got}
    reasons = {g[1] for g in got if g[0] == F.VALID}
    assert verdicts == {F.VALID, F.TOOFEW, F.SHARE, F.CONSISTENT}
    assert reasons == ({F.ROOT, F.ENCODING, F.TREE} if ns else {F.ROOT, F.ENCODING})
    assert {f.ref[1] for f, g in zip(proofs, got) if g[0] == F.VALID} == {Row, Col}
    assert {f.ref[1] for f, g in zip(proofs, got) if g[0] == F.CONSISTENT} == {Row, Col}


def test_gf16_four_proofs(lib):
    k, S = 129, 64
    sq, table = world(k, S, 0)
    W = 2 * k
    proofs = [F.honest(sq, (1, Col, 0), None, "ENCODING"),
              F.honest(sq, (1, Col, k), F.pattern("second", k), "ROOT"),
              F.honest(sq, (0, Row, k - 1), F.pattern("mixed", k), "CONSISTENT"),
              _flip(F.honest(sq, (0, Col, W - 1), F.pattern("first", k)), 5, 0, "SHARE")]
    got = F.check(lib, proofs, table, k, S)
    assert [g[:2] for g in got] == [(F.VALID, F.ENCODING), (F.VALID, F.ROOT), (F.CONSISTENT, 0), (F.SHARE, PS.ROOT)]
    assert got[3][2] == 5


@pytest.mark.parametrize("k,S,ns", [(2, 512, 0), (3, 64, 0), (8, 64, 0), (8, 64, 29), (4, 64, 1)])
def test_presence_patterns(lib, k, S, ns):
    """Exactly k present as the first half, the second half or mixed; all 2k; k - 1; none --
    on a good vector and on a bad one of either axis."""
    sq, table = world(k, S, ns)
    kinds = ("first", "second", "mixed", "all", "short", "none")
    proofs = [F.honest(sq, ref, F.pattern(kind, k, 7), kind) for ref in ((0, Row, 1), (0, Col, k), (1, Col, 0))
              for kind in kinds]
    got = F.check(lib, proofs, table, k, S, _params(k, ns))
    for f, g in zip(proofs, got):
        want = {"short": F.TOOFEW, "none": F.TOOFEW}.get(f.label, F.VALID if f.ref[0] == 1 else F.CONSISTENT)
        assert g[0] == want and g[3] == {"all": 2 * k, "short": k - 1, "none": 0}.get(f.label, k), (f.ref, f.label, g)


def _sample(sq, s):
    return np.frombuffer(sq.share(s), np.uint8), sq.record(s)


@pytest.mark.parametrize("k,S,ns", [(8, 64, 0), (8, 64, 29), (3, 64, 0)])
def test_hostile_proofs(lib, k, S, ns):
    sq, table = world(k, S, ns)
    p = _params(k, ns)
    W = 2 * k
    ref = (0, Row, 1)
    q, axis, index = ref
    base = F.honest(sq, ref, None)
    proofs, want = [base.copy("honest")], [(F.CONSISTENT, 0, 0)]

    proofs.append(_flip(base, 4, None, "share bit"))
    want.append((F.SHARE, PS.ROOT, 4))

    f = base.copy("a valid proof of another position")
    f.shares[2], f.records[2] = _sample(sq, (q, axis ^ 1, 2, index + 1))
    proofs.append(f)
    want.append((F.SHARE, None, 2))

    f = base.copy("a record of the same-axis tree")
    f.records[W - 2] = sq.record((q, axis, index, W - 2))
    proofs.append(f)
    want.append((F.SHARE, None, W - 2))

    f = base.copy("wrong header")
    f.records[5] = (int.from_bytes(f.records[5][:4], "little") + 1).to_bytes(4, "little") + f.records[5][4:]
    proofs.append(f)
    want.append((F.SHARE, PS.MALFORMED, 5))

    f = _flip(_flip(base, W - 1, 0), 3, 0, "two failing slots")
    proofs.append(f)
    want.append((F.SHARE, PS.ROOT, 3))

    f = _flip(base, 0, None, "a flipped share in an absent slot").copy()
    f.present[0] = 0
    proofs.append(f)
    want.append((F.CONSISTENT, 0, 0))

    if ns:  # a right-hand sibling whose min namespace lies below the fold's max: slot 0, pos 1
        nl = PS.node_len(p)
        n_nodes, mask = PS.proof_shape(W, index)
        i = next(i for i in range(n_nodes) if (mask >> i) & 1)
        f = base.copy("NMT siblings out of order")
        rec = bytearray(f.records[0])
        rec[8 + i * nl: 8 + i * nl + ns] = bytes(ns)
        f.records[0] = bytes(rec)
        proofs.append(f)
        want.append((F.SHARE, PS.ORDER, 0))

    got = F.check(lib, proofs, table, k, S, p)
    for f, g, w in zip(proofs, got, want):
        assert g[0] == w[0] and g[2] == w[2], (f.label, g, w)
        if w[1] is not None:
            assert g[1] == w[1], (f.label, g, w)
        else:
            assert g[1] in (PS.MALFORMED, PS.ORDER, PS.ROOT), (f.label, g)


@pytest.mark.parametrize("k,S,ns", [(8, 64, 0), (8, 64, 29)])
def test_absent_slots_do_not_show(lib, k, S, ns):
    """Two runs that differ only in the share and record bytes of the absent slots."""
    _, table = world(k, S, ns)
    proofs = mixed_batch(k, S, ns, 2 * k + 3)
    a = F.run(lib, proofs, table, k, S, _params(k, ns), fill=0xA5, record_fill=0x3C)
    b = F.run(lib, proofs, table, k, S, _params(k, ns), fill=0x00, record_fill=0xFF)
    assert a[0] == b[0]
    for i, g in enumerate(a[0]):
        if g[0] in (F.VALID, F.CONSISTENT):
            assert np.array_equal(a[1][i], b[1][i]), i


# ---- composition on device buffers ----------------------------------------------------
@pytest.mark.parametrize("tree", ["default", "nmt"])
def test_prove_repair_gather_validate(lib, tree):
    """Squares committed to bad encodings, their holder's node store (rsm_proof_nodes_dev), a
    checked Repair of the erased copies, then for every named vector rsm_proofs_dev over
    rsm_fraud_proof_samples, rsm_vectors_gather_dev and the new call on those device buffers
    as they are: VALID with the reason the Repair reported.  The valid half-erased square:
    its rows (k shares each) and, once repaired, any vector are CONSISTENT."""
    k, S = 8, 64
    W = 2 * k
    names = ["B_col_kept", "B_row_kept", "C_row_root_0", "C_col_root_last", "E_overdetermined_row", "A_row_k", "D_control"]
    count = len(names)
    p = D.nmt_params(k, RC.NS) if tree == "nmt" else None
    pp = ctypes.byref(p) if p is not None else None
    cases = [RC.case(name, k, S, tree) for name in names]
    full = np.stack([np.array(c[3]["full"]) for c in cases])
    given = [D.case_square(c[0], W, S) for c in cases]
    erased = np.stack([g[0] for g in given])
    pres = np.stack([g[1] for g in given]).astype(np.uint8)
    table = D.roots_table([(c[1], c[2]) for c in cases])
    ctx = R.device_context(0)
    rb = int(lib.rsm_proof_record_bytes(W, pp))
    bufs = dict(full=R.DeviceBuffer(full.nbytes), eds=R.DeviceBuffer(erased.nbytes), pres=R.DeviceBuffer(pres.nbytes),
                roots=R.DeviceBuffer(table.size), nodes=R.DeviceBuffer(int(lib.rsm_proof_nodes_bytes(W, pp, count))),
                before=R.DeviceBuffer(erased.nbytes), before_pres=R.DeviceBuffer(pres.nbytes))
    try:
        bufs["full"].upload(full.reshape(-1))
        bufs["roots"].upload(table)
        for name, src in (("eds", erased), ("before", erased), ("pres", pres), ("before_pres", pres)):
            bufs[name].upload(src.reshape(-1))
        R._check(lib.rsm_proof_nodes_dev(ctx, bufs["full"].ptr, W, S, count, pp, bufs["nodes"].ptr, None, None, None))
        outcome = R.repair_squares_checked_dev(bufs["eds"], bufs["pres"], k, S, bufs["roots"], count, p)
        bad = [s for s in range(count) if outcome[s][0].status == R.REPAIR_BYZANTINE]
        assert bad == list(range(count - 1)) and outcome[-1][0].status == R.REPAIR_OK

        def validate(eds, presence, refs):
            n = len(refs)
            samples = [s for r in refs for s in R.fraud_proof_samples(r[1], r[2], k, r[0])]
            recs, scratch = R.DeviceBuffer(n * W * rb), R.DeviceBuffer(n * W * S)
            shares, present = R.DeviceBuffer(n * W * S), R.DeviceBuffer(max(n * W, 16))
            try:
                arr = (R.Sample * len(samples))(*[R.Sample(*s) for s in samples])
                R._check(lib.rsm_proofs_dev(ctx, bufs["nodes"].ptr, bufs["full"].ptr, W, S, count, pp, arr, len(samples),
                                            recs.ptr, scratch.ptr, None))
                R._check(lib.rsm_vectors_gather_dev(ctx, eds.ptr, presence.ptr, k, S, count,
                                                    (R.RootRef * n)(*[R.RootRef(*r) for r in refs]), n, shares.ptr,
                                                    present.ptr, None))
                return R.verify_fraud_proofs_dev(shares, present, recs, bufs["roots"], k, S, refs, count, p)
            finally:
                for b in (recs, scratch, shares, present):
                    b.free()

        refs = [(s, outcome[s][1].axis, outcome[s][1].index) for s in bad]
        for s, v in zip(bad, validate(bufs["eds"], bufs["pres"], refs)):
            assert (v.verdict, v.reason) == (R.FRAUD_VALID, outcome[s][1].reason), (names[s], v.verdict, v.reason)
        ctl = count - 1
        rows = [(ctl, Row, i) for i in (0, k - 1, k, W - 1)]
        for v in validate(bufs["before"], bufs["before_pres"], rows):
            assert (v.verdict, v.reason, v.present) == (R.FRAUD_CONSISTENT, 0, k)
        for v in validate(bufs["eds"], bufs["pres"], rows + [(ctl, Col, i) for i in (0, k, W - 1)]):
            assert (v.verdict, v.reason, v.present) == (R.FRAUD_CONSISTENT, 0, W)
    finally:
        for b in bufs.values():
            b.free()


# ---- the Python mirror ------------------------------------------------------------------
@pytest.mark.parametrize("tree", ["default", "nmt"])
def test_bad_encoding_proof_validate(lib, tree):
    """extendeddatacrossword_test.go:116-163 through ExtendedDataSquare.BadEncodingProof and
    .Validate: the k = 2 square of constant shares, cell (0, 0) = 66..., roots committed to it.
    Row 0 is a valid fraud proof, row 1 is none.  NMT: the altered cell keeps its namespace,
    or no row root of the altered square would exist."""
    size, ns = 512, 29
    codec = R.NewLeoRSCodec()
    tree_fn = R.NewDefaultTree if tree == "default" else R.newErasuredNamespacedMerkleTreeConstructor(2, ns)
    original = R.ComputeExtendedDataSquare([bytes([v]) * size for v in (1, 2, 3, 4)], codec, tree_fn)
    corrupted = original.deepCopy(codec)
    corrupted.setCell(0, 0, bytes([66]) * size if tree == "default" else bytes([1]) * ns + bytes([66]) * (size - ns))
    rr, cr = corrupted.RowRoots(), corrupted.ColRoots()
    proof = corrupted.BadEncodingProof(R.Row, 0)
    v = proof.Validate(rr, cr, codec, tree_fn)
    assert (v.verdict, v.reason, v.present) == (R.FRAUD_VALID, R.BYZ_ENCODING, 4)
    half = R.BadEncodingProof(R.Row, 0, [None, None] + proof.shares[2:], [None, None] + proof.proofs[2:])
    v = half.Validate(rr, cr, codec, tree_fn)  # rebuilt from the parity half: another row
    assert (v.verdict, v.reason, v.present) == (R.FRAUD_VALID, R.BYZ_ROOT, 2)
    v = corrupted.BadEncodingProof(R.Row, 1).Validate(rr, cr, codec, tree_fn)
    assert (v.verdict, v.reason) == (R.FRAUD_CONSISTENT, 0)
    forged = R.BadEncodingProof(R.Row, 1, [proof.shares[0]] + corrupted.Row(1)[1:], corrupted.BadEncodingProof(R.Row, 1).proofs)
    v = forged.Validate(rr, cr, codec, tree_fn)
    assert (v.verdict, v.reason, v.pos) == (R.FRAUD_SHARE, PS.ROOT, 0)
