"""TEST INFRASTRUCTURE ONLY -- the model of rsm_fraud_proofs_verify_dev, the builders of
bad-encoding fraud proofs and the one place that runs the call between guard bands (shared
by tests/test_fraud_proofs_cpu.py and tests/test_gpu_fraud_proofs.py).  The model calls
nothing of the library under test: share proofs are judged by proof_status.expected_status,
vectors decoded and encoded with the oracle codec, trees hashed by proof_status.tree_levels
(hashlib / oracle/nmt.py).  Importing this module touches no GPU; every function that does
takes `lib`.

A proof accuses vector (square, axis, index) of a batch of squares: 2k slots, each a share,
a presence flag and the record of the share's proof in the ORTHOGONAL tree (axis ^ 1, j) at
position `index`.  The rules (include/rsmt2d_hip.h), the first that applies:
  1  fewer than k slots present                               -> TOOFEW
  2  a present slot fails proof_status.expected_status        -> SHARE, lowest slot, its status
  3  the vector rebuilt from the present slots fails its tree,
     its committed root or its own encoding, in that order    -> VALID, TREE / ROOT / ENCODING
  4  otherwise                                                 -> CONSISTENT
"""
import ctypes

import numpy as np

import oracle
import proof_status as PS
import proof_verify as V
import repair_dev_calls as D
import rsmt2d_amd as R
from device_calls import Guarded
from oracle import nmt

Row, Col = 0, 1
VALID, TOOFEW, SHARE, CONSISTENT = 0, 1, 2, 3
ROOT, ENCODING, TREE = 1, 2, 3


# ---- the model -----------------------------------------------------------------------
def vector_reason(shares, index, committed, k, p):
    """The check of one complete vector (2k byte strings) of tree `p` (None: DefaultTree):
    0 or TREE / ROOT / ENCODING.  The generalisation of repair_checked.vector_reason to any
    namespace size (tests/test_fraud_proofs_cpu.py pins the two to each other)."""
    t = PS.tree_of(p)
    if t.ns:
        names = [V.nmt_leaf(s, pos, index, t.k, t.ns)[:t.ns] for pos, s in enumerate(shares)]
        if any(names[i + 1] < names[i] for i in range(len(names) - 1)):
            return TREE  # push order
    try:
        root = PS.tree_levels(shares, index, p)[-1][0]
    except nmt.NmtError:
        return TREE
    if root != committed:
        return ROOT
    return 0 if oracle.encode(list(shares[:k])) == list(shares[k:]) else ENCODING


def model(shares, present, records, table, ref, k, p):
    """shares: 2k byte strings (an absent slot's is never looked at), present: 2k flags,
    records: 2k proof records, table: [count][2][W][node_len] uint8 committed roots, ref:
    (square, axis, index).  ((verdict, reason, pos, present count), the rebuilt vector or None)."""
    W = 2 * k
    q, axis, index = ref
    on = [bool(x) for x in present]
    have = sum(on)
    if have < k:
        return (TOOFEW, 0, 0, have), None
    for j in range(W):
        if on[j]:
            st = PS.expected_status(table[q, axis ^ 1, j].tobytes(), shares[j], records[j], index, j, W, p)
            if st:
                return (SHARE, st, j, have), None
    full = list(shares) if have == W else oracle.decode([s if on[j] else None for j, s in enumerate(shares)])
    reason = vector_reason(full, index, table[q, axis, index].tobytes(), k, p)
    return ((VALID if reason else CONSISTENT), reason, 0, have), full


# ---- proofs --------------------------------------------------------------------------
class Proof:
    """One fraud proof: ref, shares [W][S] uint8, present [W] uint8, records (list of bytes)."""

    def __init__(self, ref, shares, present, records, label=""):
        self.ref, self.label = tuple(ref), label
        self.shares = np.array(shares, np.uint8)
        self.present = np.array(present, np.uint8)
        self.records = [bytes(r) for r in records]

    def copy(self, label=None):
        return Proof(self.ref, self.shares, self.present, self.records, self.label if label is None else label)

    def expect(self, table, k, p):
        return model([s.tobytes() for s in self.shares], self.present, self.records, table, self.ref, k, p)


def honest(sq, ref, present, label=""):
    """The proof a holder of the committed squares `sq` (proof_status.Squares) gives for
    vector `ref` with the slots of `present` (flags, or None for all): the cells and their
    records in the orthogonal trees.  Absent slots keep their true share and record here;
    `run` overwrites them with FILL."""
    q, axis, index = ref
    W = sq.W
    samples = [(q, axis ^ 1, j, index) for j in range(W)]
    shares = np.stack([np.frombuffer(sq.share(s), np.uint8) for s in samples])
    flags = np.ones(W, np.uint8) if present is None else np.array(present, np.uint8)
    return Proof(ref, shares, flags, [sq.record(s) for s in samples], label)


def table_of(sq, broken=()):
    """[count][2][W][node_len] committed roots of a proof_status.Squares; the trees of
    `broken` ((square, axis, index): they fail, no root exists) get zeros."""
    nl = PS.node_len(sq.p)
    t = np.zeros((sq.count, 2, sq.W, nl), np.uint8)
    for q in range(sq.count):
        for a in (0, 1):
            for i in range(sq.W):
                if (q, a, i) not in broken:
                    t[q, a, i] = np.frombuffer(sq.root(q, a, i), np.uint8)
    return t


def pattern(kind, k, seed=0):
    """Presence flags of 2k slots: first / second (half only), mixed (k of them, seeded),
    all, short (k - 1, seeded), none."""
    W = 2 * k
    rng = np.random.default_rng([0xF4A0D, k, seed])
    f = np.zeros(W, np.uint8)
    if kind == "first":
        f[:k] = 1
    elif kind == "second":
        f[k:] = 1
    elif kind == "mixed":
        f[rng.choice(W, size=k, replace=False)] = 1
    elif kind == "all":
        f[:] = 1
    elif kind == "short":
        f[rng.choice(W, size=k - 1, replace=False)] = 1
    else:
        assert kind == "none"
    return f


def unordered_q0(k, S, ns, seed):
    """A valid extended square whose original quadrant is sorted by namespace except that
    cell (0, 0) carries the namespace of cell (1, 0): every column stays in order, row 0
    does not -- its NMT fails, nothing else does."""
    ods = np.array(V.sorted_q0_square(k, S, ns, seed)[:k, :k])
    ods[0, 0, :ns] = ods[1, 0, :ns]
    assert ods[0, 0, :ns].tobytes() > ods[0, 1, :ns].tobytes()
    return oracle.extend_square(np.ascontiguousarray(ods), nthreads=8)


# ---- the device call -----------------------------------------------------------------
def run(lib, proofs, table, k, S, p=None, fill=D.FILL, record_fill=0x3C, stream=None):
    """One rsm_fraud_proofs_verify_dev over `proofs` against `table`.  d_shares, d_present,
    d_records and d_work lie between guard bands; absent slots hold `fill` shares and
    `record_fill` records.  The bands, d_present, d_records and every present slot must come
    back byte-identical.  Returns ([(verdict, reason, pos, present)], shares [n][W][S] after)."""
    ctx = R.device_context(0)
    n, W = len(proofs), 2 * k
    pp = ctypes.byref(p) if p is not None else None
    rb = int(lib.rsm_proof_record_bytes(W, pp))
    sh = np.full((n, W, S), fill, np.uint8)
    pr = np.zeros((n, W), np.uint8)
    rec = np.full((n, W, rb), record_fill, np.uint8)
    for i, f in enumerate(proofs):
        on = f.present != 0
        pr[i] = f.present
        sh[i][on] = f.shares[on]
        for j in np.flatnonzero(on):
            assert len(f.records[j]) == rb
            rec[i, j] = np.frombuffer(f.records[j], np.uint8)
    nwork = int(lib.rsm_fraud_work_bytes(k, S, n, pp))
    assert nwork > 0
    d_sh, d_pr, d_rec, d_work = Guarded(sh.nbytes, 0, 31), Guarded(pr.nbytes, 5, 32), Guarded(rec.nbytes, 3, 33), \
        Guarded(nwork, 0, 34)
    d_roots = R.DeviceBuffer(table.nbytes)
    try:
        d_sh.buf.upload(sh.reshape(-1), d_sh.front)
        d_pr.buf.upload(pr.reshape(-1), d_pr.front)
        d_rec.buf.upload(rec.reshape(-1), d_rec.front)
        d_roots.upload(np.ascontiguousarray(table).reshape(-1))
        refs = (R.RootRef * n)(*[R.RootRef(*f.ref) for f in proofs])
        out = (R.FraudVerdict * n)()
        R._check(lib.rsm_fraud_proofs_verify_dev(ctx, d_sh.ptr, d_pr.ptr, d_rec.ptr, d_roots.ptr, k, S, table.shape[0], pp,
                                                 refs, n, d_work.ptr, out, stream))
        got = d_sh.result().reshape(n, W, S).copy()
        assert np.array_equal(d_pr.result().reshape(n, W), pr), "d_present was written"
        assert np.array_equal(d_rec.result().reshape(n, W, rb), rec), "d_records was written"
        d_work.result()
        assert np.array_equal(d_roots.download(), np.ascontiguousarray(table).reshape(-1)), "d_roots was written"
    finally:
        for b in (d_sh, d_pr, d_rec, d_work, d_roots):
            b.free()
    on = pr != 0
    assert np.array_equal(got[on], sh[on]), "a present slot was written"
    return [(v.verdict, v.reason, v.pos, v.present) for v in out], got


def check(lib, proofs, table, k, S, p=None, stream=None):
    """The device against the model, record for record; the rebuilt missing slots against
    the model's vector for VALID and CONSISTENT proofs.  Returns the records."""
    got, after = run(lib, proofs, table, k, S, p, stream=stream)
    for i, f in enumerate(proofs):
        want, full = f.expect(table, k, p)
        assert got[i] == want, (i, f.label, f.ref, got[i], want)
        if full is not None:
            assert [x.tobytes() for x in after[i]] == list(full), (i, f.label, "rebuilt vector")
    return got
