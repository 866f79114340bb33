"""GPU: the device pipelines at share sizes other than 64 bytes -- share proofs and their
verifiers, namespace proofs, range proofs, commitments, scatter and gather, both device
Repairs and fraud proofs at 128, 512 and 1088 bytes (tests/share_sizes.py says what each
size reaches), and the two compare kernels past their first grid-stride trip.

Every family makes the assertions of its 64-byte test against the same model -- the hashlib
helpers, the oracle crossword, the schedule models -- status for status and byte for byte,
on k = 8 unless a test names another width; tests/test_share_sizes_cpu.py runs the same
cases through the library's host restatements.

The smallest shapes: k = 8 (W = 16) everywhere; W = 67 and k = 40 for ranges longer than a
wave; k = 65, S = 512 for Repair's encoding compare (2.06 trips); 16 MiB + 4 KiB + 16 bytes
for rsm_dev_equal (one trip, one block, one word); k = 129, S = 512 for the GF(2^16) work
areas."""
import ctypes

import numpy as np
import pytest

import commit_calls as CK
import commitments as CM
import data_root as DR
import device_calls as DC
import fraud_proofs as F
import nmt_layouts as NL
import ns_proofs as H
import ns_verify_calls as NV
import oracle
import proof_status as P
import range_calls as RG
import range_proofs as M
import repair_cases as RC
import repair_checked as C
import repair_dev_calls as D
import repair_patterns as RP
import rsmt2d_amd as R
import share_sizes as SS
import stream_pipes as PIPES
import test_gpu_fraud_proofs as TF
import test_gpu_repair_dev as TR
from device_calls import Guarded
from test_gpu_scatter_dev import round_trip

pytestmark = pytest.mark.gpu

K, NS = SS.K, SS.NS
sizes = pytest.mark.parametrize("S", SS.SIZES)


def _free(bufs):
    for b in bufs:
        b.free()


# ---- share proofs and their verifiers ------------------------------------------------------
def chain_statuses(lib, items, W, S, p, stream=None):
    """One rsm_proofs_verify_data_root_dev over data_root.ChainItems, each with its root
    record and its data root in a slot of its own; inputs between guard bands."""
    ctx, n = R.device_context(0), len(items)
    blobs = [b"".join(it.share for it in items), b"".join(it.record for it in items),
             b"".join(it.root_record for it in items), b"".join(it.data_root for it in items)]
    gs = [Guarded(len(b), skew, 90 + i) for i, (b, skew) in enumerate(zip(blobs, (0, 2, 6, 3)))]
    st = Guarded(n * 4, 4, 95)
    try:
        for g, b in zip(gs, blobs):
            NV.fill(g, b)
        arr = (R.Sample * n)(*[R.Sample(i, *it.sample[1:]) for i, it in enumerate(items)])
        R._check(lib.rsm_proofs_verify_data_root_dev(ctx, gs[0].ptr, gs[1].ptr, gs[2].ptr, gs[3].ptr, W, S, n,
                                                     ctypes.byref(p) if p is not None else None, arr, n, st.ptr, stream))
        R._check(lib.rsm_sync(ctx))
        for g in gs:
            assert np.array_equal(g.result(), g.untouched(0, g.n)), "the verifier wrote into an input"
        return [int(x) for x in st.result().view(np.uint32)]
    finally:
        _free(gs + [st])


@pytest.mark.parametrize("tree", SS.TREES)
@sizes
def test_share_proofs(lib, S, tree):
    """rsm_proof_nodes_dev -> rsm_proofs_dev over every sample of two squares: roots of the
    root kernels and of the model, records of the host restatement that verify against the
    oracle root, shares equal to the cells."""
    batch, sq, ch = SS.proof_squares(S, tree)
    samples = DC.all_samples(sq.W, sq.count)
    dev = DC.Dev(lib, batch, sq.p, samples)
    assert dev.roots == dev.roots_ref == b"".join(b"".join(r) for r in ch.roots)
    assert not dev.status.any() and not dev.status_ref.any()
    DC.check_samples(lib, dev, batch, sq.p, samples)
    for i in range(0, len(samples), 37):  # and the model's own records
        assert dev.record(i) == sq.record(samples[i]), samples[i]


@pytest.mark.parametrize("tree", SS.TREES)
@sizes
def test_share_proof_verifiers(lib, S, tree):
    """rsm_proofs_verify_dev and rsm_proofs_verify_data_root_dev on honest proofs and every
    hostile variant of proof_status / data_root, status for status."""
    _, sq, _ = SS.proof_squares(S, tree)
    items, want = SS.verify_items(S, tree)
    P.assert_covers(want, sq.p)
    got = DC.device_statuses(items, sq.W, S, sq.p, DC.committed_roots(sq))
    bad = [(it.label, it.sample, g, w) for it, g, w in zip(items, got, want) if g != w]
    assert not bad, (len(bad), bad[:8])
    for it, w in ((items[0], want[0]), (items[1], want[1])):  # n = 1
        assert DC.device_statuses([it], sq.W, S, sq.p, DC.committed_roots(sq)) == [w]
    items, want = SS.chain_items(S, tree)
    assert {DR.OK, DR.MALFORMED, DR.ROOT} | ({DR.ORDER} if sq.p is not None else set()) == set(want)
    got = chain_statuses(lib, items, sq.W, S, sq.p)
    bad = [(it.label, it.sample, g, w) for it, g, w in zip(items, got, want) if g != w]
    assert not bad, (len(bad), bad[:8])


# ---- namespace proofs ---------------------------------------------------------------------
NS_LAYOUTS = ("runs", "carry", "max_tail")


def ns_prove_then_verify(lib, batch, k, ns, ig, S, queries, nids):
    return PIPES.run(PIPES.ns_pipe(lib, None, batch, k, ns, ig, S, queries, nids))[0]


@sizes
def test_namespace_proofs(lib, S):
    """The prover's records, offsets and shares are the model's and the host prover's, and
    verify where they lie; of every fifth query the share-bit, leaf-digest and narrowed
    variants owe what the hashlib helper and the host verifier say."""
    k, ig = K, True
    W, p = 2 * k, R.NmtParams(NS, 1, k)
    batch = np.stack([NL.square(k, NS, S, name, 7) for name in NS_LAYOUTS])
    queries, nids, records, shares = DC.expect(lib, batch, k, NS, ig, H.vectors(k))
    rec, offs, sh, st = ns_prove_then_verify(lib, batch, k, NS, ig, S, queries, nids)
    assert offs == list(np.cumsum([0] + [len(x) for x in shares]))
    assert rec == b"".join(records)
    assert sh == b"".join(b"".join(x) for x in shares)
    assert st == [H.OK] * len(queries)
    pairs = []
    for i in range(0, len(queries), 5):
        s, axis, index = queries[i]
        leaves = H.vector_shares(batch[s], axis, index)
        it = NV.Item("device prover", queries[i], nids[i], records[i], shares[i], H.Tree(leaves, index, k, NS, ig).root)
        pairs += NV.with_variants(lib, p, it, leaves, W, S)
    got = NV.compare(lib, [it for it, _ in pairs], [m for _, m in pairs], W, p, batch.shape[0], S=S)
    assert set(got) == {H.OK, H.ROOT, H.INCOMPLETE}


@sizes
def test_namespace_range_longer_than_a_wave_at_an_odd_width(lib, S):
    """W = 67, every leaf with a namespace of its own kind (square_size = W): the namespace
    of leaves [1, 67) is a range of 66 shares, hashed in two passes of the wave."""
    W = SS.ODD_W
    p = R.NmtParams(NS, 1, W)
    leaves = SS.sorted_vector(W, NS, S, SS.ODD_BOUNDS, 5)
    pairs, ranges = [], set()
    for v in (1, 2):
        it = NV.proved(lib, p, "odd width", (0, 1, 0), leaves, bytes(NS - 1) + bytes([v]))
        ranges.add(tuple(int.from_bytes(it.record[4 * i:4 * i + 4], "little") for i in (1, 2)))
        pairs += NV.with_variants(lib, p, it, leaves, W, S)
    assert ranges == {(0, 1), (1, W)}
    got = NV.compare(lib, [it for it, _ in pairs], [m for _, m in pairs], W, p, 1, S=S)
    assert set(got) == {H.OK, H.ROOT, H.INCOMPLETE}


# ---- range proofs -------------------------------------------------------------------------
def check_range_pipeline(lib, k, ns, S, ranges):
    """The range pipeline of tests/stream_pipes.py over rows and columns 0, k - 1, k and W - 1
    of one square: every record, offset, share, root, data root, root record and status word
    of the model."""
    W = 2 * k
    sq, rows, cols, drt = SS.range_world(k, ns, S)
    trees = {0: rows, 1: cols}
    queries = [(0, a, i, s, e) for a in (0, 1) for i in (0, k - 1, k, W - 1) for s, e in ranges]
    (got,) = PIPES.run(PIPES.range_pipe(lib, None, k, ns, S, sq[None], queries))
    lens = [e - s for _, _, _, s, e in queries]
    assert got[0] == b"".join(M.prove(trees[a][i], ns, s, e) for _, a, i, s, e in queries)
    assert got[1] == list(np.cumsum([0] + lens))
    assert got[2] == b"".join(b"".join(H.vector_shares(sq, a, i)[s:e]) for _, a, i, s, e in queries)
    assert got[3] == b"".join(t.root for t in rows + cols)
    assert got[4] == drt.root()
    assert got[5] == b"".join(DR.record_of(drt, W, a, i) for _, a, i, _, _ in queries)
    assert got[6] == [M.OK] * len(queries) and got[7] == [M.OK] * len(queries)


@pytest.mark.parametrize("ns", [0, NS])
@sizes
def test_range_proofs_on_device_buffers(lib, S, ns):
    check_range_pipeline(lib, K, ns, S, SS.RANGES_K8)


@pytest.mark.parametrize("ns", [0, NS])
@sizes
def test_range_longer_than_a_wave(lib, S, ns):
    """k = 40: ranges of 72 and 80 leaves, whose shares a wave hashes in two passes."""
    assert max(e - s for s, e in SS.RANGES_LONG) > 64
    check_range_pipeline(lib, SS.LONG_RANGE_K, ns, S, SS.RANGES_LONG)


@pytest.mark.parametrize("ns", [0, NS])
@sizes
def test_range_verifiers_on_the_hostile_set(lib, S, ns):
    """Device == host == model over range_proofs' hostile variants, under the root table and
    chained to the data root."""
    k, W, p = K, 2 * K, RG.params(K, ns)
    cases, rrecs, musts, dr = SS.range_cases(ns, S)
    M.named_musts(cases)
    got = RG.device_statuses(lib, p, W, S, cases)
    for c, g in zip(cases, got):
        assert g == c.must, (c.name, c.index, c.start, c.end, g, c.must)
        assert RG.host_status(lib, p, W, c, S) == c.must, c.name
    assert set(got) == ({M.OK, M.MALFORMED, M.ORDER, M.ROOT} if ns else {M.OK, M.MALFORMED, M.ROOT})
    keep = [i for i, m in enumerate(musts) if m is not None]
    got = RG.device_statuses(lib, p, W, S, [cases[i] for i in keep],
                             chained=(b"".join(rrecs[i] for i in keep), dr * len(keep)))
    assert got == [musts[i] for i in keep]
    assert set(got) == ({M.OK, M.MALFORMED, M.ORDER, M.ROOT} if ns else {M.OK, M.MALFORMED, M.ROOT})


# ---- commitments --------------------------------------------------------------------------
@pytest.mark.parametrize("t", SS.COMMIT_THRESHOLDS)
@sizes
def test_commitments(lib, S, t):
    """Every aligned blob of one k = 8 square through the node store, and the same shares
    copied out of the ODS through the shares path: subtree roots and commitments of the
    model, byte for byte."""
    sq = SS.commitment_square(S)
    blobs, want_roots, want = SS.commitment_wants(S, t)
    refs = [(0, s, n) for s, n in blobs]
    store = CK.Store(lib, sq[None], R.NmtParams(NS, 1, K))
    try:
        assert not store.tree_status.any()
        rc, com, st, roots = store.commitments(refs, t)
        assert rc == 0 and st == [0] * len(blobs)
        assert com == want
        assert roots == want_roots
        rc2, com2, st2, _ = store.commitments(refs, t, want_roots=False)
        assert (rc2, com2, st2) == (0, want, st)
    finally:
        store.free()
    rc, com3, st3 = CK.shares_path(lib, R.NmtParams(NS, 1, 1), S, [CM.ods_shares(sq, K, s, n) for s, n in blobs], t, lead=1)
    assert rc == 0 and st3 == [0] * len(blobs)
    assert com3 == want


# ---- scatter and gather -------------------------------------------------------------------
@sizes
def test_scatter_round_trip(lib, S):
    """tests/test_gpu_scatter_dev.py's flow -- prove, verify, scatter with duplicate,
    corrupted and occupied samples, repair -- with every sixth record corrupted."""
    round_trip(lib, K, 6, S)


@sizes
def test_vectors_gather_between_guard_bands(lib, S):
    """Rows and columns, first and last index, of three squares against numpy slicing; the
    outputs lie between guard bands and the squares come back as they were."""
    k, count = K, 3
    W = 2 * k
    rng = np.random.default_rng(0x6A7 + S)
    batch = rng.integers(0, 256, (count, W, W, S), dtype=np.uint8)
    pres = rng.integers(0, 3, (count, W, W), dtype=np.uint8) * 7
    refs = [(0, 0, 0), (0, 1, 0), (2, 0, W - 1), (2, 1, W - 1), (1, 1, 5), (1, 0, 5), (2, 1, 0)]
    n = len(refs)
    ctx = R.device_context(0)
    d_eds, d_pres = R.DeviceBuffer(batch.nbytes), R.DeviceBuffer(pres.nbytes)
    d_sh, d_pr = Guarded(n * W * S, 0, 81), Guarded(n * W, 5, 82)
    try:
        d_eds.upload(batch.reshape(-1))
        d_pres.upload(pres.reshape(-1))
        arr = (R.RootRef * n)(*[R.RootRef(*r) for r in refs])
        R._check(lib.rsm_vectors_gather_dev(ctx, d_eds.ptr, d_pres.ptr, k, S, count, arr, n, d_sh.ptr, d_pr.ptr, None))
        R._check(lib.rsm_sync(ctx))
        shares = d_sh.result().reshape(n, W, S)
        present = d_pr.result().reshape(n, W)
        assert np.array_equal(d_eds.download(), batch.reshape(-1)) and np.array_equal(d_pres.download(), pres.reshape(-1))
    finally:
        _free([d_eds, d_pres, d_sh, d_pr])
    for j, (s, axis, i) in enumerate(refs):
        assert np.array_equal(shares[j], batch[s, i] if axis == 0 else batch[s, :, i]), refs[j]
        assert np.array_equal(present[j], pres[s, i] if axis == 0 else pres[s, :, i]), refs[j]


# ---- Repair on device squares -------------------------------------------------------------
def run_family(lib, family, k, S, tree="default"):
    valid, rr, cr = RP.square_for(family, k, S, tree)
    pres = RP.presence(family, k)
    nmt = D.nmt_params(k, RP.NS) if tree == "nmt" else None
    (r,) = D.repair(lib, [D.given(valid, pres)], [pres], [(rr, cr)], k, S, nmt)
    return r, valid


@pytest.mark.parametrize("family", ["avalanche", "core"])
@sizes
def test_repair_families(lib, S, family):
    """avalanche (six sweeps and more) repairs to the square bit for bit with the peeling
    model's counters; core is stuck at the model's closure."""
    r, valid = run_family(lib, family, K, S)
    (TR._check_repaired if family in RP.REPAIRABLE else TR._check_stuck)(r, valid, family, K)


def _rc(name, k, S, tree="default"):
    flat, rr, cr, _ = RC.case(name, k, S, tree)
    sq, pres = D.case_square(flat, 2 * k, S)
    return sq, pres, (rr, cr)


@sizes
def test_repair_mixed_batch(lib, S):
    """tests/test_gpu_repair_dev.py's mixed batch: OK, STUCK, ROOTS and ENCODING squares in
    one call, each result what the square gives alone."""
    k = K
    items = []
    for family in ("avalanche", "core"):
        valid, rr, cr = RP.square_for(family, k, S)
        pres = RP.presence(family, k)
        items.append((D.given(valid, pres), pres, (rr, cr)))
    items.append(_rc("C_col_root_last", k, S))
    items.append(_rc("A_row_last", k, S))
    squares, presences, roots = (list(x) for x in zip(*items))
    batch = D.repair(lib, squares, presences, roots, k, S)
    assert [r.status for r in batch] == [R.REPAIR_OK, R.REPAIR_STUCK, R.REPAIR_ROOTS, R.REPAIR_ENCODING]
    TR._check_repaired(batch[0], RP.square_for("avalanche", k, S)[0], "avalanche", k)
    TR._check_stuck(batch[1], RP.square_for("core", k, S)[0], "core", k)
    assert np.array_equal(batch[2].square, RC.case("C_col_root_last", k, S)[3]["valid"])
    assert np.array_equal(batch[3].square, RC.case("A_row_last", k, S)[3]["full"])
    for i, it in enumerate(items):
        (alone,) = D.repair(lib, [it[0]], [it[1]], [it[2]], k, S)
        assert alone.stats() == batch[i].stats(), i
        assert np.array_equal(alone.presence, batch[i].presence), i
        m = alone.presence != 0
        assert np.array_equal(alone.square[m], batch[i].square[m]), i


@sizes
def test_repair_agrees_with_host_repair(lib, S):
    """rsm_eds_repair (the host square's Repair, which needs a device context) on
    avalanche's cells: the same square, sweeps and vectors."""
    k, family = K, "avalanche"
    r, valid = run_family(lib, family, k, S)
    _, rr, cr = RP.square_for(family, k, S)
    eds = D.import_host(lib, valid, RP.presence(family, k), R.NewDefaultTree)
    eds.Repair(list(rr), list(cr))
    got, pres = D.flattened_host(lib, eds, 2 * k, S)
    st = eds.repair_stats()
    assert pres.all() and r.status == R.REPAIR_OK
    assert np.array_equal(got, r.square)
    assert (st.sweeps, st.decoded_vectors) == (r.sweeps, r.vectors)


@pytest.mark.parametrize("tree", SS.TREES)
@sizes
def test_checked_repair_late_culprit(lib, S, tree):
    """One altered given cell of the avalanche map, named in round >= 3: repair_checked's
    model, the validity predicate, and no cell present that was not given or checked."""
    k = K
    sq, pres, rr, cr, want = C.late_culprit(k, tree, S=S)
    assert want.round >= 3 and sq.shape[2] == S
    nmt = D.nmt_params(k, RP.NS) if tree == "nmt" else None
    (got,) = C.repair_checked(lib, [sq], [pres], [(rr, cr)], k, S, nmt)
    C.assert_equals_model(got, want)
    assert got.status == R.REPAIR_BYZANTINE
    assert C.is_byzantine(got.shares, got.axis, got.index, (rr, cr)[got.axis][got.index], k, tree)
    allowed = np.array(pres, bool)
    for a, i in want.passed:
        if a == C.Row:
            allowed[i, :] = True
        else:
            allowed[:, i] = True
    assert not ((got.presence != 0) & ~allowed).any()


# ---- fraud proofs -------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [0, NS])
@sizes
def test_fraud_proofs_mixed_batch(lib, S, ns):
    """tests/test_gpu_fraud_proofs.py's mixed batch of 2k + 3 proofs over three squares
    (VALID for every reason, CONSISTENT, SHARE, TOOFEW; both axes) against the model."""
    TF.test_mixed_batch_equals_the_model(lib, K, S, ns)


# ---- GF(2^16) at Celestia's share size: work areas of W * W * S = 34 MB a square -----------
GF16_K, GF16_S = 129, 512


def test_gf16_repair_at_512(lib):
    r, valid = run_family(lib, "chain3", GF16_K, GF16_S)
    TR._check_repaired(r, valid, "chain3", GF16_K)


def test_gf16_fraud_proofs_at_512(lib):
    """tests/test_gpu_fraud_proofs.py's four GF(2^16) proofs, one per verdict."""
    k, S = GF16_K, GF16_S
    sq, table = TF.world(k, S, 0)
    W = 2 * k
    proofs = [F.honest(sq, (1, TF.Col, 0), None, "ENCODING"),
              F.honest(sq, (1, TF.Col, k), F.pattern("second", k), "ROOT"),
              F.honest(sq, (0, TF.Row, k - 1), F.pattern("mixed", k), "CONSISTENT"),
              TF._flip(F.honest(sq, (0, TF.Col, W - 1), F.pattern("first", k)), 5, 0, "SHARE")]
    got = F.check(lib, proofs, table, k, S)
    assert [g[:2] for g in got] == [(F.VALID, F.ENCODING), (F.VALID, F.ROOT), (F.CONSISTENT, 0), (F.SHARE, P.ROOT)]
    assert got[3][2] == 5


# ---- the long compares --------------------------------------------------------------------
LONG_CASES = ("A_row_0", "A_row_k", "A_row_last", "C_row_root_0", "C_col_root_last", "D_control")


def test_repair_encoding_compare_past_its_first_trip(lib):
    """k = 65, S = 512: repair_compare_squares_kernel needs 2.06 trips over the square.  The
    rebuilt A_row_k square differs from its re-extension in the second trip only and
    A_row_last's in the ragged third only (A_row_0's in both;
    tests/test_share_sizes_cpu.py computes where): ENCODING.  C_*: ROOTS, D_control: OK --
    the compare finds nothing in any trip."""
    k, S = SS.LONG_REPAIR
    items = [_rc(name, k, S) for name in LONG_CASES]
    squares, presences, roots = (list(x) for x in zip(*items))
    batch = D.repair(lib, squares, presences, roots, k, S)
    for name, r in zip(LONG_CASES, batch):
        assert r.missing == 0 and r.presence.all() and r.sweeps >= 1, name
        assert r.status in D.RC_STATUS[name], (name, r.stats())
        note = RC.case(name, k, S)[3]
        assert np.array_equal(r.square, note["full"] if name.startswith("A_") else note["valid"]), name


def test_repair_encoding_compare_one_word_per_trip(lib):
    """Complete squares at k = 65, S = 512 with one byte of one parity cell flipped
    (share_sizes.parity_flips): exactly one 16-byte word differs from the re-extension -- in
    the first cell of the first trip, at its end, at the start of the second trip and in the
    last word of the ragged third.  Each is ENCODING without a sweep; the untouched square
    is OK."""
    k, S = SS.LONG_REPAIR
    W = 2 * k
    valid, rr, cr = RP.square(k, S)
    flips = SS.parity_flips(k, S)
    squares = [np.array(valid) for _ in range(len(flips) + 1)]
    for sq, (r, c, b) in zip(squares, flips):
        sq[r, c, b] ^= 1
    pres = np.ones((W, W), bool)
    batch = D.repair(lib, squares, [pres] * len(squares), [(rr, cr)] * len(squares), k, S)
    assert [r.stats() for r in batch] == [(R.REPAIR_ENCODING, 0, 0, 0)] * len(flips) + [(R.REPAIR_OK, 0, 0, 0)]
    for sq, r in zip(squares, batch):
        assert np.array_equal(r.square, sq)


def _flip_word(lib, ctx, buf, word):
    """XORs the last byte of 16-byte word `word` of a device buffer, by a 16-byte copy each way."""
    w = np.empty(16, np.uint8)
    R._check(lib.rsm_memcpy(ctx, w.ctypes.data, buf.ptr + 16 * word, 16, 1))
    w[15] ^= 0x80
    R._check(lib.rsm_memcpy(ctx, buf.ptr + 16 * word, w.ctypes.data, 16, 0))


def test_dev_equal_and_fill_random(lib):
    """rsm_dev_fill_random is oracle.splitmix64_bytes (a prefix and the tail of 16 MiB + 4 KiB
    + 16 bytes: the fill strides its grid too); two buffers of one seed are equal to
    rsm_dev_equal, and unequal with one bit flipped in the first word, in the last word of
    compare_kernel's first trip, in the first word of its second trip and in the last
    word; bytes = 16; the documented RSM_EINVAL."""
    ctx, n = R.device_context(0), SS.DEV_EQUAL_BYTES
    a, b = R.DeviceBuffer(n), R.DeviceBuffer(n)
    eq = ctypes.c_int(-1)

    def equal(nbytes=n, pa=None, pb=None, stream=None):
        R._check(lib.rsm_dev_equal(ctx, a.ptr if pa is None else pa, b.ptr if pb is None else pb, nbytes, stream, ctypes.byref(eq)))
        return eq.value

    try:
        a.fill_random(0xE9A1)
        b.fill_random(0xE9A1)
        R._check(lib.rsm_sync(ctx))
        want = oracle.splitmix64_bytes(n, seed=0xE9A1)
        assert np.array_equal(a.download(8192), want[:8192])
        assert np.array_equal(b.download(8192 + 16, n - 8192 - 16), want[n - 8192 - 16:])
        assert equal() == 1
        for word in SS.DEV_EQUAL_WORDS:
            _flip_word(lib, ctx, b, word)
            assert equal() == 0, word
            _flip_word(lib, ctx, b, word)
            assert equal() == 1, word
        # one word, and one word that differs
        last = 16 * SS.DEV_EQUAL_WORDS[-1]
        assert equal(16) == 1 and equal(16, a.ptr + last, b.ptr + last) == 1
        assert equal(16, a.ptr, b.ptr + 16) == 0
        _flip_word(lib, ctx, a, 0)
        assert equal(16) == 0 and equal(16, a.ptr + 16, b.ptr + 16) == 1
        for kw in (dict(nbytes=24), dict(nbytes=n - 8), dict(pa=a.ptr + 8), dict(pb=b.ptr + 4), dict(pa=a.ptr + 1, pb=b.ptr + 1)):
            eq.value = -1
            assert lib.rsm_dev_equal(ctx, kw.get("pa", a.ptr), kw.get("pb", b.ptr), kw.get("nbytes", 64), None,
                                     ctypes.byref(eq)) == R.RSM_EINVAL, kw
        assert lib.rsm_dev_equal(ctx, None, b.ptr, 64, None, ctypes.byref(eq)) == R.RSM_EINVAL
        assert lib.rsm_dev_equal(ctx, a.ptr, b.ptr, 64, None, None) == R.RSM_EINVAL
    finally:
        _free([a, b])
