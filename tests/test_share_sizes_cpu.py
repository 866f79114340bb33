"""CPU: the cases of tests/test_gpu_share_sizes.py through the library's host restatements
(rsm_*_tree_prove / _verify, rsm_sample_verify_data_root, rsm_data_root*, rsm_nmt_namespace_*,
rsm_*_tree_range_prove / _verify, rsm_blob_commitment, rsm_square_commitment) and the oracle
crossword, at the same share sizes against the same models -- so the models and the case
builders are themselves held at S != 64 on a machine without a GPU -- and the arithmetic of
tests/share_sizes.py (which trip of Repair's encoding compare each long case lands in).

GPU cases without a twin here, because the library has no host form of the call:
  * the gathers and copies: rsm_proofs_dev's share gather, rsm_samples_scatter_dev,
    rsm_vectors_gather_dev, rsm_dev_equal, rsm_dev_fill_random;
  * Repair: rsm_repair_squares_dev and rsm_repair_squares_checked_dev are device calls, and
    the host square's rsm_eds_repair needs a device context too (its comparison is a GPU
    test).  Here the erasure families, the verification cases and the late culprit are held
    to the oracle crossword and to the schedule models at each size;
  * rsm_fraud_proofs_verify_dev (the model's verdicts are asserted here, no library call);
  * range proofs chained to the data root: only the device has that verifier;
  * the k = 129 shapes (the models take seconds; the GPU tests build them once).
"""
import ctypes

import numpy as np
import pytest

import commitments as CM
import device_calls as DC
import fraud_proofs as F
import nmt_layouts as NL
import ns_proofs as H
import ns_verify_calls as NV
import proof_status as P
import range_calls as RG
import range_proofs as M
import repair_cases as RC
import repair_checked as C
import repair_dev_calls as D
import repair_patterns as RP
import rsmt2d_amd as R
import share_sizes as SS
import test_gpu_fraud_proofs as TF
from test_commitments_cpu import blob_commitment, square_commitment
from test_data_root_cpu import host_data_root, host_root_record
from test_verify_cpu import host_status

K, NS = SS.K, SS.NS
sizes = pytest.mark.parametrize("S", SS.SIZES)


# ---- tests/share_sizes.py itself -----------------------------------------------------------
def test_classes_and_long_shapes():
    assert SS.SIZES == (128, 512, 1088) and all(c.__doc__ and S % 64 == 0 for c, S in zip(SS.CLASSES, SS.SIZES))
    # scatter_apply_kernel: w = lane, lane + 64, .. below S / 16 -- one trip up to 1024 bytes
    assert [-(-(S // 16) // 64) for S in (64,) + SS.SIZES] == [1, 1, 1, 2]
    # repair_gather_q0_kernel: k * S / 16 words in steps of 256
    assert K * 64 // 16 < 256 < K * 1088 // 16
    k, S = SS.LONG_REPAIR
    assert SS.square_words(k, S) / SS.REPAIR_COMPARE_TRIP > 2 and SS.square_words(k, S) % SS.REPAIR_COMPARE_TRIP
    assert [w // SS.DEV_EQUAL_TRIP for w in SS.DEV_EQUAL_WORDS] == [0, 0, 1, 1]
    assert SS.DEV_EQUAL_WORDS[-1] % 256 == 0 and SS.DEV_EQUAL_WORDS[-1] // 256 - 4096 == 1  # block 1, thread 0, second trip


def test_long_repair_cases_land_in_the_trips_the_tests_name():
    """What rsm_repair_squares_dev compares for A_*: the rebuilt square is `full` (rows
    decoded from valid row codewords), the other side the re-extension of its original
    quadrant.  A_row_k differs in the second trip only, A_row_last in the ragged third only,
    A_row_0 (the altered column 0 and parity columns, rows k ..) in both; the C_* and
    D_control squares differ nowhere."""
    k, S = SS.LONG_REPAIR
    trips = {name: SS.differing_trips(RC.case(name, k, S)[3]["full"], k, S)
             for name in ("A_row_0", "A_row_k", "A_row_last", "C_row_root_0", "D_control")}
    assert trips == {"A_row_0": [1, 2], "A_row_k": [1], "A_row_last": [2], "C_row_root_0": [], "D_control": []}


def test_parity_flips_change_one_word_each():
    k, S = SS.LONG_REPAIR
    valid = RP.square(k, S)[0]
    assert SS.differing_trips(valid, k, S) == []
    for (r, c, b), trip in zip(SS.parity_flips(k, S), (0, 0, 1, 2)):
        sq = np.array(valid)
        sq[r, c, b] ^= 1
        again = SS.oracle.extend_square(np.ascontiguousarray(sq[:k, :k]), nthreads=8)
        words = np.flatnonzero((sq != again).reshape(-1, 16).any(axis=1))
        assert len(words) == 1 and words[0] // SS.REPAIR_COMPARE_TRIP == trip, (r, c, b)


# ---- share proofs and their verifiers ------------------------------------------------------
@pytest.mark.parametrize("tree", SS.TREES)
@sizes
def test_share_proof_restatements(lib, S, tree):
    """rsm_default_tree_prove / rsm_nmt_tree_prove give the model's records;
    rsm_*_tree_verify and rsm_sample_verify_data_root owe the model's status for every
    hostile variant; rsm_data_root and rsm_data_root_prove give the chain's."""
    batch, sq, ch = SS.proof_squares(S, tree)
    W, p = sq.W, sq.p
    for s in DC.all_samples(W, sq.count)[::29]:
        q, a, i, pos = s
        vec = [x.tobytes() for x in (batch[q, i] if a == 0 else batch[q, :, i])]
        assert DC.host_record(lib, p, vec, i, pos) == sq.record(s), s
    items, want = SS.verify_items(S, tree)
    P.assert_covers(want, p)
    for it, w in zip(items, want):
        rc, got = host_status(lib, p, it.sample[2], it.share, W, it.sample[3], it.record, it.root)
        assert rc == 0 and got == w, (it.sample, it.label, got, w)
    items, want = SS.chain_items(S, tree)
    for it, w in zip(items, want):
        st = ctypes.c_uint32(0xDEAD)
        sm = R.Sample(*it.sample)
        assert lib.rsm_sample_verify_data_root(ctypes.byref(p) if p is not None else None, W, ctypes.byref(sm), it.share,
                                               len(it.share), it.record, it.root_record, it.data_root, ctypes.byref(st)) == 0
        assert st.value == w, (it.sample, it.label, st.value, w)
    for q in range(sq.count):
        assert host_data_root(lib, ch.roots[q], W) == ch.data_roots[q]
        for a, i in ((0, 0), (0, W - 1), (1, K), (1, W - 1)):
            assert host_root_record(lib, ch.roots[q], W, a, i) == ch.root_record(q, a, i)


# ---- namespace proofs ---------------------------------------------------------------------
@sizes
def test_namespace_proof_restatements(lib, S):
    """rsm_nmt_namespace_prove gives the model's records (device_calls.expect asserts it) and
    rsm_nmt_namespace_verify the helper's status, on the GPU test's squares and variants and
    on the odd width's 66-leaf range."""
    k, ig = K, True
    W, p = 2 * k, R.NmtParams(NS, 1, k)
    batch = np.stack([NL.square(k, NS, S, name, 7) for name in ("runs", "carry", "max_tail")])
    queries, nids, records, shares = DC.expect(lib, batch, k, NS, ig, H.vectors(k))
    seen = set()
    for i in range(0, len(queries), 5):
        s, axis, index = queries[i]
        leaves = H.vector_shares(batch[s], axis, index)
        it = NV.Item("host prover", queries[i], nids[i], records[i], shares[i], H.Tree(leaves, index, k, NS, ig).root)
        for v, must in NV.with_variants(lib, p, it, leaves, W, S):
            got = NV.owed(lib, v, W, p)
            assert got == must, (v.name, v.q, got, must)
            seen.add(got)
    assert seen == {H.OK, H.ROOT, H.INCOMPLETE}
    W = SS.ODD_W
    p = R.NmtParams(NS, 1, W)
    leaves = SS.sorted_vector(W, NS, S, SS.ODD_BOUNDS, 5)
    tree = H.Tree(leaves, 0, W, NS, True)
    for v in (1, 2):
        nid = bytes(NS - 1) + bytes([v])
        it = NV.proved(lib, p, "odd width", (0, 1, 0), leaves, nid)
        assert it.root == tree.root and it.record == H.record_of(W, NS, *H.prove_namespace(tree, nid))
        for x, must in NV.with_variants(lib, p, it, leaves, W, S):
            assert NV.owed(lib, x, W, p) == must, x.name
    assert len(it.shares) == W - 1 > 64


# ---- range proofs -------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [0, NS])
@sizes
def test_range_proof_restatements(lib, S, ns):
    """rsm_*_tree_range_prove gives the model's records for the GPU tests' queries (k = 8,
    and k = 40 with its ranges of more than 64 leaves); rsm_*_tree_range_verify owes the
    model's status over the hostile set."""
    for k, ranges in ((K, SS.RANGES_K8), (SS.LONG_RANGE_K, SS.RANGES_LONG)):
        W, p = 2 * k, RG.params(k, ns)
        sq, rows, cols, _ = SS.range_world(k, ns, S)
        for a, trees in ((0, rows), (1, cols)):
            for i in (0, k - 1, k, W - 1):
                leaves = H.vector_shares(sq, a, i)
                for start, end in ranges:
                    rc, rec, root = RG.host_prove(lib, p, i, leaves, start, end)
                    assert rc == 0 and root == trees[i].root and rec == M.prove(trees[i], ns, start, end), (k, a, i, start, end)
                    case = M.Case("valid", i, start, end, rec, leaves[start:end], root, M.OK)
                    assert RG.host_status(lib, p, W, case, S) == M.OK
    cases, _, musts, _ = SS.range_cases(ns, S)
    M.named_musts(cases)
    p = RG.params(K, ns)
    for c in cases:
        assert RG.host_status(lib, p, 2 * K, c, S) == c.must, (c.name, c.index, c.start, c.end)
    want = {M.OK, M.MALFORMED, M.ORDER, M.ROOT} if ns else {M.OK, M.MALFORMED, M.ROOT}
    assert {c.must for c in cases} == want and {m for m in musts if m is not None} == want


# ---- commitments --------------------------------------------------------------------------
@pytest.mark.parametrize("t", SS.COMMIT_THRESHOLDS)
@sizes
def test_commitment_restatements(lib, S, t):
    """rsm_square_commitment (subtree roots and commitment) over every aligned blob of the GPU
    test's square, rsm_blob_commitment over every seventh blob's shares."""
    sq = SS.commitment_square(S)
    blobs, want_roots, want = SS.commitment_wants(S, t)
    p = R.NmtParams(NS, 1, K)
    for j, ((s, n), roots, com) in enumerate(zip(blobs, want_roots, want)):
        assert square_commitment(lib, p, sq, K, s, n, t, want_roots=len(roots)) == (0, com, 0, roots), (s, n)
        if j % 7 == 0:
            shares = CM.ods_shares(sq, K, s, n)
            assert blob_commitment(lib, R.NmtParams(NS, 1, 1), [bytes(x) for x in shares], t) == (0, com, 0), (s, n)
            assert CM.commitment(shares, NS, t) == com


# ---- Repair and fraud proofs: the models at these sizes -----------------------------------
@sizes
def test_repair_models(S):
    """The squares the GPU Repair tests run, against the oracle crossword: avalanche repairs
    to the valid square, core stops at the model's closure; the verification cases of the
    mixed batch are what tests/repair_dev_calls.py's status table says; the late culprit is
    found in round >= 3 and named by the validity predicate, on both trees."""
    k = K
    for family in ("avalanche", "core"):
        valid, rr, cr = RP.square_for(family, k, S)
        assert valid.shape == (2 * k, 2 * k, S)
        pres = RP.presence(family, k)
        closure = RP.expected_stats(family, k)[3]
        got, after = RC.oracle_repair_keep(RC.cells(valid, pres), list(rr), list(cr))
        assert got == ("ok" if family == "avalanche" else "unrepairable")
        assert after == RC.cells(valid, closure)
    for name in ("C_col_root_last", "A_row_last", "D_control"):
        outcome, _ = RC.expected(name, k, S)
        assert (outcome == "ok") == (D.RC_STATUS[name] == {R.REPAIR_OK}) and outcome != "unrepairable"
        assert RC.case(name, k, S)[3]["offsets"] <= {S - 1}
    for tree in SS.TREES:
        sq, pres, rr, cr, out = C.late_culprit(k, tree, S=S)
        assert sq.shape[2] == S and out.status == C.BYZANTINE and out.round >= 3
        assert C.is_byzantine(out.shares, out.axis, out.index, (rr, cr)[out.axis][out.index], k, tree)


@pytest.mark.parametrize("ns", [0, NS])
@sizes
def test_fraud_proof_model(S, ns):
    """The mixed batch of the GPU test by the model alone: every verdict, every reason the
    tree can give, both axes."""
    p = R.NmtParams(ns, 1, K) if ns else None
    _, table = TF.world(K, S, ns)
    proofs = TF.mixed_batch(K, S, ns, 2 * K + 3)
    got = [f.expect(table, K, p)[0] for f in proofs]
    assert {g[0] for g in got} == {F.VALID, F.TOOFEW, F.SHARE, F.CONSISTENT}
    assert {g[1] for g in got if g[0] == F.VALID} == ({F.ROOT, F.ENCODING, F.TREE} if ns else {F.ROOT, F.ENCODING})
    assert all(f.shares.shape == (2 * K, S) for f in proofs)
