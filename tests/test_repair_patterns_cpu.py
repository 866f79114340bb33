"""CPU: the erasure patterns of tests/repair_patterns.py have the properties their GPU
tests rely on, and the peeling model that predicts Repair's counters agrees with the
oracle crossword (the only place the model is trusted from)."""
import numpy as np
import pytest

import repair_cases as RC
import repair_patterns as RP

KS = [8, 16, 65, 128, 129]
Row, Col = RP.Row, RP.Col


def _both_halves(idx, k):
    idx = np.asarray(idx)
    return (idx < k).any() and (idx >= k).any()


def _runs(rows):
    """[(first, last)] of the runs of consecutive indices in a sorted list."""
    out = []
    for r in rows:
        if out and out[-1][1] == r - 1:
            out[-1][1] = r
        else:
            out.append([r, r])
    return [tuple(x) for x in out]


@pytest.mark.parametrize("W", [2, 7, 16, 130])
def test_interleave_is_a_permutation(W):
    il = RP.interleave(W)
    assert sorted(il.tolist()) == list(range(W))
    assert il[:4].tolist() == [0, W - 1, 1, W - 2][:min(4, W)]


@pytest.mark.parametrize("k", KS)
def test_rows_uneven(k):
    W = 2 * k
    pres = RP.presence("rows_uneven", k)
    lost = W - pres.sum(axis=1)
    assert sorted(set(lost.tolist())) == list(range(k + 1))  # every value 0..k
    assert np.array_equal(lost, RP.uneven_losses(k))
    complete = np.flatnonzero(lost == 0).tolist()
    assert complete == RP.uneven_complete_rows(k)
    runs = _runs(complete)
    assert (0, 1) in runs and (k - 1, k) in runs and (W - 1, W - 1) in runs
    singles = [a for a, b in runs if a == b and a != W - 1]
    assert len(singles) >= 2 and any(r < k for r in singles) and any(r > k for r in singles)
    assert any(not pres[r, :k].any() and pres[r, k:].all() for r in range(W))  # all data cells lost
    assert any(pres[r, :k].all() and not pres[r, k:].any() for r in range(W))  # all parity cells lost
    assert (lost == 1).sum() >= 1 and (lost == k).sum() >= 2
    assert ((lost > 0) & (lost < k)).sum() >= k - 1  # rows with strictly more than k cells
    assert not pres.all(axis=0).any()  # no complete column
    sweeps, vecs, per, closure = RP.expected_stats("rows_uneven", k)
    assert (sweeps, vecs) == (1, W - len(complete)) and per == [(Row, W - len(complete), k, W - 1)]
    assert closure.all()


@pytest.mark.parametrize("k", KS)
def test_quadrant_families(k):
    W = 2 * k
    q = RP.presence("q1_q2", k)
    assert (q.sum(axis=1) == k).all() and (q.sum(axis=0) == k).all()
    assert not q[:k, :k].any() and q[:k, k:].all() and q[k:, :k].all() and not q[k:, k:].any()
    assert RP.expected_stats("q1_q2", k)[:3] == (1, W, [(Row, W, k, k)])
    o = RP.presence("odd_rows", k)
    assert o[1::2].all() and not o[0::2].any()
    assert RC.complete_vectors(o) == [(Row, r) for r in range(1, W, 2)]
    assert RP.expected_stats("odd_rows", k)[:3] == (1, W, [(Col, W, k, k)])
    for fam, rows in (("q0_only", slice(0, k)), ("q3_only", slice(k, W))):
        p = RP.presence(fam, k)
        assert p.sum() == k * k and p[rows, rows].all()
        assert RP.expected_stats(fam, k)[:3] == (2, 3 * k, [(Row, k, k, k), (Col, W, k, k)])
    for fam in ("q1_q2", "odd_rows", "q0_only", "q3_only"):
        assert RP.expected_stats(fam, k)[3].all()


@pytest.mark.parametrize("k", KS)
def test_chain3(k):
    W = 2 * k
    P, Q, p1, qs, w, e = RP.chain3_parts(k)
    assert len(set(P.tolist())) == k + 1 and len(set(Q.tolist())) == k + 1
    assert _both_halves(P, k) and _both_halves(Q, k)
    assert p1 in P and qs in Q and w not in P and e not in Q
    pres = RP.presence("chain3", k)
    want = np.ones((W, W), bool)
    for p in P:
        for q in Q:
            if q != qs:
                want[p, q] = False
        if p != p1:
            want[p, e] = False
    want[p1, qs] = False
    want[w, e] = False
    assert np.array_equal(pres, want)
    have_r, have_c = pres.sum(axis=1), pres.sum(axis=0)
    # every vector of the core is one cell over the limit; only row w can be decoded
    assert all(have_r[p] == k - 1 for p in P) and have_r[w] == W - 1
    assert all(have_c[q] == k - 1 for q in Q if q != qs) and have_c[e] == k - 1 and have_c[qs] == W - 1
    assert (have_r == W).sum() == W - (k + 2)
    assert RP.expected_stats("chain3", k)[:3] == (
        3, k + 4, [(Row, 1, W - 1, W - 1), (Col, 2, k, W - 1), (Row, k + 1, k, k)])
    assert np.array_equal(RP.presence("chain3_t", k), pres.T)
    # the structure is its own dual (row q* of the transpose has 2k - 1 cells): rows first again
    assert RP.expected_stats("chain3_t", k)[:3] == RP.expected_stats("chain3", k)[:3]
    assert not np.array_equal(pres, pres.T)
    # chain3_cf: no row can be decoded at first (every row complete or below k cells)
    cf = RP.presence("chain3_cf", k)
    have_r, have_c = cf.sum(axis=1), cf.sum(axis=0)
    assert ((have_r == W) | (have_r < k)).all() and ((have_c >= k) & (have_c < W)).sum() == 1
    assert not (cf & ~pres.T).any() and (pres.T & ~cf).sum() == k  # chain3_t less k cells of row q*
    assert (~cf[qs]).sum() == k + 1
    assert RP.expected_stats("chain3_cf", k)[:3] == (
        3, k + 4, [(Col, 1, W - 2, W - 2), (Row, 2, k, k), (Col, k + 1, k, k)])
    assert all(RP.expected_stats(f, k)[3].all() for f in ("chain3", "chain3_t", "chain3_cf"))


@pytest.mark.parametrize("k", KS)
def test_core_families(k):
    W = 2 * k
    A, B = RP.core_parts(k)
    assert len(set(A.tolist())) == k + 1 and len(set(B.tolist())) == k + 1
    assert _both_halves(A, k) and _both_halves(B, k)
    pres = RP.presence("core", k)
    assert (~pres).sum() == (k + 1) ** 2 and not pres[np.ix_(A, B)].any()
    sweeps, vecs, per, closure = RP.expected_stats("core", k)
    assert (sweeps, vecs, per) == (0, 0, []) and np.array_equal(closure, pres)
    A, B = RP.core_edge_parts(k)
    assert len(set(A.tolist())) == k + 4 and len(set(B.tolist())) == k + 4
    assert _both_halves(A, k) and _both_halves(B, k)
    pres = RP.presence("core_edge", k)
    want = np.ones((W, W), bool)
    for a in range(k + 4):
        for b in range(k + 4):
            want[A[a], B[b]] = a + b < 6
    assert np.array_equal(pres, want)
    sweeps, vecs, per, closure = RP.expected_stats("core_edge", k)
    assert (sweeps, vecs, per) == (2, 6, [(Row, 3, k, k + 2), (Col, 3, k, k + 2)])
    left = np.ones((W, W), bool)
    left[np.ix_(A[3:], B[3:])] = False  # the (k+1) x (k+1) core that remains
    assert np.array_equal(closure, left)


@pytest.mark.parametrize("k", sorted(RP.AVALANCHE_T))
def test_avalanche_seed_found(k):
    """Every k the GPU tests use: a seed below the cap gives a repairable map of >= 6
    sweeps that mixes short and long todo lists and under- and over-determined vectors."""
    seed = RP.avalanche_seed(k)
    assert seed is not None and 0 <= seed < RP.AVALANCHE_SEEDS
    sweeps, vecs, per, closure = RP.expected_stats("avalanche", k)
    assert closure.all() and sweeps >= RP.AVALANCHE_MIN_SWEEPS and vecs == sum(s[1] for s in per)
    assert {s[0] for s in per} == {Row, Col}
    assert min(s[1] for s in per) <= 8 and min(s[2] for s in per) == k and max(s[3] for s in per) > k
    if k >= 16:
        assert max(s[1] for s in per) >= k // 2
    if k >= 64:  # lists on both sides of the split decoder's 64-task threshold
        assert max(s[1] for s in per) > 64


@pytest.mark.parametrize("k", sorted(RP.AVALANCHE_STUCK_T))
def test_avalanche_stuck_seed_found(k):
    seed = RP.avalanche_seed(k, True)
    assert seed is not None and 0 <= seed < RP.AVALANCHE_SEEDS
    sweeps, vecs, per, closure = RP.expected_stats("avalanche_stuck", k)
    assert not closure.all() and sweeps >= RP.STUCK_MIN_SWEEPS
    pres = RP.presence("avalanche_stuck", k)
    assert (closure & ~pres).sum() >= vecs  # solved cells that must stay
    have_r, have_c = closure.sum(axis=1), closure.sum(axis=0)
    assert not (((have_r >= k) & (have_r < 2 * k)).any() or ((have_c >= k) & (have_c < 2 * k)).any())


def test_maps_are_pure_functions():
    for fam in RP.FAMILIES:
        a = RP.presence(fam, 8)
        RP._presence.cache_clear()
        RP.avalanche_seed.cache_clear()
        assert np.array_equal(a, RP.presence(fam, 8)) and a.shape == (16, 16) and a.dtype == bool


# ---------------------------------------------------------------------------
# the model against the oracle crossword
# ---------------------------------------------------------------------------
def _check_model(k, pres):
    valid, rr, cr = RP.square(k)
    sweeps, vecs, per, closure = RP.model(pres, k)
    got, after = RC.oracle_repair_keep(RC.cells(valid, pres), list(rr), list(cr))
    want = "ok" if closure.all() else "unrepairable"
    assert got == want, (per, int((~closure).sum()))
    assert after == RC.cells(valid, closure)
    return want


@pytest.mark.parametrize("k", [8, 16])
@pytest.mark.parametrize("family", RP.FAMILIES)
def test_model_matches_oracle_crossword(family, k):
    want = _check_model(k, RP.presence(family, k))
    assert want == ("unrepairable" if family in RP.STUCK else "ok")


@pytest.mark.parametrize("k", [8, 16])
def test_model_matches_oracle_crossword_random(k):
    """20 random maps per k, erasure probability 0.50..0.69 (across the threshold, so
    both outcomes occur)."""
    seen = set()
    for i in range(20):
        seen.add(_check_model(k, RP._avalanche_map(k, 128 + 2 * i + i // 2, 1000 + i)))
    assert seen == {"ok", "unrepairable"}
