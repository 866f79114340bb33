"""TEST INFRASTRUCTURE ONLY -- erasure patterns that take Repair through more than one
row sweep (the shared builders of tests/test_repair_patterns_cpu.py and
tests/test_gpu_repair_patterns.py).  Nothing here calls the library under test: maps are
pure functions of (family, k), squares come from repair_cases.valid_square, roots from
oracle/crossword.py (DefaultTree) or oracle/nmt.py, and the expected counters from
model(), the peeling model of the fast path's schedule.

BenchmarkRepair's erasures (k of every row's 2k cells) are completed by one row sweep
over 2k rows that all have exactly k cells.  The families here are what that shape
never shows: complete rows between the rows to decode, rows with more than k cells,
column sweeps, sweeps of a few vectors, sweeps that decode from cells an earlier sweep
rebuilt, and squares that cannot be completed.

A "block" of rows or columns is an index set pushed through the fixed interleave
0, W-1, 1, W-2, ... (W = 2k), so every block has members in both halves of the square.
Randomness comes from oracle.splitmix64_bytes, so a map never depends on numpy's
generators.

Families (all [2k][2k] bool, True = present):

  zero-copy (one row sweep, every incomplete row has >= k cells)
    rows_uneven      row r loses e(r) cells, e takes every value 0..k; complete rows form
                     runs at rows 0-1, k-1..k and 2k-1 and stand alone at k//2 and
                     k + k//2; the first incomplete row loses its k data cells, another
                     its k parity cells, another exactly one cell
    q1_q2            only quadrants 1 and 2: top rows hold parity only, bottom rows data
                     only, every row exactly k cells

  general loop
    odd_rows         only the k odd rows, complete: no row to decode, one column sweep
                     of 2k vectors
    q0_only, q3_only one quadrant: a row sweep of k vectors, then a column sweep of 2k
    chain3, chain3_t three sweeps of 1, 2 and k + 1 vectors, each unlocked by the one
                     before (below); chain3_t is the transpose
    chain3_cf        the same chain starting with a column sweep (below)
    avalanche        every cell erased independently with probability AVALANCHE_T[k] /
                     256; the first seed in 0..63 that the model repairs in >= 6 sweeps

  stuck
    core             a (k+1) x (k+1) block erased: nothing decodable
    core_edge        in a (k+4) x (k+4) block, cell (a, b) erased iff a + b >= 6: two
                     sweeps of 3 vectors, then a (k+1) x (k+1) core remains
    avalanche_stuck  as avalanche; the first seed that gets stuck after >= 3 sweeps

chain3: rows P and columns Q of k + 1 members each, p1 in P, q* in Q, one more row w
outside P and one more column e outside Q.  Erased: P x (Q \\ {q*}), (p1, q*), (p, e) for
p in P \\ {p1}, and (w, e).  Every row of P then misses k + 1 cells, and so does every
column of Q \\ {q*} and column e; only row w (2k - 1 cells) can be decoded.  That fills
(w, e), which brings column e down to k missing; the column sweep decodes q* (2k - 1
cells) and e (k cells); that fills (p1, q*) and every (p, e), which brings every row of P
down to k missing: [rows 1] [cols 2] [rows k + 1], k + 4 vectors.

The structure is its own dual (q* plays w's part in the transpose: row q* has 2k - 1
cells), so chain3_t runs rows, columns, rows as well, with the same counts.  chain3_cf is
the form whose first row pass finds nothing.  Before transposing, column q* is made
undecodable too: (w, q*) and (p, q*) for k - 1 further rows p of P \\ {p1} are erased as
well, so column q* misses k + 1 cells until row w (now 2k - 2 cells) is decoded.
Transposed: [cols 1, 2k - 2 cells] [rows 2, k cells each] [cols k + 1, k cells each].
"""
import functools

import numpy as np

import oracle
import repair_cases as RC
from oracle import crossword, nmt

Row, Col = crossword.Row, crossword.Col
NS = RC.NS

ZERO_COPY = ("rows_uneven", "q1_q2")
GENERAL = ("odd_rows", "q0_only", "q3_only", "chain3", "chain3_t", "chain3_cf", "avalanche")
REPAIRABLE = ZERO_COPY + GENERAL
STUCK = ("core", "core_edge", "avalanche_stuck")
FAMILIES = REPAIRABLE + STUCK

AVALANCHE_SEEDS = 64
AVALANCHE_MIN_SWEEPS = 6
STUCK_MIN_SWEEPS = 3
# A cell is erased iff its splitmix byte is below T (probability T / 256).  T per k,
# searched once over 0.53..0.66: between "one sweep" and "stuck at once" lies a window
# that narrows and moves towards 1/2 as k grows (0.62 at k = 8, 0.554 at k = 257).
AVALANCHE_T = {8: 159, 16: 159, 33: 164, 64: 151, 65: 154, 128: 148, 129: 148, 200: 143, 257: 142}
AVALANCHE_STUCK_T = {8: 169, 16: 164, 65: 148}


def interleave(W):
    """0, W-1, 1, W-2, ...: a permutation of range(W)."""
    out = np.empty(W, np.int64)
    out[0::2] = np.arange((W + 1) // 2)
    out[1::2] = W - 1 - np.arange(W // 2)
    return out


def block(W, start, n):
    """n indices of the interleave from position start (wrapping)."""
    return interleave(W)[(start + np.arange(n)) % W]


def _words(n, seed):
    return oracle.splitmix64_bytes(8 * n, seed=seed).view(np.uint64)


def _perm(n, seed):
    """A permutation of range(n) from splitmix words."""
    return np.argsort(_words(n, seed), kind="stable")


def uneven_complete_rows(k):
    return sorted({0, 1, k // 2, k - 1, k, k + k // 2, 2 * k - 1})


def uneven_losses(k):
    """e(r) of rows_uneven: 0 on the complete rows; the j-th incomplete row loses
    k - (j mod k) cells (so incomplete rows 0 and k lose k, row k - 1 loses one)."""
    W = 2 * k
    e = np.zeros(W, np.int64)
    todo = [r for r in range(W) if r not in set(uneven_complete_rows(k))]
    for j, r in enumerate(todo):
        e[r] = k - (j % k)
    return e


def _rows_uneven(k):
    W = 2 * k
    pres = np.ones((W, W), bool)
    e = uneven_losses(k)
    todo = np.flatnonzero(e)
    for j, r in enumerate(todo):
        if j == 0:
            lost = np.arange(k)  # all data cells
        elif j == k:
            lost = np.arange(k, W)  # all parity cells
        else:
            lost = _perm(W, 0x0E5E0000 + k * 4096 + int(r))[:e[r]]
        pres[r, lost] = False
    return pres


def chain3_parts(k):
    """(P, Q, p1, q*, w, e) of chain3."""
    W = 2 * k
    P = block(W, 0, k + 1)
    w = int(block(W, k + 1, 1)[0])
    Q = block(W, 3, k + 1)
    e = int(block(W, 1, 1)[0])
    return P, Q, int(P[k // 2]), int(Q[k // 3]), w, e


def _chain3(k):
    W = 2 * k
    P, Q, p1, qs, w, e = chain3_parts(k)
    pres = np.ones((W, W), bool)
    pres[np.ix_(P, Q[Q != qs])] = False
    pres[p1, qs] = False
    pres[P[P != p1], e] = False
    pres[w, e] = False
    return pres


def _chain3_cf(k):
    P, Q, p1, qs, w, e = chain3_parts(k)
    pres = _chain3(k)
    pres[w, qs] = False
    pres[P[P != p1][:k - 1], qs] = False
    return np.ascontiguousarray(pres.T)


def core_parts(k):
    W = 2 * k
    return block(W, 2, k + 1), block(W, 5, k + 1)


def core_edge_parts(k):
    W = 2 * k
    return block(W, 1, k + 4), block(W, 4, k + 4)


def _avalanche_map(k, T, seed):
    W = 2 * k
    b = oracle.splitmix64_bytes(W * W, seed=0xA7A10000 + k * 256 + seed).reshape(W, W)
    return b >= T


def avalanche_t(k, stuck=False):
    return (AVALANCHE_STUCK_T if stuck else AVALANCHE_T)[k]


@functools.lru_cache(maxsize=None)
def avalanche_seed(k, stuck=False):
    """The first seed in 0..AVALANCHE_SEEDS-1 whose map the model repairs in >=
    AVALANCHE_MIN_SWEEPS sweeps (stuck: leaves stuck after >= STUCK_MIN_SWEEPS), or None."""
    T = avalanche_t(k, stuck)
    for seed in range(AVALANCHE_SEEDS):
        sweeps, _, _, closure = model(_avalanche_map(k, T, seed), k)
        if stuck and not closure.all() and sweeps >= STUCK_MIN_SWEEPS:
            return seed
        if not stuck and closure.all() and sweeps >= AVALANCHE_MIN_SWEEPS:
            return seed
    return None


@functools.lru_cache(maxsize=None)
def _presence(family, k):
    assert family in FAMILIES and k >= 8
    W = 2 * k
    pres = np.ones((W, W), bool)
    if family == "rows_uneven":
        pres = _rows_uneven(k)
    elif family == "q1_q2":
        pres[:k, :k] = False
        pres[k:, k:] = False
    elif family == "odd_rows":
        pres[0::2] = False
    elif family == "q0_only":
        pres[:] = False
        pres[:k, :k] = True
    elif family == "q3_only":
        pres[:] = False
        pres[k:, k:] = True
    elif family == "chain3":
        pres = _chain3(k)
    elif family == "chain3_t":
        pres = np.ascontiguousarray(_chain3(k).T)
    elif family == "chain3_cf":
        pres = _chain3_cf(k)
    elif family == "core":
        A, B = core_parts(k)
        pres[np.ix_(A, B)] = False
    elif family == "core_edge":
        A, B = core_edge_parts(k)
        n = np.arange(k + 4)
        pres[np.ix_(A, B)] = n[:, None] + n[None, :] < 6
    else:
        stuck = family == "avalanche_stuck"
        seed = avalanche_seed(k, stuck)
        assert seed is not None, "no %s seed below %d at k = %d" % (family, AVALANCHE_SEEDS, k)
        pres = _avalanche_map(k, avalanche_t(k, stuck), seed)
    pres.setflags(write=False)
    return pres


def presence(family, k):
    """The [2k][2k] bool map of a family (read-only, shared)."""
    return _presence(family, k)


def model(pres, k):
    """The peeling model of the fast path's schedule: repeat a row pass, then a column
    pass; a pass decodes every vector with k <= have < 2k at once, and a pass that has
    any is one sweep.  Returns (sweeps, decoded vectors, [(axis, count, min have, max
    have)] per sweep, closure: the final presence map)."""
    p = np.array(pres, bool)
    W = 2 * k
    assert p.shape == (W, W)
    per = []
    while True:
        progress = False
        for axis in (Row, Col):
            have = p.sum(axis=1 if axis == Row else 0)
            todo = np.flatnonzero((have >= k) & (have < W))
            if todo.size == 0:
                continue
            per.append((axis, int(todo.size), int(have[todo].min()), int(have[todo].max())))
            if axis == Row:
                p[todo, :] = True
            else:
                p[:, todo] = True
            progress = True
        if not progress:
            break
    return len(per), sum(s[1] for s in per), per, p


@functools.lru_cache(maxsize=None)
def expected_stats(family, k):
    """(sweeps, decoded vectors, per-sweep list, closure) of a family's map."""
    out = model(presence(family, k), k)
    out[3].setflags(write=False)
    return out


@functools.lru_cache(maxsize=4)
def square(k, S=64, tree="default", variant=0):
    """(valid [2k][2k][S] square, row roots, column roots) -- one square per (k, S, tree,
    variant), shared by the families (read-only).  tree: "default" (oracle/crossword.py
    roots) or "nmt" (sorted 29-byte namespaces in Q0, oracle/nmt.py roots)."""
    valid = RC.valid_square(k, S, 0x9A77 + k + 0x10000 * variant, tree)
    W = 2 * k
    if tree == "nmt":
        rr, cr = nmt.eds_roots(valid, k, NS)
    else:
        cellsb = [[valid[r, c].tobytes() for c in range(W)] for r in range(W)]
        rr = [crossword.merkle_root(row) for row in cellsb]
        cr = [crossword.merkle_root([cellsb[r][c] for r in range(W)]) for c in range(W)]
    valid.setflags(write=False)
    return valid, tuple(rr), tuple(cr)


def square_for(family, k, S=64, tree="default"):
    """The square a family is tested on.  rows_uneven has one of its own: its complete rows
    are not decoded, so the zero-copy sweep leaves them to an upload of their own, and
    the device buffers outlive a Repair: on the square of the case before it a row that
    never went up would still hold the right bytes."""
    return square(k, S, tree, 1 if family == "rows_uneven" else 0)
