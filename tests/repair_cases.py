"""TEST INFRASTRUCTURE ONLY -- squares that put exactly one of Repair's verification
steps between a bad square and success (the shared builders of
tests/test_repair_cases_cpu.py and tests/test_gpu_repair_verification.py).  Nothing
here calls the library under test: squares come from oracle.extend_square, roots from
oracle/crossword.py (DefaultTree) or oracle/nmt.py, expectations from the oracle
crossword.

Repair may accept a square only when (1) every complete row and column passes the
pre-repair check, (2) the rebuilt square is a valid 2D codeword and (3) its roots are
the committed ones.  A corrupted present share under the ORIGINAL roots trips (2) and
(3) together, so either check alone gives the right answer.  The cases here commit
the roots to the altered square, or alter only a root, so one check stands alone.

The tool is a minimum-weight codeword delta(j, b): the encoding of k zero shares
except one byte 0x5A at offset b of share j.  It is non-zero in exactly k + 1 cells
(cell j and all k parity cells: the code is MDS) and only at byte b (in GF(2^16), k >
128, also at the partner byte of the same 64-byte block: the low bytes of the block's
32 symbols are its bytes 0..31, the high bytes 32..63).  XOR-ed into one row it keeps
every row a codeword and makes exactly k + 1 columns non-codewords.

Families (case names):
  A_row_k, A_row_last, A_row_0
      delta into row k (j = 0, b = 0: the first 16-byte word of the bottom half), row
      2k-1 (j = k-1, b = S-1: the last word of the square) or row 0.  Rows valid,
      columns not, nothing complete: only an encoding check after the sweeps sees it.
  B_col_kept, B_row_kept
      as A_row_k with one invalid column kept complete (erasures drawn from the other
      columns), and the transposed form (a column codeword into column k, one invalid
      row kept complete): the pre-repair check must report that vector.
  C_row_root_0, C_col_root_last, C_row_root_last
      valid square, one committed root with one byte flipped: only the root compare.
  D_control
      valid square, untouched roots: repairs on the fast path.
  E_overdetermined_row
      row 1 has k + 3 shares present, one of them altered; roots committed to the
      altered full square.  The row's shares do not lie on one codeword.

Erasures follow BenchmarkRepair (extendeddatacrossword_test.go:443-453): exactly k of
the 2k cells of every row, seeded (of every column for B_row_kept).

tree = "nmt": quadrant 0 carries sorted 29-byte namespaces (proof_verify.sorted_q0_square),
the delta byte sits at offset >= 29 so no namespace changes, and the committed roots
are the erasured NMT's (oracle/nmt.py).  The note then also carries the DefaultTree
roots of the same altered square (with the same root flipped): the solver's control
flow depends on the tree only through root equality, so the DefaultTree crossword on
the same cells gives the expected (axis, index, shares).
"""
import functools
import zlib

import numpy as np

import oracle
from oracle import crossword, nmt

Row, Col = crossword.Row, crossword.Col
NS = 29
DELTA_BYTE = 0x5A

CASES = ("A_row_k", "A_row_last", "A_row_0", "B_col_kept", "B_row_kept",
         "C_row_root_0", "C_col_root_last", "C_row_root_last", "D_control", "E_overdetermined_row")
FAMILY_A = tuple(c for c in CASES if c.startswith("A_"))


def _seed(name, k, S, tree):
    return zlib.crc32(("%s/%d/%d/%s" % (name, k, S, tree)).encode())


def delta(k, S, j, b):
    """[2k][S] uint8: the minimum-weight codeword with byte DELTA_BYTE at offset b of share j."""
    data = np.zeros((k, S), np.uint8)
    data[j, b] = DELTA_BYTE
    parity = oracle.encode([row.tobytes() for row in data])
    return np.concatenate([data, np.frombuffer(b"".join(parity), np.uint8).reshape(k, S)])


def delta_offsets(k, S, b):
    """Byte offsets at which delta(k, S, j, b) is non-zero."""
    if oracle.field_bits(k) == 8:
        return {b}
    blk, o = b // 64 * 64, b % 32
    return {blk + o, blk + o + 32}


def erase(W, k, seed, keep_col=None, keep_row=None):
    """[W][W] bool presence: k cells of every row erased (keep_col: none of them in that
    column); with keep_row, k cells of every column instead, none of them in that row."""
    rng = np.random.default_rng(seed)
    pres = np.ones((W, W), bool)
    if keep_row is not None:
        others = np.array([r for r in range(W) if r != keep_row])
        for c in range(W):
            pres[rng.choice(others, size=k, replace=False), c] = False
        return pres
    cols = np.array([c for c in range(W) if c != keep_col])
    for r in range(W):
        pres[r, rng.choice(cols, size=k, replace=False)] = False
    return pres


def complete_vectors(pres):
    """[(axis, index)] of the complete rows and columns of a presence map."""
    return ([(Row, int(i)) for i in np.flatnonzero(pres.all(axis=1))] +
            [(Col, int(i)) for i in np.flatnonzero(pres.all(axis=0))])


def cells(sq, pres=None):
    """Flattened list of a [W][W][S] square, None where pres is False."""
    W = sq.shape[0]
    flat = [sq[r, c].tobytes() for r in range(W) for c in range(W)]
    if pres is not None:
        flat = [x if p else None for x, p in zip(flat, pres.reshape(-1))]
    return flat


def default_roots(sq):
    s = crossword.Square(cells(sq))
    return s.roots(Row), s.roots(Col)


def flip_byte(root):
    return root[:-1] + bytes([root[-1] ^ 1])


def valid_square(k, S, seed, tree="default"):
    if tree == "nmt":
        import proof_verify
        ods = proof_verify.sorted_q0_square(k, S, NS, seed)[:k, :k]
    else:
        ods = np.random.default_rng(seed).integers(0, 256, (k, k, S), dtype=np.uint8)
    return oracle.extend_square(np.ascontiguousarray(ods), nthreads=8)


@functools.lru_cache(maxsize=16)
def case(name, k, S=64, tree="default"):
    """(flat, row_roots, col_roots, note) of one case.  flat: 4k^2 cells, None = erased.
    note: family; valid / full ([2k][2k][S]: the valid square and the one the roots are
    committed to); present ([2k][2k] bool); bad = {axis: indices of the non-codeword
    vectors of full}; touched = {axis: indices whose committed root differs from the
    valid square's}; offsets (byte offsets at which full differs from valid); complete
    ([(axis, index)] of complete vectors); default_roots (the DefaultTree roots the
    oracle crossword runs with: the committed ones unless tree == "nmt")."""
    assert name in CASES and tree in ("default", "nmt")
    W, seed = 2 * k, _seed(name, k, S, tree)
    lo = NS if tree == "nmt" else 0  # the first byte past the namespace
    valid = valid_square(k, S, seed, tree)
    full = valid.copy()
    bad = {Row: [], Col: []}
    touched = {Row: [], Col: []}
    offsets = set()
    keep_col = keep_row = flip = None
    family = name[0]
    if name in ("A_row_k", "A_row_last", "A_row_0", "B_col_kept"):
        r, j, b = {"A_row_k": (k, 0, lo), "A_row_last": (W - 1, k - 1, S - 1), "A_row_0": (0, 0, lo),
                   "B_col_kept": (k, 0, lo)}[name]
        full[r] ^= delta(k, S, j, b)
        bad[Col] = [j] + list(range(k, W))
        touched = {Row: [r], Col: list(bad[Col])}
        offsets = delta_offsets(k, S, b)
        if name == "B_col_kept":
            keep_col = k + k // 2
    elif name == "B_row_kept":
        c, j, b = k, 0, lo
        full[:, c] ^= delta(k, S, j, b)
        bad[Row] = [j] + list(range(k, W))
        touched = {Row: list(bad[Row]), Col: [c]}
        offsets = delta_offsets(k, S, b)
        keep_row = k + k // 2
    elif family == "C":
        flip = {"C_row_root_0": (Row, 0), "C_col_root_last": (Col, W - 1), "C_row_root_last": (Row, W - 1)}[name]
        touched[flip[0]] = [flip[1]]
    pres = erase(W, k, seed + 1, keep_col=keep_col, keep_row=keep_row)
    if family == "E":
        r = 1
        extra = np.flatnonzero(~pres[r])[:3]
        pres[r, extra] = True  # k + 3 present
        c, b = int(np.flatnonzero(pres[r])[k // 2]), S // 2
        full[r, c, b] ^= DELTA_BYTE
        bad = {Row: [r], Col: [c]}
        touched = {Row: [r], Col: [c]}
        offsets = {b}
    complete = complete_vectors(pres)
    want_complete = [(Col, keep_col)] if keep_col is not None else [(Row, keep_row)] if keep_row is not None else []
    assert complete == want_complete, (name, k, complete)
    rr_d, cr_d = default_roots(full)
    if tree == "nmt":
        rr, cr = nmt.eds_roots(full, k, NS)
    else:
        rr, cr = list(rr_d), list(cr_d)
    if flip is not None:
        for roots in ((rr, rr_d) if flip[0] == Row else (cr, cr_d)):
            roots[flip[1]] = flip_byte(roots[flip[1]])
    note = dict(name=name, family=family, k=k, S=S, tree=tree, valid=valid, full=full, present=pres, bad=bad,
                touched=touched, offsets=offsets, complete=complete, default_roots=(tuple(rr_d), tuple(cr_d)))
    return tuple(cells(full, pres)), tuple(rr), tuple(cr), note


def oracle_repair_keep(flat, rr, cr):
    """oracle crossword.repair, returning ("ok" | "unrepairable" | (axis, index, shares),
    the square's cells afterwards): the reference leaves the cells it solved in place
    when it gives up (extendeddatacrossword.go:74-122)."""
    sq = crossword.Square(list(flat))
    try:
        crossword.pre_repair_sanity_check(sq, rr, cr)
        while True:
            solved, progress = True, False
            for i in range(sq.w):
                s1, p1 = crossword.solve_vector(sq, crossword.Row, i, rr, cr)
                s2, p2 = crossword.solve_vector(sq, crossword.Col, i, cr, rr)
                solved = solved and s1 and s2
                progress = progress or p1 or p2
            if solved:
                return "ok", sq.flattened()
            if not progress:
                return "unrepairable", sq.flattened()
    except crossword.Byzantine as b:
        return (b.axis, b.index, b.shares), sq.flattened()


@functools.lru_cache(maxsize=16)
def expected(name, k, S=64, tree="default"):
    """(outcome, cells afterwards) of the oracle crossword on the case's cells, with the
    DefaultTree roots of the square the case's roots are committed to."""
    flat, _, _, note = case(name, k, S, tree)
    rr, cr = note["default_roots"]
    return oracle_repair_keep(flat, list(rr), list(cr))
