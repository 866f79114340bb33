"""TEST INFRASTRUCTURE ONLY -- the model of rsm_repair_squares_checked_dev's schedule, the
validity predicate of a named vector, the squares built for it (late culprit, stage
order) and the one place that runs the call between guard bands (shared by
tests/test_repair_checked_cpu.py and tests/test_gpu_repair_checked.py).  The model calls
nothing of the library under test: it decodes and encodes with the oracle codec and
hashes with hashlib (DefaultTree) or oracle/nmt.py.  Importing this module touches no
GPU; every function that does takes `lib`.

The schedule (include/rsmt2d_hip.h, "Repair of device-resident squares with
attribution"): the passes of repair_patterns.model, and around them check rounds.  Round
0 checks the vectors complete on entry and names the lowest (index, axis).  After the
square's p-th decoding pass, round p: stage 1 checks the decoded vectors, and only if it
is clean stage 2 checks the vectors of the other axis that the pass completed; each names
its lowest failing index.  A check is: tree status, root, parity == encode(first half).
A square that fails in round 0 or in a stage 1 keeps its presence map as the failing
pass's plan found it (the pass's decoded vectors are not marked); one that fails in a
stage 2 also has the pass's decoded vectors marked -- they all passed stage 1 -- so the
named vector is complete.  Either way every present cell was given or lies in a vector that
passed, and the named vector has at least k cells.
"""
import ctypes
import functools
import hashlib

import numpy as np

import oracle
import repair_cases as RC
import repair_dev_calls as D
import repair_patterns as P
import rsmt2d_amd as R
from device_calls import Guarded
from oracle import nmt

Row, Col = 0, 1
NS = RC.NS
OK, STUCK, BYZANTINE = 0, 1, 4
ROOT, ENCODING, TREE = 1, 2, 3


# ---- trees ---------------------------------------------------------------------------
def _split_root(nodes, join):
    """RFC 6962: split at the largest power of two below n."""
    n = len(nodes)
    if n == 1:
        return nodes[0]
    h = 1
    while h * 2 < n:
        h *= 2
    return join(_split_root(nodes[:h], join), _split_root(nodes[h:], join))


class Trees:
    """Leaf records per cell (computed once, counted) and the root of a vector."""

    def __init__(self, k, tree):
        self.k, self.W, self.tree = k, 2 * k, tree
        self.leaf = {}

    def _leaf(self, data, r, c):
        if (r, c) not in self.leaf:
            share = data[r, c].tobytes()
            if self.tree == "nmt":
                ns = share[:NS] if (r < self.k and c < self.k) else b"\xff" * NS
                self.leaf[(r, c)] = nmt.hash_leaf(ns + share, NS)
            else:
                self.leaf[(r, c)] = hashlib.sha256(b"\x00" + share).digest()
        return self.leaf[(r, c)]

    def record(self, data, axis, i):
        for p in range(self.W):
            self._leaf(data, *((i, p) if axis == Row else (p, i)))

    def root(self, data, axis, i):
        """(tree failed, root bytes or None)"""
        leaves = [self._leaf(data, *((i, p) if axis == Row else (p, i))) for p in range(self.W)]
        if self.tree != "nmt":
            return False, _split_root(leaves, lambda a, b: hashlib.sha256(b"\x01" + a + b).digest())
        if any(leaves[p + 1][:NS] < leaves[p][:NS] for p in range(self.W - 1)):
            return True, None  # push order
        try:
            return False, _split_root(leaves, lambda a, b: nmt.hash_node(a, b, NS, True))
        except nmt.NmtError:
            return True, None


def vector_reason(shares, axis, i, committed, k, tree):
    """The check of one complete vector given as 2k byte strings: 0 or TREE / ROOT / ENCODING."""
    W = 2 * k
    data = np.zeros((W, W, len(shares[0])), np.uint8)
    v = np.frombuffer(b"".join(shares), np.uint8).reshape(W, -1)
    if axis == Row:
        data[i] = v
    else:
        data[:, i] = v
    failed, root = Trees(k, tree).root(data, axis, i)
    if failed:
        return TREE
    if root != committed:
        return ROOT
    return 0 if oracle.encode(list(shares[:k])) == list(shares[k:]) else ENCODING


def is_byzantine(shares, axis, i, committed, k, tree="default"):
    """The validity predicate, independent of any schedule: at least k shares are present,
    and oracle decoding of them gives a vector whose tree fails, or whose root differs from
    the committed one, or whose parity is not the encoding of its first half."""
    if sum(x is not None for x in shares) < k:
        return False
    full = list(shares) if all(x is not None for x in shares) else oracle.decode(list(shares))
    return vector_reason(full, axis, i, committed, k, tree) != 0


# ---- the model -----------------------------------------------------------------------
class Outcome:
    """status, sweeps, decoded_vectors, missing; axis, index, round, reason;
    checked_vectors, hashed_cells; presence ([W][W] bool, final); shares (the named vector's
    cells under the final presence, None where absent, or None); passed (set of (axis,
    index) that passed a check)."""

    def stats(self):
        return self.status, self.sweeps, self.decoded_vectors, self.missing

    def check(self):
        return self.axis, self.index, self.round, self.reason, self.checked_vectors, self.hashed_cells


def model(square, pres, rr, cr, k, tree="default"):
    """square: [W][W][S] uint8 (only the given cells are read), pres: [W][W] bool, rr / cr:
    the committed roots."""
    W = 2 * k
    data = np.array(square, np.uint8)
    p = np.array(pres, bool)
    data[~p] = 0
    trees = Trees(k, tree)
    checked = np.zeros((2, W), bool)
    recorded = np.zeros((W, W), bool)
    out = Outcome()
    out.status, out.sweeps, out.decoded_vectors = None, 0, 0
    out.axis = out.index = out.round = out.reason = out.checked_vectors = 0
    out.shares, out.passed = None, set()

    def vec(axis, i):
        return [(data[i, q] if axis == Row else data[q, i]).tobytes() for q in range(W)]

    def run_stage(vectors, rnd):
        """Checks [(axis, index)]; True when one failed (the lowest (index, axis))."""
        if not vectors:
            return False
        for a, i in vectors:
            checked[a, i] = True
            trees.record(data, a, i)
            if a == Row:
                recorded[i, :] = True
            else:
                recorded[:, i] = True
        out.checked_vectors += len(vectors)
        failures = []
        for a, i in vectors:
            failed, root = trees.root(data, a, i)
            v = vec(a, i)
            reason = TREE if failed else ROOT if root != (rr, cr)[a][i] else \
                0 if oracle.encode(v[:k]) == v[k:] else ENCODING
            if reason:
                failures.append((i, a, reason))
            else:
                out.passed.add((a, i))
        if not failures:
            return False
        i, a, reason = min(failures)
        out.status, out.axis, out.index, out.round, out.reason = BYZANTINE, a, i, rnd, reason
        return True

    def finish():
        out.missing = int((~p).sum())
        out.presence = p.copy()
        out.hashed_cells = int(recorded.sum())
        if out.status == BYZANTINE:
            a, i = out.axis, out.index
            out.shares = [(data[i, q] if a == Row else data[q, i]).tobytes() if (p[i, q] if a == Row else p[q, i])
                          else None for q in range(W)]
        return out

    if run_stage(P.RC.complete_vectors(p), 0):
        return finish()
    while True:
        progress = False
        for axis in (Row, Col):
            have = p.sum(axis=1 if axis == Row else 0)
            todo = [int(i) for i in np.flatnonzero((have >= k) & (have < W))]
            if not todo:
                continue
            progress = True
            out.sweeps += 1
            out.decoded_vectors += len(todo)
            after = p.copy()  # the marks the next plan would apply
            for i in todo:
                on = p[i] if axis == Row else p[:, i]
                full = oracle.decode([s if on[q] else None for q, s in enumerate(vec(axis, i))])
                for q in np.flatnonzero(~on):
                    cell = np.frombuffer(full[q], np.uint8)
                    if axis == Row:
                        data[i, q] = cell
                    else:
                        data[q, i] = cell
                if axis == Row:
                    after[i, :] = True
                else:
                    after[:, i] = True
            if run_stage([(axis, i) for i in todo], out.sweeps):
                return finish()
            other = 1 - axis
            done = after.all(axis=1 if other == Row else 0)
            p = after  # stage 1 was clean: the decoded vectors passed, their cells count from here on
            if run_stage([(other, int(i)) for i in np.flatnonzero(done & ~checked[other])], out.sweeps):
                return finish()
        if not progress:
            break
    out.status = OK if p.all() else STUCK
    return finish()


# ---- squares -------------------------------------------------------------------------
def roots_of(k, tree="default"):
    return P.square(k, 64, tree)


@functools.lru_cache(maxsize=None)
def late_culprit(k, tree="default", min_round=3, S=64):
    """(square, presence, rr, cr, outcome): the avalanche map at k on its valid square of S-byte
    shares with one given cell altered (one byte, past the namespace) under the original roots -- the
    first seed in 0..255 (the seed picks the cell) for which the model names a vector in
    round >= min_round."""
    valid, rr, cr = P.square_for("avalanche", k, S, tree)
    pres = np.array(P.presence("avalanche", k), bool)
    given = np.flatnonzero(pres.reshape(-1))
    W = 2 * k
    for seed in range(256):
        cell = int(given[int(oracle.splitmix64_bytes(8, seed=0x1A7E0000 + k * 256 + seed).view(np.uint64)[0] % given.size)])
        sq = np.array(valid)
        sq[cell // W, cell % W, 40] ^= 0x5A
        out = model(sq, pres, rr, cr, k, tree)
        if out.status == BYZANTINE and out.round >= min_round:
            return D.given(sq, pres), pres, rr, cr, out
    raise AssertionError("no late culprit below seed 256 at k = %d" % k)


@functools.lru_cache(maxsize=None)
def stage_order(k, tree="default"):
    """(square, presence, rr, cr): k cells of every row given (no vector complete), the
    first given cell of row W - 1 altered under the original roots.  The row pass decodes
    row W - 1 to another codeword -- wrong in its k rebuilt cells, so its root fails in
    stage 1 -- and completes every column, k + 1 of which now hold a wrong cell and have a
    lower index than the row."""
    valid, rr, cr = P.square(k, 64, tree)
    W = 2 * k
    pres = RC.erase(W, k, 0x57A6E + k)
    sq = np.array(valid)
    sq[W - 1, int(np.flatnonzero(pres[W - 1])[0]), 40] ^= 0x5A
    return D.given(sq, pres), pres, rr, cr


# ---- the device call -----------------------------------------------------------------
class Checked:
    def __init__(self, res, chk, square, presence, shares, present):
        self.status, self.sweeps, self.decoded_vectors, self.missing = res.status, res.sweeps, res.decoded_vectors, res.missing
        self.axis, self.index, self.round, self.reason = chk.axis, chk.index, chk.round, chk.reason
        self.checked_vectors, self.hashed_cells = chk.checked_vectors, chk.hashed_cells
        self.square, self.presence = square, presence
        self.shares = None
        if res.status == BYZANTINE:
            self.shares = [shares[q].tobytes() if present[q] else None for q in range(len(present))]

    def stats(self):
        return self.status, self.sweeps, self.decoded_vectors, self.missing

    def check(self):
        return self.axis, self.index, self.round, self.reason, self.checked_vectors, self.hashed_cells


def repair_checked(lib, squares, presences, roots, k, S, nmt=None, table=None, stream=None):
    """One rsm_repair_squares_checked_dev over the batch, operands as repair_dev_calls.repair
    (squares between guard bands, absent cells D.FILL; table: the roots as bytes instead of
    `roots`), then one rsm_vectors_gather_dev of the named vectors.  Given cells must come
    back byte-identical with their presence bytes, the bands intact.  One Checked per square."""
    ctx = R.device_context(0)
    count, W = len(squares), 2 * k
    pp = ctypes.byref(nmt) if nmt is not None else None
    batch = np.ascontiguousarray(np.stack(squares))
    pres = np.ascontiguousarray(np.stack(presences)).astype(np.uint8)
    assert batch.shape == (count, W, W, S) and pres.shape == (count, W, W)
    nwork = int(lib.rsm_repair_checked_work_bytes(k, S, count, pp))
    assert nwork > 0
    table = D.roots_table(roots) if table is None else table
    assert table.size == count * 2 * W * (32 if nmt is None else 2 * nmt.namespace_size + 32)
    d_eds, d_pres, d_work = Guarded(batch.nbytes, 0, 21), Guarded(pres.nbytes, 0, 22), Guarded(nwork, 0, 23)
    d_roots = R.DeviceBuffer(table.size)
    extra = []
    try:
        d_eds.buf.upload(batch.reshape(-1), d_eds.front)
        d_pres.buf.upload(pres.reshape(-1), d_pres.front)
        d_roots.upload(table)
        res, chk = (R.RepairResult * count)(), (R.RepairCheck * count)()
        R._check(lib.rsm_repair_squares_checked_dev(ctx, d_eds.ptr, d_pres.ptr, k, S, count, pp, d_roots.ptr, d_work.ptr,
                                                    res, chk, stream))
        bad = [s for s in range(count) if res[s].status == BYZANTINE]
        shares = present = None
        if bad:
            refs = (R.RootRef * len(bad))(*[R.RootRef(s, chk[s].axis, chk[s].index) for s in bad])
            d_sh, d_pr = Guarded(len(bad) * W * S, 0, 24), Guarded(len(bad) * W, 5, 25)
            extra += [d_sh, d_pr]
            R._check(lib.rsm_vectors_gather_dev(ctx, d_eds.ptr, d_pres.ptr, k, S, count, refs, len(bad), d_sh.ptr, d_pr.ptr,
                                                stream))
            R._check(lib.rsm_stream_check(ctx, stream))
            shares = d_sh.result().reshape(len(bad), W, S).copy()
            present = d_pr.result().reshape(len(bad), W).copy()
        got = d_eds.result().reshape(count, W, W, S).copy()
        got_pres = d_pres.result().reshape(count, W, W).copy()
        d_work.result()
    finally:
        for b in [d_eds, d_pres, d_work, d_roots] + extra:
            b.free()
    out = []
    for s in range(count):
        m = np.asarray(presences[s], bool)
        assert np.array_equal(got[s][m], batch[s][m]), "a given cell of square %d was written" % s
        assert got_pres[s][m].all(), "a given cell of square %d lost its presence byte" % s
        j = bad.index(s) if s in bad else None
        out.append(Checked(res[s], chk[s], got[s], got_pres[s], None if j is None else shares[j],
                           None if j is None else present[j]))
    return out


def assert_equals_model(got, want, where=""):
    """A device outcome against the model's: status, counters, check record, final presence,
    the named vector's shares."""
    assert got.stats() == want.stats(), (where, got.stats(), want.stats())
    assert got.check() == want.check(), (where, got.check(), want.check())
    assert np.array_equal(got.presence != 0, want.presence), where
    assert got.shares == want.shares, where
