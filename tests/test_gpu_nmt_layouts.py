"""GPU: the namespaced-Merkle-tree kernels (kernels_nmt.hip) on squares whose namespaces
have structure -- repeats, compares that only a late byte decides, quadrant-0 cells
carrying 0xFF.. and the namespace just below it (tests/nmt_layouts.py) -- where every
other NMT test draws them from uniform random bytes.  Every case compares the full 2W
status vector of every square, and the root of every tree the oracle (oracle/nmt.py)
does not fail, with nmt_layouts.expected(); the set of failing trees is worked out
from the layout and its size asserted.  The host tree meets the same squares in
tests/test_nmt_layouts_cpu.py."""
import ctypes
import functools

import numpy as np
import pytest

import nmt_layouts as NL
import proof_verify as V
import rsmt2d_amd as R
from test_gpu_proofs import Dev, all_samples, host_record, picked_samples

pytestmark = pytest.mark.gpu

S = 64
NS = 29


def device_roots(lib, batch, k, ns, ignore_max=True, single=False, offset=0):
    """(status uint32[count][2W], roots uint8[count][2W][2 ns + 32]) of a [count][W][W][S]
    batch: rsm_nmt_roots_dev (`single`) or rsm_nmt_roots_squares_dev, the squares `offset`
    bytes into their device buffer; the status words start out as 0xFFFFFFFF."""
    count, W, _, S_ = batch.shape
    RL = 2 * ns + 32
    ctx = R.device_context(0)
    bufs = [R.DeviceBuffer(batch.nbytes + 16), R.DeviceBuffer(count * 2 * W * RL), R.DeviceBuffer(count * 2 * W * 4)]
    d, roots, status = bufs
    try:
        d.upload(np.ascontiguousarray(batch).reshape(-1), offset)
        status.upload(np.full(count * 2 * W, 0xFFFFFFFF, np.uint32).view(np.uint8))
        p = R.NmtParams(ns, 1 if ignore_max else 0, k)
        if single:
            assert count == 1
            R._check(lib.rsm_nmt_roots_dev(ctx, d.ptr + offset, W, S_, ctypes.byref(p), roots.ptr, status.ptr, None))
        else:
            R._check(lib.rsm_nmt_roots_squares_dev(ctx, d.ptr + offset, W, S_, count, ctypes.byref(p), roots.ptr,
                                                   status.ptr, None))
        R._check(lib.rsm_sync(ctx))
        got = roots.download().reshape(count, 2 * W, RL)
        st = status.download().view(np.uint32).reshape(count, 2 * W).copy()
    finally:
        for b in bufs:
            b.free()
    return st, got


@functools.lru_cache(maxsize=None)
def case(k, ns, layout, seed, inv=None, ignore_max=True):
    """(square, oracle status, oracle roots) of a layout, with `inv` = (a, b) swapped or
    ("max", cell) set to 0xFF..; computed once."""
    sq = NL.square(k, ns, S, layout, seed)
    if inv is not None:
        sq = NL.plant_max(sq, inv[1], ns) if inv[0] == "max" else NL.invert(sq, inv[0], inv[1], ns)
    status, roots = NL.expected(sq, k, ns, ignore_max)
    assert (status == NL.decreasing_status(sq, k, ns)).all()
    sq.setflags(write=False)
    status.setflags(write=False)
    return sq, status, roots


def compare(st, got, status, roots, failing, label):
    """One square: the whole status vector; every root the oracle has (a list, or a
    {tree: root} sample of a large square)."""
    assert set(int(t) for t in np.nonzero(status)[0]) == set(failing), label
    assert (st == status).all(), (label, np.nonzero(st != status)[0][:8], st[st != status][:8])
    items = roots.items() if isinstance(roots, dict) else enumerate(roots)
    n = 0
    for t, r in items:
        if r is not None:
            assert bytes(got[t]) == r, (label, t)
            n += 1
    assert n == len(roots) - len(set(failing))  # nothing skipped but the failing trees


def run_cases(lib, k, ns, cases, ignore_max=True, single=True, batched=True, offset=0):
    """cases: [(layout, seed, inv, failing trees)].  Each as one square through
    rsm_nmt_roots_dev; then in batches of 3 through rsm_nmt_roots_squares_dev, the case
    in the middle between two other cases' valid squares, which must come out untouched."""
    built = [case(k, ns, lay, seed, inv, ignore_max) for lay, seed, inv, _f in cases]
    if single:
        for (lay, seed, inv, failing), (sq, status, roots) in zip(cases, built):
            st, got = device_roots(lib, sq[None], k, ns, ignore_max, single=True, offset=offset)
            compare(st[0], got[0], status, roots, failing, (lay, inv, "single"))
    if batched:
        n = len(cases)
        for i, ((lay, seed, inv, failing), (sq, status, roots)) in enumerate(zip(cases, built)):
            lo, hi = cases[(i + 1) % n], cases[(i + 2) % n]
            side = [case(k, ns, c[0], c[1], None, ignore_max) for c in (lo, hi)]
            batch = np.stack([side[0][0], sq, side[1][0]])
            st, got = device_roots(lib, batch, k, ns, ignore_max, offset=offset)
            compare(st[1], got[1], status, roots, failing, (lay, inv, "middle of 3"))
            compare(st[0], got[0], side[0][1], side[0][2], (), (lo[0], "first of 3"))
            compare(st[2], got[2], side[1][1], side[1][2], (), (hi[0], "last of 3"))


@pytest.mark.parametrize("k", [3, 4, 8])
def test_valid_layouts(lib, k):
    """Every layout at ns = 29: one square (rsm_nmt_roots_dev) and batches of three
    different layouts (rsm_nmt_roots_squares_dev); status all zero, every root the oracle's."""
    run_cases(lib, k, NS, [(lay, 20 + k, None, ()) for lay in NL.all_layouts(NS)])


@pytest.mark.parametrize("ns", [1, 3, 8, 30, 32])
def test_valid_layouts_other_namespace_sizes(lib, ns):
    """The generic leaf kernel and nmt_tree_kernel (any ns but 29)."""
    run_cases(lib, 4, ns, [(lay, 30 + ns, None, ()) for lay in NL.all_layouts(ns)])


@pytest.mark.parametrize("k", [4, 8])
def test_unaligned_square(lib, k):
    """A device pointer 4 bytes off 16-byte alignment: the word-load leaf kernel feeds the
    wave kernel."""
    lays = ["single", "runs", "carry", "max_tail", "near_max", "ladder:28", "ladder:27", "ladder:3"]
    run_cases(lib, k, NS, [(lay, 40 + k, None, ()) for lay in lays], offset=4)
    inv = [("ladder:28", 40 + k, ((1, 1), (1, 2)), (1,)), ("ladder:27", 40 + k, (0, 1), range(2 * k, 3 * k)),
           ("ladder:28", 40 + k, ("max", (1, 2)), (1, 2 * k + 2))]
    run_cases(lib, k, NS, inv + [("single", 40 + k, None, ())], offset=4)


@pytest.mark.parametrize("ns", [29, 8])
@pytest.mark.parametrize("k", [4, 8])
def test_ignore_max_namespace_off(lib, ns, k):
    """ignore_max_namespace = 0: every quadrant-0 row and column root reports max 0xFF.."""
    cases = [(lay, 50 + k, None, ()) for lay in ("max_tail", "runs", "near_max")]
    run_cases(lib, k, ns, cases, ignore_max=False)
    W = 2 * k
    for lay, seed, _inv, _f in cases:
        sq, _status, roots = case(k, ns, lay, seed, None, False)
        on = case(k, ns, lay, seed, None, True)[2]
        assert all(r[ns:2 * ns] == b"\xff" * ns for r in roots)  # what the device roots were just held to
        assert any(on[t][ns:2 * ns] != b"\xff" * ns for t in range(k)) and on[:k] != roots[:k]
        st, got = device_roots(lib, sq[None], k, ns, ignore_max=True, single=True)  # and 1 still gives the other roots
        compare(st[0], got[0], np.zeros(2 * W, np.uint32), on, (), (lay, "ignore_max on"))


def test_inversion_only_byte_p_decides(lib):
    """Strict ladder on byte p with (1, 1) <-> (1, 2) swapped: row 1 fails and nothing else,
    for every p -- a compare that drops or misorders any byte misses one of them."""
    k = 4
    rows = [("ladder:%d" % p, 60, ((1, 1), (1, 2)), (1,)) for p in range(NS)]
    run_cases(lib, k, NS, rows)
    # the same along a column, where the rows through the two cells fail with it
    cols = []
    for p in range(NS):
        failing = NL.col_swap_failing(case(k, NS, "ladder:%d" % p, 60)[0], k, NS, 1, 2)
        assert failing == {2 * k + 2, 1, 2}
        cols.append(("ladder:%d" % p, 60, ((1, 2), (2, 2)), tuple(failing)))
    run_cases(lib, k, NS, cols, batched=False)


@pytest.mark.parametrize("k", [8, 3, 7])
def test_inversion_positions(lib, k):
    """Strict ladder on the last byte, (r, c) <-> (r, c + 1) for c in {0, 1, 2, 3, 4, k - 2},
    r in {0, k - 1}: the leaf pairs (2j, 2j+1), (2j+1, 2j+2), (4j+3, 4j+4) and the last
    quadrant-0 pair; two whole rows swapped: every quadrant-0 column, no row.  And the first
    cell of each pair set to 0xFF..: IgnoreMaxNamespace keeps that one out of its parent's
    max, so the sibling-order checks of the upper levels (which catch every other
    inversion a second time) pass, and only the push-order check between the pair is left
    -- in the F2 form the extra load of leaf 4j + 4, in the others that of leaf 2j + 2.
    k = 8: the F2 form (W % 4 == 0); k = 3, 7: the other.  One square, and the middle one
    of three."""
    W = 2 * k
    lay, seed = "ladder:%d" % (NS - 1), 70
    base = case(k, NS, lay, seed)[0]
    cases = []
    for (r, c), b in NL.position_swaps(k):
        failing = NL.row_swap_failing(base, k, NS, r, c)
        assert failing == {r}
        cases.append((lay, seed, ((r, c), b), (r,)))
        cases.append((lay, seed, ((c, r), (c + 1, r)), tuple(NL.col_swap_failing(base, k, NS, c, r))))
        for cell in ((r, c), (c, r)):
            failing = NL.plant_max_failing(base, k, NS, *cell)
            assert failing and failing <= {cell[0], W + cell[1]}
            cases.append((lay, seed, ("max", cell), tuple(failing)))
    for r in sorted({0, k - 2}):
        cases.append((lay, seed, (r, r + 1), tuple(range(W, W + k))))
    assert len(cases) == {8: 50, 7: 50, 3: 18}[k]
    run_cases(lib, k, NS, cases)


@pytest.mark.parametrize("ns", [1, 3, 8, 30, 32])
def test_inversions_other_namespace_sizes(lib, ns):
    """nmt_tree_kernel's own push-order and sibling checks (any ns but 29): the last byte
    alone decides; a carry; 0xFF.. ahead of smaller namespaces at the pairs (2j, 2j+1) and
    (2j+1, 2j+2)."""
    k, seed = 4, 80 + ns
    W = 2 * k
    cases = []
    for lay in ("ladder:%d" % (ns - 1), "carry"):
        base = case(k, ns, lay, seed)[0]
        cases.append((lay, seed, ((1, 1), (1, 2)), tuple(NL.row_swap_failing(base, k, ns, 1, 1))))
        cases.append((lay, seed, ((1, 2), (2, 2)), tuple(NL.col_swap_failing(base, k, ns, 1, 2))))
        for cell in ((1, 1), (0, 2), (2, 0)):
            failing = NL.plant_max_failing(base, k, ns, *cell)
            assert failing == {cell[0], W + cell[1]}
            cases.append((lay, seed, ("max", cell), tuple(failing)))
    run_cases(lib, k, ns, cases)
    run_cases(lib, k, ns, cases[:5], ignore_max=False, batched=False)


# --- kernel forms ---------------------------------------------------------------------------
def wave_form(W, count):
    """(TPW, WPB, F2) of the nmt_tree_wave_kernel<29, ...> that launch_nmt_tree_wave picks,
    restated from nmt_tree_shape: a node is 2 * 8 + 8 words; a tree holds W/4 (F2) or
    ceil(W/2) nodes; a wave TPW trees and a spare node; a batch takes two trees per wave in
    the largest of 4 or 2 waves whose LDS stays within 52 KiB, one square one tree per wave."""
    f2 = W % 4 == 0
    wave_words = lambda tpw: (tpw * (W // 4 if f2 else (W + 1) // 2) + 1) * 24
    if count > 1:
        for wpb in (4, 2):
            if wpb * wave_words(2) * 4 <= 52 * 1024:
                return 2, wpb, f2
    return 1, 4, f2


def planted(k, c, axis, seed, kind="swap"):
    """A `runs` square with one inversion between positions c and c + 1 of a row (axis 0)
    or column (axis 1) where the run changes there; or (kind "max") a ladder square with
    0xFF.. at position c of row / column 1; (square, failing trees)."""
    if kind == "max":
        base = NL.square(k, NS, S, "ladder:%d" % (NS - 1), seed)
        cell = (1, c) if axis == 0 else (c, 1)
        return NL.plant_max(base, cell, NS), NL.plant_max_failing(base, k, NS, *cell)
    for s in range(seed, seed + 64):
        base = NL.square(k, NS, S, "runs", s)
        for line in range(k):
            if NL.first_step(base, k, NS, line, c, axis) == c:
                if axis == 0:
                    return NL.invert(base, (line, c), (line, c + 1), NS), NL.row_swap_failing(base, k, NS, line, c)
                return NL.invert(base, (c, line), (c + 1, line), NS), NL.col_swap_failing(base, k, NS, c, line)
    raise AssertionError("no run ends at %d" % c)


FORMS = [
    # k, count, (row position, column position) of the inversions, the form
    (67, 1, (65, 32), (1, 4, False)),
    (128, 1, (63, 126), (1, 4, True)),
    (67, 2, (33, 65), (2, 4, False)),
    (128, 2, (63, 126), (2, 4, True)),
    (131, 2, (127, 128), (2, 2, False)),
    (131, 2, (128, 127), (2, 2, False)),
    (131, 1, (127, 128), (1, 4, False)),
    (258, 2, (255, 255), (2, 2, True)),
    (258, 1, (255, 255), (1, 4, True)),
]


@pytest.mark.parametrize("k,count,at,form", FORMS)
def test_kernel_forms_and_lane_boundaries(lib, k, count, at, form):
    """Each nmt_tree_wave_kernel<29, TPW, WPB, F2> on `runs` squares with one planted
    inversion per square, once in a row and once in a column; then the same positions
    with 0xFF.. ahead of a smaller namespace on a ladder square (which only the push-order
    loads see: test_inversion_positions).  From nmt_tree_shape and launch_nmt_roots
    (W = 2k; F2 = W % 4 == 0; words of LDS per workgroup in brackets):

        one square, any W            -> <1, 4, F2>
        batch, k = 67   (W = 134)    -> <2, 4, false>   [4 * (2 * 67 + 1) * 24 = 12960 <= 13312]
        batch, k = 128  (W = 256)    -> <2, 4, true>    [4 * (2 * 64 + 1) * 24 = 12384]
        batch, k = 131  (W = 262)    -> <2, 2, false>   [4 waves: 25248 > 13312; 2 waves: 12624]
        batch, k = 258  (W = 516)    -> <2, 2, true>    [4 waves: 24864; 2 waves: 12432]

    A pass gives 64 consecutive level nodes to a wave's lanes.  In the F2 form lane 63 of the
    first pass hashes leaves 252..255 and loads leaf 256 for the push order (k = 258:
    255/256); in the other form lane 63 hashes leaves 126, 127 and loads 128, and the next
    pass starts at 128, 129 (k = 131: 127/128 and 128/129).  Status by the adjacent-pair
    predicate over all 2W trees; the oracle on the failing trees (it must raise), and its
    roots of the edge trees of both halves of both axes and of 16 seeded trees per square."""
    W = 2 * k
    assert wave_form(W, count) == form
    for kind in ("swap", "max"):  # "max": 0xFF.. before smaller namespaces, which only the push-order loads see
        squares, wants = [], []
        for axis in (0, 1):
            sq, failing = planted(k, at[axis], axis, 100 + k, kind)
            squares.append(sq)
            wants.append((failing,) + NL.expected_sampled(sq, k, NS, True, others=16, seed=k + axis))
        if count == 1:  # one launch holds one square
            outs = [device_roots(lib, s[None], k, NS, single=True) for s in squares]
            outs = [(st[0], got[0]) for st, got in outs]
        else:
            st, got = device_roots(lib, np.stack(squares), k, NS)
            outs = [(st[q], got[q]) for q in range(count)]
        for (st, got), (failing, status, roots) in zip(outs, wants):
            assert 1 <= len(failing) <= 3
            compare(st, got, status, roots, failing, (k, count, at, kind))


def test_forms_table_is_covered():
    assert {f for *_x, f in FORMS} == {(t, w, f2) for (t, w) in ((1, 4), (2, 4), (2, 2)) for f2 in (False, True)}


# --- node store -----------------------------------------------------------------------------
def node_cases(k, ns):
    seed = 200 + k + ns
    runs = NL.square(k, ns, S, "runs", seed)
    row, r = next((line, NL.first_step(runs, k, ns, line, 0, 0)) for line in range(1, k)
                  if NL.first_step(runs, k, ns, line, 0, 0) is not None)
    c = NL.first_step(runs, k, ns, k - 1, 0, 1)
    assert c is not None
    return [("single", seed, None, ()), ("runs", seed, None, ()), ("max_tail", seed, None, ()),
            ("runs", seed, ((row, r), (row, r + 1)), tuple(NL.row_swap_failing(runs, k, ns, row, r))),
            ("runs", seed, ((c, k - 1), (c + 1, k - 1)), tuple(NL.col_swap_failing(runs, k, ns, c, k - 1))),
            # 0xFF.. ahead of smaller namespaces, at the pairs (2j+1, 2j+2) and the last one of quadrant 0
            ("runs", seed, ("max", (1, 1)), tuple(NL.plant_max_failing(runs, k, ns, 1, 1))),
            ("runs", seed, ("max", (0, k - 2)), tuple(NL.plant_max_failing(runs, k, ns, 0, k - 2)))]


@pytest.mark.parametrize("k", [4, 35])
@pytest.mark.parametrize("ns", [29, 8])
def test_node_store(lib, ns, k):
    """rsm_proof_nodes_dev / rsm_proofs_dev (nmt_nodes_kernel<29>, <0>): statuses and roots
    against the oracle, every sampled record byte-equal to the host restatement and
    verified against the oracle root of its tree; only the oracle's failing trees skipped."""
    W = 2 * k
    cases = node_cases(k, ns)
    built = [case(k, ns, lay, seed, inv) for lay, seed, inv, _f in cases]
    batch = np.stack([b[0] for b in built])
    count = len(cases)
    p = R.NmtParams(ns, 1, k)
    samples = all_samples(W, count) if W <= 24 else sorted(
        {(q, a, i, pos) for q in range(count) for (_q, a, i, pos) in picked_samples(W, W + ns + q, n=96)})
    dev = Dev(lib, batch, p, samples)
    st = dev.status.reshape(count, 2 * W)
    got = np.frombuffer(dev.roots, np.uint8).reshape(count, 2 * W, dev.nl)
    assert (dev.status == dev.status_ref).all()
    for q, ((lay, _seed, inv, failing), (_sq, status, roots)) in enumerate(zip(cases, built)):
        compare(st[q], got[q], status, roots, failing, (lay, inv, "node store"))
    checked = 0
    for i, (q, a, idx, pos) in enumerate(samples):
        cell = batch[q, idx, pos] if a == 0 else batch[q, pos, idx]
        assert dev.share(i) == cell.tobytes()
        root = built[q][2][a * W + idx]
        if root is None:
            continue
        vec = NL.tree_leaves(batch[q], a * W + idx)
        rec = dev.record(i)
        nodes, mask = V.parse_record(rec, dev.nl)
        assert len(nodes) == V.level_count(W, pos)
        assert V.verify_nmt(root, vec[pos], nodes, mask, pos, idx, k, ns), (q, a, idx, pos)
        if W <= 24 or i % 8 == 0:
            assert rec == host_record(lib, p, vec, idx, pos), (q, a, idx, pos)
        checked += 1
    skipped = {(q, a * W + idx) for (q, a, idx, _p) in samples if built[q][2][a * W + idx] is None}
    assert skipped <= {(q, t) for q, c_ in enumerate(cases) for t in c_[3]} and checked >= len(samples) * 3 // 4


# --- end to end -----------------------------------------------------------------------------
def test_eds_last_byte_inversion_end_to_end(lib):
    """An ODS whose only defect is (2, 1) <-> (2, 2) of a ladder on the last namespace byte:
    RowRoots fails on tree 2, ColRoots does what the oracle says, and Repair from that
    complete row alone reports ErrByzantineData{Row, 2}."""
    k, ns = 4, NS
    W = 2 * k
    codec = R.NewLeoRSCodec()
    ctor = R.newErasuredNamespacedMerkleTreeConstructor(k, ns)
    good = NL.square(k, ns, S, "ladder:%d" % (ns - 1), 300)
    bad = NL.invert(good, (2, 1), (2, 2), ns)
    assert (good[..., :ns - 1] == bad[..., :ns - 1]).all()  # the last byte alone tells the two apart
    flat = lambda sq: [sq[r, c].tobytes() for r in range(k) for c in range(k)]
    header = R.ComputeExtendedDataSquare(flat(good), codec, ctor)
    rr, cr = header.RowRoots(), header.ColRoots()
    eds = R.ComputeExtendedDataSquare(flat(bad), codec, ctor)
    full = np.frombuffer(b"".join(eds.Flattened()), np.uint8).reshape(W, W, S)
    status, roots = NL.expected(full, k, ns)
    assert set(np.nonzero(status)[0]) == {2}
    with pytest.raises(R.RSMError, match=r"root 2 \(") as ei:
        eds.RowRoots()
    assert ei.value.code == R.RSM_ETREE
    assert eds.ColRoots() == roots[W:]
    cells = eds.Flattened()
    only_row = [cells[i] if i // W == 2 else None for i in range(W * W)]
    rep = R.ImportExtendedDataSquare(only_row, codec, ctor)
    with pytest.raises(R.ErrByzantineData) as ei:
        rep.Repair(rr, cr)
    assert ei.value.Axis == R.Row and ei.value.Index == 2
