"""CPU: blob share commitments -- the host helpers (rsm_subtree_width, rsm_subtree_sizes),
the two host restatements (rsm_blob_commitment from the blob's own runs,
rsm_square_commitment from the row trees' levels) against the hashlib model
(tests/commitments.py), and every argument error of the two device entry points, which
return before a device is selected (`ctx` is the address of a zeroed buffer, device
pointers are small integers never dereferenced: tests/test_dev_entry_errors_cpu.py)."""
import ctypes

import numpy as np
import pytest

import commitments as C
import rsmt2d_amd as R

S = 64


def params(ns, ig=True, k=1):
    return R.NmtParams(ns, int(ig), k)


def blob_commitment(lib, p, shares, t):
    out, st = ctypes.create_string_buffer(32), ctypes.c_uint32(99)
    rc = lib.rsm_blob_commitment(ctypes.byref(p), b"".join(shares), len(shares), len(shares[0]), t, out, ctypes.byref(st))
    return rc, out.raw, int(st.value)


def square_commitment(lib, p, sq, k, start, length, t, ods=False, want_roots=0):
    out, st = ctypes.create_string_buffer(32), ctypes.c_uint32(99)
    nl = 2 * p.namespace_size + 32
    roots = ctypes.create_string_buffer(max(want_roots * nl, 1))
    keep = None
    if ods:
        keep, ptrs, _ = R._bufs([sq[r, c].tobytes() for r in range(k) for c in range(k)])
        rc = lib.rsm_square_commitment(ctypes.byref(p), ptrs, None, k, sq.shape[2], start, length, t, out,
                                       roots if want_roots else None, ctypes.byref(st))
    else:
        flat = np.ascontiguousarray(sq)
        rc = lib.rsm_square_commitment(ctypes.byref(p), None, flat.ctypes.data, k, sq.shape[2], start, length, t, out,
                                       roots if want_roots else None, ctypes.byref(st))
    return rc, out.raw, int(st.value), [roots.raw[i * nl:(i + 1) * nl] for i in range(want_roots)]


# ---- the model itself -------------------------------------------------------------------
def test_model_matches_the_derived_values():
    for (n, t), w in C.WIDTHS.items():
        assert C.width(n, t) == w, (n, t)
    for (n, w), z in C.SIZES.items():
        assert C.sizes(n, w) == z, (n, w)


@pytest.mark.parametrize("k,ns,ig", [(4, 8, True), (8, 29, True), (4, 29, False)])
def test_model_statements_agree(k, ns, ig):
    sq = C.make_square(k, S, ns, 1, tail=3)
    for t in (1, 2, 64):
        levels = {}
        for start, n in C.aligned_blobs(k, t):
            sh = C.ods_shares(sq, k, start, n)
            assert C.commitment(sh, ns, t, ig) == C.square_commitment(sq, k, ns, start, n, t, ig, levels), (t, start, n)


# ---- the helpers ------------------------------------------------------------------------
def test_subtree_width_and_sizes(lib):
    for (n, t), w in C.WIDTHS.items():
        assert lib.rsm_subtree_width(n, t) == w
    for t in (1, 2, 3, 64, 1 << 20):
        for n in range(1, 301):
            w = C.width(n, t)
            assert lib.rsm_subtree_width(n, t) == w, (n, t)
            assert R.SubTreeWidth(n, t) == w
            assert R.MerkleMountainRangeSizes(n, w) == C.sizes(n, w), (n, t)
    for (n, w), z in C.SIZES.items():
        assert R.MerkleMountainRangeSizes(n, w) == z
    assert lib.rsm_subtree_width(0, 64) == 0 and lib.rsm_subtree_width(5, 0) == 0
    assert lib.rsm_subtree_width(0xFFFFFFFF, 1) == 65536 and lib.rsm_subtree_width(0xFFFFFFFF, 0xFFFFFFFF) == 1


def test_subtree_sizes_errors(lib):
    m = ctypes.c_uint32(7)
    out = (ctypes.c_uint32 * 8)(*[9] * 8)
    assert lib.rsm_subtree_sizes(0, 4, out, 8, ctypes.byref(m)) == R.RSM_EINVAL
    assert lib.rsm_subtree_sizes(11, 0, out, 8, ctypes.byref(m)) == R.RSM_EINVAL
    assert lib.rsm_subtree_sizes(11, 3, out, 8, ctypes.byref(m)) == R.RSM_EINVAL
    assert lib.rsm_subtree_sizes(11, 4, out, 8, None) == R.RSM_EINVAL
    assert lib.rsm_subtree_sizes(11, 4, out, 3, ctypes.byref(m)) == R.RSM_EINVAL
    assert m.value == 4 and list(out) == [9] * 8  # the count is reported, nothing written
    assert lib.rsm_subtree_sizes(11, 4, None, 0, ctypes.byref(m)) == 0 and m.value == 4
    assert lib.rsm_subtree_sizes(11, 4, out, 4, ctypes.byref(m)) == 0 and list(out)[:5] == [4, 4, 2, 1, 9]


# ---- the restatements -------------------------------------------------------------------
@pytest.mark.parametrize("k,ns,ig", [(4, 1, True), (4, 8, True), (4, 29, True), (4, 32, True), (8, 29, True), (8, 8, False),
                                     (4, 29, False)])
def test_restatements_equal_both_model_statements(lib, k, ns, ig):
    """Every (start, len) of the square through rsm_blob_commitment; the aligned ones also
    through rsm_square_commitment (both square layouts), with its subtree roots.  The last
    shares carry 0xFF..: with ignore_max a run that ends in them keeps its left maximum."""
    sq = C.make_square(k, S, ns, 2, tail=k + 1)
    p = params(ns, ig, k)
    for t in (1, 2, 64):
        aligned = set(C.aligned_blobs(k, t))
        levels, by_shares = {}, {}
        for start, n in C.all_blobs(k):
            sh = C.ods_shares(sq, k, start, n)
            want = C.commitment(sh, ns, t, ig)
            assert blob_commitment(lib, p, sh, t) == (0, want, 0), (t, start, n)
            if (start, n) not in aligned:
                continue
            roots = C.square_subtree_roots(sq, k, ns, start, n, t, ig, levels)
            assert C.mth(roots) == want
            assert roots == C.subtree_roots(sh, ns, t, ig)
            got = square_commitment(lib, p, sq, k, start, n, t, want_roots=len(roots))
            assert got == (0, want, 0, roots), (t, start, n)
            if n % 5 == 0:
                assert square_commitment(lib, p, sq, k, start, n, t, ods=True)[:3] == (0, want, 0)


def test_ignore_max_namespace_shows_in_the_commitment(lib):
    k, ns = 4, 8
    sq = C.make_square(k, S, ns, 3, tail=5)
    sh = C.ods_shares(sq, k, 8, 8)  # ends in five 0xFF.. shares
    a = blob_commitment(lib, params(ns, True), sh, 2)
    b = blob_commitment(lib, params(ns, False), sh, 2)
    assert a == (0, C.commitment(sh, ns, 2, True), 0) and b == (0, C.commitment(sh, ns, 2, False), 0)
    assert a[1] != b[1]


def test_push_order_inside_a_run_and_across_a_boundary(lib):
    ns, t = 8, 2
    sq = C.make_square(4, S, ns, 4, distinct=16)
    sh = C.ods_shares(sq, 4, 0, 11)  # w = 4: runs [0, 4) [4, 8) [8, 10) [10, 11)
    assert C.runs(11, t) == [(0, 4), (4, 4), (8, 2), (10, 1)]
    p = params(ns)
    low, high = b"\x00" * ns, b"\xfe" * ns

    def with_name(i, name):
        out = list(sh)
        out[i] = name + out[i][ns:]
        return out

    for i, name in ((1, low), (5, low), (9, low), (2, high), (8, high)):  # inside a run: a later leaf is lower
        bad = with_name(i, name)
        with pytest.raises(C.OrderError):
            C.commitment(bad, ns, t)
        assert blob_commitment(lib, p, bad, t) == (0, b"\x00" * 32, R.RSM_COMMIT_ORDER), i
    for i, name in ((4, low), (8, low), (10, low), (3, high), (7, high), (9, high)):  # only across a boundary
        ok = with_name(i, name)
        assert blob_commitment(lib, p, ok, t) == (0, C.commitment(ok, ns, t), 0), i


def test_square_commitment_reports_a_failing_row(lib):
    k, ns, t = 4, 8, 1
    sq = C.make_square(k, S, ns, 5, distinct=16)
    sq[1, 2, :ns] = 0  # row 1 out of order
    p = params(ns, True, k)
    with pytest.raises(C.OrderError):
        C.square_commitment(sq, k, ns, 4, 2, t)
    assert square_commitment(lib, p, sq, k, 4, 2, t)[:3] == (0, b"\x00" * 32, R.RSM_COMMIT_TREE)   # within row 1
    assert square_commitment(lib, p, sq, k, 0, 12, t)[:3] == (0, b"\x00" * 32, R.RSM_COMMIT_TREE)  # through row 1
    for start, n in ((0, 4), (8, 8), (12, 1)):  # the other rows
        assert square_commitment(lib, p, sq, k, start, n, t)[:3] == (0, C.square_commitment(sq, k, ns, start, n, t), 0)


def test_restatement_argument_errors(lib):
    sq = C.make_square(4, S, 8, 6)
    sh = C.ods_shares(sq, 4, 0, 4)
    flat, out, st = b"".join(sh), ctypes.create_string_buffer(32), ctypes.c_uint32(0)
    p = params(8, True, 4)
    pr, sr = ctypes.byref(p), ctypes.byref(st)
    f = lib.rsm_blob_commitment
    assert f(None, flat, 4, S, 64, out, sr) == R.RSM_EINVAL
    assert f(pr, None, 4, S, 64, out, sr) == R.RSM_EINVAL
    assert f(pr, flat, 0, S, 64, out, sr) == R.RSM_EINVAL
    assert f(pr, flat, 4, S, 0, out, sr) == R.RSM_EINVAL
    assert f(pr, flat, 4, S, 64, None, sr) == R.RSM_EINVAL
    assert f(pr, flat, 4, S, 64, out, None) == R.RSM_EINVAL
    assert f(ctypes.byref(params(0)), flat, 4, S, 64, out, sr) == R.RSM_EINVAL
    assert f(ctypes.byref(params(33)), flat, 4, S, 64, out, sr) == R.RSM_EINVAL
    assert f(pr, flat, 4, 4, 64, out, sr) == R.RSM_ETREE
    g = lib.rsm_square_commitment
    eds = np.ascontiguousarray(sq).ctypes.data
    keep, ptrs, _ = R._bufs([sq[r, c].tobytes() for r in range(4) for c in range(4)])
    assert g(pr, None, eds, 4, S, 0, 4, 64, out, None, sr) == 0
    assert g(pr, None, None, 4, S, 0, 4, 64, out, None, sr) == R.RSM_EINVAL   # no square
    assert g(pr, ptrs, eds, 4, S, 0, 4, 64, out, None, sr) == R.RSM_EINVAL    # two squares
    assert g(pr, None, eds, 3, S, 0, 4, 64, out, None, sr) == R.RSM_EINVAL    # k no power of two
    assert g(pr, None, eds, 4, S, 0, 0, 64, out, None, sr) == R.RSM_EINVAL    # empty
    assert g(pr, None, eds, 4, S, 13, 4, 64, out, None, sr) == R.RSM_EINVAL   # past the ODS
    assert g(pr, None, eds, 4, S, 1, 4, 1, out, None, sr) == R.RSM_EINVAL     # start not a multiple of w = 2
    assert g(pr, None, eds, 4, S, 0, 4, 0, out, None, sr) == R.RSM_EINVAL     # threshold
    assert g(pr, None, eds, 4, 4, 0, 4, 64, out, None, sr) == R.RSM_ETREE
    ptrs[5] = None
    assert g(pr, ptrs, None, 4, S, 4, 2, 64, out, None, sr) == R.RSM_ETREE    # a nil share in a touched row


# ---- the square object on the host path (no context) ---------------------------------------
def imported(sq, k, ns):
    cells = [sq[r, c].tobytes() for r in range(2 * k) for c in range(2 * k)]
    return R.ImportExtendedDataSquare(cells, R.NewLeoRSCodec(), R.newErasuredNamespacedMerkleTreeConstructor(k, ns))


def test_square_object_on_the_host_path(lib):
    k, ns, t = 8, 29, 2
    sq = C.make_square(k, S, ns, 7, tail=4)
    eds = imported(sq, k, ns)
    levels = {}
    for start, n in C.aligned_blobs(k, t)[::11]:
        roots = C.square_subtree_roots(sq, k, ns, start, n, t, True, levels)
        assert eds.SubtreeRoots(start, n, t) == roots
        assert eds.Commitment(start, n, t) == C.mth(roots)
        assert R.CreateCommitment(C.ods_shares(sq, k, start, n), R.NmtParams(ns, 1, k), t, device=None) == C.mth(roots)
    eds.setCell(2 * k - 1, 2 * k - 1, None)  # a nil parity cell is no obstacle
    assert eds.Commitment(0, k * k, 64) == C.commitment(C.ods_shares(sq, k, 0, k * k), ns, 64)
    eds.setCell(3, 6, None)  # a nil quadrant-0 cell fails the blobs that touch its row
    assert eds.Commitment(0, 24, 64) == C.commitment(C.ods_shares(sq, k, 0, 24), ns, 64)
    for bad, code in (((24, 1), R.RSM_ETREE), ((0, 25), R.RSM_ETREE), ((1, 4), R.RSM_EINVAL), ((60, 5), R.RSM_EINVAL),
                      ((0, 0), R.RSM_EINVAL)):
        with pytest.raises(R.RSMError) as e:
            eds.Commitment(bad[0], bad[1], 2)
        assert e.value.code == code, bad
    with pytest.raises(R.RSMError) as e:
        eds.Commitment(0, 4, 0)
    assert e.value.code == R.RSM_EINVAL
    plain = R.ImportExtendedDataSquare([sq[r, c].tobytes() for r in range(2 * k) for c in range(2 * k)], R.NewLeoRSCodec(),
                                       R.NewDefaultTree)
    with pytest.raises(R.RSMError) as e:
        plain.Commitment(0, 4)
    assert e.value.code == R.RSM_EUNSUPPORTED


def test_square_object_reports_a_failing_row_per_blob(lib):
    k, ns, t = 4, 8, 1
    sq = C.make_square(k, S, ns, 5, distinct=16)
    sq[1, 2, :ns] = 0
    eds = imported(sq, k, ns)
    blobs = [(0, 0, 4), (0, 4, 2), (0, 0, 12), (0, 8, 8)]
    tf = eds._tree_fn
    keep, fn, user = R._tree_callback(tf)
    out, st = ctypes.create_string_buffer(32 * len(blobs)), (ctypes.c_uint32 * len(blobs))()
    arr = (R.BlobRef * len(blobs))(*[R.BlobRef(*b) for b in blobs])
    assert lib.rsm_eds_commitments(eds._h, fn, user, arr, len(blobs), t, out, st) == 0
    assert list(st) == [0, R.RSM_COMMIT_TREE, R.RSM_COMMIT_TREE, 0]
    for i, (_, start, n) in enumerate(blobs):
        want = b"\x00" * 32 if st[i] else C.square_commitment(sq, k, ns, start, n, t)
        assert out.raw[32 * i:32 * i + 32] == want
    with pytest.raises(R.RSMError) as e:
        eds.Commitment(4, 2, t)
    assert e.value.code == R.RSM_ETREE
    arr[1].square = 1
    assert lib.rsm_eds_commitments(eds._h, fn, user, arr, len(blobs), t, out, st) == R.RSM_EINVAL
    assert "blob 1 " in lib.rsm_last_error().decode()


# ---- the device entry points' argument errors --------------------------------------------
A, A8, A2 = 4096, 4096 + 8, 4096 + 2  # 16-byte aligned, 8-byte only, 2-byte only
_FAKE = ctypes.create_string_buffer(4096)
CTX = ctypes.addressof(_FAKE)

SHARES = "rsm_blob_commitments_dev"
STORE = "rsm_commitments_dev"
FUNCS = {
    SHARES: (["ctx", "d_shares", "S", "nmt", "threshold", "offsets", "n", "d_work", "d_commitments", "d_status", "stream"],
             dict(ctx=CTX, d_shares=A, S=64, nmt=(29, 1, 1), threshold=64, offsets=[0, 3], d_work=A, d_commitments=A2,
                  d_status=A)),
    STORE: (["ctx", "d_nodes", "d_status_trees", "width", "count", "nmt", "threshold", "blobs", "n", "d_roots_out",
             "d_root_offsets", "d_commitments", "d_status", "stream"],
            dict(ctx=CTX, d_nodes=A, d_status_trees=A, width=16, count=2, nmt=(29, 1, 8), threshold=64, blobs=[(1, 0, 64)],
                 d_roots_out=A2, d_root_offsets=A, d_commitments=A2, d_status=A)),
}


def call(fn, **over):
    names, base = FUNCS[fn]
    v = dict(base, **over)
    keep = []
    if v.get("offsets") is not None:
        v.setdefault("n", len(v["offsets"]) - 1)
        keep.append((ctypes.c_uint32 * len(v["offsets"]))(*v["offsets"]))
        v["offsets"] = keep[-1]
    if v.get("blobs") is not None:
        v.setdefault("n", len(v["blobs"]))
        keep.append((R.BlobRef * max(len(v["blobs"]), 1))(*[R.BlobRef(*b) for b in v["blobs"]]))
        v["blobs"] = keep[-1]
    v.setdefault("n", 1)
    if v.get("nmt") is not None:
        keep.append(R.NmtParams(*v["nmt"]))
        v["nmt"] = ctypes.byref(keep[-1])
    lib = R.library()
    rc = getattr(lib, fn)(*[v.get(a) for a in names])
    return int(rc), (lib.rsm_last_error() or b"").decode() if rc else ""


BIG20 = (1 << 20) + 1
SHARES_CASES = {
    "no_ctx": (dict(ctx=None), R.RSM_EINVAL, "bad arguments"),
    "threshold_0": (dict(threshold=0), R.RSM_EINVAL, "bad arguments"),
    "no_offsets": (dict(offsets=None), R.RSM_EINVAL, "bad arguments"),
    "no_shares": (dict(d_shares=None), R.RSM_EINVAL, "bad arguments"),
    "no_work": (dict(d_work=None), R.RSM_EINVAL, "bad arguments"),
    "no_commitments": (dict(d_commitments=None), R.RSM_EINVAL, "bad arguments"),
    "no_status": (dict(d_status=None), R.RSM_EINVAL, "bad arguments"),
    "default_tree": (dict(nmt=None), R.RSM_EUNSUPPORTED, "NMT only"),
    "ns_0": (dict(nmt=(0, 1, 1)), R.RSM_EINVAL, "namespace size 0"),
    "ns_33": (dict(nmt=(33, 1, 1)), R.RSM_EINVAL, "namespace size 33"),
    "shares_misaligned": (dict(d_shares=A8), R.RSM_EINVAL, "16-byte aligned"),
    "work_misaligned": (dict(d_work=A8), R.RSM_EINVAL, "16-byte aligned"),
    "status_misaligned": (dict(d_status=A2), R.RSM_EINVAL, "4-byte aligned"),
    "share_size": (dict(S=96), R.RSM_ESHARESIZE, "multiple of 64"),
    "share_shorter_than_ns": (dict(S=0), R.RSM_ETREE, "too short"),
    "alignment_before_share_size": (dict(d_shares=A8, S=96), R.RSM_EINVAL, "16-byte aligned"),
    "too_many_blobs": (dict(offsets=[0, 1], n=BIG20), R.RSM_EUNSUPPORTED, "blobs per call"),
    "empty_blob": (dict(offsets=[0, 2, 2, 5]), R.RSM_EINVAL, "blob 1 (shares [2, 2))"),
    "offsets_decrease": (dict(offsets=[0, 4, 7, 6]), R.RSM_EINVAL, "blob 2 (shares [7, 6))"),
    "first_bad_blob_named": (dict(offsets=[3, 3, 2]), R.RSM_EINVAL, "blob 0"),
    "too_many_shares": (dict(offsets=[0, (1 << 24) + 1]), R.RSM_EUNSUPPORTED, "shares (at most"),
    "width_2048": (dict(offsets=[0, 1 << 22], threshold=2048), R.RSM_EUNSUPPORTED, "subtree width 2048"),
    "width_1024_at_ns_32": (dict(offsets=[0, 1 << 20], threshold=1024, nmt=(32, 1, 1)), R.RSM_EUNSUPPORTED,
                            "subtree width 1024"),
    "roots_4097": (dict(offsets=[5, 5 + 4097], threshold=1 << 20), R.RSM_EUNSUPPORTED, "4097 subtree roots"),
}


@pytest.mark.parametrize("name", sorted(SHARES_CASES))
def test_shares_entry_errors(lib, name):
    over, code, text = SHARES_CASES[name]
    rc, msg = call(SHARES, **over)
    assert rc == code and text in msg, (rc, msg)


def test_shares_entry_n_0_returns_before_a_device(lib):
    assert call(SHARES, offsets=[0], n=0) == (0, "")
    assert call(SHARES, offsets=None, d_shares=None, d_work=None, d_commitments=None, d_status=None, n=0) == (0, "")


STORE_CASES = {
    "no_ctx": (dict(ctx=None), R.RSM_EINVAL, "bad arguments"),
    "width_0": (dict(width=0), R.RSM_EINVAL, "bad arguments"),
    "threshold_0": (dict(threshold=0), R.RSM_EINVAL, "bad arguments"),
    "no_nodes": (dict(d_nodes=None), R.RSM_EINVAL, "bad arguments"),
    "no_status_trees": (dict(d_status_trees=None), R.RSM_EINVAL, "bad arguments"),
    "no_blobs": (dict(blobs=None), R.RSM_EINVAL, "bad arguments"),
    "no_commitments": (dict(d_commitments=None), R.RSM_EINVAL, "bad arguments"),
    "no_status": (dict(d_status=None), R.RSM_EINVAL, "bad arguments"),
    "default_tree": (dict(nmt=None), R.RSM_EUNSUPPORTED, "NMT only"),
    "ns_33": (dict(nmt=(33, 1, 8)), R.RSM_EINVAL, "namespace size 33"),
    "square_size_0": (dict(nmt=(29, 1, 0)), R.RSM_EINVAL, "square size 0"),
    "nodes_misaligned": (dict(d_nodes=A8), R.RSM_EINVAL, "aligned"),
    "status_trees_misaligned": (dict(d_status_trees=A2), R.RSM_EINVAL, "aligned"),
    "status_misaligned": (dict(d_status=A2), R.RSM_EINVAL, "aligned"),
    "root_offsets_misaligned": (dict(d_root_offsets=A2), R.RSM_EINVAL, "aligned"),
    "odd_width": (dict(width=15), R.RSM_EUNSUPPORTED, "width 15"),
    "k_not_a_power_of_two": (dict(width=12), R.RSM_EUNSUPPORTED, "width 12"),
    "width_past_the_store": (dict(width=2048), R.RSM_EUNSUPPORTED, "width 2048"),
    "too_many_blobs": (dict(n=BIG20), R.RSM_EUNSUPPORTED, "blobs per call"),
    "square": (dict(blobs=[(0, 0, 1), (2, 0, 1)]), R.RSM_EINVAL, "blob 1 (square 2"),
    "empty": (dict(blobs=[(0, 0, 0)]), R.RSM_EINVAL, "blob 0"),
    "past_the_ods": (dict(blobs=[(0, 0, 64), (0, 60, 5)]), R.RSM_EINVAL, "blob 1"),
    "start_overflow": (dict(blobs=[(0, 0xFFFFFFFF, 2)]), R.RSM_EINVAL, "blob 0"),
    "unaligned_start": (dict(blobs=[(0, 8, 8), (1, 4, 4), (0, 1, 4)], threshold=1), R.RSM_EINVAL, "blob 2"),
    "roots_4097": (dict(width=256, nmt=(29, 1, 128), blobs=[(0, 0, 4096), (0, 0, 4097)], threshold=1 << 20),
                   R.RSM_EUNSUPPORTED, "blob 1 has 4097 subtree roots"),
}


@pytest.mark.parametrize("name", sorted(STORE_CASES))
def test_store_entry_errors(lib, name):
    over, code, text = STORE_CASES[name]
    rc, msg = call(STORE, **over)
    assert rc == code and text in msg, (rc, msg)


def test_store_entry_nothing_to_do_returns_before_a_device(lib):
    assert call(STORE, blobs=[], n=0) == (0, "")
    assert call(STORE, count=0) == (0, "")
    assert call(STORE, count=0, d_nodes=None, d_status_trees=None) == (0, "")
    assert call(STORE, d_roots_out=None, d_root_offsets=None, blobs=[], n=0) == (0, "")


def test_commit_work_bytes(lib):
    p = params(29)
    f = lib.rsm_commit_work_bytes
    nl = 2 * 29 + 32

    def rounded(x):
        return -(-x // 256) * 256

    assert f(100, 7, ctypes.byref(p)) == rounded(100 * 64) + rounded(7 * nl) + rounded(7 * 4)
    assert f(1 << 24, 1 << 24, ctypes.byref(p)) > 0
    assert f((1 << 24) + 1, 1, ctypes.byref(p)) == 0
    assert f(5, 6, ctypes.byref(p)) == 0
    assert f(100, 7, None) == 0
    assert f(100, 7, ctypes.byref(params(0))) == 0 and f(100, 7, ctypes.byref(params(33))) == 0
