"""TEST INFRASTRUCTURE ONLY -- what tests/test_ns_verify_cpu.py, tests/test_gpu_ns_verify.py
and tests/test_gpu_ns_verify_classes.py share: the items a verification call is given
(record, shares, namespace, root), the one device call that verifies a list of them
(rsm_ns_proofs_verify_dev between guard bands), what each owes by the hashlib helper of
tests/ns_proofs.py and by the host verifier, and the NamespaceData answers, honest and
dishonest, that verify_namespace_data is asked about.  Importing this module touches no
GPU."""
import ctypes
import functools
from collections import namedtuple

import numpy as np

import ns_proofs as H
import rsmt2d_amd as R
from device_calls import Guarded
from test_ns_proofs_cpu import _square, c_prove, c_verify, flip

S = 64

# q: (square, axis, index) of the roots table the item is verified under
Item = namedtuple("Item", "name q nid record shares root")


def roots_table(items, count, W, nl):
    """[count][2][W][nl]: every item's root at its (square, axis, index), zeros elsewhere."""
    out = np.zeros((count, 2, W, nl), np.uint8)
    seen = {}
    for it in items:
        assert seen.setdefault(it.q, it.root) == it.root, "two roots for one slot of the table"
        out[it.q] = np.frombuffer(it.root, np.uint8)
    return out


def fill(g, data):
    """Puts `data` into the operand of a Guarded buffer."""
    a = np.frombuffer(bytes(data), np.uint8)
    assert len(a) <= g.n
    if len(a):
        g.sent[g.front:g.front + len(a)] = a
        g.buf.upload(a, offset=g.front)


def device_ns_statuses(lib, items, W, p, roots, rec_skew=3, offsets=None, shares_total=None, n=None, count=None, S=S):
    """One rsm_ns_proofs_verify_dev call over `items` (shares of S bytes); the status words.  Records sit
    `rec_skew` bytes past a 64-byte boundary; d_status lies between guard bands.  `offsets`
    / `shares_total` / `n` / `count` override what the items dictate (framing tests)."""
    ns = int(p.namespace_size)
    rb = H.record_bytes(W, ns)
    assert all(len(it.record) == rb for it in items)
    if offsets is None:
        offsets = np.cumsum([0] + [len(it.shares) for it in items])
    offsets = np.asarray(offsets, np.uint32)
    packed = b"".join(b"".join(it.shares) for it in items)
    total = len(packed) // S if shares_total is None else shares_total
    n = len(items) if n is None else n
    count = roots.shape[0] if count is None else count
    ctx = R.device_context(0)
    recs, offs = Guarded(max(len(items) * rb, 16), rec_skew, 21), Guarded(offsets.nbytes, 4, 22)
    shs, rts, st = Guarded(max(len(packed), 16), 0, 23), Guarded(roots.nbytes, 1, 24), Guarded(max(len(items), 1) * 4, 8, 25)
    try:
        fill(recs, b"".join(it.record for it in items))
        fill(offs, offsets.tobytes())
        fill(shs, packed)
        fill(rts, roots.tobytes())
        arr = (R.NsQuery * max(len(items), 1))(*[R.NsQuery(*it.q) for it in items])
        R._check(lib.rsm_ns_proofs_verify_dev(ctx, recs.ptr, offs.ptr, shs.ptr, total, rts.ptr, W, S, count, ctypes.byref(p),
                                              arr, b"".join(it.nid for it in items), n, st.ptr, None))
        del arr  # copied before the call returned
        R._check(lib.rsm_sync(ctx))
        for g in (recs, offs, shs, rts):
            g.result()  # the call writes status words only
        return st.result().view(np.uint32).copy(), st
    finally:
        for g in (recs, offs, shs, rts, st):
            g.free()


def owed(lib, it, W, p):
    """The status the item owes: the hashlib helper's, which the host verifier must share."""
    ns, k, ig = int(p.namespace_size), int(p.square_size), bool(p.ignore_max_namespace)
    want = H.expected_status(W, ns, ig, it.q[2], k, it.nid, it.shares, it.record, it.root)
    host = c_verify(lib, p, it.q[2], it.nid, it.shares, W, it.record, it.root)
    assert host == want, (it.name, it.q, it.nid.hex(), host, want)
    return want


def host_status(lib, it, W, p):
    return c_verify(lib, p, it.q[2], it.nid, it.shares, W, it.record, it.root)


def compare(lib, items, musts, W, p, count, **kw):
    got, _ = device_ns_statuses(lib, items, W, p, roots_table(items, count, W, 2 * p.namespace_size + 32), **kw)
    assert len(got) == len(items)
    for it, must, g in zip(items, musts, got):
        want = owed(lib, it, W, p)
        assert g == want, (it.name, it.q, it.nid.hex(), it.record[:16].hex(), int(g), want)
        assert must is None or g == must, (it.name, it.q, it.nid.hex(), int(g), must)
    return [int(g) for g in got]


def proved(lib, p, name, q, leaves, nid):
    """The host prover's item for `nid` in the vector `leaves` of tree `q[2]`."""
    rc, rec, root = c_prove(lib, p, q[2], leaves, nid)
    assert rc == 0
    kind, start, end = (int.from_bytes(rec[4 * i:4 * i + 4], "little") for i in range(3))
    return Item(name, q, nid, rec, leaves[start:end] if kind == H.INCLUSION else [], root)


def with_variants(lib, p, it, leaves, W, S=S):
    """The item (0), its first share with one bit flipped (3; ABSENCE: the leaf node's
    digest) and the range narrowed by its first share (6)."""
    ns, k, ig = int(p.namespace_size), int(p.square_size), bool(p.ignore_max_namespace)
    kind, start, end = (int.from_bytes(it.record[4 * i:4 * i + 4], "little") for i in range(3))
    out = [(it, H.OK)]
    if kind == H.ABSENCE:
        at = 16 + 2 * H.levels(W) * (2 * ns + 32) + 2 * ns + 31
        out.append((it._replace(name=it.name + ", leaf digest bit", record=flip(it.record, at)), H.ROOT))
    if kind == H.INCLUSION:
        out.append((it._replace(name=it.name + ", share bit", shares=[flip(it.shares[0], S - 1)] + it.shares[1:]), H.ROOT))
        if end - start >= 2:
            tree = H.Tree(leaves, it.q[2], k, ns, ig)
            r2 = H.record_of(W, ns, kind, start + 1, end, H.prove_range(tree, start + 1, end), None)
            out.append((it._replace(name=it.name + ", narrowed", record=r2, shares=it.shares[1:]), H.INCOMPLETE))
    return out


# ---- NamespaceData answers (verify_namespace_data) --------------------------------------
Case = namedtuple("Case", "what nid data roots p sq k")


@functools.lru_cache(maxsize=None)
def namespace_data_cases(k, ns):
    """A "runs" square (row 0: namespaces ..01 ..02 ..02 ..04) asked for a namespace that
    is present, one that is absent inside row 0's range, one below every root's range, and
    the run that ends row 1."""
    assert k == 4
    sq, eds = _square(k, ns, "runs")
    roots, p = eds.RowRoots(), eds._tree_fn.params
    two, run = bytes(ns - 1) + b"\x02", sq[1, k - 1, :ns].tobytes()
    assert [sq[0, c, ns - 1] for c in range(k)] == [1, 2, 2, 4] and run != b"\xff" * ns
    out = []
    for what, nid in (("present", two), ("absent", bytes(ns - 1) + b"\x03"), ("outside", bytes(ns)), ("run", run)):
        data = eds.NamespaceData(nid)
        kinds = [pr.kind for _, pr in data]
        assert kinds == {"present": [H.INCLUSION], "absent": [H.ABSENCE], "outside": []}.get(what, kinds)
        out.append(Case(what, nid, data, roots, p, sq, k))
    return out


def answers(case):
    """(name, data, the status list it owes): the honest answer, and where the namespace
    is present a row dropped, a range narrowed and a share of another namespace."""
    W = 2 * case.k
    ns = int(case.p.namespace_size)
    out = [("honest", case.data, [H.OK] * W)]
    if case.what in ("present", "run"):
        r0 = case.data[0][0]
        want = [H.OK] * W
        want[r0] = H.INCOMPLETE
        out.append(("row dropped", case.data[1:], want))
    if case.what == "present":
        r0, pr = case.data[0]
        assert r0 == 0 and pr.end - pr.start == 2
        tree = H.Tree(H.vector_shares(case.sq, 0, 0), 0, case.k, ns, True)
        narrow = R.NamespaceProof(H.INCLUSION, pr.start + 1, pr.end, H.prove_range(tree, pr.start + 1, pr.end), None,
                                  pr.shares[1:], W, case.p, 0)
        out.append(("narrowed", [(0, narrow)], [H.INCOMPLETE] + [H.OK] * (W - 1)))
        alien = R.NamespaceProof(pr.kind, pr.start, pr.end, pr.nodes, None, pr.shares[:-1] + [flip(pr.shares[-1], 0)], W,
                                 case.p, 0)
        out.append(("alien share", [(0, alien)], [H.NAMESPACE] + [H.OK] * (W - 1)))
    return out
