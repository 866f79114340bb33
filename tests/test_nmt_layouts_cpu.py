"""CPU: the host namespaced Merkle tree (merkle.cpp rsm_nmt_tree_root /
rsm_nmt_tree_prove) on squares whose namespaces have structure -- repeats, compares
that only a late byte decides, quadrant-0 cells carrying 0xFF.. and the namespace just
below it -- instead of uniform random ones (tests/nmt_layouts.py), against the Python
oracle (oracle/nmt.py), with both IgnoreMaxNamespace values.  The device kernels meet
the same squares in tests/test_gpu_nmt_layouts.py."""
import ctypes

import numpy as np
import pytest

import nmt_layouts as NL
import proof_verify as V
import rsmt2d_amd as R
from oracle import nmt

S = 64
NS_ALL = [1, 3, 8, 29, 30, 32]
K_ALL = [1, 2, 3, 4, 8]


def host_root(lib, p, index, leaves):
    """rsm_nmt_tree_root itself (the Python Tree's Push checks the order before it)."""
    keep, ptrs, _ = R._bufs(leaves)
    cap = 2 * p.namespace_size + 32
    out = (ctypes.c_uint8 * cap)()
    ln = ctypes.c_uint32(cap)
    rc = lib.rsm_nmt_tree_root(ctypes.byref(p), 0, index, ptrs, len(leaves), len(leaves[0]), out, ctypes.byref(ln))
    assert rc in (0, R.RSM_ETREE)
    return bytes(out[:ln.value]) if rc == 0 else None


def tree_root(ctor, axis, index, leaves):
    """The same through the TreeConstructorFn, as the EDS layer's host path pushes."""
    try:
        t = ctor(axis, index)
        for x in leaves:
            t.Push(x)
        return t.Root()
    except R.RSMError:
        return None


def check_square(lib, sq, k, ns, ignore_max, want_failing=None):
    W = 2 * k
    status, roots = NL.expected(sq, k, ns, ignore_max)
    assert (status == NL.decreasing_status(sq, k, ns)).all()
    if want_failing is not None:
        assert set(np.nonzero(status)[0]) == set(want_failing)
    p = R.NmtParams(ns, 1 if ignore_max else 0, k)
    ctor = R.ErasuredNamespacedMerkleTreeConstructor(k, ns, ignore_max)
    for t in range(2 * W):
        leaves = NL.tree_leaves(sq, t)
        assert host_root(lib, p, t % W, leaves) == roots[t], (t, "rsm_nmt_tree_root")
        assert tree_root(ctor, t // W, t % W, leaves) == roots[t], (t, "Tree")
    return status, roots


def test_layouts_have_the_structure_they_name():
    k, ns = 4, 29
    q = lambda name: NL.square(k, ns, S, name, 1)[:k, :k, :ns].reshape(k * k, ns)
    assert len({bytes(x) for x in q("single")}) == 1
    for p_ in range(ns):
        lad = q("ladder:%d" % p_)
        assert (np.delete(lad, p_, axis=1) == np.delete(lad[0], p_)).all()
        assert (np.diff(lad[:, p_].astype(int)) > 0).all()
    car = q("carry").astype(int)
    for i in range(0, k * k, 2):  # one byte rises by one, every later byte falls from FF to 00
        p_ = int(np.argmax(car[i] != car[i + 1]))
        assert car[i + 1, p_] == car[i, p_] + 1 and p_ == (ns - 2 - i // 2) % (ns - 1)
        assert (car[i, p_ + 1:] == 0xFF).all() and (car[i + 1, p_ + 1:] == 0).all()
    ff = (NL.square(k, ns, S, "max_tail", 1)[:k, :k, :ns] == 0xFF).all(axis=2)
    assert ff[k - 1].all() and ff[k - 2].any() and not ff[k - 2].all() and not ff[0].any()
    runs = NL.square(k, ns, S, "runs", 1)[:k, :k]
    names = [bytes(x[:ns]) for x in runs.reshape(k * k, S)]
    assert names[0] == bytes(28) + b"\x01" and names[-1] == b"\xff" * ns
    assert len(set(names)) < len(names)                        # namespaces repeat ...
    assert any(names[r * k - 1] == names[r * k] for r in range(1, k))  # ... across a row end
    assert all(n_[:19] == bytes(19) for n_ in names if n_ != b"\xff" * ns)
    nm = NL.square(k, ns, S, "near_max", 1)[:k, :k].reshape(k * k, S)
    near = [x for x in nm if bytes(x[:ns]) == b"\xff" * 28 + b"\x00"]
    assert near and all(bytes(x[ns:ns + 4]) == b"\xff" * 4 for x in near)
    assert any(bytes(x[:ns]) == b"\xff" * ns for x in nm)


@pytest.mark.parametrize("ignore_max", [True, False])
@pytest.mark.parametrize("k", K_ALL)
@pytest.mark.parametrize("ns", NS_ALL)
def test_host_tree_on_layouts(lib, ns, k, ignore_max):
    """Every layout, every tree: rsm_nmt_tree_root and the Tree == the oracle; no valid
    layout fails a tree."""
    for name in NL.all_layouts(ns):
        sq = NL.square(k, ns, S, name, 10 * k + ns)
        status, roots = check_square(lib, sq, k, ns, ignore_max, want_failing=())
        if name in ("runs", "max_tail") and k >= 3:  # the last quadrant-0 row is 0xFF.. all through
            r = roots[k - 1]
            assert r[:ns] == b"\xff" * ns and r[ns:2 * ns] == b"\xff" * ns
        if name == "max_tail" and k >= 3:  # a row that ends in 0xFF.. cells: its max is theirs only when
            r = roots[k - 2]               # the max namespace is not ignored
            last_data = sq[k - 2, k - 1 - max(k // 2, 1), :ns].tobytes()
            assert r[ns:2 * ns] == (last_data if ignore_max else b"\xff" * ns)


@pytest.mark.parametrize("ignore_max", [True, False])
@pytest.mark.parametrize("p_", range(29))
def test_host_inversion_only_byte_p_decides(lib, p_, ignore_max):
    k, ns = 4, 29
    sq = NL.invert(NL.square(k, ns, S, "ladder:%d" % p_, 3), (1, 1), (1, 2), ns)
    check_square(lib, sq, k, ns, ignore_max, want_failing=[1])


@pytest.mark.parametrize("k", [3, 4, 7, 8])
def test_host_inversion_positions(lib, k):
    ns = 29
    W = 2 * k
    base = NL.square(k, ns, S, "ladder:%d" % (ns - 1), 5)
    for (r, c), b in NL.position_swaps(k):
        check_square(lib, NL.invert(base, (r, c), b, ns), k, ns, True, want_failing=NL.row_swap_failing(base, k, ns, r, c))
        check_square(lib, NL.invert(base, (c, r), (c + 1, r), ns), k, ns, True,
                     want_failing=NL.col_swap_failing(base, k, ns, c, r))
        for cell in ((r, c), (c, r)):  # 0xFF.. ahead of smaller namespaces: a push-order error only
            for ignore_max in (True, False):
                check_square(lib, NL.plant_max(base, cell, ns), k, ns, ignore_max,
                             want_failing=NL.plant_max_failing(base, k, ns, *cell))
    for r in sorted({0, k - 2}):  # two whole rows: every quadrant-0 column fails, no row does
        check_square(lib, NL.invert(base, r, r + 1, ns), k, ns, True, want_failing=range(W, W + k))


@pytest.mark.parametrize("ns", [1, 3, 8, 30, 32])
def test_host_inversions_other_namespace_sizes(lib, ns):
    k = 4
    for name in ("ladder:%d" % (ns - 1), "carry", "runs", "max_tail", "near_max"):
        base = NL.square(k, ns, S, name, 7)
        for ignore_max in (True, False):
            for r in range(k):
                c = NL.first_step(base, k, ns, r, 0, 0)
                if c is not None:
                    check_square(lib, NL.invert(base, (r, c), (r, c + 1), ns), k, ns, ignore_max,
                                 want_failing=NL.row_swap_failing(base, k, ns, r, c))
            for cell in ((1, 1), (0, 2), (2, 0)):
                check_square(lib, NL.plant_max(base, cell, ns), k, ns, ignore_max,
                             want_failing=NL.plant_max_failing(base, k, ns, *cell))
            r = NL.first_step(base, k, ns, 2, 0, 1)
            assert r is not None
            check_square(lib, NL.invert(base, (r, 2), (r + 1, 2), ns), k, ns, ignore_max,
                         want_failing=NL.col_swap_failing(base, k, ns, r, 2))


@pytest.mark.parametrize("ignore_max", [True, False])
@pytest.mark.parametrize("name", ["single", "runs", "max_tail"])
def test_host_prove_on_layouts(lib, name, ignore_max):
    """rsm_nmt_tree_prove records of every leaf of every tree fold to the oracle's root,
    bottom-up and in nmt's in-order node order."""
    k, ns = 4, 29
    W, nl = 2 * k, 2 * ns + 32
    sq = NL.square(k, ns, S, name, 11)
    _status, roots = NL.expected(sq, k, ns, ignore_max)
    p = R.NmtParams(ns, 1 if ignore_max else 0, k)
    for t in range(2 * W):
        leaves = NL.tree_leaves(sq, t)
        keep, ptrs, _ = R._bufs(leaves)
        for pos in range(W):
            rec = ctypes.create_string_buffer(V.record_bytes(W, nl))
            root = ctypes.create_string_buffer(nl)
            assert lib.rsm_nmt_tree_prove(ctypes.byref(p), t % W, ptrs, W, S, pos, rec, root) == 0
            assert root.raw == roots[t]
            nodes, mask = V.parse_record(rec.raw, nl)
            assert len(nodes) == V.level_count(W, pos)
            assert V.verify_nmt(roots[t], leaves[pos], nodes, mask, pos, t % W, k, ns, ignore_max)
            pr = R.Proof(leaves[pos], nodes, mask, pos, W, p, t % W)
            assert pr.root == roots[t]
            assert V.verify_nmt_inorder(roots[t], V.nmt_leaf(leaves[pos], pos, t % W, k, ns), pr.nmt_nodes(), pos, W,
                                        ns, ignore_max)


def test_eds_roots_passes_ignore_max():
    k, ns = 4, 8
    sq = NL.square(k, ns, S, "max_tail", 13)
    for ig in (True, False):
        rows, cols = nmt.eds_roots(sq, k, ns, ig)
        assert rows + cols == NL.expected(sq, k, ns, ig)[1]
    assert nmt.eds_roots(sq, k, ns) == nmt.eds_roots(sq, k, ns, True) != nmt.eds_roots(sq, k, ns, False)
