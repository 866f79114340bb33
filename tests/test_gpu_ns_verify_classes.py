"""GPU: rsm_ns_proofs_verify_dev's generic kernel form (any namespace size: the node
message laid out in the lane's LDS bytes) at every namespace size 1..32, so that every
SHA-256 padding class of the node message is met (tests/nmt_classes.py), and one call at
the limit of a wave's LDS: width 1024 with 32-byte namespaces.  Every status word is
compared with the hashlib helper and the host verifier."""
import numpy as np
import pytest

import nmt_classes as NC
import ns_proofs as H
import rsmt2d_amd as R
from device_calls import expect
from ns_verify_calls import S, Item, compare, owed, proved, with_variants
from test_ns_proofs_cpu import hostile

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ns", NC.NS_ALL)
def test_every_namespace_size(lib, ns):
    """The five valid squares of nmt_classes (k = 3: a node is carried up; k = 4): every
    honest proof of the host prover, and of every fourth query the first hostile variant of
    each status class."""
    seen = set()
    for k in NC.KS:
        ig = bool((ns + k) & 1)
        W, p = 2 * k, R.NmtParams(ns, int(ig), k)
        batch = np.stack(NC.squares(k, ns)[0])
        queries, nids, records, shares = expect(lib, batch, k, ns, ig, H.vectors(k))
        items, musts = [], []
        for i, (q, nid) in enumerate(zip(queries, nids)):
            s, axis, index = q
            tree = H.Tree(H.vector_shares(batch[s], axis, index), index, k, ns, ig)
            items.append(Item("host prover", q, nid, records[i], shares[i], tree.root))
            musts.append(H.OK)
            if i % 4:
                continue
            classes = {}
            for name, r2, sh2, root2, must in hostile(tree, W, ns, index, k, nid, H.prove_namespace(tree, nid), shares[i],
                                                      tree.root):
                it = Item(name, q, nid, r2, sh2, root2)
                if classes.setdefault(owed(lib, it, W, p), it) is it:
                    items.append(it)
                    musts.append(must)
        seen |= set(compare(lib, items, musts, W, p, batch.shape[0]))
    assert seen == {H.OK, H.MALFORMED, H.ORDER, H.ROOT, H.NAMESPACE, H.INCOMPLETE}


def test_width_1024_with_32_byte_namespaces(lib):
    """The widest tree with the longest namespace: one wave's LDS holds 1024 nodes and the
    64 lanes' four-block node messages.  One sorted vector of a square of k = 512 (runs of
    1, 2, 61, 64, 65 and 319 shares, then 512 parity leaves) and one all-parity vector, whose
    inclusion proof for 0xFF.. is all 1024 leaves and no node."""
    W, ns, k = 1024, 32, 512
    p = R.NmtParams(ns, 0, k)
    rng = np.random.default_rng(1024)
    runs = [1, 2, 61, 64, 65, 319]
    names = [bytes(ns - 1) + bytes([2 * (v + 1)]) for v, m in enumerate(runs) for _ in range(m)]
    assert len(names) == k
    vec = [nm + rng.integers(0, 256, S - ns, dtype=np.uint8).tobytes() for nm in names] + \
          [rng.integers(0, 256, S, dtype=np.uint8).tobytes() for _ in range(k)]
    parity = [rng.integers(0, 256, S, dtype=np.uint8).tobytes() for _ in range(W)]
    asked = sorted(set(names)) + [bytes(ns), bytes(ns - 1) + b"\x03", bytes(ns - 1) + b"\x0d", b"\xff" * ns]
    pairs, heads = [], set()
    for nid in asked:
        it = proved(lib, p, "sorted vector", (0, 0, 5), vec, nid)
        heads.add(tuple(int.from_bytes(it.record[4 * i:4 * i + 4], "little") for i in range(3)))
        pairs += with_variants(lib, p, it, vec, W)
    assert {(H.EMPTY, 0, 0), (H.INCLUSION, 0, 1), (H.INCLUSION, 193, 512), (H.INCLUSION, 512, 1024), (H.ABSENCE, 1, 2),
            (H.ABSENCE, 512, 513)} <= heads
    it = proved(lib, p, "parity vector", (0, 1, 600), parity, b"\xff" * ns)
    assert it.record[:16] == b"".join(v.to_bytes(4, "little") for v in (H.INCLUSION, 0, W, 0)) and len(it.shares) == W
    pairs += with_variants(lib, p, it, parity, W)
    got = compare(lib, [it for it, _ in pairs], [m for _, m in pairs], W, p, 1)
    assert set(got) == {H.OK, H.ROOT, H.INCOMPLETE}
