"""TEST INFRASTRUCTURE ONLY -- the squares, references and width classes that
tests/test_default_tree_classes_cpu.py and tests/test_gpu_default_tree_classes.py share:
the DefaultTree kernels of kernels_sha.hip (tree_root_kernel, tree_nodes_kernel,
proof_verify_kernel) pick their form by the width of the square, and every form is met on
both sides of the width where it changes.  Nothing here calls the library under test:
hashlib, oracle/crossword.py, tests/data_root.py and tests/proof_status.py only (the
kernel source is read as text, for the constants the classes follow from).

The tree has two independent hashlib statements, asserted equal wherever both are
computed: oracle.crossword.merkle_root (the NebulousLabs stack fold: perfect subtrees for
the set bits of n, folded from the right) and tests/data_root.py's RfcTree / mth (RFC
6962's recursive split, pinned to the RFC's vectors).  square_roots hashes every cell
once and folds the digests both ways.

    width class                          rsm_roots_squares_dev (count > 1)   widths here
    4 trees per wave                     W <= 177                            3, 5, 176, 177
    2 trees per wave                     178 <= W <= 385                     178, 384, 385
    1 tree per wave                      W >= 386                            386, 514, 1026
    one square (rsm_roots_dev)           1 tree per wave at any W            3 .. 2048
    node store, trees per workgroup      32 .. 2 for W <= 256, 1 above       255, 257, 258
    node store, 256-lane passes/level    two from W = 513                    514, 2047
An odd W has a height-0 carried subtree (the last leaf) in tree_root_kernel and a raw leaf
digest carried up in tree_nodes_kernel; 126, 254, 510 and 2046 carry one at every height;
with an odd W a wave of the batch form holds row trees and column trees together."""
import functools
import hashlib
import os
import re

import numpy as np

import data_root as D
import proof_status as P
from oracle import crossword

S = 64
KERNELS_SHA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rsmt2d_amd", "csrc",
                           "kernels_sha.hip")

# ---- the launcher's choices, restated (kernels_sha.hip launch_tree_kernel, launch_tree_nodes) ----
TREES_PER_BLOCK = 4         # kTreesPerBlock: one wave per tree-group, four waves per workgroup
BATCH_LDS_BUDGET = 52 * 1024  # trees_per_wave: four waves' LDS within a third of the CU
MAX_WIDTH = 2048            # 2 * kMaxLevel1
NODES_LANES, NODES_MAX_TREES = 256, 32  # proof_trees_per_block


def tree_lds_words(W):
    """One tree's LDS: level 1 in place (W / 2 digests) and 16 carried-subtree slots."""
    return (W // 2) * 8 + 16 * 8


def trees_per_wave(W):
    """The batch form's trees per wave (rsm_roots_squares_dev with more than one square)."""
    for t in (4, 2):
        if TREES_PER_BLOCK * t * tree_lds_words(W) * 4 <= BATCH_LDS_BUDGET:
            return t
    return 1


def root_form(W, squares):
    """(trees per wave, dynamic LDS bytes, workgroups per square) of the tree_root_kernel
    launch for `squares` squares: one square takes the latency form."""
    tpw = 1 if squares == 1 else trees_per_wave(W)
    per_block = TREES_PER_BLOCK * tpw
    return tpw, per_block * tree_lds_words(W) * 4, (2 * W + per_block - 1) // per_block


def proof_trees_per_block(W):
    return min(max(NODES_LANES // ((W + 1) // 2), 1), NODES_MAX_TREES)


def nodes_form(W):
    """(trees per workgroup, dynamic LDS bytes, 256-lane passes of level 1) of tree_nodes_kernel."""
    tpb, half = proof_trees_per_block(W), (W + 1) // 2
    return tpb, tpb * half * 8 * 4, (tpb * half + NODES_LANES - 1) // NODES_LANES


#: the class table, as literals: W -> trees per wave of the batch form
TREES_PER_WAVE = {3: 4, 5: 4, 176: 4, 177: 4, 178: 2, 384: 2, 385: 2, 386: 1, 514: 1, 1026: 1, 2048: 1}
#: W -> (trees per workgroup, LDS bytes, level-1 passes) of the node store
NODES_FORMS = {3: (32, 2048, 1), 9: (32, 5120, 1), 33: (15, 8160, 1), 255: (2, 8192, 1), 256: (2, 8192, 1),
               257: (1, 4128, 1), 258: (1, 4128, 1), 510: (1, 8160, 1), 512: (1, 8192, 1), 514: (1, 8224, 2),
               2047: (1, 32768, 4)}
LATENCY_LDS_2048 = 133120
MOVED = ("the width classes of kernels_sha.hip moved: restate tests/default_tree_classes.py from the launch code and "
         "move the widths of tests/test_gpu_default_tree_classes.py to both sides of the new boundaries")


def source_constants(path=KERNELS_SHA):
    """The constants the classes follow from, read out of the kernel source: a changed
    kTreesPerBlock, LDS budget or tree_lds_words must not leave the tests on one side of a
    boundary twice.  A line that no longer reads as below fails here too."""
    with open(path) as f:
        src = f.read()

    def one(pattern):
        m = re.findall(pattern, src)
        assert len(m) == 1, (MOVED, pattern, m)
        return m[0]

    return {
        "trees_per_block": int(one(r"constexpr uint32_t kTreesPerBlock = (\d+);")),
        "budget": int(one(r"kTreesPerBlock \* t \* tree_lds_words\(W\) \* 4u <= (\d+)u \* 1024u\) return t;")) * 1024,
        "tpw_steps": one(r"for \(uint32_t t = (\d+; t > \d+; t >>= \d+)\)\n\s+if \(\(size_t\)kTreesPerBlock \* t"),
        "lds_words": one(r"tree_lds_words\(uint32_t W\) \{ return ([^;]+); \}"),
        "max_width": 2 * int(one(r"constexpr uint32_t kMaxLevel1 = (\d+);")),
        "latency": one(r"const uint32_t tpw = (latency \? 1u : trees_per_wave\(W\));"),
        "latency_when": one(r"return launch_tree_kernel\(d_leaf, W, d_roots, 0u, 2 \* W, squares, (squares == 1), st\);"),
        "nodes_tpb": one(r"const uint32_t t = (\d+u / half);\n\s+return t < 1u \? 1u : \(t > 32u \? 32u : t\);"),
    }


SOURCE_WANT = {"trees_per_block": TREES_PER_BLOCK, "budget": BATCH_LDS_BUDGET, "tpw_steps": "4; t > 1; t >>= 1",
               "lds_words": "(W / 2) * 8u + 16u * 8u", "max_width": MAX_WIDTH,
               "latency": "latency ? 1u : trees_per_wave(W)", "latency_when": "squares == 1", "nodes_tpb": "256u / half"}


def check_classes():
    """The restatement against the source's constants and against the pinned literals."""
    got = source_constants()
    assert got == SOURCE_WANT, (MOVED, got)
    assert {W: trees_per_wave(W) for W in TREES_PER_WAVE} == TREES_PER_WAVE, MOVED
    assert [trees_per_wave(W) for W in (176, 177, 178, 384, 385, 386, 2048)] == [4, 4, 2, 2, 2, 1, 1], MOVED
    # each boundary is the last width that fits the budget, not merely a width that does
    for W, t in ((177, 4), (385, 2)):
        assert TREES_PER_BLOCK * t * tree_lds_words(W) * 4 <= BATCH_LDS_BUDGET < TREES_PER_BLOCK * t * tree_lds_words(W + 1) * 4, MOVED
    assert root_form(2048, 1) == (1, LATENCY_LDS_2048, 1024) and root_form(2047, 1) == (1, 132992, 1024), MOVED
    assert root_form(386, 3)[0] == root_form(386, 1)[0] == 1 and root_form(385, 3)[:2] == (2, 53248), MOVED
    assert root_form(177, 3) == (4, 53248, 23) and root_form(3, 3) == (4, 8704, 1), MOVED
    assert {W: nodes_form(W) for W in NODES_FORMS} == NODES_FORMS, MOVED


check_classes()


# ---- the tree in hashlib, two ways ------------------------------------------------------
def tree_root(leaves):
    """The root of one vector by both statements."""
    a, b = crossword.merkle_root(leaves), D.mth(leaves)
    assert a == b, (len(leaves), a.hex(), b.hex())
    return a


def fold_digests(digests):
    """crossword.merkle_root's stack fold over leaf digests already taken."""
    stack = []
    for d in digests:
        cur = (0, d)
        while stack and stack[-1][0] == cur[0]:
            h, left = stack.pop()
            cur = (h + 1, hashlib.sha256(b"\x01" + left + cur[1]).digest())
        stack.append(cur)
    acc = stack[-1][1]
    for _h, d in reversed(stack[:-1]):
        acc = hashlib.sha256(b"\x01" + d + acc).digest()
    return acc


def split_digests(digests, lo=0, hi=None):
    """RFC 6962's MTH over leaf digests already taken: split at the largest power of two below n."""
    hi = len(digests) if hi is None else hi
    if hi - lo == 1:
        return digests[lo]
    k = D.split(hi - lo)
    return hashlib.sha256(b"\x01" + split_digests(digests, lo, lo + k) + split_digests(digests, lo + k, hi)).digest()


def tree_leaves(sq, t):
    """Tree t of a [W][W][S] square: row t below W, else column t - W."""
    W = sq.shape[0]
    return [sq[t, p].tobytes() for p in range(W)] if t < W else [sq[p, t - W].tobytes() for p in range(W)]


def pinned_trees(W):
    """The trees of square_roots that are also hashed from their shares by tree_root."""
    return sorted({0, W - 1, W, 2 * W - 1, W // 2, W + W // 2})


def square_roots(sq):
    """All 2W roots of a [W][W][S] square as [2W][32] bytes: every cell hashed once; rows
    folded by the stack, columns by the recursive split, and the other way round wherever
    the square is small; pinned_trees also from their shares by both oracle functions."""
    W = sq.shape[0]
    flat = sq.reshape(W * W, -1)
    leaf = [hashlib.sha256(b"\x00" + flat[c].tobytes()).digest() for c in range(W * W)]
    out = []
    for t in range(2 * W):
        d = leaf[t * W:(t + 1) * W] if t < W else leaf[t - W::W]
        r = fold_digests(d) if t < W else split_digests(d)
        if W <= 130 or t % 61 == 0:
            assert r == (split_digests(d) if t < W else fold_digests(d)), (W, t)
        out.append(r)
    for t in pinned_trees(W):
        assert out[t] == tree_root(tree_leaves(sq, t)), (W, t)
    return np.frombuffer(b"".join(out), np.uint8).reshape(2 * W, 32)


def sampled_trees(W, tpw, seed=0):
    """For a width too wide to hash whole: the first and the last workgroup's trees, the four
    around the row / column boundary, 16 seeded ones."""
    n = TREES_PER_BLOCK * tpw
    t = set(range(n)) | set(range(2 * W - n, 2 * W)) | set(range(W - 2, W + 2))
    rng = np.random.default_rng([0xD7, W, tpw, seed])
    while len(t) < 2 * n + 4 + 16:
        t.add(int(rng.integers(2 * W)))
    return sorted(t)


def sampled_roots(sq, trees):
    """{tree: root} by both statements, from the shares."""
    return {t: tree_root(tree_leaves(sq, t)) for t in trees}


# ---- squares ----------------------------------------------------------------------------
def make_batch(W, count, S_=S):
    """`count` [W][W][S] squares of seeded random bytes, every square different."""
    b = np.random.default_rng([0xDEF, W, count, S_]).integers(0, 256, (count, W, W, S_), dtype=np.uint8)
    assert all(not np.array_equal(b[0], b[q]) for q in range(1, count))
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def batch(W, count, S_=S):
    """make_batch, kept (widths up to 514): with batch_roots the reference the tests of one width share."""
    assert W <= 514
    return make_batch(W, count, S_)


@functools.lru_cache(maxsize=None)
def batch_roots(W, count, S_=S):
    """[count][2W][32]: square_roots of every square of batch(W, count)."""
    r = np.stack([square_roots(sq) for sq in batch(W, count, S_)])
    r.setflags(write=False)
    return r


def class_samples(W, count=1, n=64, seed=0):
    """(square, axis, index, pos) for widths of any parity: the four corners; position W - 1
    (odd W: the carried leaf and its short proof) and W - 2 of the first, middle and last trees
    of both axes; both sides of the tree's top split; n seeded ones over `count` squares."""
    top = D.split(W) if W > 1 else 0
    idx = sorted({0, 1 % W, W // 2, W - 1})
    pos = sorted({0, W - 1, max(W - 2, 0), max(top - 1, 0), top % W})
    s = {(q, a, i, p) for q in range(count) for a in (0, 1) for i in idx for p in pos if q == 0 or p == W - 1}
    rng = np.random.default_rng([0x5A, W, count, seed])
    s |= {(int(rng.integers(count)), int(rng.integers(2)), int(rng.integers(W)), int(rng.integers(W))) for _ in range(n)}
    return sorted(s)


def proof_squares(W, count):
    """proof_status.Squares (the level picture, a third statement) over batch(W, count), its
    roots held to batch_roots."""
    sq = P.Squares(batch(W, count), None)
    want = batch_roots(W, count)
    for q in range(count):
        for t in range(2 * W):
            assert sq.root(q, t // W, t % W) == want[q, t].tobytes(), (W, q, t)
    return sq
