"""GPU: the device calls on caller streams (rsm_stream_create) -- whole pipelines enqueued
alternately on two streams with no host synchronisation in between, the same asynchronous
call twice in a row on one stream (the second call's staged arguments overwrite the first's,
and its device copy grows while the first call is in flight: stage_bytes in rsm_proof.cpp),
and the synchronous Repair and fraud-proof calls from eight host threads on one context.

All of it runs in this process, with threads; every step ends in rsm_stream_check, which
reports a stuck wait.  The pipelines run at 512-byte shares (tests/share_sizes.py); what they
write is compared with the same calls on the context stream and with the models the other
tests use."""
import ctypes
import threading

import numpy as np
import pytest

import commit_calls as CK
import data_root as DR
import device_calls as DC
import fraud_proofs as F
import nmt_layouts as NL
import ns_proofs as H
import range_calls as RG
import range_proofs as M
import repair_cases as RC
import repair_checked as C
import repair_dev_calls as D
import repair_patterns as RP
import rsmt2d_amd as R
import share_sizes as SS
import stream_pipes as PIPES
import test_gpu_fraud_proofs as TF
from device_calls import Guarded
from test_gpu_scatter_dev import _batch

pytestmark = pytest.mark.gpu

K, NS, S = SS.K, SS.NS, 512
W = 2 * K


def _make_streams(lib, n):
    ctx, out = R.device_context(0), []
    for _ in range(n):
        s = ctypes.c_void_p()
        R._check(lib.rsm_stream_create(ctx, ctypes.byref(s)))
        out.append(s)
    return out


def _destroy(lib, streams):
    for s in streams:
        R._check(lib.rsm_stream_destroy(R.device_context(0), s))


@pytest.fixture
def streams(lib):
    st = _make_streams(lib, 2)
    yield st
    _destroy(lib, st)


@pytest.fixture
def stream(lib):
    st = _make_streams(lib, 1)
    yield st[0]
    _destroy(lib, st)


def _free(bufs):
    for b in bufs:
        b.free()


def _same(want, got):
    if isinstance(want, dict):
        assert want.keys() == got.keys()
        want, got = [want[x] for x in sorted(want)], [got[x] for x in sorted(want)]
    assert len(want) == len(got)
    for i, (w, g) in enumerate(zip(want, got)):
        assert np.array_equal(w, g) if isinstance(w, np.ndarray) else w == g, i


# ---- 1. pipelines on two caller streams -----------------------------------------------------
def _share_args(which, tree):
    """Stream `which`'s square (its own), samples (the second stream's in reverse without the
    first seven: another count to stage, the duplicates of one cell still among them) and
    receiving square."""
    valid, rr, cr = RP.square(K, S, tree, which)
    samples, _, held = _batch(K, 6)
    if which:
        samples = samples[::-1][:-7]
    pres0 = np.zeros((W, W), bool)
    for r, c in held:
        pres0[r, c] = True
    p = D.nmt_params(K, RP.NS) if tree == "nmt" else None
    return (np.array(valid), p, samples, D.given(np.array(valid), pres0), pres0), (rr, cr)


@pytest.mark.parametrize("tree", SS.TREES)
def test_share_pipelines_on_two_streams(lib, streams, tree):
    """node store -> share proofs -> verify -> scatter, alternately on two streams."""
    args = [_share_args(i, tree) for i in (0, 1)]
    want = [PIPES.run(PIPES.share_pipe(lib, None, *a))[0] for a, _ in args]
    got = PIPES.run(*[PIPES.share_pipe(lib, s, *a) for s, (a, _) in zip(streams, args)])
    assert len(args[0][0][2]) != len(args[1][0][2])
    for (a, (rr, cr)), w, g in zip(args, want, got):
        _same(w, g)
        square, _, samples = a[0], a[1], a[2]
        assert g["roots"] == b"".join(rr) + b"".join(cr)
        assert g["shares"] == b"".join((square[i, pos] if ax == 0 else square[pos, i]).tobytes() for _, ax, i, pos in samples)
        assert set(g["status"]) == {R.RSM_PROOF_OK, R.RSM_PROOF_OCCUPIED}
        m = g["presence"] != 0
        assert int(m.sum()) == int(a[4].sum()) + g["status"].count(R.RSM_PROOF_OK)
        assert np.array_equal(g["square"][m], square[m]) and (g["square"][~m] == D.FILL).all()


def _ns_args(lib, which):
    layouts = ("runs", "carry") if which else ("max_tail", "runs", "carry")
    batch = np.stack([NL.square(K, NS, S, name, 7 + which) for name in layouts])
    queries, nids, records, shares = DC.expect(lib, batch, K, NS, True, H.vectors(K))
    if which:
        queries, nids, records, shares = (x[::-1][:len(x) - 5] for x in (queries, nids, records, shares))
    return (batch, K, NS, True, S, queries, nids), (records, shares)


def test_namespace_pipelines_on_two_streams(lib, streams):
    """node store -> namespace proofs -> namespace verify, alternately on two streams."""
    args = [_ns_args(lib, i) for i in (0, 1)]
    want = [PIPES.run(PIPES.ns_pipe(lib, None, *a))[0] for a, _ in args]
    got = PIPES.run(*[PIPES.ns_pipe(lib, s, *a) for s, (a, _) in zip(streams, args)])
    for (a, (records, shares)), w, g in zip(args, want, got):
        _same(w, g)
        assert g[0] == b"".join(records) and g[1] == list(np.cumsum([0] + [len(x) for x in shares]))
        assert g[2] == b"".join(b"".join(x) for x in shares) and g[3] == [H.OK] * len(records)


@pytest.mark.parametrize("ns", [0, NS])
def test_range_pipelines_on_two_streams(lib, streams, ns):
    """node store -> range proofs -> range verify -> data roots -> root proofs -> chained
    verify, alternately on two streams: squares of 512- and of 1088-byte shares."""
    args = []
    for which, size in enumerate((S, 1088)):
        sq, rows, cols, drt = SS.range_world(K, ns, size)
        queries = [(0, a, i, s, e) for a in (0, 1) for i in range(which, W, 3 + which) for s, e in SS.RANGES_K8[which:]]
        args.append(((K, ns, size, sq[None], queries), ({0: rows, 1: cols}, drt)))
    want = [PIPES.run(PIPES.range_pipe(lib, None, *a))[0] for a, _ in args]
    got = PIPES.run(*[PIPES.range_pipe(lib, s, *a) for s, (a, _) in zip(streams, args)])
    for (a, (trees, drt)), w, g in zip(args, want, got):
        _same(w, g)
        queries = a[4]
        assert g[0] == b"".join(M.prove(trees[ax][i], ns, s, e) for _, ax, i, s, e in queries)
        assert g[4] == drt.root() and g[5] == b"".join(DR.record_of(drt, W, ax, i) for _, ax, i, _, _ in queries)
        assert g[6] == [M.OK] * len(queries) == g[7]


# ---- 2. back-to-back calls on one caller stream ---------------------------------------------
class Job:
    """One call with its own host arguments and outputs: enqueue(stream), then check()."""

    def __init__(self, enqueue, check, bufs):
        self.enqueue, self.check, self.bufs = enqueue, check, bufs


class Env:
    """The device inputs one kind of call reads (built on the context stream and complete
    before a job runs) and job(n, seed): that call over n samples, queries, refs or blobs."""

    def __init__(self, lib):
        self.lib, self.ctx, self.keep = lib, R.device_context(0), []

    def dev(self, data):
        a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        b = R.DeviceBuffer(max(a.size, 16))
        if a.size:
            b.upload(a)
        self.keep.append(b)
        return b

    def pick(self, items, n, seed):
        g = np.random.default_rng([0x57AE, n, seed])
        return [items[int(i)] for i in g.integers(0, len(items), n)]

    def close(self):
        _free(self.keep)


class ProofsEnv(Env):
    SMALL, BIG = 5, 700

    def __init__(self, lib):
        super().__init__(lib)
        self.batch, self.sq, _ = SS.proof_squares(S, "nmt")
        self.pp = ctypes.byref(self.sq.p)
        self.src = self.dev(self.batch)
        self.nodes = R.DeviceBuffer(int(lib.rsm_proof_nodes_bytes(W, self.pp, 2)))
        self.keep.append(self.nodes)
        R._check(lib.rsm_proof_nodes_dev(self.ctx, self.src.ptr, W, S, 2, self.pp, self.nodes.ptr, None, None, None))
        R._check(lib.rsm_sync(self.ctx))
        self.rb = int(lib.rsm_proof_record_bytes(W, self.pp))

    def job(self, n, seed):
        samples = self.pick(DC.all_samples(W, 2), n, seed)
        recs, shs = Guarded(n * self.rb, 0, 1), Guarded(n * S, 0, 2)
        arr = (R.Sample * n)(*[R.Sample(*s) for s in samples])

        def enqueue(stream):
            R._check(self.lib.rsm_proofs_dev(self.ctx, self.nodes.ptr, self.src.ptr, W, S, 2, self.pp, arr, n, recs.ptr, shs.ptr,
                                             stream))

        def check():
            assert recs.result().tobytes() == b"".join(self.sq.record(s) for s in samples)
            assert shs.result().tobytes() == b"".join(self.sq.share(s) for s in samples)
        return Job(enqueue, check, [recs, shs])


class VerifyEnv(Env):
    SMALL, BIG = 7, 600

    def __init__(self, lib):
        super().__init__(lib)
        _, self.sq, _ = SS.proof_squares(S, "nmt")
        self.items, self.want = SS.verify_items(S, "nmt")
        self.base = DC.committed_roots(self.sq)

    def job(self, n, seed):
        idx = self.pick(range(len(self.items)), n, seed)
        items = [self.items[i] for i in idx]
        samples, roots = DC.place(items, self.base)
        shs, recs = self.dev(np.frombuffer(b"".join(it.share for it in items), np.uint8)), \
            self.dev(np.frombuffer(b"".join(it.record for it in items), np.uint8))
        rts, st = self.dev(roots), Guarded(n * 4, 4, 3)
        arr = (R.Sample * n)(*[R.Sample(*s) for s in samples])

        def enqueue(stream):
            R._check(self.lib.rsm_proofs_verify_dev(self.ctx, shs.ptr, recs.ptr, rts.ptr, W, S, roots.shape[0],
                                                    ctypes.byref(self.sq.p), arr, n, st.ptr, stream))

        def check():
            assert [int(x) for x in st.result().view(np.uint32)] == [self.want[i] for i in idx]
        return Job(enqueue, check, [st])


class NsProofsEnv(Env):
    SMALL, BIG = 4, 500

    def __init__(self, lib):
        super().__init__(lib)
        self.batch = np.stack([NL.square(K, NS, S, name, 7) for name in ("runs", "carry", "max_tail")])
        self.p = R.NmtParams(NS, 1, K)
        self.pp, count = ctypes.byref(self.p), self.batch.shape[0]
        self.all = list(zip(*DC.expect(lib, self.batch, K, NS, True, H.vectors(K))))
        self.src = self.dev(self.batch)
        self.nodes, self.tstat = R.DeviceBuffer(int(lib.rsm_proof_nodes_bytes(W, self.pp, count))), R.DeviceBuffer(count * 2 * W * 4)
        self.keep += [self.nodes, self.tstat]
        R._check(lib.rsm_proof_nodes_dev(self.ctx, self.src.ptr, W, S, count, self.pp, self.nodes.ptr, None, self.tstat.ptr, None))
        R._check(lib.rsm_sync(self.ctx))

    def job(self, n, seed):
        queries, nids, records, shares = zip(*self.pick(self.all, n, seed))
        cap = sum(len(x) for x in shares)
        rb = H.record_bytes(W, NS)
        recs, offs, shs = Guarded(n * rb, 3, 4), Guarded((n + 1) * 4, 4, 5), Guarded(max(cap, 1) * S, 0, 6)
        arr, flat = (R.NsQuery * n)(*[R.NsQuery(*q) for q in queries]), b"".join(nids)

        def enqueue(stream):
            R._check(self.lib.rsm_ns_proofs_dev(self.ctx, self.nodes.ptr, self.tstat.ptr, self.src.ptr, W, S, self.batch.shape[0],
                                                self.pp, arr, flat, n, recs.ptr, offs.ptr, shs.ptr, cap, stream))

        def check():
            assert recs.result().tobytes() == b"".join(records)
            assert list(offs.result().view(np.uint32)) == list(np.cumsum([0] + [len(x) for x in shares]))
            assert shs.result()[:cap * S].tobytes() == b"".join(b"".join(x) for x in shares)
        return Job(enqueue, check, [recs, offs, shs])


class RangeProofsEnv(Env):
    SMALL, BIG = 3, 400

    def __init__(self, lib):
        super().__init__(lib)
        self.sq, rows, cols, _ = SS.range_world(K, NS, S)
        self.trees = {0: rows, 1: cols}
        self.p = RG.params(K, NS)
        self.src = self.dev(self.sq)
        self.nodes = R.DeviceBuffer(int(lib.rsm_proof_nodes_bytes(W, RG.pref(self.p), 1)))
        self.keep.append(self.nodes)
        R._check(lib.rsm_proof_nodes_dev(self.ctx, self.src.ptr, W, S, 1, RG.pref(self.p), self.nodes.ptr, None, None, None))
        R._check(lib.rsm_sync(self.ctx))
        self.all = [(0, a, i, s, e) for a in (0, 1) for i in range(W) for s, e in M.all_ranges(W)]

    def job(self, n, seed):
        queries = self.pick(self.all, n, seed)
        cap, rb = sum(q[4] - q[3] for q in queries), M.record_bytes(W, NS)
        recs, offs, shs = Guarded(n * rb, 3, 7), Guarded((n + 1) * 4, 4, 8), Guarded(cap * S, 0, 9)
        arr = (R.RangeQuery * n)(*[R.RangeQuery(*q) for q in queries])

        def enqueue(stream):
            R._check(self.lib.rsm_range_proofs_dev(self.ctx, self.nodes.ptr, self.src.ptr, W, S, 1, RG.pref(self.p), arr, n,
                                                   recs.ptr, offs.ptr, shs.ptr, cap, stream))

        def check():
            assert recs.result().tobytes() == b"".join(M.prove(self.trees[a][i], NS, s, e) for _, a, i, s, e in queries)
            assert list(offs.result().view(np.uint32)) == list(np.cumsum([0] + [q[4] - q[3] for q in queries]))
            assert shs.result().tobytes() == b"".join(b"".join(H.vector_shares(self.sq, a, i)[s:e]) for _, a, i, s, e in queries)
        return Job(enqueue, check, [recs, offs, shs])


class RangeVerifyEnv(Env):
    SMALL, BIG = 6, 450

    def __init__(self, lib):
        super().__init__(lib)
        self.cases = SS.range_cases(NS, S)[0]
        self.p = RG.params(K, NS)

    def job(self, n, seed):
        cases = self.pick(self.cases, n, seed)
        nl = M.node_len(NS)
        packed = b"".join(b"".join(c.shares) for c in cases)
        offsets = np.cumsum([0] + [len(c.shares) for c in cases]).astype(np.uint32)
        roots = np.zeros((n, 2, W, nl), np.uint8)
        for i, c in enumerate(cases):
            roots[i, 0, c.index] = np.frombuffer(c.root, np.uint8)
        recs, offs, shs, rts = (self.dev(x) for x in (np.frombuffer(b"".join(c.record for c in cases), np.uint8), offsets,
                                                      np.frombuffer(packed, np.uint8), roots))
        st = Guarded(n * 4, 4, 10)
        arr = (R.RangeQuery * n)(*[R.RangeQuery(i, 0, c.index, c.start, c.end) for i, c in enumerate(cases)])

        def enqueue(stream):
            R._check(self.lib.rsm_range_proofs_verify_dev(self.ctx, recs.ptr, offs.ptr, shs.ptr, len(packed) // S, rts.ptr, W, S, n,
                                                          RG.pref(self.p), arr, n, st.ptr, stream))

        def check():
            assert [int(x) for x in st.result().view(np.uint32)] == [c.must for c in cases]
        return Job(enqueue, check, [st])


class RootProofsEnv(Env):
    SMALL, BIG = 5, 300

    def __init__(self, lib):
        super().__init__(lib)
        self.count = 2
        table = np.random.default_rng(0x5254).integers(0, 256, (self.count, 2 * W, 90), dtype=np.uint8)
        self.trees = [DR.RfcTree([r.tobytes() for r in table[q]]) for q in range(self.count)]
        roots, drs = self.dev(table), self.dev(np.zeros(self.count * 32, np.uint8))
        self.nodes = R.DeviceBuffer(int(lib.rsm_data_root_nodes_bytes(W, self.count)))
        self.keep.append(self.nodes)
        R._check(lib.rsm_data_roots_dev(self.ctx, roots.ptr, W, 90, self.count, drs.ptr, self.nodes.ptr, None))
        R._check(lib.rsm_sync(self.ctx))
        assert drs.download(self.count * 32).tobytes() == b"".join(t.root() for t in self.trees)

    def job(self, n, seed):
        refs = self.pick([(q, a, i) for q in range(self.count) for a in (0, 1) for i in range(W)], n, seed)
        rb = DR.record_bytes(W)
        recs = Guarded(n * rb, 2, 11)
        arr = (R.RootRef * n)(*[R.RootRef(*r) for r in refs])

        def enqueue(stream):
            R._check(self.lib.rsm_root_proofs_dev(self.ctx, self.nodes.ptr, W, self.count, arr, n, recs.ptr, stream))

        def check():
            assert recs.result().tobytes() == b"".join(DR.record_of(self.trees[q], W, a, i) for q, a, i in refs)
        return Job(enqueue, check, [recs])


class CommitmentsEnv(Env):
    SMALL, BIG = 4, 350
    T = 2

    def __init__(self, lib):
        super().__init__(lib)
        self.store = CK.Store(lib, SS.commitment_square(S)[None], R.NmtParams(NS, 1, K))
        self.keep += [self.store.nodes, self.store.status]
        blobs, _, want = SS.commitment_wants(S, self.T)
        self.all = list(zip(blobs, want))

    def job(self, n, seed):
        blobs, want = zip(*self.pick(self.all, n, seed))
        com, st = Guarded(n * 32, 3, 12), Guarded(n * 4, 4, 13)
        arr = (R.BlobRef * n)(*[R.BlobRef(0, s, m) for s, m in blobs])
        s_ = self.store

        def enqueue(stream):
            R._check(self.lib.rsm_commitments_dev(self.ctx, s_.nodes.ptr, s_.status.ptr, W, 1, ctypes.byref(s_.p), self.T, arr, n,
                                                  None, None, com.ptr, st.ptr, stream))

        def check():
            assert com.result().tobytes() == b"".join(want) and not st.result().any()
        return Job(enqueue, check, [com, st])


class ScatterEnv(Env):
    SMALL, BIG = 6, 200

    def job(self, n, seed):
        g = np.random.default_rng([0x5CA7, n, seed])
        cells = g.permutation(W * W)[:n]  # distinct cells, none of them held
        samples = [(0, 0, int(c) // W, int(c) % W) if i % 2 else (0, 1, int(c) % W, int(c) // W) for i, c in enumerate(cells)]
        shares = g.integers(0, 256, (n, S), dtype=np.uint8)
        status = np.where(np.arange(n) % 5 == 3, R.RSM_PROOF_ROOT, R.RSM_PROOF_OK).astype(np.uint32)
        dst, dpres, dst_st = Guarded(W * W * S, 0, 14), Guarded(W * W, 0, 15), Guarded(n * 4, 4, 16)
        dst.buf.upload(np.full(W * W * S, D.FILL, np.uint8), dst.front)
        dpres.buf.upload(np.zeros(W * W, np.uint8), dpres.front)
        dst_st.buf.upload(status.view(np.uint8), dst_st.front)
        shs = self.dev(shares)
        arr = (R.Sample * n)(*[R.Sample(*s) for s in samples])

        def enqueue(stream):
            R._check(self.lib.rsm_samples_scatter_dev(self.ctx, dst.ptr, dpres.ptr, K, S, 1, arr, n, shs.ptr, dst_st.ptr, stream))

        def check():
            want, pres = np.full((W * W, S), D.FILL, np.uint8), np.zeros(W * W, np.uint8)
            ok = status == R.RSM_PROOF_OK
            want[cells[ok]], pres[cells[ok]] = shares[ok], 1
            assert np.array_equal(dst.result().reshape(W * W, S), want) and np.array_equal(dpres.result(), pres)
            assert np.array_equal(dst_st.result().view(np.uint32), status)
        return Job(enqueue, check, [dst, dpres, dst_st])


class GatherEnv(Env):
    SMALL, BIG = 5, 150

    def __init__(self, lib):
        super().__init__(lib)
        g = np.random.default_rng(0x6A7)
        self.count = 3
        self.batch = g.integers(0, 256, (self.count, W, W, S), dtype=np.uint8)
        self.pres = g.integers(0, 3, (self.count, W, W), dtype=np.uint8) * 7
        self.d_eds, self.d_pres = self.dev(self.batch), self.dev(self.pres)

    def job(self, n, seed):
        refs = self.pick([(q, a, i) for q in range(self.count) for a in (0, 1) for i in range(W)], n, seed)
        d_sh, d_pr = Guarded(n * W * S, 0, 17), Guarded(n * W, 5, 18)
        arr = (R.RootRef * n)(*[R.RootRef(*r) for r in refs])

        def enqueue(stream):
            R._check(self.lib.rsm_vectors_gather_dev(self.ctx, self.d_eds.ptr, self.d_pres.ptr, K, S, self.count, arr, n, d_sh.ptr,
                                                     d_pr.ptr, stream))

        def check():
            sh, pr = d_sh.result().reshape(n, W, S), d_pr.result().reshape(n, W)
            for j, (q, a, i) in enumerate(refs):
                assert np.array_equal(sh[j], self.batch[q, i] if a == 0 else self.batch[q, :, i]), refs[j]
                assert np.array_equal(pr[j], self.pres[q, i] if a == 0 else self.pres[q, :, i]), refs[j]
        return Job(enqueue, check, [d_sh, d_pr])


ENVS = {"rsm_proofs_dev": ProofsEnv, "rsm_proofs_verify_dev": VerifyEnv, "rsm_ns_proofs_dev": NsProofsEnv,
        "rsm_range_proofs_dev": RangeProofsEnv, "rsm_range_proofs_verify_dev": RangeVerifyEnv,
        "rsm_root_proofs_dev": RootProofsEnv, "rsm_commitments_dev": CommitmentsEnv,
        "rsm_samples_scatter_dev": ScatterEnv, "rsm_vectors_gather_dev": GatherEnv}


@pytest.mark.parametrize("call", sorted(ENVS))
def test_back_to_back_calls_on_one_stream(lib, stream, call):
    """The same call twice with different host arguments and no synchronisation between: first
    a small one and then a larger one than the fresh stream has staged before, so the device
    copy of the staged arguments grows while the first call is in flight; then a large one
    followed by a small one, which overwrites the front of what the large one reads.  All four
    results are the model's."""
    env = ENVS[call](lib)
    jobs = []
    try:
        for seed, sizes in enumerate(((env.SMALL, env.BIG), (env.BIG + 37, env.SMALL + 1))):
            pair = [env.job(n, 2 * seed + j) for j, n in enumerate(sizes)]
            jobs += pair
            for job in pair:
                job.enqueue(stream)
            R._check(lib.rsm_stream_check(env.ctx, stream))
            for job in pair:
                job.check()
    finally:
        _free([b for job in jobs for b in job.bufs])
        env.close()


# ---- 3. host threads on one context ---------------------------------------------------------
THREADS, ROUNDS = 8, 3
FAMILIES = ("avalanche", "chain3", "core", "chain3_cf", "q0_only", "core_edge", "odd_rows", "chain3_t")
CHECKED = ("B_col_kept", "A_row_k", "E_overdetermined_row", "D_control", "B_row_kept", "C_row_root_0", "A_row_last", "C_col_root_last")


def _thread_work(t):
    """Thread t's inputs: k = 8 (128-byte shares) or k = 65 (64-byte shares), an erasure family,
    a verification case and a slice of the fraud-proof batch of its own."""
    k, size = ((8, 128), (65, 64))[t % 2]
    valid, rr, cr = RP.square_for(FAMILIES[t], k, size)
    pres = RP.presence(FAMILIES[t], k)
    flat, crr, ccr, _ = RC.case(CHECKED[t], k, size)
    csq, cpres = D.case_square(flat, 2 * k, size)
    _, table = TF.world(k, size, 0)
    proofs = TF.mixed_batch(k, size, 0, 14)[t % 4:t % 4 + 8]
    return dict(k=k, S=size, repair=([D.given(valid, pres)], [pres], [(rr, cr)]), checked=([csq], [cpres], [(crr, ccr)]),
                fraud=(proofs, table))


def _thread_calls(lib, w, stream):
    """The three synchronous calls on `stream`; what they returned, in a comparable form."""
    (r,) = D.repair(lib, *w["repair"], w["k"], w["S"], stream=stream)
    (c,) = C.repair_checked(lib, *w["checked"], w["k"], w["S"], stream=stream)
    verdicts, after = F.run(lib, *w["fraud"], w["k"], w["S"], stream=stream)
    m, cm = r.presence != 0, c.presence != 0
    return [r.stats(), r.presence, r.square[m], c.stats(), c.check(), c.presence, c.square[cm], c.shares, verdicts,
            [after[i] for i, v in enumerate(verdicts) if v[0] in (F.VALID, F.CONSISTENT)]]


def _equal(a, b):
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    if isinstance(a, list) and a and isinstance(a[0], np.ndarray):
        return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("own_streams", [True, False])
def test_host_threads_on_one_context(lib, own_streams):
    """Eight host threads, one context: each makes rsm_repair_squares_dev,
    rsm_repair_squares_checked_dev and rsm_fraud_proofs_verify_dev calls on squares of its own
    (k = 8 and k = 65, a family and a verification case per thread), three rounds, on a stream
    of its own or all on the context stream (the calls take a lane of the context's pool).
    Every result is the single-threaded one."""
    work = [_thread_work(t) for t in range(THREADS)]
    want = [_thread_calls(lib, w, None) for w in work]
    assert {x[0][0] for x in want} == {R.REPAIR_OK, R.REPAIR_STUCK}
    assert {x[3][0] for x in want} == {R.REPAIR_OK, R.REPAIR_BYZANTINE}
    assert {v[0] for x in want for v in x[8]} == {F.VALID, F.TOOFEW, F.SHARE, F.CONSISTENT}
    streams = _make_streams(lib, THREADS) if own_streams else [None] * THREADS
    errors = []

    def worker(t):
        try:
            for rnd in range(ROUNDS):
                got = _thread_calls(lib, work[t], streams[t])
                bad = [i for i, (a, b) in enumerate(zip(want[t], got)) if not _equal(a, b)]
                if bad:
                    errors.append((t, rnd, bad))
                    return
        except Exception as e:  # reported below
            errors.append((t, repr(e)))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(THREADS)]
    try:
        for x in th:
            x.start()
        for x in th:
            x.join(timeout=100)
        assert not any(x.is_alive() for x in th), "a caller hung"
    finally:
        if own_streams and not any(x.is_alive() for x in th):
            _destroy(lib, streams)
    assert not errors, errors[:5]
