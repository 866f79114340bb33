"""GPU: the sampling flow closed on the device -- prove (rsm_proofs_dev), verify
(rsm_proofs_verify_dev), scatter (rsm_samples_scatter_dev), repair
(rsm_repair_squares_dev) -- with shares, records and statuses that never leave device
memory between the steps, against rsm_eds_import_samples on a host square fed the same
batch.

The batch samples the present cells of RP's `avalanche` map: rows and columns
alternating, some proofs corrupted (status ROOT), one cell sampled several times at
scattered positions of the batch (one of them corrupted, one of them first), and samples
aimed at cells the receiving square already holds."""
import ctypes

import numpy as np
import pytest

import repair_dev_calls as D
import repair_patterns as RP
import rsmt2d_amd as R

pytestmark = pytest.mark.gpu
S = 64


def _batch(k, corrupt_every):
    """(samples [(0, axis, index, pos)], indices whose record gets a flipped byte, the
    cells the receiver holds on entry)."""
    W = 2 * k
    pres = RP.presence("avalanche", k)
    cells = [(int(r), int(c)) for r, c in zip(*np.nonzero(pres))]
    held = cells[3::97][:4]  # already present in the receiving square
    samples = [(0, 0, r, c) if (r + c) % 2 == 0 else (0, 1, c, r) for r, c in cells]
    # one cell several times: as a column sample near the front (corrupted below, so it
    # does not count), as a row sample in the middle and as a column sample at the end;
    # its own sample stays where it is, before those two, and wins
    r, c = cells[len(cells) // 3]
    assert (r, c) not in held
    samples.insert(1, (0, 1, c, r))
    samples.insert(len(samples) // 2, (0, 0, r, c))
    samples.append((0, 1, c, r))
    corrupt = set(range(7, len(samples), corrupt_every))
    corrupt.add(1)  # the first duplicate is rejected: the next one of that cell wins
    assert W * W > len(samples) > 0
    return samples, sorted(corrupt), held


@pytest.mark.parametrize("k,corrupt_every", [(8, 40), (8, 6), (65, 1500), (65, 300)])
def test_round_trip_on_the_device(lib, k, corrupt_every):
    round_trip(lib, k, corrupt_every, S)


def round_trip(lib, k, corrupt_every, S):
    """The flow of the module docstring at share size S (tests/test_gpu_share_sizes.py runs
    it at the other sizes)."""
    W = 2 * k
    ctx = R.device_context(0)
    valid, rr, cr = RP.square(k, S)
    valid = np.array(valid)
    samples, corrupt, held = _batch(k, corrupt_every)
    n = len(samples)
    pres0 = np.zeros((W, W), bool)
    for r, c in held:
        pres0[r, c] = True
    start = D.given(valid, pres0)
    rb = int(lib.rsm_proof_record_bytes(W, None))
    arr = (R.Sample * n)(*[R.Sample(*s) for s in samples])
    bufs = [R.DeviceBuffer(valid.nbytes), R.DeviceBuffer(int(lib.rsm_proof_nodes_bytes(W, None, 1))),
            R.DeviceBuffer(2 * W * 32), R.DeviceBuffer(n * rb), R.DeviceBuffer(n * S), R.DeviceBuffer(n * 4),
            R.DeviceBuffer(valid.nbytes), R.DeviceBuffer(W * W)]
    src, nodes, roots, recs, shs, status, dst, dpres = bufs
    try:
        # the serving side: a complete square, its node store and committed roots
        src.upload(valid.reshape(-1))
        R._check(lib.rsm_proof_nodes_dev(ctx, src.ptr, W, S, 1, None, nodes.ptr, roots.ptr, None, None))
        R._check(lib.rsm_proofs_dev(ctx, nodes.ptr, src.ptr, W, S, 1, None, arr, n, recs.ptr, shs.ptr, None))
        R._check(lib.rsm_sync(ctx))
        assert roots.download().tobytes() == b"".join(rr) + b"".join(cr)
        # some proofs are damaged on the way
        rec = recs.download().reshape(n, rb).copy()
        for i in corrupt:
            rec[i, 8 + 5] ^= 0x40
        recs.upload(rec.reshape(-1))
        # the receiving side
        dst.upload(start.reshape(-1))
        dpres.upload(pres0.astype(np.uint8).reshape(-1))
        R._check(lib.rsm_proofs_verify_dev(ctx, shs.ptr, recs.ptr, roots.ptr, W, S, 1, None, arr, n, status.ptr, None))
        R._check(lib.rsm_samples_scatter_dev(ctx, dst.ptr, dpres.ptr, k, S, 1, arr, n, shs.ptr, status.ptr, None))
        R._check(lib.rsm_sync(ctx))
        got_status = status.download().view(np.uint32).copy()
        got_pres = dpres.download().reshape(W, W).copy()
        got = dst.download().reshape(W, W, S).copy()
        shares = shs.download().tobytes()

        # the host call on a square that holds the same cells, fed the same batch
        eds = D.import_host(lib, valid, pres0, R.NewDefaultTree)
        R._check(lib.rsm_eds_set_context(eds._h, ctx))
        want_status = (ctypes.c_uint32 * n)()
        accepted = ctypes.c_uint32()
        R._check(lib.rsm_eds_import_samples(eds._h, b"".join(rr), b"".join(cr), 32, None, None, arr, n, shares,
                                            rec.tobytes(), want_status, ctypes.byref(accepted)))
        want, want_pres = D.flattened_host(lib, eds, W, S)
        assert list(got_status) == list(want_status)
        assert {R.RSM_PROOF_OK, R.RSM_PROOF_ROOT, R.RSM_PROOF_OCCUPIED} == set(int(x) for x in got_status)
        assert got_status[1] == R.RSM_PROOF_ROOT and got_status[n - 1] == R.RSM_PROOF_OCCUPIED
        assert np.array_equal(got_pres != 0, want_pres)
        assert int((got_pres != 0).sum()) - len(held) == accepted.value == int((got_status == 0).sum())
        assert np.array_equal(got[want_pres], want[want_pres])
        assert (got[~want_pres] == D.FILL).all()  # nothing else was written

        # the device repair completes the square exactly when the model says it does
        sweeps, vectors, _, closure = RP.model(want_pres, k)
        (r,) = D.repair(lib, [got], [want_pres], [(rr, cr)], k, S)
        if closure.all():
            assert r.stats() == (R.REPAIR_OK, sweeps, vectors, 0)
            assert np.array_equal(r.square, valid)
        else:
            assert r.stats() == (R.REPAIR_STUCK, sweeps, vectors, int((~closure).sum()))
            assert np.array_equal(r.presence != 0, closure)
            assert np.array_equal(r.square[closure], valid[closure])
    finally:
        for b in bufs:
            b.free()
