"""CPU: what rsm_repair_squares_dev and rsm_samples_scatter_dev decide before any device
use -- the scratch size and its limits, the result record's size, the argument errors --
and the statuses tests/test_gpu_repair_dev.py expects of RC's cases against RC.expected."""
import ctypes

import pytest

import repair_cases as RC
import repair_dev_calls as D
import rsmt2d_amd as R


def _nmt(ns, k):
    return ctypes.byref(R.NmtParams(ns, 1, k))


def test_work_bytes_inside_and_outside_the_limits(lib):
    wb = lib.rsm_repair_work_bytes
    for k, S, count in [(1, 64, 1), (8, 64, 4), (65, 64, 1), (128, 512, 64), (1024, 64, 1)]:
        W = 2 * k
        # at least the re-extension copies and the leaf digests
        assert wb(k, S, count, None) >= count * W * W * (S + 32), (k, S, count)
    assert wb(8, 64, 0, None) > 0
    for k in (8, 65, 512):
        assert wb(k, 64, 2, _nmt(29, k)) >= 2 * 4 * k * k * (64 + 64)
        assert wb(k, 64, 2, _nmt(1, k)) > 0
        # (the device NMT's own limit: a tree of 1024 leaves with 32-byte namespaces is past its LDS)
        assert (wb(k, 64, 2, _nmt(32, k)) > 0) == bool(lib.rsm_proof_nodes_bytes(2 * k, _nmt(32, k), 2))
    assert wb(1025, 64, 1, None) == 0          # W = 2050: past the DefaultTree kernels
    assert wb(513, 64, 1, _nmt(29, 513)) == 0  # W = 1026: past the NMT kernels
    assert wb(8, 64, 1, _nmt(0, 8)) == 0 and wb(8, 64, 1, _nmt(33, 8)) == 0
    assert wb(0, 64, 1, None) == 0 and wb(8, 96, 1, None) == 0
    assert wb(1024, 64, 1024, None) == 0       # count * W * W reaches 2^32: not one root launch


def test_result_record_is_four_words():
    assert ctypes.sizeof(R.RepairResult) == 16
    assert [f[0] for f in R.RepairResult._fields_] == ["status", "sweeps", "decoded_vectors", "missing"]
    assert (R.REPAIR_OK, R.REPAIR_STUCK, R.REPAIR_ENCODING, R.REPAIR_ROOTS) == (0, 1, 2, 3)


def test_argument_errors_before_any_device_use(lib):
    """NULL ctx, k = 0 and S = 96 are refused before the context is looked at: `ctx` here
    is the address of a zeroed buffer, no rsm_ctx."""
    fake = ctypes.create_string_buffer(4096)
    ctx = ctypes.addressof(fake)
    res = (R.RepairResult * 1)()
    rep, sc = lib.rsm_repair_squares_dev, lib.rsm_samples_scatter_dev
    sample = (R.Sample * 1)(R.Sample(0, 0, 0, 0))
    assert rep(None, None, None, 8, 64, 1, None, None, None, res, None) == R.RSM_EINVAL
    assert rep(ctx, None, None, 0, 64, 1, None, None, None, res, None) == R.RSM_EINVAL
    assert rep(ctx, None, None, 8, 96, 1, None, None, None, res, None) == R.RSM_ESHARESIZE
    assert b"multiple of 64" in lib.rsm_last_error()
    assert rep(ctx, None, None, 1025, 64, 1, None, None, None, res, None) == R.RSM_EUNSUPPORTED
    assert rep(ctx, None, None, 8, 64, 1, _nmt(33, 8), None, None, res, None) == R.RSM_EUNSUPPORTED
    assert rep(ctx, None, None, 8, 64, 1, None, None, None, res, None) == R.RSM_EINVAL  # NULL operands
    assert rep(ctx, None, None, 8, 64, 0, None, None, None, None, None) == R.RSM_OK      # nothing to do
    assert sc(None, None, None, 8, 64, 1, sample, 1, None, None, None) == R.RSM_EINVAL
    assert sc(ctx, None, None, 0, 64, 1, sample, 1, None, None, None) == R.RSM_EINVAL
    assert sc(ctx, None, None, 8, 96, 1, sample, 1, None, None, None) == R.RSM_ESHARESIZE
    assert sc(ctx, None, None, 8, 64, 1, sample, 1, None, None, None) == R.RSM_EINVAL    # NULL operands
    assert sc(ctx, None, None, 8, 64, 1, sample, 0, None, None, None) == R.RSM_OK        # nothing to do


@pytest.mark.parametrize("tree", ["default", "nmt"])
@pytest.mark.parametrize("name", RC.CASES)
def test_expected_statuses_agree_with_the_oracle(name, tree):
    """`ok` <-> OK; a byzantine outcome <-> not OK and not STUCK (these squares all
    complete: k cells of every row, or of every column, are given)."""
    outcome, _ = RC.expected(name, 8, 64, tree)
    assert outcome != "unrepairable"
    want = D.RC_STATUS[name]
    if outcome == "ok":
        assert want == {R.REPAIR_OK}
    else:
        assert want and want <= {R.REPAIR_ENCODING, R.REPAIR_ROOTS}
    assert set(D.RC_STATUS) == set(RC.CASES)
