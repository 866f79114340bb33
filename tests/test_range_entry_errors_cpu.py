"""CPU: the error surface of the three device entry points of the range proofs
(rsm_range_proofs_dev, rsm_range_proofs_verify_dev, rsm_range_proofs_verify_data_root_dev).

As tests/test_dev_entry_errors_cpu.py: every case returns before the call selects a device
-- `ctx` is the address of a zeroed buffer (no rsm_ctx), device pointers are small integers
chosen for their alignment and never dereferenced.  Each case overrides operands that would
otherwise pass every check and names the (code, message) it owes; a case in which two
neighbouring checks would both fire pins their order."""
import ctypes

import pytest

import rsmt2d_amd as R

A, A8, A2 = 4096, 4096 + 8, 4096 + 2  # 16-byte aligned, 8-byte only, 2-byte only
_FAKE = ctypes.create_string_buffer(4096)
CTX = ctypes.addressof(_FAKE)
GOOD = (0, 1, 15, 3, 16)  # in range for one square of width 16
BIG20 = (1 << 20) + 1

PROVE = "rsm_range_proofs_dev"
VERIFY = "rsm_range_proofs_verify_dev"
CHAINED = "rsm_range_proofs_verify_data_root_dev"

FUNCS = {
    PROVE: (["ctx", "d_nodes", "d_eds", "width", "S", "count", "nmt", "queries", "n", "d_records", "d_offsets", "d_shares",
             "shares_cap", "stream"],
            dict(ctx=CTX, d_nodes=A, d_eds=A, width=16, S=64, count=1, nmt=None, queries=[GOOD], d_records=A, d_offsets=A,
                 d_shares=A, shares_cap=0)),
    VERIFY: (["ctx", "d_records", "d_offsets", "d_shares", "shares_total", "d_roots", "width", "S", "count", "nmt", "queries",
              "n", "d_status", "stream"],
             dict(ctx=CTX, d_records=A, d_offsets=A, d_shares=A, shares_total=1, d_roots=A, width=16, S=64, count=1, nmt=None,
                  queries=[GOOD], d_status=A)),
    CHAINED: (["ctx", "d_records", "d_offsets", "d_shares", "shares_total", "d_root_records", "d_data_roots", "width", "S",
               "count", "nmt", "queries", "n", "d_status", "stream"],
              dict(ctx=CTX, d_records=A, d_offsets=A, d_shares=A, shares_total=1, d_root_records=A, d_data_roots=A, width=16,
                   S=64, count=1, nmt=None, queries=[GOOD], d_status=A)),
}


def call(fn, **over):
    names, base = FUNCS[fn]
    v = dict(base, **over)
    q = v.get("queries")
    keep = []
    if q is not None:
        v.setdefault("n", len(q))
        arr = (R.RangeQuery * max(len(q), 1))(*[R.RangeQuery(*x) for x in q])
        keep.append(arr)
        v["queries"] = arr
    else:
        v.setdefault("n", 1)
    if v.get("nmt") is not None:
        p = R.NmtParams(*v["nmt"])
        keep.append(p)
        v["nmt"] = ctypes.byref(p)
    lib = R.library()
    rc = getattr(lib, fn)(*[v.get(a) for a in names])
    return int(rc), (lib.rsm_last_error() or b"").decode() if rc else ""


def bad_queries():
    out = {}
    for f, wrong in (("square", (1, 1, 15, 3, 16)), ("axis", (0, 2, 15, 3, 16)), ("index", (0, 1, 16, 3, 16)),
                     ("empty", (0, 1, 15, 3, 3)), ("reversed", (0, 1, 15, 4, 3)), ("end", (0, 1, 15, 3, 17))):
        for at in (0, 2):
            arr = [GOOD] * 3
            arr[at] = wrong
            out[f"{f}_at_{at}"] = (arr, at, wrong)
    return out


VERIFY_OPS = {VERIFY: ["queries", "d_records", "d_offsets", "d_roots", "d_status"],
              CHAINED: ["queries", "d_records", "d_offsets", "d_root_records", "d_data_roots", "d_status"]}


@pytest.mark.parametrize("fn", [VERIFY, CHAINED])
def test_verify_entry_errors(lib, fn):
    bad = f"{fn}: bad arguments"
    ops = VERIFY_OPS[fn]
    assert call(fn, ctx=None) == (R.RSM_EINVAL, bad)
    assert call(fn, width=0) == (R.RSM_EINVAL, bad)
    for op in ops:
        assert call(fn, **{op: None}) == (R.RSM_EINVAL, bad), op
    assert call(fn, d_shares=None) == (R.RSM_EINVAL, bad)           # shares_total = 1 needs d_shares
    # early RSM_OK: n == 0 and count == 0 need no operands
    assert call(fn, **dict({op: None for op in ops}, n=0)) == (R.RSM_OK, "")
    assert call(fn, **dict({op: None for op in ops if op != "queries"}, count=0, d_shares=None)) == (R.RSM_OK, "")
    # namespace parameters, before alignment
    for nmt in ((0, 1, 8), (33, 1, 8), (8, 1, 0)):
        rc, msg = call(fn, nmt=nmt, d_shares=A8)
        assert rc == R.RSM_EINVAL and msg == f"{fn}: namespace size {nmt[0]} (1..32) or square size 0"
    # alignment: d_shares, then d_offsets / d_status, then the share size
    assert call(fn, d_shares=A8, d_offsets=A2) == (R.RSM_EINVAL, f"{fn}: d_shares must be 16-byte aligned")
    for op in ("d_offsets", "d_status"):
        assert call(fn, S=96, **{op: A2}) == (R.RSM_EINVAL, f"{fn}: d_offsets and d_status must be 4-byte aligned")
    # share size, then width, then short shares, then n
    rc, msg = call(fn, S=96, width=4096)
    assert rc == R.RSM_ESHARESIZE and "96" in msg and "multiple of 64" in msg
    assert call(fn, width=2049, n=BIG20) == (R.RSM_EUNSUPPORTED, f"{fn}: width 2049 not supported (at most 2048)")
    assert call(fn, width=2048, n=0)[0] == R.RSM_OK
    assert call(fn, width=1025, nmt=(8, 1, 8), S=0) == (R.RSM_EUNSUPPORTED, f"{fn}: width 1025 not supported (at most 1024)")
    assert call(fn, width=1024, nmt=(32, 1, 8), n=0)[0] == R.RSM_OK
    assert call(fn, nmt=(8, 1, 8), S=0, n=BIG20) == (R.RSM_ETREE, "data is too short to contain namespace ID")
    assert call(fn, n=BIG20) == (R.RSM_EINVAL, f"{fn}: at most 1048576 queries per call")
    # the limit check precedes the early OK and the range loop
    assert call(fn, n=BIG20, count=0)[0] == R.RSM_EINVAL
    assert call(fn, n=0)[0] == R.RSM_OK and call(fn, count=0)[0] == R.RSM_OK
    assert call(fn, count=0, queries=[(5, 5, 99, 9, 1)])[0] == R.RSM_OK   # nothing is validated for no squares
    for name, (arr, at, w) in bad_queries().items():
        want = f"{fn}: query {at} (square {w[0]}, axis {w[1]}, index {w[2]}, leaves [{w[3]}, {w[4]})) is out of range"
        assert call(fn, queries=arr) == (R.RSM_EINVAL, want), name


def test_prove_entry_errors(lib):
    fn = PROVE
    bad = f"{fn}: bad arguments"
    assert call(fn, ctx=None) == (R.RSM_EINVAL, bad)
    assert call(fn, d_nodes=None) == (R.RSM_EINVAL, bad)
    assert call(fn, width=0) == (R.RSM_EINVAL, bad)
    for op in ("queries", "d_records", "d_offsets"):
        assert call(fn, **{op: None}) == (R.RSM_EINVAL, bad), op
    assert call(fn, d_eds=None, d_nodes=A8) == (R.RSM_EINVAL, f"{fn}: d_shares needs d_eds")
    assert call(fn, d_eds=None, d_shares=None, n=0)[0] == R.RSM_OK
    for over in (dict(d_shares=A8), dict(d_eds=A8)):
        assert call(fn, d_nodes=A8, **over) == (R.RSM_EINVAL, f"{fn}: d_eds and d_shares must be 16-byte aligned")
    for over in (dict(d_nodes=A8), dict(d_offsets=A2)):
        assert call(fn, S=96, **over) == (R.RSM_EINVAL, f"{fn}: d_nodes must be 16-byte, d_offsets 4-byte aligned")
    rc, msg = call(fn, S=96, width=4096)
    assert rc == R.RSM_ESHARESIZE and "multiple of 64" in msg
    # the node store's limits, DefaultTree and NMT; nmt == NULL is accepted
    assert call(fn, width=2050, n=BIG20) == (R.RSM_EUNSUPPORTED, f"{fn}: 1 squares of width 2050 not supported")
    assert call(fn, width=2048, n=0)[0] == R.RSM_OK
    assert call(fn, width=1026, nmt=(8, 1, 513), n=BIG20) == (R.RSM_EUNSUPPORTED,
                                                              f"{fn}: 1 squares of width 1026 (NMT) not supported")
    assert call(fn, width=1, n=0)[0] == R.RSM_EUNSUPPORTED           # the store holds trees of two leaves and more
    assert call(fn, n=BIG20) == (R.RSM_EINVAL, f"{fn}: at most 1048576 queries per call")
    assert call(fn, n=BIG20, count=0)[0] == R.RSM_EINVAL
    assert call(fn, n=0)[0] == R.RSM_OK and call(fn, count=0)[0] == R.RSM_OK
    assert call(fn, n=0, queries=None, d_records=None, d_offsets=None)[0] == R.RSM_OK
    for name, (arr, at, w) in bad_queries().items():
        want = f"{fn}: query {at} (square {w[0]}, axis {w[1]}, index {w[2]}, leaves [{w[3]}, {w[4]})) is out of range"
        assert call(fn, queries=arr) == (R.RSM_EINVAL, want), name
