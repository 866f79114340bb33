"""CPU: the error surface of the twelve device-resident entry points -- for every case of
CASES the pair (return code, rsm_last_error text) equals tests/golden/dev_entry_errors.json.

Every case returns before the call selects a device: `ctx` is the address of a zeroed
buffer (no rsm_ctx), device pointers are small integers chosen for their alignment and are
never dereferenced.  The cases hit every fail(...) and every early RSM_OK (n == 0,
count == 0) that precedes use_device in those functions, pin the order of each pair of
neighbouring checks with a case in which both would fire, try out-of-range samples, refs
and queries at element 0 and at the last element of three, and try each `n` limit at
limit + 1 with a one-element array (the limit check precedes the range loop everywhere).
Two sites no argument reaches: "data is too short to contain namespace ID" of
rsm_proof_nodes_dev and of the two Repair calls, where a share has at least 64 bytes and a
device namespace at most 32.

The golden file was recorded with this module run as a script
(python tests/test_dev_entry_errors_cpu.py) before the host code of these calls was
restructured; a line of it changes only with a deliberate change of the C ABI's behaviour.
"""
import ctypes
import json
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import rsmt2d_amd as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dev_entry_errors.json")

A = 4096        # a 16-byte aligned address
A8 = A + 8      # 8-byte aligned only
A2 = A + 2      # 2-byte aligned only
_FAKE = ctypes.create_string_buffer(4096)
CTX = ctypes.addressof(_FAKE)
_RES, _CHK = (R.RepairResult * 1)(), (R.RepairCheck * 1)()
_NIDS = bytes(range(3 * 32))  # three namespaces of up to 32 bytes
BIG24, BIG20 = (1 << 24) + 1, (1 << 20) + 1

GOOD4, GOOD3 = (0, 1, 15, 15), (0, 1, 15)  # in range for one square of width 16


def _bad(good, width=16):
    """Three-element arrays with one field of element 0, or of the last element, out of range."""
    out = {}
    for f, name in enumerate(("square", "axis", "index", "pos")[:len(good)]):
        wrong = list(good)
        wrong[f] = 1 if f == 0 else 2 if f == 1 else width
        for at in (0, 2):
            arr = [good] * 3
            arr[at] = tuple(wrong)
            out[f"{name}_at_{at}"] = arr
    return out


# per function: the argument names in ABI order, and operands that pass every check (such
# a call would go on to the device: every case below overrides something)
FUNCS = {
    "rsm_proof_nodes_dev": (
        ["ctx", "d_eds", "width", "S", "count", "nmt", "d_nodes", "d_roots", "d_status", "stream"],
        dict(ctx=CTX, d_eds=A, width=16, S=64, count=1, nmt=None, d_nodes=A)),
    "rsm_proofs_dev": (
        ["ctx", "d_nodes", "d_eds", "width", "S", "count", "nmt", "samples", "n", "d_records", "d_shares", "stream"],
        dict(ctx=CTX, d_nodes=A, d_eds=A, width=16, S=64, count=1, nmt=None, samples=[GOOD4], d_records=A, d_shares=A)),
    "rsm_proofs_verify_dev": (
        ["ctx", "d_shares", "d_records", "d_roots", "width", "S", "count", "nmt", "samples", "n", "d_status", "stream"],
        dict(ctx=CTX, d_shares=A, d_records=A, d_roots=A, width=16, S=64, count=1, nmt=None, samples=[GOOD4], d_status=A)),
    "rsm_data_roots_dev": (
        ["ctx", "d_roots", "width", "root_len", "count", "d_data_roots", "d_nodes", "stream"],
        dict(ctx=CTX, d_roots=A, width=16, root_len=32, count=1, d_data_roots=A, d_nodes=A)),
    "rsm_root_proofs_dev": (
        ["ctx", "d_nodes", "width", "count", "refs", "n", "d_records", "stream"],
        dict(ctx=CTX, d_nodes=A, width=16, count=1, refs=[GOOD3], d_records=A)),
    "rsm_proofs_verify_data_root_dev": (
        ["ctx", "d_shares", "d_records", "d_root_records", "d_data_roots", "width", "S", "count", "nmt", "samples", "n",
         "d_status", "stream"],
        dict(ctx=CTX, d_shares=A, d_records=A, d_root_records=A, d_data_roots=A, width=16, S=64, count=1, nmt=None,
             samples=[GOOD4], d_status=A)),
    "rsm_ns_proofs_dev": (
        ["ctx", "d_nodes", "d_status", "d_eds", "width", "S", "count", "nmt", "queries", "nids", "n", "d_records",
         "d_offsets", "d_shares", "shares_cap", "stream"],
        dict(ctx=CTX, d_nodes=A, d_status=A, d_eds=A, width=16, S=64, count=1, nmt=(8, 1, 8), queries=[GOOD3], nids=_NIDS,
             d_records=A, d_offsets=A, d_shares=A, shares_cap=0)),
    "rsm_ns_proofs_verify_dev": (
        ["ctx", "d_records", "d_offsets", "d_shares", "shares_total", "d_roots", "width", "S", "count", "nmt", "queries",
         "nids", "n", "d_status", "stream"],
        dict(ctx=CTX, d_records=A, d_offsets=A, d_shares=A, shares_total=1, d_roots=A, width=16, S=64, count=1,
             nmt=(8, 1, 8), queries=[GOOD3], nids=_NIDS, d_status=A)),
    "rsm_repair_squares_dev": (
        ["ctx", "d_eds", "d_presence", "k", "S", "count", "nmt", "d_roots", "d_work", "results", "stream"],
        dict(ctx=CTX, d_eds=A, d_presence=A, k=8, S=64, count=1, nmt=None, d_roots=A, d_work=A, results=_RES)),
    "rsm_repair_squares_checked_dev": (
        ["ctx", "d_eds", "d_presence", "k", "S", "count", "nmt", "d_roots", "d_work", "results", "checks", "stream"],
        dict(ctx=CTX, d_eds=A, d_presence=A, k=8, S=64, count=1, nmt=None, d_roots=A, d_work=A, results=_RES, checks=_CHK)),
    "rsm_vectors_gather_dev": (
        ["ctx", "d_eds", "d_presence", "k", "S", "count", "refs", "n", "d_shares", "d_present", "stream"],
        dict(ctx=CTX, d_eds=A, d_presence=A, k=8, S=64, count=1, refs=[GOOD3], d_shares=A, d_present=A)),
    "rsm_samples_scatter_dev": (
        ["ctx", "d_eds", "d_presence", "k", "S", "count", "samples", "n", "d_shares", "d_status", "stream"],
        dict(ctx=CTX, d_eds=A, d_presence=A, k=8, S=64, count=1, samples=[GOOD4], d_shares=A, d_status=A)),
}

_ARRAYS = {"samples": R.Sample, "refs": R.RootRef, "queries": R.NsQuery}


def _nulls(names, **more):
    return {f"null_{x}": dict(more, **{x: None}) for x in names}


def _verify_cases(extra):
    """rsm_proofs_verify_dev and rsm_proofs_verify_data_root_dev (`extra`: the further operands)."""
    ops = ["samples", "d_shares", "d_records", "d_status"] + extra
    c = {"null_ctx": dict(ctx=None), "width_0": dict(width=0), "width_65537": dict(width=65537)}
    c.update(_nulls(ops))
    c["nulls_n_0"] = dict({x: None for x in ops}, n=0)                                 # RSM_OK
    c["nulls_count_0"] = dict({x: None for x in ops if x != "samples"}, count=0)       # RSM_OK
    c.update(ns_0=dict(nmt=(0, 1, 8)), ns_33=dict(nmt=(33, 1, 8)), square_size_0=dict(nmt=(8, 1, 0)))
    c.update(shares_misaligned=dict(d_shares=A8), status_misaligned=dict(d_status=A2), S_96=dict(S=96))
    c.update(short_share=dict(nmt=(8, 1, 8), S=0), n_limit=dict(n=BIG24), n_0=dict(n=0), count_0=dict(count=0))
    c.update({f"bad_{k}": dict(samples=v) for k, v in _bad(GOOD4).items()})
    # two checks fire: the earlier one answers
    c["order_args_nmt"] = dict(width=0, nmt=(0, 1, 8))
    c["order_nmt_shares"] = dict(nmt=(33, 1, 8), d_shares=A8)
    c["order_shares_status"] = dict(d_shares=A8, d_status=A2)
    c["order_status_S"] = dict(d_status=A2, S=96)
    c["order_S_n"] = dict(S=96, n=BIG24)
    c["order_short_n"] = dict(nmt=(8, 1, 8), S=0, n=BIG24)
    c["order_n_count"] = dict(n=BIG24, count=0)
    c["order_count_sample"] = dict(count=0, samples=[(0, 2, 0, 0)])                    # RSM_OK
    return c


def _repair_cases(operands):
    c = {"null_ctx": dict(ctx=None), "k_0": dict(k=0), "S_96": dict(S=96), "S_0": dict(S=0), "k_1025": dict(k=1025),
         "ns_33": dict(nmt=(33, 1, 8)), "count_65536": dict(count=65536), "count_0": dict(count=0)}
    c.update(_nulls(operands))
    c.update(eds_misaligned=dict(d_eds=A8), presence_misaligned=dict(d_presence=A8), work_misaligned=dict(d_work=A8))
    c["order_k_S"] = dict(k=0, S=96)
    c["order_S_shape"] = dict(S=96, k=1025)
    c["order_empty_shape"] = dict(S=0, k=1025)
    c["order_shape_count"] = dict(k=1025, count=0)
    c["order_count_nulls"] = dict({x: None for x in operands}, count=0)                # RSM_OK
    c["order_null_misaligned"] = dict(d_roots=None, d_eds=A8)
    return c


def _gather_scatter_cases(arr, good, operands):
    c = {"null_ctx": dict(ctx=None), "k_0": dict(k=0), "k_32769": dict(k=32769), "S_96": dict(S=96), "S_0": dict(S=0),
         "n_limit": dict(n=BIG24), "n_0": dict(n=0), "count_0": dict(count=0)}
    c.update(_nulls(operands))
    c.update(eds_misaligned=dict(d_eds=A8), shares_misaligned=dict(d_shares=A8))
    c.update({f"bad_{k}": dict({arr: v}) for k, v in _bad(good).items()})
    c["order_k_S"] = dict(k=0, S=96)
    c["order_S_empty_n"] = dict(S=96, n=BIG24)
    c["order_empty_n"] = dict(S=0, n=BIG24)
    c["order_n_count"] = dict(n=BIG24, count=0)
    c["order_n_0_nulls"] = dict({x: None for x in operands}, n=0)                      # RSM_OK
    c["order_null_misaligned"] = dict(d_presence=None, d_eds=A8)
    c["order_misaligned_range"] = dict({arr: [tuple([1] + list(good[1:]))]}, d_shares=A8)
    return c


def _ns_range(c):
    c.update({f"bad_{k}": dict(queries=v) for k, v in _bad(GOOD3).items()})


CASES = {}

c = CASES["rsm_proof_nodes_dev"] = {"null_ctx": dict(ctx=None), "width_0": dict(width=0)}
c.update(_nulls(["d_eds", "d_nodes"]))
c.update(nodes_misaligned=dict(d_nodes=A8), eds_misaligned=dict(d_eds=A8), S_96=dict(S=96), S_0=dict(S=0))
c.update(width_4096=dict(width=4096), ns_33=dict(nmt=(33, 1, 8)), count_65536=dict(count=65536), count_0=dict(count=0))
c["nmt_past_its_square"] = dict(nmt=(8, 1, 4))
c["order_args_aligned"] = dict(ctx=None, d_nodes=A8)
c["order_aligned_S"] = dict(d_eds=A8, S=96)
c["order_S_shape"] = dict(S=96, width=4096)
c["order_empty_shape"] = dict(S=0, width=4096)
c["order_shape_count"] = dict(width=4096, count=0)

c = CASES["rsm_proofs_dev"] = {"null_ctx": dict(ctx=None), "width_0": dict(width=0)}
c.update(_nulls(["d_nodes", "samples", "d_records"]))
c["nulls_n_0"] = dict(samples=None, d_records=None, n=0)                               # RSM_OK
c["shares_without_eds"] = dict(d_eds=None)
c.update(shares_misaligned=dict(d_shares=A8), eds_misaligned=dict(d_eds=A8))
c["eds_misaligned_unused"] = dict(d_eds=A8, d_shares=None, n=0)                        # RSM_OK
c.update(S_96=dict(S=96), width_4096=dict(width=4096), ns_33=dict(nmt=(33, 1, 8)), count_65536=dict(count=65536))
c["count_0"] = dict(count=0)                                                           # sample 0 is out of range
c["count_0_n_0"] = dict(count=0, n=0)                                                  # RSM_OK
c.update(n_limit=dict(n=BIG24), n_0=dict(n=0))
c.update({f"bad_{k}": dict(samples=v) for k, v in _bad(GOOD4).items()})
c["order_args_eds"] = dict(d_nodes=None, d_eds=None)
c["order_eds_aligned"] = dict(d_eds=None, d_shares=A8)
c["order_aligned_S"] = dict(d_shares=A8, S=96)
c["order_S_shape"] = dict(S=96, width=4096)
c["order_shape_n"] = dict(width=4096, n=BIG24)
c["order_n_sample"] = dict(n=BIG24, samples=[(1, 0, 0, 0)])

CASES["rsm_proofs_verify_dev"] = _verify_cases(["d_roots"])
CASES["rsm_proofs_verify_data_root_dev"] = _verify_cases(["d_root_records", "d_data_roots"])

c = CASES["rsm_data_roots_dev"] = {"null_ctx": dict(ctx=None), "width_0": dict(width=0)}
c.update(_nulls(["d_roots", "d_data_roots"]))
c["nulls_count_0"] = dict(d_roots=None, d_data_roots=None, count=0)                    # RSM_OK
c.update(root_len_31=dict(root_len=31), root_len_97=dict(root_len=97), nodes_misaligned=dict(d_nodes=A8))
c.update(width_2049=dict(width=2049), count_0=dict(count=0), count_0_no_nodes=dict(count=0, d_nodes=None))
c["order_args_root_len"] = dict(width=0, root_len=31)
c["order_root_len_aligned"] = dict(root_len=97, d_nodes=A8)
c["order_aligned_width"] = dict(d_nodes=A8, width=2049)
c["order_width_count"] = dict(width=2049, count=0)

c = CASES["rsm_root_proofs_dev"] = {"null_ctx": dict(ctx=None), "width_0": dict(width=0)}
c.update(_nulls(["d_nodes", "refs", "d_records"]))
c["nulls_n_0"] = dict(refs=None, d_records=None, n=0)                                  # RSM_OK
c.update(nodes_misaligned=dict(d_nodes=A8), width_2049=dict(width=2049), n_limit=dict(n=BIG24), n_0=dict(n=0))
c.update({f"bad_{k}": dict(refs=v) for k, v in _bad(GOOD3).items()})
c["order_args_aligned"] = dict(refs=None, d_nodes=A8)
c["order_aligned_width"] = dict(d_nodes=A8, width=2049)
c["order_width_n"] = dict(width=2049, n=BIG24)
c["order_n_ref"] = dict(n=BIG24, refs=[(1, 0, 0)])
c["count_0"] = dict(count=0)                                                           # ref 0 is out of range

c = CASES["rsm_ns_proofs_dev"] = {"null_ctx": dict(ctx=None), "width_0": dict(width=0), "no_nmt": dict(nmt=None)}
c.update(_nulls(["d_nodes", "d_status", "queries", "nids", "d_records", "d_offsets"]))
c["nulls_n_0"] = dict(queries=None, nids=None, d_records=None, d_offsets=None, n=0)    # RSM_OK
c["shares_without_eds"] = dict(d_eds=None)
c.update(shares_misaligned=dict(d_shares=A8), eds_misaligned=dict(d_eds=A8))
c.update(nodes_misaligned=dict(d_nodes=A8), offsets_misaligned=dict(d_offsets=A2), status_misaligned=dict(d_status=A2))
c.update(S_96=dict(S=96), width_2048=dict(width=2048, nmt=(8, 1, 1024)), ns_33=dict(nmt=(33, 1, 8)))
c.update(count_65536=dict(count=65536), square_size_0=dict(nmt=(8, 1, 0)), nmt_past_its_square=dict(nmt=(8, 1, 4)))
c.update(n_limit=dict(n=BIG20), n_0=dict(n=0), count_0=dict(count=0), no_shares=dict(d_shares=None, d_eds=None, n=0))
_ns_range(c)
c["order_args_nmt"] = dict(d_status=None, nmt=None)
c["order_nmt_eds"] = dict(nmt=None, d_eds=None)
c["order_eds_aligned"] = dict(d_eds=None, d_nodes=A8)
c["order_aligned_aligned"] = dict(d_shares=A8, d_offsets=A2)
c["order_aligned_S"] = dict(d_status=A2, S=96)
c["order_S_shape"] = dict(S=96, width=2048)
c["order_shape_n"] = dict(nmt=(33, 1, 8), n=BIG20)
c["order_n_count"] = dict(n=BIG20, count=0)
c["order_count_query"] = dict(count=0, queries=[(0, 2, 0)])                            # RSM_OK

ops = ["queries", "nids", "d_records", "d_offsets", "d_roots", "d_status", "d_shares"]
c = CASES["rsm_ns_proofs_verify_dev"] = {"null_ctx": dict(ctx=None), "width_0": dict(width=0), "no_nmt": dict(nmt=None)}
c.update(_nulls(ops))
c["nulls_n_0"] = dict({x: None for x in ops}, n=0)                                     # RSM_OK
c["nulls_count_0"] = dict({x: None for x in ops if x not in ("queries", "nids")}, count=0)  # RSM_OK
c["no_shares_none_expected"] = dict(d_shares=None, shares_total=0, queries=[(1, 0, 0)])  # goes on to the range check
c.update(ns_0=dict(nmt=(0, 1, 8)), ns_33=dict(nmt=(33, 1, 8)), square_size_0=dict(nmt=(8, 1, 0)))
c.update(shares_misaligned=dict(d_shares=A8), offsets_misaligned=dict(d_offsets=A2), status_misaligned=dict(d_status=A2))
c.update(S_96=dict(S=96), width_1025=dict(width=1025), short_share=dict(S=0), n_limit=dict(n=BIG20), n_0=dict(n=0))
c["count_0"] = dict(count=0)
_ns_range(c)
c["order_args_nmt"] = dict(width=0, nmt=None)
c["order_nmt_params"] = dict(d_roots=None, nmt=(0, 1, 8))
c["order_params_shares"] = dict(nmt=(33, 1, 8), d_shares=A8)
c["order_shares_offsets"] = dict(d_shares=A8, d_offsets=A2)
c["order_status_S"] = dict(d_status=A2, S=96)
c["order_S_width"] = dict(S=96, width=1025)
c["order_width_short"] = dict(width=1025, S=0)
c["order_short_n"] = dict(S=0, n=BIG20)
c["order_n_count"] = dict(n=BIG20, count=0)
c["order_count_query"] = dict(count=0, queries=[(0, 2, 0)])                            # RSM_OK

CASES["rsm_repair_squares_dev"] = _repair_cases(["d_eds", "d_presence", "d_roots", "d_work", "results"])
CASES["rsm_repair_squares_checked_dev"] = _repair_cases(["d_eds", "d_presence", "d_roots", "d_work", "results", "checks"])
CASES["rsm_vectors_gather_dev"] = _gather_scatter_cases(
    "refs", GOOD3, ["d_eds", "d_presence", "refs", "d_shares", "d_present"])
c = CASES["rsm_samples_scatter_dev"] = _gather_scatter_cases(
    "samples", GOOD4, ["d_eds", "d_presence", "samples", "d_shares", "d_status"])
c["status_misaligned"] = dict(d_status=A2)
c["order_shares_status"] = dict(d_shares=A8, d_status=A2)
c["order_status_range"] = dict(d_status=A2, samples=[(0, 0, 16, 0)])
del c, ops


def _call(lib, fn, overrides):
    names, base = FUNCS[fn]
    v = dict(base, **overrides)
    keep, args = [], []
    for name in names:
        x = v.get(name)
        if name == "n" and "n" not in v:
            arr = v.get("samples") or v.get("refs") or v.get("queries")
            x = len(arr) if arr else 1  # a NULL array of one element
        elif name in _ARRAYS and x is not None:
            x = (_ARRAYS[name] * len(x))(*[_ARRAYS[name](*e) for e in x])
        elif name == "nmt" and x is not None:
            keep.append(R.NmtParams(*x))
            x = ctypes.byref(keep[-1])
        args.append(x)
    rc = getattr(lib, fn)(*args)
    return [int(rc), (lib.rsm_last_error() or b"").decode() if rc else ""]


def record(lib):
    return {f"{fn}/{label}": _call(lib, fn, ov) for fn, cases in CASES.items() for label, ov in cases.items()}


def test_every_entry_point_has_cases():
    assert set(CASES) == set(FUNCS)
    for fn, (names, _) in FUNCS.items():
        assert len(names) == len(R.SIGNATURES[fn][1]), fn


def test_error_surface_matches_the_recorded_one(lib):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = record(lib)
    assert set(got) == set(want)
    for key in want:
        assert got[key] == want[key], key
    # nothing got as far as the device, and each function returns its early RSM_OK somewhere
    assert all(rc != R.RSM_EDEVICE for rc, _ in got.values())
    for fn in CASES:
        assert any(got[f"{fn}/{label}"][0] == R.RSM_OK for label in CASES[fn]), fn


if __name__ == "__main__":
    out = record(R.library())
    reached = [key for key, (rc, _) in out.items() if rc == R.RSM_EDEVICE]
    if reached:
        sys.exit(f"these cases reach the device: {reached}")
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases -> {GOLDEN}")
