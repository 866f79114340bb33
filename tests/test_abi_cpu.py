"""CPU: what the single-GPU entry points of the C ABI launch.  tests/native/abi_check.cpp
drives every entry point that builds a CodewordSet or a DecodeSet (device and host
extensions, their phases, row / column ranges and blocks, the Codec, batch encode,
vector decode, Repair's decode sweeps by rows and by columns and its verifyEncoding,
the latter also by a corrupted cell that only the re-encoding can find) through the
product's host code, built against a stubbed HIP runtime whose launches compute with
the C oracle (tests/native/hip_stub.cpp, RSM_STUB_ORACLE), and compares the results
with the oracle's own extension, encode and decode.  Built twice: plain, and with
AddressSanitizer and UBSan on every translation unit, so a descriptor that points
outside its buffers is reported even where the bytes happen to agree.

Not reached here: the bit-sliced, queue and fused launches (the stub declines them) and
Repair's zero-copy row sweep with its column re-encode (eds.cpp
fast_repair_rows_zero_copy: 65 <= k <= 128 or GF(2^16), and leaf / tree launches the
stub does not compute); tests/test_gpu_eds.py::test_repair_half_of_each_row* and
tests/test_gpu_runtime.py check those on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rsmt2d_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
CPP = [os.path.join(CSRC, f) for f in ("rsm_runtime.cpp", "rsm_multi.cpp", "eds.cpp", "merkle.cpp", "gf16_tables.cpp")] + [
    os.path.join(NATIVE, f) for f in ("hip_stub.cpp", "rccl_stub.cpp", "abi_check.cpp")]
ORACLE_C = os.path.join(ROOT, "oracle", "leopard_oracle.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def _build(tmp, san):
    extra = SAN if san else []
    flags = ["-O1", "-g", *extra, "-D__HIP_PLATFORM_AMD__", "-DRSM_STUB_ORACLE", "-I/opt/rocm/include"]
    procs, objs = [], []
    for s in CPP + [ORACLE_C]:
        o = os.path.join(tmp, os.path.basename(s) + (".san" if san else "") + ".o")
        lang = ["-x", "c", "-std=c11"] if s.endswith(".c") else ["-x", "c++", "-std=c++20"]
        procs.append((s, subprocess.Popen([CXX, *flags, *lang, "-c", s, "-o", o], stdout=subprocess.PIPE,
                                          stderr=subprocess.STDOUT)))
        objs.append(o)
    for s, p in procs:
        out = p.communicate(timeout=600)[0].decode(errors="replace")
        assert p.returncode == 0, f"{s}:\n{out[-3000:]}"
    exe = os.path.join(tmp, "abi_check" + ("_san" if san else ""))
    subprocess.run([CXX, *extra, *objs, "-o", exe, "-lpthread"], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("ROCm clang++ not present")
    return str(tmp_path_factory.mktemp("abi"))


@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan_ubsan"])
def test_entry_points_launch_what_the_oracle_computes(tmp, san):
    exe = _build(tmp, san)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, timeout=600, env=env)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-6000:]
    assert "Sanitizer" not in err and "runtime error" not in err, err[-6000:]
    assert b"abi_check: ok" in r.stdout
