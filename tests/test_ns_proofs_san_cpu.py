"""CPU: merkle.cpp's namespace proofs under AddressSanitizer and UBSan, as a stand-alone
program (tests/native/ns_proof_host.cpp): every record, root and share buffer is a heap
allocation of exactly its documented size, headers are driven to every boundary value,
and an inclusion record cut off after its derived nodes must still verify."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
SRC = [os.path.join(ROOT, "rsmt2d_amd", "csrc", "merkle.cpp"), os.path.join(ROOT, "tests", "native", "ns_proof_host.cpp")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_namespace_proofs_under_sanitizers(tmp_path):
    if not os.path.exists(CXX):
        pytest.skip("ROCm clang++ not present")
    exe = str(tmp_path / "ns_proof_host")
    b = subprocess.run([CXX, "-O1", "-g", *SAN, "-std=c++20", *SRC, "-o", exe], capture_output=True, timeout=600)
    assert b.returncode == 0, b.stderr.decode(errors="replace")[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, timeout=600, env=env)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-6000:]
    assert "Sanitizer" not in err and "runtime error" not in err, err[-6000:]
    assert b"ns_proof_host: ok" in r.stdout
