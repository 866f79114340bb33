"""CPU: the parts of namespace-proof verification on the device that need no GPU: the
export and its ctypes mirror, the argument check that precedes any device work, and
verify_namespace_data (the client side of NamespaceData) on its host path
(NamespaceProof.verify per row), for an honest answer and the three dishonest ones a
server can give: a row dropped, a range narrowed, a share of another namespace."""
import ctypes

import pytest

import ns_proofs as H
import rsmt2d_amd as R
from ns_verify_calls import S, answers, namespace_data_cases

K = 4


def test_export_and_mirror(lib):
    assert "rsm_ns_proofs_verify_dev" in R.SIGNATURES
    fn = lib.rsm_ns_proofs_verify_dev
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 15
    assert (R.RSM_PROOF_NAMESPACE, R.RSM_PROOF_INCOMPLETE) == (H.NAMESPACE, H.INCOMPLETE)


def test_null_context(lib):
    p = R.NmtParams(8, 1, 2)
    q = (R.NsQuery * 1)(R.NsQuery(0, 0, 0))
    rc = lib.rsm_ns_proofs_verify_dev(None, None, None, None, 0, None, 4, S, 1, ctypes.byref(p), q, bytes(8), 1, None, None)
    assert rc == R.RSM_EINVAL


@pytest.mark.parametrize("ns", [8, 29])
def test_verify_namespace_data_host(lib, ns):
    for case in namespace_data_cases(K, ns):
        for name, data, want in answers(case):
            got = R.verify_namespace_data(case.roots, case.nid, data, case.p, 2 * K, device=None)
            assert got == want, (ns, case.what, name, got, want)


def test_verify_namespace_data_arguments(lib):
    case = namespace_data_cases(K, 8)[0]
    with pytest.raises(R.RSMError):
        R.verify_namespace_data(case.roots[:-1], case.nid, case.data, case.p, 2 * K, device=None)
    with pytest.raises(R.RSMError):
        R.verify_namespace_data(case.roots, case.nid + b"\x00", case.data, case.p, 2 * K, device=None)
    with pytest.raises(R.RSMError):
        R.verify_namespace_data(case.roots, case.nid, [(2 * K, case.data[0][1])], case.p, 2 * K, device=None)
