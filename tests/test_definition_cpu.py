"""CPU: the oracle pinned, at every size class, to the algebraic definition of the code.

``rs_definition`` derives the code from the field polynomials and the Cantor bases alone
(Lagrange interpolation, and the Cauchy closed form it reduces to).  The definition's
constants and point order are pinned to the reference by its 1x1 and 2x2 grids
(``golden/kat_grids.json``); the oracle (encode, extend_square, and decode of consistent
input) is then pinned to the definition.  Every comparison is bit-exact.
"""
import json
import os

import numpy as np
import pytest

import oracle
import rs_definition as rsd

GOLD = os.path.join(os.path.dirname(__file__), "golden")

LAGRANGE_KS = list(range(1, 65)) + [65, 100, 127, 128, 129, 200, 256]
ENCODE_KS = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32, 33, 64, 65, 100, 127, 128,
             129, 130, 200, 255, 256, 257, 300, 511, 512]
LARGE_KS = [513, 1000, 1024, 1025, 4100, 16385, 32768]
DECODE_KS = [1, 2, 3, 5, 33, 64, 65, 100, 128, 129, 200, 256, 257, 400, 512, 513, 1025]


def _rng(*key):
    return np.random.default_rng([0x52534D54] + [int(x) for x in key])


@pytest.mark.parametrize("k", LAGRANGE_KS)
def test_lagrange_equals_cauchy(k):
    assert np.array_equal(rsd.lagrange_matrix(k), rsd.cauchy_matrix(k))


@pytest.mark.parametrize("name", ["1x1", "2x2"])
def test_definition_reproduces_reference_grids(name):
    """The reference's own known answers, from the definition alone (no oracle)."""
    kat = json.load(open(os.path.join(GOLD, "kat_grids.json")))[name]
    ods = np.array(kat["ods"], dtype=np.uint8)
    want = np.array(kat["eds"], dtype=np.uint8)
    eds = rsd.extend_square(np.repeat(ods[:, :, None], 64, axis=2))
    assert np.array_equal(eds, np.repeat(want[:, :, None], 64, axis=2))


@pytest.mark.parametrize("S", [64, 192])
@pytest.mark.parametrize("k", ENCODE_KS)
def test_oracle_encode_equals_definition(k, S):
    data = _rng(1, k, S).integers(0, 256, (k, S), dtype=np.uint8)
    got = oracle.encode([d.tobytes() for d in data])
    assert got == rsd.encode(data)


@pytest.mark.parametrize("k", LARGE_KS)
def test_oracle_encode_equals_definition_sampled(k):
    S = 64
    data = _rng(2, k).integers(0, 256, (k, S), dtype=np.uint8)
    rows = rsd.sample_indices(k, 16, always=(0, 1, k // 2, k - 1))
    assert len(rows) >= 16 and {0, 1, k // 2, k - 1} <= set(rows)
    got = oracle.encode([d.tobytes() for d in data])
    assert [got[r] for r in rows] == rsd.parity_shares(data, rows)


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 16, 33])
def test_oracle_extend_square_equals_definition(k):
    ods = _rng(3, k).integers(0, 256, (k, k, 64), dtype=np.uint8)
    assert np.array_equal(oracle.extend_square(ods), rsd.extend_square(ods))


@pytest.mark.parametrize("k", [128, 130])
def test_oracle_extend_square_equals_definition_sampled(k):
    ods = _rng(4, k).integers(0, 256, (k, k, 64), dtype=np.uint8)
    idx = rsd.sample_indices(k, 6, always=(0, k // 2, k - 1))
    assert {0, k // 2, k - 1} <= set(idx)
    eds = oracle.extend_square(ods, nthreads=4)
    q1_rows, q2_cols, q3_cols = rsd.extend_square(ods, rows=idx, cols=idx)
    assert np.array_equal(eds[:k, :k], ods)
    assert np.array_equal(eds[idx, k:], q1_rows)
    assert np.array_equal(eds[k:, idx], q2_cols)
    assert np.array_equal(eds[k:][:, [k + c for c in idx]], q3_cols)


_codewords = {}


def _codeword(k):
    if k not in _codewords:
        data = _rng(5, k).integers(0, 256, (k, 64), dtype=np.uint8)
        _codewords[k] = rsd.codeword(data)
    return _codewords[k]


@pytest.mark.parametrize("k", DECODE_KS)
def test_oracle_decode_structured_patterns(k):
    """Consistent input has a unique answer: the definitional codeword."""
    full = _codeword(k)
    pats = rsd.erasure_patterns(k)
    assert tuple(pats) == rsd.PATTERN_NAMES
    for name, missing in pats.items():
        sh = list(full)
        for p in missing:
            sh[p] = None
        assert oracle.decode(sh) == full, (k, name)
