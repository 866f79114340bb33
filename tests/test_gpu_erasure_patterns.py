"""GPU: the decoders on structured erasure patterns, against the definitional codeword.

The decoders build the error locator from a log-domain Walsh transform of the presence
vector, whose modular sums may equal the modulus.  Random erasures almost never produce
the many zero or modulus-valued terms that structured ones do: all data missing, all
parity missing, a single erasure at 0, k - 1, k or 2k - 1, every other cell, a
contiguous block, half of each half, a coset of a subspace (bit 5 set), nothing missing
(``rs_definition.erasure_patterns``).

The inputs are consistent, so the answer is unique: the codeword of the definition
(``rs_definition``), compared bit-exact with no oracle in between.  Decode of
INCONSISTENT input (the byzantine formula, what a decoder returns when the present
shares lie on no codeword) stays pinned to the oracle only: tests/test_gpu_codec.py,
tests/test_gpu_eds.py.

Squares for rsm_decode_vectors_dev: a single-axis decode treats every vector as an
independent codeword, so the square's vectors need not form a two-dimensional extension.
Vector v is the XOR of a subset of a few definitional codewords with its symbol
positions rotated -- a codeword again, because the code is linear and acts on every
symbol position alike (addition is XOR in the definition) -- which keeps every vector
distinct at k = 512 without 2k definitional encodes.
"""
import ctypes

import numpy as np
import pytest

import rs_definition as rsd
import rsmt2d_amd as R

pytestmark = pytest.mark.gpu

CODEC_KS = [1, 2, 3, 5, 33, 64, 65, 100, 128, 129, 200, 256, 257, 400, 512, 513, 1025]
NPAT = len(rsd.PATTERN_NAMES)


def _rng(*key):
    return np.random.default_rng([0xE7A5] + [int(x) for x in key])


@pytest.mark.parametrize("k,S", [(k, 64) for k in CODEC_KS] + [(100, 320), (400, 320)])
def test_codec_decode_structured_patterns(lib, k, S):
    """Codec.Decode (rsm_decode), every pattern: k <= 64 decode_gf8_kernel<M>;
    65 <= k <= 128 decode_gf8_split_kernel<16, true> (one codeword: the per-wave locator);
    m = 256 errloc16_kernel + dec16f_kernel; m = 512 errloc16_kernel + dec16h_kernel;
    k > 512 errloc16g_kernel + g16_pass_kernel / g16_deriv_kernel."""
    data = _rng(1, k, S).integers(0, 256, (k, S), dtype=np.uint8)
    full = rsd.codeword(data)
    codec = R.NewLeoRSCodec()
    pats = rsd.erasure_patterns(k)
    assert tuple(pats) == rsd.PATTERN_NAMES
    for name, missing in pats.items():
        sh = list(full)
        for p in missing:
            sh[p] = None
        assert codec.Decode(sh) == full, (k, name)


# ---------------------------------------------------------------------------
# rsm_decode_vectors_dev
# ---------------------------------------------------------------------------
_squares = {}


def _codeword_square(k, S):
    """[2k][2k][S] whose ROWS are codewords (module docstring); cached, never modified."""
    if (k, S) not in _squares:
        W = 2 * k
        c = 8   # 255 subsets x 32 rotations: more than the 2k <= 1024 vectors needed
        base = np.stack([np.concatenate([d, rsd.parity_array(d)])
                         for d in _rng(2, k, S).integers(0, 256, (c, k, S), dtype=np.uint8)])   # [c][2k][S]
        sq = np.zeros((W, W, S), np.uint8)
        ncomb = (1 << c) - 1
        for v in range(W):
            combo, shift = v % ncomb + 1, v // ncomb
            row = np.zeros((W, S), np.uint8)
            for b in range(c):
                if (combo >> b) & 1:
                    row ^= base[b]
            # rotate the symbol positions of every 64-byte block: both 32-byte halves alike,
            # so GF(2^16) symbols (byte[t] | byte[32 + t] << 8) move whole
            sq[v] = np.roll(row.reshape(W, S // 64, 2, 32), shift, axis=3).reshape(W, S)
        assert len({sq[v].tobytes() for v in range(W)}) == W
        sq.setflags(write=False)
        _squares[(k, S)] = sq
    return _squares[(k, S)]


def _presence(k):
    """[2k][2k] presence of the row form: vector v takes pattern v mod NPAT."""
    W = 2 * k
    pats = list(rsd.erasure_patterns(k).values())
    pres = np.ones((W, W), np.uint8)
    for v in range(W):
        pres[v, pats[v % NPAT]] = 0
    return pres


def _decode(lib, ctx, dmg, pres, k, S, axis, vecs):
    bufs = [R.DeviceBuffer(dmg.nbytes), R.DeviceBuffer(pres.nbytes), R.DeviceBuffer(4 * len(vecs))]
    try:
        bufs[0].upload(dmg)
        bufs[1].upload(pres)
        bufs[2].upload(np.asarray(vecs, dtype=np.uint32))
        R._check(lib.rsm_decode_vectors_dev(ctx, bufs[0].ptr, bufs[1].ptr, k, S, axis, bufs[2].ptr, len(vecs), None))
        R._check(lib.rsm_sync(ctx))
        return bufs[0].download(dmg.nbytes).reshape(dmg.shape)
    finally:
        for b in bufs:
            b.free()


def _run_patterns(lib, ctx, k, S, axis):
    W = 2 * k
    rows = _codeword_square(k, S)
    pres = _presence(k)
    want = rows
    if axis == 1:  # the columns are the codewords
        want = np.ascontiguousarray(rows.transpose(1, 0, 2))
        pres = np.ascontiguousarray(pres.T)
    dmg = want * pres[:, :, None]   # missing cells zeroed, as the callers of the device decode do
    # one launch covers every pattern
    got = _decode(lib, ctx, dmg, pres, k, S, axis, range(W))
    assert np.array_equal(got, want)
    # the same launch over every third vector: the others -- with damaged filler bytes in
    # their present cells -- and every present cell keep their bytes exactly
    listed = np.arange(0, W, 3)
    unlisted = np.setdiff1d(np.arange(W), listed)
    filler = _rng(3, k, S, axis).integers(0, 256, (len(unlisted), W, S), dtype=np.uint8)
    dmg2 = dmg.copy()
    if axis == 0:
        dmg2[unlisted] ^= filler * pres[unlisted][:, :, None]
    else:
        dmg2[:, unlisted] ^= filler.transpose(1, 0, 2) * pres[:, unlisted][:, :, None]
    want2 = dmg2.copy()
    if axis == 0:
        want2[listed] = want[listed]
    else:
        want2[:, listed] = want[:, listed]
    got2 = _decode(lib, ctx, dmg2, pres, k, S, axis, listed)
    m = pres.astype(bool)
    assert np.array_equal(got2[m], dmg2[m]), "a cell marked present changed"
    assert np.array_equal(got2, want2)


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("k,S", [(64, 64), (128, 64), (128, 320), (256, 64), (512, 64)])
def test_decode_vectors_structured_patterns(lib, k, S, axis):
    """rsm_decode_vectors_dev, vector v on pattern v mod 12: k = 64 decode_gf8_kernel<64>;
    k = 128 decode_gf8_split_kernel<16, false> (over 64 tasks: wave 0's locator; the
    every-third launch at S = 64 has 86 tasks, still that form); k = 256 errloc16_kernel<256>
    + dec16f_kernel; k = 512 errloc16_kernel<512> + dec16h_kernel."""
    _run_patterns(lib, R.device_context(0), k, S, axis)


@pytest.fixture
def pctx(lib):
    """A private context: its limits are lowered, the shared one keeps the defaults."""
    h = ctypes.c_void_p()
    R._check(lib.rsm_ctx_create(0, ctypes.byref(h)))
    yield h.value
    lib.rsm_ctx_destroy(h.value)


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("k,S", [(64, 64), (200, 64)])
def test_decode_vectors_structured_patterns_wide(lib, pctx, k, S, axis):
    """The wide decoders (offset_limit = 1): decode_gf8_wide_kernel<64>, and for k = 200
    the multi-pass GF(2^16) form (errloc16g_kernel, g16_pass_kernel, g16_deriv_kernel)."""
    R._check(lib.rsm_ctx_set_limits(pctx, 1, 0))
    try:
        _run_patterns(lib, pctx, k, S, axis)
    finally:
        R._check(lib.rsm_ctx_set_limits(pctx, 0, 0))
