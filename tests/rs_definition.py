"""The Reed-Solomon code of the codec, from its algebraic definition (plain numpy).

Test helper, next to ``proof_verify.py``.  It imports neither ``oracle`` nor
``rsmt2d_amd`` and shares none of their machinery: no FFT, no skew table, no Walsh
transform.  Its only inputs are two pieces of data, copied below: the field polynomials
and the two Cantor bases.  Everything else is derived here.

Field.  A *label* x (the integer a share byte or 16-bit symbol holds) stands for the
element  sum_j bit_j(x) * basis[j]  written in the polynomial representation modulo the
field polynomial.  Addition is XOR of labels (the map is linear); multiplication goes
through the polynomial representation.  basis[0] == 1, so label 1 is the identity.

Code.  With m = ceil_pow2(k), P is the unique polynomial of degree < m with
P(label m + j) = data[j] for j < m, where data[j] = 0 for j >= k.  Parity share i
(i < k) is P(label i).  The 2k-share codeword is data followed by parity.

GF(2^8) serves 2k <= 256, one symbol per byte.  GF(2^16) serves 2k > 256: each 64-byte
block of a share holds 32 symbols, symbol t being ``byte[t] | byte[32 + t] << 8``.
"""
import numpy as np

# --- data: the field polynomials and the Cantor bases (constants, not code) ---
POLY8 = 0x11D
BASIS8 = (1, 214, 152, 146, 86, 200, 88, 230)
POLY16 = 0x1002D
BASIS16 = (0x0001, 0xACCA, 0x3C0E, 0x163E, 0xC582, 0xED2E, 0x914C, 0x4012,
           0x6C98, 0x10D8, 0x6A72, 0xB900, 0xFDB8, 0xFB34, 0xFF38, 0x991E)


class Field:
    """exp/log arrays over labels.  ``log[0]`` is a sentinel that ``exp`` maps to 0, so
    products need no zero test: exp[log[a] + log[b]] (no reduction: exp is extended)."""

    def __init__(self, bits, poly, basis):
        self.bits = bits
        self.order = 1 << bits
        self.mod = self.order - 1
        n = self.order
        # element (polynomial representation) of every label
        elem = np.zeros(n, dtype=np.int64)
        for j, b in enumerate(basis):
            w = 1 << j
            elem[w:2 * w] = elem[:w] ^ b
        assert len(np.unique(elem)) == n, "basis is not a basis"
        # discrete log of every element to the generator x (the polynomial 2)
        dlog = np.zeros(n, dtype=np.int64)
        state = 1
        for i in range(self.mod):
            dlog[state] = i
            state <<= 1
            if state >= n:
                state ^= poly
        assert state == 1, "x does not generate the field"
        self.zero = 2 * self.mod          # log of label 0: past every real sum
        log = dlog[elem]
        log[0] = self.zero
        self.log = log
        exp = np.zeros(2 * self.zero + 1, dtype=np.int64)
        labels = np.arange(1, n)
        exp[log[labels]] = labels
        exp[self.mod:2 * self.mod - 1] = exp[:self.mod - 1]
        self.exp = exp
        assert self.exp[self.log[1]] == 1 and self.log[1] == 0

    def mul(self, a, b):
        return self.exp[self.log[np.asarray(a)] + self.log[np.asarray(b)]]


_fields = {}


def field_bits(k):
    return 8 if 2 * k <= 256 else 16


def field(k):
    bits = field_bits(k)
    if bits not in _fields:
        _fields[bits] = Field(8, POLY8, BASIS8) if bits == 8 else Field(16, POLY16, BASIS16)
    return _fields[bits]


def ceil_pow2(k):
    m = 1
    while m < k:
        m <<= 1
    return m


def lagrange_matrix(k):
    """log G, [k, k]: G[i][j] = prod_{l != j} (i - x_l) / (x_j - x_l) over the m points
    x_l = label m + l, literally (subtraction is XOR).  Entries are never zero."""
    F = field(k)
    m = ceil_pow2(k)
    i = np.arange(k).reshape(k, 1)
    j = np.arange(k).reshape(1, k)
    num = np.zeros((k, k), dtype=np.int64)
    den = np.zeros((k, k), dtype=np.int64)
    for l in range(m):
        keep = (j != l)
        num += np.where(keep, F.log[i ^ (m + l)], 0)
        den += np.where(keep, F.log[((m + j) ^ (m + l)) | (~keep)], 0)   # |1 at l == j: unused
    return (num - den) % F.mod


def cauchy_rows(k, rows):
    """log G for the listed parity rows, [len(rows), k]: G[i][j] = C_m / (i ^ j ^ m) with
    C_m = prod_{x=m}^{2m-1} x / prod_{v=1}^{m-1} v.  (The data points are the coset
    m + {0..m-1} of a subspace, so both Lagrange products collapse.)"""
    F = field(k)
    m = ceil_pow2(k)
    c = (int(F.log[np.arange(m, 2 * m)].sum()) - int(F.log[np.arange(1, m)].sum())) % F.mod
    i = np.asarray(rows, dtype=np.int64).reshape(-1, 1)
    j = np.arange(k).reshape(1, k)
    return (c - F.log[i ^ j ^ m]) % F.mod


def cauchy_matrix(k):
    return cauchy_rows(k, np.arange(k))


# --- symbols <-> bytes ---
def _to_symbols(bits, a):
    """[..., S] uint8 -> [..., nsym] int64 labels."""
    a = np.asarray(a, dtype=np.uint8)
    if bits == 8:
        return a.astype(np.int64)
    S = a.shape[-1]
    assert S % 64 == 0
    b = a.reshape(a.shape[:-1] + (S // 64, 2, 32)).astype(np.int64)
    return (b[..., 0, :] | (b[..., 1, :] << 8)).reshape(a.shape[:-1] + (S // 2,))


def _to_bytes(bits, s):
    if bits == 8:
        return s.astype(np.uint8)
    n = s.shape[-1]
    b = s.reshape(s.shape[:-1] + (n // 32, 1, 32))
    out = np.concatenate([b & 0xFF, b >> 8], axis=-2)
    return out.reshape(s.shape[:-1] + (2 * n,)).astype(np.uint8)


def _apply(F, logG, sym, budget=1 << 21):
    """out[r, n] = XOR_j G[r][j] * sym[j][n];  logG [R, k], sym [k, N] labels."""
    R, k = logG.shape
    N = sym.shape[1]
    logD = F.log[sym]
    out = np.zeros((R, N), dtype=np.int64)
    step = max(1, budget // max(1, R * N))
    for j0 in range(0, k, step):
        t = F.exp[logG[:, j0:j0 + step, None] + logD[None, j0:j0 + step, :]]
        out ^= np.bitwise_xor.reduce(t, axis=1)
    return out


def _as_array(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.stack([np.frombuffer(bytes(d), dtype=np.uint8) for d in data])


def parity_array(data, rows=None):
    """data [k, S] uint8 -> the listed parity shares [len(rows), S] (all k by default)."""
    data = _as_array(data)
    k = data.shape[0]
    F = field(k)
    rows = np.arange(k) if rows is None else np.asarray(rows)
    out = _apply(F, cauchy_rows(k, rows), _to_symbols(F.bits, data))
    return _to_bytes(F.bits, out)


def parity_shares(data, rows):
    """Only the listed parity shares, as bytes (for large k)."""
    return [p.tobytes() for p in parity_array(data, rows)]


def encode(data):
    """k data shares -> k parity shares (bytes)."""
    return [p.tobytes() for p in parity_array(data)]


def codeword(data):
    """k data shares -> the 2k shares (bytes)."""
    return [bytes(d) for d in _as_array(data)] + encode(data)


def encode_vectors(vecs, rows=None):
    """vecs [V, k, S]: V independent data vectors -> [V, len(rows), S] parity."""
    V, k, S = vecs.shape
    F = field(k)
    rows = np.arange(k) if rows is None else np.asarray(rows)
    sym = _to_symbols(F.bits, vecs)                      # [V, k, n]
    n = sym.shape[-1]
    flat = sym.transpose(1, 0, 2).reshape(k, V * n)
    out = _apply(F, cauchy_rows(k, rows), flat)          # [R, V*n]
    out = out.reshape(len(rows), V, n).transpose(1, 0, 2)
    return _to_bytes(F.bits, np.ascontiguousarray(out))


def extend_square(ods, rows=None, cols=None):
    """ods [k, k, S] uint8.

    With neither ``rows`` nor ``cols``: the full [2k, 2k, S] EDS.  Q1 = row parity of Q0,
    Q2 = column parity of Q0, Q3 = column parity of Q1.

    Otherwise a tuple ``(q1_rows, q2_cols, q3_cols)``: ``q1_rows[a]`` is eds[rows[a], k:],
    ``q2_cols[:, b]`` is eds[k:, cols[b]] and ``q3_cols[:, b]`` is eds[k:, k + cols[b]],
    the last taken from the definitional Q1 column (one parity share of every row).
    """
    ods = np.ascontiguousarray(ods, dtype=np.uint8)
    k, k2, S = ods.shape
    assert k == k2
    if rows is None and cols is None:
        eds = np.empty((2 * k, 2 * k, S), dtype=np.uint8)
        eds[:k, :k] = ods
        eds[:k, k:] = encode_vectors(ods)                                   # rows of Q0
        eds[k:, :] = encode_vectors(eds[:k].transpose(1, 0, 2)).transpose(1, 0, 2)
        return eds
    rows = [] if rows is None else list(rows)
    cols = [] if cols is None else list(cols)
    q1_rows = encode_vectors(ods[rows]) if rows else np.empty((0, k, S), np.uint8)
    if cols:
        q2_cols = encode_vectors(ods[:, cols].transpose(1, 0, 2)).transpose(1, 0, 2)
        q1_cols = encode_vectors(ods, rows=cols)                            # [k, C, S]
        q3_cols = encode_vectors(q1_cols.transpose(1, 0, 2)).transpose(1, 0, 2)
    else:
        q2_cols = q3_cols = np.empty((k, 0, S), np.uint8)
    return q1_rows, q2_cols, q3_cols


# --- the structured erasure patterns shared by the CPU and GPU decode tests ---
def erasure_patterns(k):
    """name -> sorted list of missing positions of a 2k-cell vector (never more than k)."""
    n = 2 * k
    pats = {
        "all_data": list(range(k)),
        "all_parity": list(range(k, n)),
        "one_at_0": [0],
        "one_at_k-1": [k - 1],
        "one_at_k": [k],
        "one_at_2k-1": [n - 1],
        "even": list(range(0, n, 2))[:k],
        "odd": list(range(1, n, 2))[:k],
        "block_mid": list(range(k // 2, k // 2 + k)),
        "half_data_half_parity": list(range(k // 2)) + list(range(k, k + k // 2)),
        "bit5": [p for p in range(n) if p & 32][:k],
        "none": [],
    }
    for v in pats.values():
        assert len(v) <= k and all(0 <= p < n for p in v)
    return pats


PATTERN_NAMES = ("all_data", "all_parity", "one_at_0", "one_at_k-1", "one_at_k", "one_at_2k-1",
                 "even", "odd", "block_mid", "half_data_half_parity", "bit5", "none")


def sample_indices(n, count=16, always=(), seed=0x5EED):
    """Sorted sample of range(n): ``always`` plus seeded picks, at least ``count`` of them
    (or all of range(n) if smaller)."""
    pick = set(int(a) for a in always if 0 <= a < n)
    if n <= count:
        return list(range(n))
    g = np.random.default_rng(seed + n)
    while len(pick) < count:
        pick.add(int(g.integers(0, n)))
    return sorted(pick)
