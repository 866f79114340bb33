"""CPU model of the half-split exchange the k = 128 set body runs (the generated blocks
of rsmt2d_amd/csrc/bs8_small.inc and bs8_small_diag.inc written by
gen/gen_bs8_small.cpp emit_phase_x / emit_read_tail, and the address constants of
kernels_gf8_bs.hip bs_split_wave).

Every ds_write_b32 / ds_write_b64 / ds_read_b64 line is parsed with its operand, base
register and offset and executed on a model of the LDS for 8 waves x 64 lanes: half G
is a transpose (wave u's register 8G + v arrives as wave v's register 8G + u in the same
lane), no two stores of one exchange alias, and the footprint stays inside the 128 KiB
exchange region.  The VALU text of the store windows that hold a large IFFT / FFT (and,
for the diagnostic forms that move its tail, of the read statements that hold it) is
executed in kernel order and compared with the oracle's butterflies, as
test_bs8_asm_cpu.py does for the unsplit blocks.  Operands are identified by parsing
each block's constraint list, not by position.  The GPU code never runs here."""
import os
import re

import numpy as np
import pytest

from test_bs8_asm_cpu import GEN, M32, butterfly, gf, planes, tp_fn, unplanes  # noqa: F401 (gf: fixture)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rsmt2d_amd", "csrc")
XCH_BYTES = 128 * 1024  # the exchange region: 4 plane pairs x 8 x 8 entries of 512 B
OPERAND = re.compile(r'"([=+&]*[vs])"\(([^()]*(?:\([^()]*\))?[^()]*)\)')
DS = re.compile(r'"(ds_write_b32|ds_write_b64) %(\d+), %(\d+) offset:(\d+)|"(ds_read_b64) %(\d+), %(\d+) offset:(\d+)')

# (store window, read statement) of each exchange in kernel order, production first
PRODUCTION = [("ph_w0_tr1_w64", "xch_read_h0", 0), ("ph_w1_lifft0_w64", "xch_read_h1", 1),
              ("ph_w0_lfft1_w64", "xch_read_h0", 0), ("ph_w1_tr0_w64", "xch_read_h1", 1)]
DIAGNOSTIC = [("ph_w1_lifft0a", "xch_read_h1_lifft0b", 1), ("ph_w0_lfft1a", "xch_read_h0_lfft1b", 0),
              ("ph_w1_lifft0a_w64", "xch_read_h1_lifft0b", 1), ("ph_w0_lfft1a_w64", "xch_read_h0_lfft1b", 0),
              ("ph_w0_tr1", "xch_read_h0", 0), ("ph_w1_lifft0", "xch_read_h1", 1),
              ("ph_w0_lfft1", "xch_read_h0", 0), ("ph_w1_tr0", "xch_read_h1", 1)]


@pytest.fixture(scope="module")
def text():
    """bs8_small.inc (the product's blocks, then a section under RSM_DIAG) followed by
    bs8_small_diag.inc (blocks of the diagnostic build only)."""
    small = open(os.path.join(CSRC, "bs8_small.inc")).read()
    assert "#ifdef RSM_DIAG" in small
    return small + open(os.path.join(CSRC, "bs8_small_diag.inc")).read()


@pytest.fixture(scope="module")
def kernel():
    return open(os.path.join(CSRC, "kernels_gf8_bs.hip")).read()


def whole(text, name):
    """A generated function: (C text before the asm, asm text, C text after it)."""
    fn = re.search(r"void %s\(.*?\{(.*?)\n\}" % name, text, re.S).group(1)
    head, rest = fn.split("asm volatile(", 1)
    asm, tail = rest.split(");\n", 1) if ");\n" in rest else (rest, "")
    return head, asm, tail


def operands(asm):
    """Operand number -> C expression, from the constraint list (outputs, then inputs)."""
    return [m.group(2).strip() for m in OPERAND.finditer(asm)]


def addresses(kernel):
    """Per-(wave, lane) byte addresses the kernel passes: writer base, reader base and
    the distance of the second address register."""
    m = re.search(r"xw = lds_base \+ lane \* (\d+)u \+ A \* (\d+)u, xr = lds_base \+ lane \* (\d+)u \+ A \* (\d+)u;", kernel)
    assert m, "exchange address constants not found"
    wl, wa, rl, ra = map(int, m.groups())
    A = np.arange(8)[:, None]
    lane = np.arange(64)[None, :]
    hi = {int(x) for x in re.findall(r"\(X, x[wr], x[wr] \+ (\d+)u\)", kernel)}
    assert len(hi) == 1
    return A * wa + lane * wl, A * ra + lane * rl, hi.pop()


def token(half):
    """Distinct value of register X[8 half + r][p] of wave u, lane l: shape [8][8][8][64]."""
    u, r, p, l = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), np.arange(64), indexing="ij")
    return ((((half * 8 + u) * 8 + r) * 8 + p) * 64 + l + 1).astype(np.int64)


def run_stores(text, name, G, wbase, hi, lds, hits):
    head, asm, _ = whole(text, name)
    ops = operands(asm)
    tok = token(G)
    pair = re.search(r"T\[v\]\[q\] = \(uint64_t\)X\[(\d+) \+ v\]\[2 \* q\] \| \(\(uint64_t\)X\[(\d+) \+ v\]\[2 \* q \+ 1\] << 32\)", head)
    n = 0
    for m in DS.finditer(asm):
        if not m.group(1):
            continue
        base = {"va": wbase, "vb": wbase + hi}[ops[int(m.group(2))]]
        addr = base + int(m.group(4))
        src = ops[int(m.group(3))]
        if m.group(1) == "ds_write_b64":
            assert pair and int(pair.group(1)) == int(pair.group(2)) == 8 * G, name
            v, q = map(int, re.fullmatch(r"T\[(\d)\]\[(\d)\]", src).groups())
            assert (addr % 8 == 0).all(), (name, m.group(0))
            words = [(addr // 4, tok[:, v, 2 * q, :]), (addr // 4 + 1, tok[:, v, 2 * q + 1, :])]
        else:
            j, p = map(int, re.fullmatch(r"X\[(\d+)\]\[(\d)\]", src).groups())
            assert j // 8 == G, (name, src)
            assert (addr % 4 == 0).all()
            words = [(addr // 4, tok[:, j % 8, p, :])]
        for w, val in words:
            assert w.min() >= 0 and w.max() < XCH_BYTES // 4, (name, m.group(0))
            np.add.at(hits, w.ravel(), 1)
            lds[w.ravel()] = val.ravel()
        n += 1
    return n, asm


def run_reads(text, name, G, rbase, hi, lds):
    _, asm, tail = whole(text, name)
    ops = operands(asm)
    assert re.search(r"X\[%d \+ u\]\[2 \* q\] = \(uint32_t\)T\[u\]\[q\];" % (8 * G), tail), name
    assert re.search(r"X\[%d \+ u\]\[2 \* q \+ 1\] = \(uint32_t\)\(T\[u\]\[q\] >> 32\);" % (8 * G), tail), name
    got = np.zeros((8, 8, 8, 64), np.int64)  # [reader wave][register u][plane][lane]
    n = 0
    for m in DS.finditer(asm):
        if not m.group(5):
            continue
        u, q = map(int, re.fullmatch(r"T\[(\d)\]\[(\d)\]", ops[int(m.group(6))]).groups())
        addr = {"ra": rbase, "rb": rbase + hi}[ops[int(m.group(7))]] + int(m.group(8))
        assert (addr % 8 == 0).all() and addr.min() >= 0 and addr.max() + 8 <= XCH_BYTES, (name, m.group(0))
        got[:, u, 2 * q, :] = lds[addr // 4]
        got[:, u, 2 * q + 1, :] = lds[addr // 4 + 1]
        n += 1
    return n, got, asm


@pytest.mark.parametrize("writer,reader,G", PRODUCTION + DIAGNOSTIC)
def test_exchange_is_a_transpose(text, kernel, writer, reader, G):
    wbase, rbase, hi = addresses(kernel)
    lds = np.zeros(XCH_BYTES // 4, np.int64)
    hits = np.zeros(XCH_BYTES // 4, np.int64)
    nw, wasm = run_stores(text, writer, G, wbase, hi, lds, hits)
    wide = writer.endswith("_w64")
    assert nw == (32 if wide else 64) and ("ds_write_b32" in wasm) != wide
    # every word of the region is written exactly once: no two stores alias, and the
    # footprint (8 waves x 64 lanes x 64 words) is the region itself
    assert (hits == 1).all(), (writer, int(hits.min()), int(hits.max()))
    nr, got, rasm = run_reads(text, reader, G, rbase, hi, lds)
    assert nr == 32
    want = token(G).transpose(1, 0, 2, 3)  # reader v's register u = writer u's register v
    assert (got == want).all(), (writer, reader)
    # the store window does not wait for its stores (the kernel does, before the
    # barrier); the read statement waits for its own data as its last instruction
    assert "s_waitcnt" not in wasm
    ins = re.findall(r'"([a-z][^"\\]*)', rasm.split("\n        :", 1)[0])
    assert ins[-1] == "s_waitcnt lgkmcnt(0)" and rasm.count("s_waitcnt") == 1


def test_production_forms_are_outside_the_diagnostic_section(text, kernel):
    product = text[:text.index("#ifdef RSM_DIAG")]
    for w, r, _ in PRODUCTION:
        assert "void %s(" % w in product and "void %s(" % r in product
        assert "bs8::%s(" % w in kernel and "bs8::%s(" % r in kernel
    for w, r, _ in DIAGNOSTIC:
        assert "void %s(" % w not in product
        assert r in ("xch_read_h0", "xch_read_h1") or "void %s(" % r not in product


def run_valu_named(asm, regs):
    """run_valu of test_bs8_asm_cpu.py on registers named by their C expression."""
    ops = operands(asm)
    n = 0
    for m in GEN.finditer(asm):
        op, d, a, b = m.group(1), ops[int(m.group(2))], ops[int(m.group(3))], ops[int(m.group(4))]
        if op == "v_alignbit_b32":
            regs[d] = (((regs[a] << 32) | regs[b]) >> int(m.group(6))) & M32
        elif op == "v_xor_b32":
            regs[d] = regs[a] ^ regs[b]
        else:
            c = regs[ops[int(m.group(5))]]
            if m.group(7) == "0x96":
                regs[d] = regs[a] ^ regs[b] ^ c
            else:
                assert m.group(7) == "0xd8", m.group(0)
                regs[d] = (regs[b] & c) | (regs[a] & ~c & M32)
        n += 1
    return n, ops


def named_regs(sym):
    regs = {"X[%d][%d]" % (j, i): v for j, s in enumerate(sym) for i, v in enumerate(planes(s))}
    regs.update({"t%d" % t: 0x9E3779B9 * (t + 1) & M32 for t in range(8)})  # garbage temporaries
    return regs


@pytest.mark.parametrize("blocks,V,kind", [
    (("ph_w1_lifft0a_w64", "xch_read_h1_lifft0b"), 0, "ifft2_asm"),
    (("ph_w0_lfft1a_w64", "xch_read_h0_lfft1b"), 1, "fft2_asm"),
    (("ph_w1_lifft0a", "xch_read_h1_lifft0b"), 0, "ifft2_asm"),
    (("ph_w0_lfft1a", "xch_read_h0_lfft1b"), 1, "fft2_asm"),
    (("ph_w1_lifft0_w64",), 0, "ifft2_asm"),
    (("ph_w0_lfft1_w64",), 1, "fft2_asm")])
def test_split_large_layers(gf, text, blocks, V, kind):
    """Store window + read statement, in kernel order, compute the whole large IFFT of
    h0 / large FFT of h1 (bs8.hpp large_ifft_h / large_fft_h) and touch nothing else."""
    mul, skew = gf
    rng = np.random.default_rng(21 + V)
    sym = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(16)]
    regs = named_regs(sym)
    counts = []
    for name in blocks:
        _, asm, _ = whole(text, name)
        n, ops = run_valu_named(asm, regs)
        counts.append(n)
        # the VALU half keeps its numbers relative to the half: operand 8b + i = X[8V + b][i]
        assert ops[:64] == ["X[%d][%d]" % (8 * V + b, i) for b in range(8) for i in range(8)], name
        # the LDS operands (pairs read / data stored) are never VALU operands
        lds_ops = {int(m.group(3) or m.group(6)) for m in DS.finditer(asm)}
        valu_ops = {int(x) for m in GEN.finditer(asm) for x in (m.group(2), m.group(3), m.group(4), m.group(5)) if x}
        assert not (lds_ops & valu_ops), name
    if len(blocks) == 2:
        assert 0 < counts[1] <= 80 and counts[0] > counts[1]  # the tail fits the read burst
    ref = [x.copy() for x in sym]
    for dh in ((1, 2, 4) if kind == "ifft2_asm" else (4, 2, 1)):
        for bb in range(0, 8, 2 * dh):
            hb = 8 * V + bb
            L = skew[127 + 8 * hb + 8 * dh] if kind == "ifft2_asm" else skew[-1 + 8 * hb + 8 * dh]
            for q in range(dh):
                ref[hb + q], ref[hb + q + dh] = butterfly(kind, L, ref[hb + q], ref[hb + q + dh], mul)
    for j in range(16):
        assert unplanes([regs["X[%d][%d]" % (j, i)] for i in range(8)]).tobytes() == ref[j].tobytes(), (blocks, j)


def test_split_keeps_the_unsplit_instruction_count(text):
    """The cut is at an op boundary of the block optimized as a whole, so head + tail
    are exactly the instructions of the unsplit block (no fold across layers is lost)."""
    def valu(name):
        return len(GEN.findall(whole(text, name)[1]))
    assert valu("ph_w1_lifft0a_w64") + valu("xch_read_h1_lifft0b") == valu("ph_w1_lifft0")
    assert valu("ph_w0_lfft1a_w64") + valu("xch_read_h0_lfft1b") == valu("ph_w0_lfft1")


@pytest.mark.parametrize("name,V,inverse", [("ph_w0_tr1_w64", 1, False), ("ph_w1_tr0_w64", 0, True)])
def test_wide_store_transposes(text, name, V, inverse):
    """The transposes interleaved with the 64-bit exchange stores of the other half."""
    _, asm, _ = whole(text, name)
    fwd, _ = tp_fn(text, "tp_fwd_dev")
    inv, _ = tp_fn(text, "tp_inv_dev")
    rng = np.random.default_rng(12)
    X = [int(x) for x in rng.integers(0, 2**32, 128, dtype=np.uint64)]
    regs = {"X[%d][%d]" % (j, i): X[8 * j + i] for j in range(16) for i in range(8)}
    regs.update({"t0": 0xDEADBEEF, "t1": 0x12345678})
    for m in re.findall(r'"s"\((0x[0-9A-Fa-f]+)u\)', asm):
        regs[m + "u"] = int(m, 16)
    n, _ = run_valu_named(asm, regs)
    assert n == 8 * 41
    for j in range(16):
        got = [regs["X[%d][%d]" % (j, i)] for i in range(8)]
        want = X[8 * j:8 * j + 8]
        if j // 8 == V:
            want = (inv if inverse else fwd)(want)
        assert got == want, (name, j)
