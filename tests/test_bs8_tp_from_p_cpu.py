"""CPU check of the set body's "h1 from its landing registers" blocks (rsmt2d_amd/csrc/
bs8_small.inc, written by gen/gen_bs8_small.cpp emit_tp1_from_p and emit_phase_x with
from_p): tp1_h1_from_p runs the FIRST stage of h1's forward transposes reading the
landing registers P and writing X[8..15], and ph_w0_tr1s_w64 runs the other two stages
and the fix-ups inside the first exchange's store window.  Together they must be the
parent's whole tp_fwd_dev on the same bytes, bit for bit, with P read only, and the
store window must still be the same exchange of half 0.  The instruction text is executed
with the interpreter of test_bs8_asm_cpu.py / test_bs8_xch_cpu.py; the GPU code never
runs here."""
import os
import re

import numpy as np
import pytest

from test_bs8_asm_cpu import GEN, tp_fn
from test_bs8_xch_cpu import (DS, OPERAND, XCH_BYTES, addresses, operands, run_reads, run_stores, run_valu_named,
                              token, whole)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rsmt2d_amd", "csrc")
TOP, WINDOW = "tp1_h1_from_p", "ph_w0_tr1s_w64"


@pytest.fixture(scope="module")
def text():
    return open(os.path.join(CSRC, "bs8_small.inc")).read()


@pytest.fixture(scope="module")
def kernel():
    return open(os.path.join(CSRC, "kernels_gf8_bs.hip")).read()


def constraints(asm):
    """C expression -> constraint string of every operand of a block."""
    return {m.group(2).strip(): m.group(1) for m in OPERAND.finditer(asm)}


def run_both(text, P, garbage):
    regs = {"P[%d][%d]" % (j, i): P[j][i] for j in range(8) for i in range(8)}
    regs.update({"X[%d][%d]" % (j, i): int(garbage[8 * j + i]) for j in range(16) for i in range(8)})
    regs.update({"t0": int(garbage[128]), "t1": int(garbage[129])})
    counts = []
    for name in (TOP, WINDOW):
        _, asm, _ = whole(text, name)
        for m in re.findall(r'"s"\((0x[0-9A-Fa-f]+)u\)', asm):
            regs[m + "u"] = int(m, 16)
        n, _ = run_valu_named(asm, regs)
        counts.append(n)
    return regs, counts


def test_two_blocks_equal_the_whole_forward_transpose(text):
    fwd, _ = tp_fn(text, "tp_fwd_dev")
    rng = np.random.default_rng(31)
    for rep in range(16):
        P = [[int(x) for x in rng.integers(0, 2**32, 8, dtype=np.uint64)] for _ in range(8)]
        garbage = rng.integers(0, 2**32, 130, dtype=np.uint64)
        regs, counts = run_both(text, P, garbage)
        # the first stage (4 pairs x 3 instructions per symbol) moved, nothing added
        assert counts == [8 * 12, 8 * 29] and sum(counts) == 8 * 41
        for j in range(8):
            assert [regs["X[%d][%d]" % (8 + j, i)] for i in range(8)] == fwd(P[j]), (rep, j)
            assert [regs["P[%d][%d]" % (j, i)] for i in range(8)] == P[j], (rep, j)  # P is not written
            # h0 (the half whose pairs the window stores) is not a VALU operand
            assert [regs["X[%d][%d]" % (j, i)] for i in range(8)] == [int(x) for x in garbage[8 * j:8 * j + 8]]


def test_result_does_not_depend_on_what_x_and_the_temporaries_held(text):
    rng = np.random.default_rng(32)
    P = [[int(x) for x in rng.integers(0, 2**32, 8, dtype=np.uint64)] for _ in range(8)]
    a, _ = run_both(text, P, rng.integers(0, 2**32, 130, dtype=np.uint64))
    b, _ = run_both(text, P, rng.integers(0, 2**32, 130, dtype=np.uint64))
    for j in range(8, 16):
        for i in range(8):
            assert a["X[%d][%d]" % (j, i)] == b["X[%d][%d]" % (j, i)]


def test_p_operands_are_inputs_only(text):
    _, asm, _ = whole(text, TOP)
    ops = operands(asm)
    cons = constraints(asm)
    p_ops = [e for e in ops if e.startswith("P[")]
    assert sorted(p_ops) == sorted("P[%d][%d]" % (j, i) for j in range(8) for i in range(8))
    assert all(cons[e] == "v" for e in p_ops)  # no '=' / '+': the landing quads stay where the loads put them
    # the planes are written while P is still being read: the outputs must not share P's registers
    x_ops = [e for e in ops if e.startswith("X[")]
    assert sorted(x_ops) == sorted("X[%d][%d]" % (j, i) for j in range(8, 16) for i in range(8))
    assert all(cons[e] == "=&v" for e in x_ops) and cons["t0"] == cons["t1"] == "=&v"
    dests, reads = set(), set()
    for m in GEN.finditer(asm):
        dests.add(ops[int(m.group(2))])
        reads.update(ops[int(x)] for x in (m.group(3), m.group(4), m.group(5)) if x)
    assert not any(d.startswith("P[") for d in dests)
    assert set(p_ops) <= reads  # every landing register is consumed here: P is dead after the block
    # no X output is read in the block (write-only: nothing of the previous set leaks in)
    assert not any(r.startswith("X[") for r in reads)
    assert "ds_" not in asm and "s_waitcnt" not in asm


def test_store_window_keeps_the_pairs_and_the_exchange(text, kernel):
    head, asm, _ = whole(text, WINDOW)
    # the stored pairs are (X[v][2q], X[v][2q + 1]) of half 0, as the reader's ds_read_b64 fills them
    assert re.search(r"T\[v\]\[q\] = \(uint64_t\)X\[0 \+ v\]\[2 \* q\] \| \(\(uint64_t\)X\[0 \+ v\]\[2 \* q \+ 1\] << 32\)", head)
    ops = operands(asm)
    cons = constraints(asm)
    data = [ops[int(m.group(3))] for m in DS.finditer(asm) if m.group(1)]
    assert sorted(data) == sorted("T[%d][%d]" % (v, q) for v in range(8) for q in range(4))
    assert all(cons[d] == "v" for d in data)
    # VALU operands: h1 only (relative numbering, operand 8b + i = X[8 + b][i]), never the stored pairs
    assert ops[:64] == ["X[%d][%d]" % (8 + b, i) for b in range(8) for i in range(8)]
    valu_ops = {ops[int(x)] for m in GEN.finditer(asm) for x in (m.group(2), m.group(3), m.group(4), m.group(5)) if x}
    assert not (valu_ops & set(data))
    assert "0xF0F0F0F0u" not in asm  # the first stage's mask is not carried into the window
    # and the window is still the transpose exchange of half 0 (as test_bs8_xch_cpu.py)
    wbase, rbase, hi = addresses(kernel)
    lds = np.zeros(XCH_BYTES // 4, np.int64)
    hits = np.zeros(XCH_BYTES // 4, np.int64)
    nw, wasm = run_stores(text, WINDOW, 0, wbase, hi, lds, hits)
    assert nw == 32 and "ds_write_b32" not in wasm and "s_waitcnt" not in wasm
    assert (hits == 1).all()
    nr, got, _ = run_reads(text, "xch_read_h0", 0, rbase, hi, lds)
    assert nr == 32 and (got == token(0).transpose(1, 0, 2, 3)).all()


def test_kernel_runs_the_first_stage_before_the_next_loads_into_p(kernel):
    """The block that reads P stands at the top of the set, in front of the next set's
    loads into P, and the short window is used with it (bs_split_wave)."""
    body = kernel[kernel.index("void bs_split_wave("):]
    top = body.index("bs8::%s(X, P);" % TOP)
    assert top < body.index("issue_direct(nrow, nxt & kQ1, an);") < body.index("bs8::%s(X, xw" % WINDOW)


def test_blocks_are_diagnostic_only(text):
    """The form lost its A/B: both blocks stand in the
    section of bs8_small.inc that only the diagnostic build compiles."""
    product, diag = text.split("#ifdef RSM_DIAG", 1)
    diag = diag[:diag.index("#endif")]
    for name in (TOP, WINDOW):
        assert "void %s(" % name not in product and "void %s(" % name in diag
