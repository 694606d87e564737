"""ALU and jump code at operand edges, per lane, on every kernel (tests/opmatrix.py).

The directed quirk cases (cases.py, Q1-Q26) run one packet a case on the general interpreter, and
the fuzzers' per-lane values are random bytes: no compiled kernel, tile interpreter or dag kernel
was pinned on a signed "unsigned" jump whose high words are equal, a JMP32 compare differing in
bit 31 only, a multiply of 0xFFFFFFFF halves, or a division by zero in some lanes of a wave. The
matrix runs every ALU operation, END form and jump operator, in both classes, with a register
operand and with inline and literal immediates, over one batch of 640 (a, b) pairs.

CPU: every program loads and compiles; the C oracle, oracle/pyref.py and the closed form below
agree on status and all 11 registers for every program and pair; the batch diverges inside waves;
the forward programs' emitted code holds every jump emission form of jit.cpp jtail_code.
GPU: every program on every kernel route -- the route asserted with Program.batch_kernel -- equal
to oracle.Program.run_full per lane: status, 11 registers, verdict byte, the 8 counters, and a
production-style launch (no registers asked for) with the same r0, status, verdict and counters.
Equality is exact.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import opmatrix as M
import pyref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
ARITH = 4

PROGRAMS = M.programs()
PAIRS = M.pairs()
GROUPS = M.groups()


# ---- the closed form: the reference's rules restated with Python integers --------------------
def _sx(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def alu(op, cls, d, s):
    """-> (u64 result, status). d, s: u64 register values (an immediate sign-extended,
    emu.rs:67)."""
    if cls == 32:                                        # emu.rs:76-79 both truncated to u32
        d, s = d & M32, s & M32
    if op == "add":   r = d + s                          # emu.rs:82 wrapping
    elif op == "sub": r = d - s                          # emu.rs:85
    elif op == "mul": r = d * s                          # emu.rs:88
    elif op == "div": r = d // s if s else 0             # emu.rs:91-99 unsigned; by zero: 0
    elif op == "or":  r = d | s                          # emu.rs:102
    elif op == "and": r = d & s                          # emu.rs:105
    elif op == "lsh": r = (d << ((s & M32) % cls)) & ((1 << cls) - 1)   # emu.rs:112-116 count masked
    elif op == "rsh": r = d >> ((s & M32) % cls)         # emu.rs:119-123
    elif op == "neg": r = -d                             # emu.rs:125
    elif op == "mod": r = d % s if s else d              # emu.rs:127-134 by zero: unchanged
    elif op == "xor": r = d ^ s                          # emu.rs:137
    elif op == "mov": r = s                              # emu.rs:140
    elif op == "arsh":                                   # emu.rs:143-162 a rotate times the sign
        k = (s & M32) % cls
        rot = ((d >> k) | (d << (cls - k))) & ((1 << cls) - 1)
        r = _sx(rot, cls) * (-1 if _sx(d, cls) < 0 else 1)
        if not -(1 << 63) <= r < (1 << 63):              # emu.rs:162 i64 multiply overflows (Q21)
            return 0, ARITH
    else:
        raise AssertionError(op)
    return r & (M32 if cls == 32 else M64), 0            # emu.rs:214-216


def end(op, d):
    """emu.rs:165-209: by the source bit, the low imm bits kept, in either class (no truncation
    to 32 bits: emu.rs:76,214 exclude END)."""
    w = int(op[2:]) // 8
    v = d & ((1 << (8 * w)) - 1)
    return int.from_bytes(v.to_bytes(w, "little"), "big") if op.startswith("be") else v


def pred(op, cls, d, s):
    """emu.rs:221-224 JMP32 sign-extends the low words; every ordering is signed (emu.rs:234-299:
    `dst as i64 > src` for jgt as for jsgt)."""
    d, s = _sx(d, cls), _sx(s, cls)
    return {"jeq": d == s, "jne": d != s, "jset": (d & s) != 0,       # emu.rs:230,252,246
            "jgt": d > s, "jsgt": d > s, "jge": d >= s, "jsge": d >= s,  # emu.rs:235,256,240,261
            "jlt": d < s, "jslt": d < s, "jle": d <= s, "jsle": d <= s}[op]  # emu.rs:281,291,286,296


def closed(p, a, b, pkt_len=16):
    """(status, 11 registers) of program p on the pair (a, b), main.rs register layout."""
    r = [0] * 11
    r[2], r[6], r[7], r[10] = pkt_len, a, b, 512
    if p.kind == "alu":
        if any(reg == 7 for reg, _, _ in p.slots):
            b = a  # (mov r7, r6 before the operations)
        for reg, op, src in p.slots:
            s = b if src == "r7" else 0 if src is None else src & M64
            r[reg], st = (end(op, a), 0) if op in M.END_OPS else alu(op, p.cls, a, s)
            if st:
                return st, r
        return 0, r
    s = b if p.operand == "r7" else p.operand & M64
    t = lambda x: pred(p.op, p.cls, x & M64, s)  # noqa: E731
    if p.kind == "loop":  # three rounds if the test is taken, else one
        r[0], r[9] = (27, 3) if t(a) else (1, 1)
        return 0, r
    r0 = 0 if t(a) else 1                                     # bit 0
    if not t(a):                                              # the rule chain
        r0 |= 2
        r[3] = (a + 1) & M64
        if not t(r[3]):
            r0 |= 4
            r[4] = (a - 1) & M64
            if not t(r[4]):
                r0 |= 8
    r[8] = (a + 1) & M64
    if t(a):                                                  # two targets
        r0 |= 64
    else:
        r0 |= 16
        if not t(r[8]):
            r0 |= 32 | 64
    r[5] = a if t(a) else alu("div", 64, a, b)[0]             # a test before the divider
    r[2] = a if t(r[8]) else alu("mod", 32, a, b)[0]
    if not t(a):
        r0 |= 256                                             # the taken side left past the end
    r[0] = r0
    return 0, r


# ---- CPU ------------------------------------------------------------------------------------
_BODY = {}  # forward program -> its compiled code in variant 1's assembly (_bodies), read once


def _bodies(text):
    """The compiled programs' code in a variant's assembly: what jit.cpp wrote into each kernel
    statement (not the kernels' own, tab-indented, code)."""
    out = []
    for b in re.findall(r"; compiled eBPF program[^\n]*\n(.*?)\n\.Ldone", text, re.S):
        out.append("\n".join(ln for ln in b.splitlines() if not ln.startswith("\t")))
    return "\n".join(out)


def test_every_program_loads_and_compiles(oracle_mod, product_lib):
    from ebpf_emu import Program

    assert len(PROGRAMS) == 346 and len(PAIRS) == 640
    assert {(a, b) for a in M.EDGE64 for b in M.EDGE64} <= set(PAIRS) and len(M.EDGE64) == 24
    for p in PROGRAMS:
        oracle_mod.Program(p.image)
        q = Program(p.image)
        assert q.tier == 0, p.name
        assert q.compile(), p.name
        assert q.jit_error == "", (p.name, q.jit_error)
        if p.kind == "loop":
            assert not q.forward_only, p.name
            assert q.jit_asm(2), p.name
        else:
            assert q.forward_only, p.name
            assert q.jit_asm(0), p.name
            _BODY[p.name] = _bodies(q.jit_asm(1))
            assert _BODY[p.name], p.name
        q.close()
        q = Program(p.stack_image)  # the stack-window form: memory tier 0.5, compiled too
        assert q.stack_window == 8 and q.compile(), p.name
        q.close()


def test_three_statements_agree(oracle_mod):
    """The C oracle, the Python restatement and the closed form above: status and all 11
    registers, every program, every pair."""
    for p in PROGRAMS:
        img = p.image
        op = oracle_mod.Program(img)
        ins = pyref.decode(img)
        for a, b in PAIRS:
            pkt = M.packet(a, b)
            st, regs, _m, _s = op.run_full(pkt, 1024, 512, M.STEPS)
            pst, pregs, _m, _s = pyref.run_full(ins, pkt, 1024, 512, M.STEPS)
            cst, cregs = closed(p, a, b)
            ctx = f"{p.what} [{p.name}] (a, b) = ({a:#x}, {b:#x}) image {img.hex()}"
            assert st == pst == cst, ctx
            if st == 0:
                assert regs == pregs == cregs, ctx


# jump programs where one outcome is impossible: the predicate is constant over all 640 pairs
ONE_SIDED = {
    "jset.64.imm0x0", "jset.32.imm0x0",                       # x & 0
    "jeq.64.imm0x64", "jeq.32.imm0x64",                       # no operand (or its low word) is 100
    "jne.64.imm0x64", "jne.32.imm0x64",
    "jgt.32.imm0x7fffffff", "jsgt.32.imm0x7fffffff",          # nothing above i32::MAX
    "jle.32.imm0x7fffffff", "jsle.32.imm0x7fffffff",
    "jlt.32.imm-0x80000000", "jslt.32.imm-0x80000000",        # nothing below i32::MIN
    "jge.32.imm-0x80000000", "jsge.32.imm-0x80000000",
}


def test_batch_diverges(oracle_mod):
    """Inside waves, not only across them: for every jump program both outcomes occur and some
    wave holds both; ARSH64 by a register both completes and overflows; every wave of the
    register div / mod programs has zero and non-zero divisors."""
    waves = [range(w, w + 64) for w in range(0, 640, 64)]
    constant = set()
    for p in PROGRAMS:
        if p.kind == "alu":
            continue
        s = [b if p.operand == "r7" else p.operand & M64 for _a, b in PAIRS]
        key = f"{p.op}.{p.cls}.{M.fmt_operand(p.operand)}"
        if len({pred(p.op, p.cls, a, s[i]) for i, (a, _b) in enumerate(PAIRS)}) == 1:
            constant.add(key)
        op = oracle_mod.Program(p.image)
        r0 = [op.run_full(M.packet(a, b), 1024, 512, M.STEPS)[1][0] for a, b in PAIRS]
        # (bit 0 of the forward program, the round count of the loop program: the first test)
        taken = [(v & 1) == 0 for v in r0] if p.kind == "fwd" else [v == 27 for v in r0]
        if key in ONE_SIDED:
            assert len(set(taken)) == 1, p.name
            continue
        assert set(taken) == {True, False}, p.name
        assert any(len({taken[i] for i in w}) == 2 for w in waves), p.name
    assert ONE_SIDED == constant  # (no more exemptions than constant predicates)
    arsh = next(p for p in PROGRAMS if p.name == "alu.arsh.64.r7")
    op = oracle_mod.Program(arsh.image)
    st = [op.run_full(M.packet(a, b), 1024, 512, M.STEPS)[0] for a, b in PAIRS]
    assert set(st) == {0, ARITH}
    # (cases.py q21_arsh64_overflow and q4_arsh64_pos_rotates: their operands are in the matrix)
    assert st[PAIRS.index((0x8000000000000000, 0x40))] == ARITH and st[PAIRS.index((1, 1))] == 0
    assert any(len({st[i] for i in w}) == 2 for w in waves)
    for w in waves:
        for mask in (M64, M32):  # (the 64-bit and the 32-bit divisor)
            assert {PAIRS[i][1] & mask == 0 for i in w} == {True, False}


# the emission forms of a conditional jump (jit.cpp jtail_code, cmpx_pass), as the emitted text
# has them
FORMS = {
    "folded v_cmpx": r"^v_cmpx_(eq|ne|gt|ge|lt|le)_[iu](32|64) vcc, ",
    "pending mask": r"^s_or_b64 (s\[7[4-9]:7[5-9]\]), \1, (vcc|s\[64:65\])$",
    "complement region": r"^s_mov_b64 s\[72:73\], exec$",
    "complement region leave": r"^s_andn2_b64 s\[72:73\], s\[72:73\], (vcc|s\[64:65\])$",
    "LPC select, taken lanes leave": r"^v_cndmask_b32_e64 v28, v28, (\d+|v37), vcc$",
    "LPC select, not-taken lanes leave": r"^v_cndmask_b32_e64 v28, (\d+|v38), v28, vcc$",
}


def test_matrix_reaches_every_emission_form(product_lib):
    from ebpf_emu import Program

    seen = {k: [] for k in FORMS}
    for p in PROGRAMS:
        if p.kind != "fwd":
            continue
        if p.name not in _BODY:
            q = Program(p.image)
            assert q.compile()
            _BODY[p.name] = _bodies(q.jit_asm(1))
            q.close()
        body = _BODY[p.name]
        assert body, p.name
        for k, rx in FORMS.items():
            if re.search(rx, body, re.M):
                seen[k].append(p.name)
    for k, names in seen.items():
        assert names, f"no forward program's code has the form: {k}"


# ---- GPU ------------------------------------------------------------------------------------
_REF = {}  # (image, packets' length, caller registers?) -> oracle_ref, computed once


def _ref(oracle_mod, img, pkts, init_regs=None):
    key = (img, len(pkts[0]), init_regs is not None)
    if key not in _REF:
        _REF[key] = M.oracle_ref(oracle_mod, img, pkts, init_regs)
    return _REF[key]


@pytest.fixture(scope="module")
def batch(cuda):
    """The 640 packets on the device, once: fixed 64-byte slots and offsets + lens."""
    import torch

    from test_gpu_parity import _stage

    pk64, fixed, fixed_kw = M.fixed_frames(PAIRS, cuda)
    pk16 = [M.packet(a, b) for a, b in PAIRS]
    var, var_kw = _stage(pk16, cuda, offsets_layout=True)
    junk = torch.tensor(np.array(M.JUNK_REGS, dtype=np.uint64).view(np.int64), device=cuda)
    return dict(pk64=pk64, fixed=fixed, fixed_kw=fixed_kw, pk16=pk16, var=var, var_kw=var_kw,
                junk=junk)


def _routes(p, batch):
    """(route, image, packets, frames, layout, flags, caller registers, the kernels it may land
    on) for program p."""
    from ebpf_emu import _lib as L

    loop = p.kind == "loop"
    fx = (batch["pk64"], batch["fixed"], batch["fixed_kw"])
    vr = (batch["pk16"], batch["var"], batch["var_kw"])
    yield ("fixed slots", p.image, *fx, {}, None,
           [L.EBPF_KERNEL_JIT_LOOP if loop else L.EBPF_KERNEL_JIT_FIXED_OCC])
    yield ("offsets + lens", p.image, *vr, {}, None,
           [L.EBPF_KERNEL_JIT_LOOP if loop else L.EBPF_KERNEL_JIT_VARL])
    # (compiled variant 0: the kernels of the fixed-slot layout, the registers from the caller)
    yield ("caller registers", p.image, *fx, dict(init_regs=batch["junk"]), M.JUNK_REGS,
           [L.EBPF_KERNEL_JIT_LOOP if loop else L.EBPF_KERNEL_JIT_FIXED_OCC])
    yield ("tile / dag interpreter", p.image, *fx, dict(no_jit=True), None,
           [L.EBPF_KERNEL_TILE_LOOP] if loop else [L.EBPF_KERNEL_TILE, L.EBPF_KERNEL_DAG])
    yield ("general interpreter", p.image, *fx, dict(generic=True), None,
           [L.EBPF_KERNEL_GENERAL_T0])
    yield ("stack window", p.stack_image, *fx, {}, None,
           [L.EBPF_KERNEL_JIT_LOOP_STACK if loop else L.EBPF_KERNEL_JIT_STACK])


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_matrix_on_every_route(cuda, oracle_mod, batch, group):
    from ebpf_emu import Program

    n = 0
    for p in PROGRAMS:
        if p.group != group:
            continue
        progs = {}
        try:
            for route, img, pkts, frames, kw, flags, regs, kernels in _routes(p, batch):
                if img not in progs:
                    progs[img] = Program(img)
                    assert progs[img].compile(), p.name
                ref = _ref(oracle_mod, img, pkts, regs)
                try:
                    got = M.launch(progs[img], frames, kw, kernels, **flags)
                    prod = M.launch(progs[img], frames, kw, kernels, prod=True, **flags)
                except AssertionError as e:
                    raise AssertionError(f"{p.what} [{p.name}] route {route}: {e}") from None
                bad = M.mismatch(p, route, img, PAIRS, got, ref)
                assert bad is None, bad
                bad = M.mismatch(p, route + " (production outputs)", img, PAIRS, prod, ref, full=got)
                assert bad is None, bad
                n += 1
        finally:
            for q in progs.values():
                q.close()
    assert n and n % 6 == 0
    _REF.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("half", [0, 1])
def test_matrix_fixed_slots_without_occupancy_variant(half):
    """EBPFEMU_FIXED_OCC=0 is read once, when the library first compiles: a fresh process
    (opmatrix_child.py) runs the forward programs on fixed slots there, on ebpf_tile_jit_fixed,
    and checks each against the oracle itself. (Two processes, each with every second program:
    one with all 192 took 17 s, most of it their compiles.)"""
    from ebpf_emu import _lib

    r = subprocess.run([sys.executable, os.path.join(HERE, "opmatrix_child.py"),
                        os.path.join(ROOT, "ebpf-emu_amd"), os.path.join(ROOT, "oracle"), HERE,
                        f"{half}/2"],
                       capture_output=True, text=True, timeout=170,
                       env=dict(os.environ, EBPFEMU_FIXED_OCC="0"))
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["failures"] == [], d["failures"][0]
    assert d["kernels"] == [_lib.EBPF_KERNEL_JIT_FIXED]
    assert d["programs"] == len([p for p in PROGRAMS if p.kind != "loop"]) // 2 == 96
