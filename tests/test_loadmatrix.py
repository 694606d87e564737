"""Packet and stack loads at address edges, per lane, on every kernel (tests/loadmatrix.py).

The directed constant-address programs (test_gpu_parity.py) use one address in every lane and the
fuzzers' per-lane addresses are random packet bytes: a load straddling byte 64 by exactly three
bytes, one straddling len by one, one starting at mem - 1 with width 2, an address whose high word
is 1 and low word 0, an 8-byte load overlapping the stack window by one byte at either end -- and a
wave holding them side by side -- were reached by luck only.

CPU: every program and form loads and compiles; the C oracle, oracle/pyref.py and the closed form
below agree on status and all 11 registers for every program, form and lane; every width of every
program family meets every address class (test_coverage: the condition that keeps the matrix from
being hollow); the matrix's compiled code holds every load emission form of jit.cpp.
GPU: every program on every kernel route -- the route asserted with Program.batch_kernel -- equal
to oracle.Program.run_full per lane: status, 11 registers, verdict byte, the 8 counters, and a
production-style launch (no registers asked for) with the same r0, status, verdict and counters.
Equality is exact.

Routes against DESIGN 3.6: an xdp_md batch in place is not taken by the occupancy variant, so
xdp_md forward programs on fixed slots land on ebpf_tile_jit_fixed (EBPF_KERNEL_JIT_FIXED);
ebpf_tile_jit_var takes offsets + lens batches only when the var tile loop does not (here: the
lens array at 2 mod 4), so that route is added; dag_kernel needs more than 62 micro-ops, which
only reg.chain has.

Emission forms with no text of their own in jit_asm (the kernels' statement handlers, compiled
from gen_tile.py, serve them): the constant-address far form (ldxkfar; programs const.asc.70,
.100, .127, .128 and the mem range) and the constant-address loads of the var statements (every
const program on the offsets + lens routes). zwin needs every load of the program one byte wide,
the head's too (loop.bytes.*: a & 0xFFFF and b & 0xFF read bytewise), and qcache also that no
other code names v[50:55], which the multiply does (loop.bytes.+0x41 has none).
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import loadmatrix as M
import pyref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
M64 = M.M64
ST_MEM, ST_MEM_UB, ST_BADPKT = 1, 2, 7

PROGRAMS = M.programs()
GROUPS = M.groups()


# ---- the closed form: the reference's load rule restated with Python integers ----------------
def closed(p, form, lane, mem=M.MEM, r10=M.R10, size=None, trace=None):
    """(status, 11 registers) of program p's form on a lane, main.rs register layout. The image is
    the packet followed by zeros up to mem_size (main.rs:16); the stack forms' two stores are
    applied to it first. trace(load index, width, base, offset): every load reached."""
    pkt = M.lane_image(lane, form, size)
    r = [0] * 11
    if len(pkt) > mem:
        return ST_BADPKT, r
    image = bytearray(mem)
    image[:len(pkt)] = pkt
    r[2], r[10] = len(pkt), r10
    a, b, _n = lane
    if p.byte_head:
        r[6], r[7], r[4] = a & 0xFFFF, b & 0xFF, a & 0xFF00
    elif p.kind != "const":
        r[6], r[7] = a, b
    if form in M.STACK_FORMS:                             # emu.rs:354-372, little endian
        image[r10 - 8:r10] = a.to_bytes(8, "little")
        image[r10 - 16:r10 - 12] = (a & 0xFFFFFFFF).to_bytes(4, "little")

    def load(i):
        w, d, base, off = p.loads[i]
        if trace:
            trace(i, w, r[base], off)
        sb = r[base] - (1 << 64) if r[base] >> 63 else r[base]
        s = sb + off                                      # emu.rs:343 a debug-build i64 add:
        if not -(1 << 63) <= s < (1 << 63):               # overflow panics (ebpf_oracle.c:96)
            return ST_MEM
        ea = s & M64                                      # emu.rs:344 as usize
        if ea >= mem:                                     # mmu.rs:23-30 memory[a..a+1] (oracle :98)
            return ST_MEM
        if ea + w > mem:                                  # Q16: the tail past the image (oracle :99)
            return ST_MEM_UB
        m = (1 << (8 * w)) - 1                            # emu.rs:341-349 (Q1): the low w bytes
        r[d] = (r[d] & ~m & M64) | int.from_bytes(image[ea:ea + w], "little")
        return 0

    if p.kind == "loop":
        for _ in range(M.ROUNDS):
            for i in range(len(p.loads)):
                st = load(i)
                if st:
                    return st, r
            r[0] = (r[0] * (31 if p.mul else 1) + sum(r[d] for _w, d, _b, _o in p.loads)) & M64
            r[6] = (r[6] + r[7]) & M64
            r[9] += 1
        return 0, r
    for _w, d, _b, _o in p.loads:
        r[d] = M64 if p.kind == "const" else b
    if p.rebase:
        r[1] = p.rebase
    for i in range(len(p.loads)):
        st = load(i)
        if st:
            return st, r
    r[0] = 0
    for d in dict.fromkeys(d for _w, d, _b, _o in p.loads):
        r[0] ^= r[d]
    return 0, r


def lane_classes(p, form, lane, mem=M.MEM, r10=M.R10, size=None):
    """[(width, classes)] of the loads the lane reaches, by the closed form."""
    out = []
    n = len(M.lane_image(lane, form, size))

    def trace(i, w, base, off):
        out.append((w, M.classify(base, off, w, n, mem, form in M.STACK_FORMS, r10)))
    closed(p, form, lane, mem, r10, size, trace)
    return out


def lane_text(p, form, lanes, mem=M.MEM, r10=M.R10, size=None):
    def text(i):
        cls = " ".join(f"w{w}:{'+'.join(sorted(c))}" for w, c in
                       lane_classes(p, form, lanes[i], mem, r10, size)[:8])
        return f"{M.fmt_lane(lanes[i])} class [{cls}]"
    return text


# ---- CPU ------------------------------------------------------------------------------------
_BODY = {}  # (program, form) -> its compiled code in variants 0..2 (bodies), read once


def bodies(text):
    """The compiled programs' code in a variant's assembly: what jit.cpp wrote into each kernel
    statement (not the kernels' own, tab-indented, code)."""
    out = []
    for b in re.findall(r"; compiled eBPF (?:loop )?program[^\n]*\n(.*?)\n\.Ldone", text, re.S):
        out.append("\n".join(ln for ln in b.splitlines() if not ln.startswith("\t")))
    return "\n".join(out)


def _body(p, form):
    from ebpf_emu import Program, _lib

    if (p.name, form) not in _BODY:
        q = Program(p.image(form))
        assert q.compile(), p.name
        text = []
        for v in (0, 1, 2):
            try:
                text.append(bodies(q.jit_asm(v)))
            except _lib.EbpfError:
                pass
        q.close()
        _BODY[p.name, form] = "\n".join(text)
    return _BODY[p.name, form]


def test_every_program_loads_and_compiles(oracle_mod, product_lib):
    from ebpf_emu import Program

    assert len(PROGRAMS) == 122
    assert (len(M.lanes("reg")), len(M.lanes("loop")), len(M.lanes("const"))) == (1191, 675, 88)
    assert {n for _a, _b, n in M.lanes("reg")} == set(M.LENGTHS)
    for p in PROGRAMS:
        for form in M.forms(p):
            img = p.image(form)
            oracle_mod.Program(img)
            q = Program(img)
            if form in M.STACK_FORMS:
                # (memory tier 0.5: the loader reports tier 1 and no forward-jump fast path; the
                # compiled stack-window kernels take its batches)
                assert q.stack_window == M.STACK_K and q.tier == 1, p.name
                assert not q.forward_only, p.name
            else:
                assert q.tier == 0 and q.stack_window == 0, p.name
                assert q.forward_only == (p.kind != "loop"), p.name
            assert q.compile(), p.name
            assert q.jit_error == "", (p.name, form, q.jit_error)
            q.close()
            assert _body(p, form), (p.name, form)


def test_three_statements_agree(oracle_mod):
    """The C oracle, the Python restatement and the closed form above: status and all 11
    registers, every program, every form, every lane -- and the oracle against the closed form on
    the small image (mem_size = r10 = 72) and with every length set to 64, 80 and 128 (the
    fixed-slot routes)."""
    for p in PROGRAMS:
        lanes = M.lanes(p.batch)
        for form in M.forms(p):
            img = p.image(form)
            op = oracle_mod.Program(img)
            ins = pyref.decode(img)
            for mem, r10, size in [(M.MEM, M.R10, None), (M.SMALL_MEM, M.SMALL_MEM, None),
                                   (M.MEM, M.R10, 64), (M.MEM, M.R10, 80), (M.MEM, M.R10, 128)]:
                if mem == M.SMALL_MEM and form in M.STACK_FORMS:
                    continue
                for lane in lanes:
                    pkt = M.lane_image(lane, form, size)
                    if mem == M.SMALL_MEM and len(pkt) > mem:
                        continue
                    st, regs, _m, _s = op.run_full(pkt, mem, r10, M.STEPS)
                    cst, cregs = closed(p, form, lane, mem, r10, size)
                    ctx = (f"{p.what} [{p.name}] form {form} mem {mem} {M.fmt_lane(lane)} "
                           f"size {size} image {img.hex()}")
                    assert st == cst, ctx
                    if st == 0:
                        assert regs == cregs, ctx
                    if mem == M.MEM and size is None:
                        pst, pregs, _m, _s = pyref.run_full(ins, pkt, mem, r10, M.STEPS)
                        assert pst == st, ctx
                        if st == 0:
                            assert pregs == regs, ctx


def _required(w, stack):
    req = ({"win", "far-in-len", "past-len", "mem-at-mem", "mem-highword", "mem-overflow", "wrap"} |
           {f"split64-{k}" for k in range(1, w)} | {f"lensplit-{k}" for k in range(1, w)} |
           {f"ub-{k}" for k in range(1, w)})
    if stack:
        req |= ({f"stk-lo-{k}" for k in range(1, w + 1)} | {f"stk-hi-{k}" for k in range(1, w + 1)} |
                {"stk-miss-lo", "stk-miss-hi", "stk-gap"})
    return req


def _off_exempt(fam, off, widths=M.WIDTHS):
    """What base + off cannot do: a sum that wraps to a valid address needs off > 0, a signed
    overflow needs off != 0."""
    out = set()
    for w in widths:
        if off <= 0:
            out.add((fam, w, "wrap"))
        if off == 0:
            out.add((fam, w, "mem-overflow"))
    return out


def _order_exempt(fam):
    """A family of an asc and a desc program only (no single-load programs): ST_MEM depends on the
    address alone, so the program's first load (width 1 or 8) takes it, and at mem - 1 the 2-byte
    load (asc) or the 8-byte load (desc) faults before the 4-byte one."""
    return ({(fam, w, c) for w in (2, 4) for c in ("mem-at-mem", "mem-highword", "mem-overflow")} |
            {(fam, 4, "ub-1")})


# classes a family cannot reach, asserted equal to what the closed form finds missing
IMPOSSIBLE = set()
for _off in M.OFFSETS:
    for _f in ("plain", "xdp"):
        IMPOSSIBLE |= _off_exempt(f"reg{_off:+#x}/{_f}", _off)
        if _off not in (0, 65):   # (the offsets with single-load programs)
            IMPOSSIBLE |= _order_exempt(f"reg{_off:+#x}/{_f}")
for _off in M.STACK_OFFSETS:
    for _f in M.STACK_FORMS:
        IMPOSSIBLE |= _off_exempt(f"reg{_off:+#x}/{_f}", _off) | _order_exempt(f"reg{_off:+#x}/{_f}")
for _off in M.LOOP_OFFSETS:
    for _f in ("plain", "xdp"):
        IMPOSSIBLE |= _off_exempt(f"loop{_off:+#x}/{_f}", _off)
for _f in M.STACK_FORMS:
    IMPOSSIBLE |= _off_exempt(f"loop+0x0/{_f}", 0, [1, 4, 8])
# constant addresses r1 + off with r1 = 0 or 8 and a 16-bit offset: no high word, no overflow, no
# wrap; and asc / desc programs only
for _f in ("plain", "xdp"):
    IMPOSSIBLE |= {(f"const/{_f}", w, c) for w in M.WIDTHS
                   for c in ("mem-highword", "mem-overflow", "wrap")}
    IMPOSSIBLE |= _order_exempt(f"const/{_f}")


def test_coverage():
    """For every width and every program family (the programs of one offset; all constant-address
    programs) and form, the batch holds a lane in each address class, counting only loads the lane
    reaches. Some wave of 64 holds at least four classes, a faulting and a clean one among them.
    Every loop program refills (its walk leaves [WB, WB + 64) inside the packet) and some lane of
    it walks backwards across byte 64."""
    seen = {}       # (family/form, width) -> classes
    missing = set()
    for p in PROGRAMS:
        if not p.family:
            continue
        lanes = M.lanes(p.batch)
        for form in M.forms(p):
            per_lane = []
            refills = back = False
            for lane in lanes:
                tr = lane_classes(p, form, lane)
                first = set()
                for w, c in tr:
                    seen.setdefault((f"{p.family}/{form}", w), set()).update(c)
                first |= tr[0][1] if tr else set()
                per_lane.append(first)
                if p.kind == "loop":
                    a, st, n = lane
                    n = len(M.lane_image(lane, form))
                    addr = [(a + p.off + k * st) & M64 for k in range(len(tr) // len(p.loads))]
                    wb = 0                         # the window's base: moved by a refill
                    for x, y in zip(addr, addr[1:]):
                        if y < n and not wb <= y < wb + 64:
                            refills, wb = True, y & ~63 & M64
                        if y < 64 <= x < n:
                            back = True
            if p.kind == "loop":
                assert refills, (p.name, form)
                assert back, (p.name, form)
            waves = [per_lane[i:i + 64] for i in range(0, len(per_lane), 64)]
            if p.kind != "const":  # (a constant address: every lane the same class but for len)
                assert any(len(set().union(*w)) >= 4 for w in waves), (p.name, form)
                assert any(any(any(c.startswith(("mem-", "ub-")) for c in x) for x in w) and
                           any(x and not any(c.startswith(("mem-", "ub-")) for c in x) for x in w)
                           for w in waves), (p.name, form)
    for (fam, w), got in seen.items():
        for c in _required(w, fam.endswith(("/stack", "/xstack"))) - got:
            missing.add((fam, w, c))
    assert missing == IMPOSSIBLE, (sorted(missing - IMPOSSIBLE), sorted(IMPOSSIBLE - missing))
    fams = {f"{p.family}/{f}" for p in PROGRAMS if p.family for f in M.forms(p)}
    assert {f for f, _w in seen} == fams
    for fam in fams:  # (the stack loop forms: widths 1, 4 and 8)
        assert {w for f, w in seen if f == fam} >= ({1, 4, 8} if fam in ("loop+0x0/stack", "loop+0x0/xstack")
                                                     else set(M.WIDTHS)), fam


# the load emission forms of jit.cpp, as the emitted text has them. Where each was read:
#   ldx_fixed: the window test after .Lok (fixed: a + w against 64; loop: a - WB against 64 - w),
#     `lenmask` (var), `win` for w == 1, the out-of-line `far` string (.Lfar ... .Lfd);
#   ldxk_fast: v_perm_b32 (one dword), one v_alignbyte_b32 (two), two in a row (width 8: three)
#     over the preloaded window registers v[64 + k];
#   ldx1_loop: its own window test; ldx1_zero_window's (zwin); ldx1_qword_cache's hit (qcache);
#   stack_overlay: the s_swappc_b64 call; overlay_routines: overlay_label(w).
# A register renumbering in jit.cpp changes these texts without changing behaviour: update them.
EMISSION_FORMS = {
    "ldx_fixed, fixed slots": r"^v_cmp_lt_u32_e64 s\[62:63\], 64, v38$",
    "ldx_fixed, var (bytes at or past LEN masked)": r"^v_sub_u32 v46, v31, v36\nv_cmp_lt_u32 vcc, v36, v31$",
    "ldx_fixed, loop (window at WB)": r"^v_sub_u32 v41, v36, v22\nv_cmp_lt_u32_e64 s\[62:63\], \d+, v41$",
    "ldx_fixed, one byte": r"^v_xad_u32 v42, v35, v36, v34\nds_read_u8 v26, v42$",
    "ldx_fixed, the out-of-line far read": r"^\.Lfar\w+:\n(?:.*\n)+?\.Lfd\w+:$",
    "constant address, 1 dword": r"^v_perm_b32 v\d+, v(6[4-9]|7\d), v\d+, s36$",
    "constant address, 2 dwords": r"^v_alignbyte_b32 v\d+, v(6[5-9]|7\d), v(6[4-9]|7\d), [123]$",
    "constant address, 3 dwords": (r"^v_alignbyte_b32 v\d+, v(?:6[5-9]|7\d), v(?:6[4-9]|7\d), ([123])\n"
                                   r"v_alignbyte_b32 v\d+, v(?:6[6-9]|7\d), v(?:6[5-9]|7\d), \1$"),
    "ldx1_loop": r"^v_cndmask_b32_e64 v43, 0, v42, s\[60:61\]\nv_cmp_le_u32 vcc, 64, v43$",
    "ldx1_loop, zwin": r"^v_cmp_le_u32 vcc, 64, v42\ns_cbranch_vccnz \.Lrf\w+$",
    "ldx1_loop, qcache": r"^v_perm_b32 v26, v53, v52, v42$",
    "stack overlay call": r"^s_swappc_b64 s\[62:63\], s\[60:61\]$",
    "overlay routine, width 1": r"^\.Lovr\w*_1:$",
    "overlay routine, width 2": r"^\.Lovr\w*_2:$",
    "overlay routine, width 4": r"^\.Lovr\w*_4:$",
    "overlay routine, width 8": r"^\.Lovr\w*_8:$",
}


def test_matrix_reaches_every_emission_form(product_lib):
    src = open(os.path.join(ROOT, "ebpf-emu_amd", "csrc", "jit.cpp")).read()
    for name in ("ldx_fixed", "ldxk_fast", "ldx1_loop", "ldx1_zero_window", "ldx1_qword_cache",
                 "stack_overlay", "overlay_routines"):   # (the emitters the forms above are read from)
        assert re.search(r"std::string " + name + r"\(", src), name
    seen = {k: [] for k in EMISSION_FORMS}
    for p in PROGRAMS:
        for form in M.forms(p):
            body = _body(p, form)
            for k, rx in EMISSION_FORMS.items():
                if not seen[k] and re.search(rx, body, re.M):
                    seen[k].append(f"{p.name}/{form}")
    for k, names in seen.items():
        assert names, f"no matrix program's code has the form: {k}"


# ---- GPU ------------------------------------------------------------------------------------
_REF = {}     # oracle_ref per (image, batch, ...) of the group being run
_STAGED = {}  # (batch, packet form, layout) -> (oracle images, frames, layout kwargs), on the device
REACHED = set()  # kernel ids the matrix ran on (test_every_kernel_reached)


def _staged(batch, form, layout, dev):
    key = (batch, "xdp" if form in M.XDP_FORMS else "plain", layout)
    if key not in _STAGED:
        lanes = M.lanes(batch)
        idx = list(range(len(lanes)))
        size = None
        if layout[0] == "fixed":  # (xdp_md: the slot holds the packet, the image is 8 bytes longer)
            size = layout[1] + (8 if form in M.XDP_FORMS else 0)
        if layout[0] == "small":
            idx = [i for i in idx if len(M.lane_image(lanes[i], form)) <= M.SMALL_MEM]
        pkts = [M.lane_packet(lanes[i], form, size) for i in idx]
        if layout[0] == "fixed":
            frames, kw = M.stage_fixed(pkts, layout[1], dev)
        elif layout[0] == "stride":
            frames, kw = M.stage_stride_lens(pkts, dev)
        elif layout[0] == "lens2":   # the lens array at 2 mod 4: not the var tile loop's layout
            import torch

            frames, kw = M.stage_offsets(pkts, dev)
            buf = torch.zeros(len(pkts) + 2, dtype=torch.int16, device=dev)
            buf[1:len(pkts) + 1] = kw["lens"]
            kw["lens_buf"] = buf
            kw["lens"] = buf[1:len(pkts) + 1]
            assert kw["lens"].data_ptr() % 4 == 2
        else:
            first, gap, align = {"aligned": (0, 0, 16), "misaligned": (0, 3, 1),
                                 "pcap": (8, 16, 16), "small": (0, 0, 16)}[layout[0]]
            frames, kw = M.stage_offsets(pkts, dev, first, gap, align)
        images = [M.xdp_image(q) for q in pkts] if form in M.XDP_FORMS else pkts
        _STAGED[key] = ([lanes[i] for i in idx], images, frames, kw, size)
    return _STAGED[key]


def _routes(p):
    """(route, form, layout, flags, caller registers, kernels it may land on, staged?)"""
    from ebpf_emu import _lib as L

    loop = p.kind == "loop"
    fixed = [L.EBPF_KERNEL_JIT_LOOP if loop else L.EBPF_KERNEL_JIT_FIXED_OCC]
    var = [L.EBPF_KERNEL_JIT_LOOP if loop else L.EBPF_KERNEL_JIT_VARL]
    for s in (64, 80, 128):
        yield f"fixed slots, stride {s}", "plain", ("fixed", s), {}, None, fixed, None
    yield "offsets + lens, aligned", "plain", ("aligned",), {}, None, var, None
    yield "offsets + lens, misaligned", "plain", ("misaligned",), {}, None, var, None
    yield "offsets + lens, records at 8 mod 16", "plain", ("pcap",), {}, None, var, None
    yield "stride + lens", "plain", ("stride",), {}, None, var, None
    yield ("offsets + lens, lens at 2 mod 4", "plain", ("lens2",), {}, None,
           [L.EBPF_KERNEL_JIT_LOOP if loop else L.EBPF_KERNEL_JIT_VAR], None)
    yield "caller registers", "plain", ("fixed", 64), {}, M.JUNK_REGS, fixed, None
    tile = ([L.EBPF_KERNEL_TILE_LOOP] if loop else
            [L.EBPF_KERNEL_DAG] if p.name == "reg.chain" else [L.EBPF_KERNEL_TILE])
    yield "tile / dag interpreter, fixed slots", "plain", ("fixed", 64), dict(no_jit=True), None, tile, None
    yield "tile / dag interpreter, offsets + lens", "plain", ("aligned",), dict(no_jit=True), None, tile, None
    yield ("general interpreter", "plain", ("aligned",), dict(generic=True), None,
           [L.EBPF_KERNEL_GENERAL_T0], None)
    yield ("small image", "plain", ("small",), dict(mem_size=M.SMALL_MEM, r10=M.SMALL_MEM), None,
           var, None)
    if p.has_stack_form:
        yield ("stack window, fixed slots", "stack", ("fixed", 64), {}, None,
               [L.EBPF_KERNEL_JIT_LOOP_STACK if loop else L.EBPF_KERNEL_JIT_STACK], None)
        yield ("stack window, offsets + lens", "stack", ("aligned",), {}, None,
               [L.EBPF_KERNEL_JIT_LOOP_STACK if loop else L.EBPF_KERNEL_JIT_VARL_STACK], None)
        yield ("stack window, lens at 2 mod 4", "stack", ("lens2",), {}, None,
               [L.EBPF_KERNEL_JIT_LOOP_STACK if loop else L.EBPF_KERNEL_JIT_VAR_STACK], None)
    # xdp_md: forward programs in place; the loop programs' loads cannot be proven past the ctx
    # (DESIGN 3.17), so their batches are staged
    yield "xdp_md, offsets + lens", "xdp", ("misaligned",), dict(xdp_md=True), None, var, loop
    yield ("xdp_md, fixed slots", "xdp", ("fixed", 64), dict(xdp_md=True), None,
           [L.EBPF_KERNEL_JIT_LOOP if loop else L.EBPF_KERNEL_JIT_FIXED], loop)
    if p.has_stack_form:   # (in place for forward programs; nothing is asked of the loops' staging)
        yield ("xdp_md, stack window, offsets + lens", "xstack", ("misaligned",), dict(xdp_md=True),
               None, [L.EBPF_KERNEL_JIT_LOOP_STACK] if loop else
               [L.EBPF_KERNEL_JIT_VARL_STACK, L.EBPF_KERNEL_JIT_VAR_STACK], None if loop else False)


def run_route(prog, p, route, form, staged, flags, regs, kernels, oracle_mod, want_staged=None,
              junk=None):
    """One program form on one route: the full and the production launch against the oracle.
    Returns the first mismatch's text or None; the kernel id is added to REACHED."""
    import torch

    lanes, images, frames, kw, size = staged
    kw = {k: v for k, v in kw.items() if k != "lens_buf"}
    img = prog.image
    mem, r10 = flags.get("mem_size", M.MEM), flags.get("r10", M.R10)
    key = (img, route, regs is not None)
    if key not in _REF:
        _REF[key] = M.oracle_ref(oracle_mod, img, images, regs, mem, r10)
    ref = _REF[key]
    fl = dict(flags)
    if regs is not None:
        fl["init_regs"] = junk
    b = prog.make_batch(frames, max_steps=M.STEPS, **kw, **fl)
    if want_staged is not None and prog.batch_staged(b) != want_staged:
        return f"{p.what} [{p.name}] route {route}: batch_staged is {not want_staged}"
    try:
        got = M.launch(prog, frames, kw, kernels, **fl)
        prod = M.launch(prog, frames, kw, kernels, prod=True, **fl)
    except AssertionError as e:
        return f"{p.what} [{p.name}] route {route}: {e}"
    torch.cuda.synchronize()
    REACHED.add(prog.batch_kernel(b))
    # (caller registers: r1 = 0, so a and b still come from the packet and the classes hold)
    text = lane_text(p, form, lanes, mem, r10, size)
    return (M.mismatch(p, route, img, None, got, ref, lane_text=text) or
            M.mismatch(p, route + " (production outputs)", img, None, prod, ref, full=got,
                       lane_text=text))


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_matrix_on_every_route(cuda, oracle_mod, group):
    import torch

    from ebpf_emu import Program

    junk = torch.tensor(np.array(M.JUNK_REGS, dtype=np.uint64).view(np.int64), device=cuda)
    n = 0
    for p in PROGRAMS:
        if p.group != group:
            continue
        progs = {}
        try:
            for route, form, layout, flags, regs, kernels, staged in _routes(p):
                if form not in progs:
                    progs[form] = Program(p.image(form))
                    assert progs[form].compile(), p.name
                bad = run_route(progs[form], p, route, form, _staged(p.batch, form, layout, cuda),
                                flags, regs, kernels, oracle_mod, staged, junk)
                assert bad is None, bad
                n += 1
        finally:
            for q in progs.values():
                q.close()
    assert n
    _REF.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("half", [0, 1])
def test_matrix_fixed_slots_without_occupancy_variant(half):
    """EBPFEMU_FIXED_OCC=0 is read once, when the library first compiles: a fresh process
    (loadmatrix_child.py) runs the forward programs on fixed 64-byte slots there, on
    ebpf_tile_jit_fixed, and checks each against the oracle itself. (Two processes, each with
    every second program: one with all 104 took 13 s.)"""
    from ebpf_emu import _lib

    r = subprocess.run([sys.executable, os.path.join(HERE, "loadmatrix_child.py"),
                        os.path.join(ROOT, "ebpf-emu_amd"), os.path.join(ROOT, "oracle"), HERE,
                        f"{half}/2"],
                       capture_output=True, text=True, timeout=170,
                       env=dict(os.environ, EBPFEMU_FIXED_OCC="0"))
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["failures"] == [], d["failures"][0]
    assert d["kernels"] == [_lib.EBPF_KERNEL_JIT_FIXED]
    assert d["programs"] == len([p for p in PROGRAMS if p.kind != "loop"]) // 2 == 52
    REACHED.update(d["kernels"])


@pytest.mark.gpu
def test_every_kernel_reached():
    """Every kernel id of _lib.py but the tier-1 general interpreter ran some matrix program (the
    set recorded by the tests above: this one runs after them)."""
    from ebpf_emu import _lib

    want = set(range(len(_lib.KERNEL_NAMES))) - {_lib.EBPF_KERNEL_GENERAL_T1}
    missing = [_lib.KERNEL_NAMES[k] for k in sorted(want - REACHED)]
    assert not missing, (f"not reached: {missing} (the set is recorded by test_matrix_on_every_route "
                         "and test_matrix_fixed_slots_without_occupancy_variant: run the whole "
                         "module in one process)")
    _STAGED.clear()   # (the module's device buffers)
