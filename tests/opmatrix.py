"""The operand-edge matrix (test infrastructure): every ALU operation, END form and jump operator
of the reference (emu.rs:65-309), in both classes, with a register operand and with every
immediate of the lists below, over ONE batch of 640 packets whose two 64-bit operands are
per-lane run-time values -- so a wave holds taken and not-taken lanes, zero and non-zero divisors,
faulting and clean lanes side by side. fuzzgen.py reaches these operands only by luck (its edge
values are lddw immediates, the same in every lane).

Every program starts `ldxdw r6, [r1+0]; ldxdw r7, [r1+8]` (a, b: the packet's 16 bytes) and is
described by a `Prog`: the image plus the facts the closed form in test_opmatrix.py needs to
state its result without running it. No program relies on the step budget to end.
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field

from ebpf_emu.asm import assemble

M64 = (1 << 64) - 1

EDGE64 = [0, 1, 2, 3, 7, 0x1F, 0x20, 0x21, 0x3F, 0x40, 0x41,
          0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x100000000, 0x100000001,
          0x7FFFFFFFFFFFFFFF, 0x8000000000000000, 0x8000000000000001,
          0xFFFFFFFF00000000, 0xFFFFFFFF7FFFFFFF, 0xFFFFFFFF80000000,
          0xFFFFFFFFFFFFFFFE, 0xFFFFFFFFFFFFFFFF]
IMMS = [0, 1, -1, 0x7FFFFFFF, -0x80000000, 100]       # 0, 1, -1: inline constants; the rest literals
SHIFT_IMMS = [0, 1, 31, 32, 33, 63, 64, 65, -1, -4]
PAIR_SEED = 20241220     # the 64 random pairs
SHUFFLE_SEED = 1         # the order of the 640 pairs (test_opmatrix.test_batch_diverges holds for it)

ALU_REG_OPS = ["add", "sub", "mul", "div", "or", "and", "lsh", "rsh", "neg", "mod", "xor", "mov"]
ALU_IMM_OPS = ["add", "sub", "mul", "div", "or", "and", "mod", "xor", "mov"]
END_OPS = ["le16", "le32", "le64", "be16", "be32", "be64"]
JMP_OPS = ["jeq", "jgt", "jge", "jset", "jne", "jsgt", "jsge", "jlt", "jle", "jslt", "jsle"]
RESULT_REGS = [0, 2, 3, 4, 5, 8, 9, 1, 7]  # (r1 and r7 once the operands are copied: imm forms)

HEAD = "ldxdw r6, [r1+0]\nldxdw r7, [r1+8]\n"
STACK_STORE = "stxdw [r10-8], r6\n"  # the stack-window form of every program (memory tier 0.5)


def pairs() -> list[tuple[int, int]]:
    """All 576 ordered pairs of EDGE64 and 64 seeded random pairs, shuffled once: 10 waves."""
    ps = [(a, b) for a in EDGE64 for b in EDGE64]
    rng = random.Random(PAIR_SEED)
    ps += [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(64)]
    random.Random(SHUFFLE_SEED).shuffle(ps)
    return ps


def packet(a: int, b: int, size: int = 16) -> bytes:
    return a.to_bytes(8, "little") + b.to_bytes(8, "little") + bytes(size - 16)


def fmt_operand(src) -> str:
    return "none" if src is None else src if isinstance(src, str) else f"imm{src:#x}"


@dataclass
class Prog:
    name: str              # <kind>.<operator>.<class>.<operand form>[.<shape>]
    group: str             # the GPU tests' parametrisation
    kind: str              # "alu" | "fwd" | "loop"
    src: str               # assembly, without the stack store
    cls: int               # 64 | 32
    operand: object        # "r7" or the immediate
    op: str = ""           # the jump operator (kind fwd / loop)
    slots: list = field(default_factory=list)  # alu: (register, operation, operand) per result
    end64: bool = False    # END decoded in class ALU64 (emu.rs:74: either class)

    def _asm(self, text: str) -> bytes:
        img = bytearray(assemble(text))
        if self.end64:  # le/be assemble in class ALU (0xD4 / 0xDC): the same opcodes in ALU64
            for i in range(0, len(img), 8):
                if img[i] in (0xD4, 0xDC):
                    img[i] |= 0x03
        return bytes(img)

    @property
    def image(self) -> bytes:
        return self._asm(self.src)

    @property
    def stack_image(self) -> bytes:
        assert self.src.startswith(HEAD)
        return self._asm(HEAD + STACK_STORE + self.src[len(HEAD):])

    @property
    def what(self) -> str:
        """Operator, class and operand form, for failure messages."""
        ops = self.op or ",".join(dict.fromkeys(s[1] for s in self.slots))
        return f"{self.kind} {ops} class {self.cls} operand {fmt_operand(self.operand)}"


def _alu(name, group, cls, operand, slots, end64=False) -> Prog:
    sfx = "32" if cls == 32 else ""
    lines = [HEAD]
    for reg, op, src in slots:
        if reg != 7:
            lines.append(f"mov r{reg}, r6\n")
    if any(reg == 7 for reg, _, _ in slots):
        lines.append("mov r7, r6\n")  # (last: the other slots of an immediate program read no r7)
    for reg, op, src in slots:
        if op in END_OPS:
            lines.append(f"{op} r{reg}\n")
        elif op == "neg":
            lines.append(f"neg{sfx} r{reg}\n")
        else:
            lines.append(f"{op}{sfx} r{reg}, {src}\n")
    lines.append("exit\n")
    return Prog(name, group, "alu", "".join(lines), cls, operand, slots=list(slots), end64=end64)


def _fwd(op, cls, operand) -> Prog:
    """The forward program: r0 bits record which way each emission shape went.
      bit 0        taken lanes skip a single ALU instruction
      bits 1-3     a rule chain: three tests (r6, r6 + 1, r6 - 1) leave to one common target, with
                   only register ALU work in between (a complement region)
      bits 4-6     two tests with two different targets (a pending mask)
      r5, r2       a test directly before a div / a mod32 by the per-lane r7 (the out-of-line
                   divider entered with a partial exec)
      bit 8        the taken side leaves the program by a jump past its end"""
    j = op + ("32" if cls == 32 else "")
    b = operand if isinstance(operand, str) else str(operand)
    src = HEAD + f"""
        mov r0, 0
        {j} r6, {b}, s1
        or r0, 1
    s1: {j} r6, {b}, next
        or r0, 2
        mov r3, r6
        add r3, 1
        {j} r3, {b}, next
        or r0, 4
        mov r4, r6
        sub r4, 1
        {j} r4, {b}, next
        or r0, 8
    next:
        mov r8, r6
        add r8, 1
        {j} r6, {b}, t3a
        or r0, 16
        {j} r8, {b}, t3b
        or r0, 32
    t3a:
        or r0, 64
    t3b:
        mov r5, r6
        {j} r6, {b}, s5
        div r5, r7
    s5: mov r2, r6
        {j} r8, {b}, s6
        mod32 r2, r7
    s6: {j} r6, {b}, +4
        or r0, 256
        exit
    """
    name = f"jmp.{op}.{cls}.{fmt_operand(operand)}.fwd"
    return Prog(name, f"jmp-{op}-{cls}", "fwd", src, cls, operand, op=op)


def _loop(op, cls, operand) -> Prog:
    """The same test on a back edge; r9 ends every lane after three rounds whatever it does."""
    j = op + ("32" if cls == 32 else "")
    b = operand if isinstance(operand, str) else str(operand)
    src = HEAD + f"""
        mov r0, 0
        mov r9, 0
    L:  add r9, 1
        lsh r0, 2
        or r0, r9
        jge r9, 3, out
        {j} r6, {b}, L
    out:
        exit
    """
    name = f"jmp.{op}.{cls}.{fmt_operand(operand)}.loop"
    return Prog(name, f"jmp-{op}-{cls}", "loop", src, cls, operand, op=op)


def _chunks(xs, n):
    return [xs[i:i + n] for i in range(0, len(xs), n)]


def programs() -> list[Prog]:
    out = []
    for cls in (64, 32):
        g = f"alu-{cls}"
        # register forms: op rX, r7 after mov rX, r6 (six operations a program)
        for k, ops in enumerate(_chunks(ALU_REG_OPS, 6)):
            out.append(_alu(f"alu.{'+'.join(ops)}.{cls}.r7", g, cls, "r7",
                            [(RESULT_REGS[i], op, "r7") for i, op in enumerate(ops)]))
        # ARSH can end a lane with ST_ARITH (Q21): programs of its own
        out.append(_alu(f"alu.arsh.{cls}.r7", g, cls, "r7", [(0, "arsh", "r7")]))
        # END decodes in either class (Q7): the six valid forms, once per class
        out.append(_alu(f"alu.end.{cls}", g, cls, None,
                        [(RESULT_REGS[i], op, None) for i, op in enumerate(END_OPS)],
                        end64=cls == 64))
        for imm in IMMS:
            out.append(_alu(f"alu.nonshift.{cls}.{fmt_operand(imm)}", g, cls, imm,
                            [(RESULT_REGS[i], op, imm) for i, op in enumerate(ALU_IMM_OPS)]))
        shifts = [(op, imm) for imm in SHIFT_IMMS for op in ("lsh", "rsh")]
        for k, part in enumerate(_chunks(shifts, 7)):
            out.append(_alu(f"alu.lsh+rsh.{cls}.imms{k}", g, cls, "shift imms",
                            [(RESULT_REGS[i], op, imm) for i, (op, imm) in enumerate(part)]))
        if cls == 32:  # (arsh32 cannot overflow, emu.rs:156-159: its immediates share programs)
            for k, part in enumerate(_chunks(SHIFT_IMMS, 5)):
                out.append(_alu(f"alu.arsh.32.imms{k}", g, cls, "shift imms",
                                [(RESULT_REGS[i], "arsh", imm) for i, imm in enumerate(part)]))
        else:
            for imm in SHIFT_IMMS:
                out.append(_alu(f"alu.arsh.64.{fmt_operand(imm)}", "alu-arsh64", cls, imm,
                                [(0, "arsh", imm)]))
    for op in JMP_OPS:
        for cls in (64, 32):
            for operand in ["r7"] + IMMS:
                out.append(_fwd(op, cls, operand))
                out.append(_loop(op, cls, operand))
    names = [p.name for p in out]
    assert len(set(names)) == len(names)
    return out


def groups() -> list[str]:
    return list(dict.fromkeys(p.group for p in programs()))


# ---------------------------------------------------------------------------------------------
# The GPU side, shared by test_opmatrix.py and its child process (opmatrix_child.py).
STEPS = 20000  # (test_gpu_jit.STEPS: no program here comes near it)
# caller registers: r1 = 0 (the image address) and non-zero junk in every other register
JUNK_REGS = [0x0123456789ABCDEF, 0, 0xFFFFFFFF00000010, 0x8000000000000003, 0x7FFFFFFF, 0xDEADBEEFCAFEF00D,
             0x1111111122222222, 0x3333333344444444, 0xFFFFFFFFFFFFFFFF, 0x80000000, 0x5555555566666666]


def oracle_ref(oracle_mod, img: bytes, pkts, init_regs=None, mem_size=1024, r10=512):
    """oracle.Program.run_full over the batch, once: statuses, registers, verdict bytes and the 8
    counters (test_gpu_jit._vs_oracle's rule: r0 < 5 its own bucket, else bucket 5; faults bucket 6;
    retired steps bucket 7). pkts: what the oracle runs on (an xdp_md batch's ctx-prefixed
    images)."""
    import numpy as np

    op = oracle_mod.Program(img)
    n = len(pkts)
    st = np.zeros(n, dtype=np.uint8)
    regs = np.zeros((n, 11), dtype=np.uint64)
    verdict = np.zeros(n, dtype=np.uint8)
    cnt = np.zeros(8, dtype=np.uint64)
    for i, p in enumerate(pkts):
        kw = {} if init_regs is None else dict(init_regs=list(init_regs))
        s, r, _mem, steps = op.run_full(p, mem_size, r10, STEPS, **kw)
        st[i] = s
        regs[i] = r
        if s == 0:
            verdict[i] = r[0] if r[0] < 5 else 0xFE
            cnt[r[0] if r[0] < 5 else 5] += 1
        else:
            verdict[i] = 0xFF
            cnt[6] += 1
        cnt[7] += steps
    return dict(status=st, regs=regs, verdict=verdict, counters=cnt)


def launch(prog, frames, kw, want_kernels, prod=False, **flags):
    """One batch on the kernel it must land on (asserted with Program.batch_kernel for this very
    batch and these outputs, before anything runs). prod: the production outputs -- a verdict +
    counters launch and an r0 + status launch, neither asking for registers, so the compiled
    kernels run their liveness-pruned register init and dead-register sinking."""
    import numpy as np
    import torch

    from ebpf_emu import _lib

    dev = frames.device
    n = kw["n"]
    b = prog.make_batch(frames, max_steps=STEPS, **kw, **flags)
    t = dict(verdict=torch.empty(n, dtype=torch.uint8, device=dev),
             r0=torch.empty(n, dtype=torch.int64, device=dev),
             status=torch.empty(n, dtype=torch.uint8, device=dev),
             counters=torch.zeros(8, dtype=torch.int64, device=dev))
    if not prod:
        t["regs"] = torch.empty((n, 11), dtype=torch.int64, device=dev)
    outs = ([("verdict", "counters"), ("r0", "status")] if prod
            else [("verdict", "r0", "status", "regs", "counters")])
    for fields in outs:
        o = _lib.BatchOut()
        for f in fields:
            setattr(o, f, t[f].data_ptr())
        k = prog.batch_kernel(b, o)
        assert k in want_kernels, (f"lands on {_lib.KERNEL_NAMES[k]}, wanted "
                                   f"{[_lib.KERNEL_NAMES[w] for w in want_kernels]}")
        prog.launch(b, o)
    torch.cuda.synchronize()
    out = {f: v.cpu().numpy() for f, v in t.items()}
    for f in ("r0", "regs", "counters"):
        if f in out:
            out[f] = out[f].view(np.uint64)
    return out


def mismatch(p, route: str, img: bytes, prs, got, ref, full=None, lane_text=None):
    """None, or the first difference as one line that reproduces it: the program's operator,
    class and operand form, the route, the lane's (a, b) and the image. `got` against the oracle's
    `ref`; a production launch (no registers) also against the full launch of the same batch.
    lane_text(i): another matrix's description of lane i (loadmatrix.py), in place of (a, b)."""
    import numpy as np

    def lane(i, what, g, w):
        if lane_text is not None:
            where = lane_text(i)
        else:
            a, b = prs[i]
            where = f"(a, b) = ({a:#x}, {b:#x})"
        return (f"{p.what} [{p.name}] route {route}: {what} got {g} want {w} at lane {i} "
                f"{where} image {img.hex()}")

    ok = ref["status"] == 0
    for key in ("status", "verdict"):
        bad = np.nonzero(got[key] != ref[key])[0]
        if len(bad):
            i = int(bad[0])
            return lane(i, key, int(got[key][i]), int(ref[key][i]))
    if "regs" in got:
        bad = np.nonzero((got["regs"] != ref["regs"]).any(axis=1) & ok)[0]
        if len(bad):
            i = int(bad[0])
            r = int(np.nonzero(got["regs"][i] != ref["regs"][i])[0][0])
            slot = [f" ({op} {fmt_operand(src)})" for reg, op, src in p.slots if reg == r]
            return lane(i, f"r{r}{''.join(slot)}", hex(int(got["regs"][i][r])),
                        hex(int(ref["regs"][i][r])))
    bad = np.nonzero((got["r0"] != ref["regs"][:, 0]) & ok)[0]
    if len(bad):
        i = int(bad[0])
        return lane(i, "r0", hex(int(got["r0"][i])), hex(int(ref["regs"][i][0])))
    if list(got["counters"]) != list(ref["counters"]):
        return (f"{p.what} [{p.name}] route {route}: counters got {list(got['counters'])} want "
                f"{list(ref['counters'])} image {img.hex()}")
    if full is not None:
        for key in ("r0", "status", "verdict", "counters"):
            if not np.array_equal(got[key], full[key]):
                return (f"{p.what} [{p.name}] route {route}: {key} differs from the full-output "
                        f"launch image {img.hex()}")
    return None


def fixed_frames(prs, dev):
    """The batch on fixed 64-byte slots, no lens: (a, b) then 48 zero bytes a packet."""
    import numpy as np
    import torch

    pk = [packet(a, b, 64) for a, b in prs]
    frames = torch.tensor(np.frombuffer(b"".join(pk), dtype=np.uint8).copy(), device=dev)
    return pk, frames, dict(n=len(pk), stride=64)
