"""The load-edge matrix (test infrastructure): packet and stack loads of every width at the
address edges -- the 64-byte window's end, the packet's length, mem_size, a nonzero high word, a
signed overflow of base + offset, the stack window's two ends -- with per-lane run-time addresses,
so a wave holds window, straddling, far, past-len and faulting lanes side by side. The directed
constant-address programs of test_gpu_parity.py use one address in every lane and the fuzzers'
addresses are random packet bytes. Modelled on opmatrix.py, whose launch / oracle_ref / mismatch it
reuses.

Packets: byte i is (i * 73 + 41) % 255 + 1 (never zero: a byte wrongly taken as past len shows;
neighbours differ: an off-by-one shows), but bytes 0..7 = a and 8..15 = b of the lane, little
endian. Forward programs load at [a + off] into registers pre-filled with b; loop programs walk
from a with the stride b. Three batches: REG (register-address forward programs), LOOP, CONST (one
lane per packet length, constant addresses). Every program is described by a `Prog` holding the
facts the closed form in test_loadmatrix.py needs to state its result without running it. No
program relies on the step budget to end.

The xdp_md form of a program reads a and b at [r1+8] and [r1+16]: its image is [u32 8][u32 8 +
len][packet], so a lane's image length L runs as a packet of L - 8 bytes (L + 8 - 8 below 24).
"""
from __future__ import annotations

import random
import struct
from dataclasses import dataclass, field

from ebpf_emu.asm import assemble
from opmatrix import JUNK_REGS, STEPS, launch, mismatch, oracle_ref  # noqa: F401 (re-exported)

M64 = (1 << 64) - 1
MEM, R10 = 1024, 512
SMALL_MEM = 72            # the small-image route: mem_size = r10 = 72
WIDTHS = [1, 2, 4, 8]
LDX = {1: "ldxb", 2: "ldxh", 4: "ldxw", 8: "ldxdw"}
LENGTHS = [16, 17, 20, 23, 24, 31, 48, 56, 60, 63, 64, 65, 67, 68, 72, 80, 100, 127, 128, 129, 200,
           1023, 1024]
LEN_CLASSES = [[16, 17, 20, 23, 24, 31, 48], [56, 60, 63], [64], [65, 67, 68, 72, 80],
               [100, 127, 128, 129, 200, 1023, 1024]]
OFFSETS = [0, 1, -1, 3, 64, 65, -64, 0x7FFF, -0x8000]   # -16..64: inline constants; else literals
OFF_GROUPS = [[0, 1, -1, 3], [64, 65], [-64], [0x7FFF], [-0x8000]]
STACK_OFFSETS = [0, -1, 65]
LOOP_OFFSETS = [0, -1, 65]
STRIDES = [0, 1, 2, 3, 4, 7, 8, 15, 16, 17, 48, 63, 64, 65, M64, M64 - 15]
ROUNDS = 5                # a loop program's iterations
B_FIXED = [0, M64, 0xA5A5A5A55A5A5A5A]
SEED = 20250117           # b's random values
SHUFFLE_SEED = 3          # the lanes' order (test_loadmatrix.test_coverage holds for it)
STACK_K = 16              # the stack forms' window: [r10 - 16, r10)
STACK_E = list(range(480, 521))

XDP_FORMS, STACK_FORMS = ("xdp", "xstack"), ("stack", "xstack")
HEAD = "ldxdw r6, [r1+0]\nldxdw r7, [r1+8]\n"
XDP_HEAD = "ldxdw r6, [r1+8]\nldxdw r7, [r1+16]\n"
# (bytes 500..503 stay zero inside the 16-byte window)
STACK_STORES = "stxdw [r10-8], r6\nstxw [r10-16], r6\n"

# effective addresses whose behaviour does not depend on the packet's length (len >= 16)
E_FIXED = (list(range(0, 10)) + list(range(MEM - 9, MEM + 2)) +
           [0xFFFFFFFF, 1 << 32, (1 << 32) + 0x10, (1 << 63) - 1, 1 << 63, M64])
# around the window's end (every width at every split and alignment; up to SMALL_MEM + 1) and the
# 16-byte chunk edges past it
E_WINDOW = list(range(52, SMALL_MEM + 2)) + [79, 80, 95, 96, 111, 112, 127, 128]


_PATTERN = bytes((i * 73 + 41) % 255 + 1 for i in range(MEM + 16))


def pattern(n: int) -> bytearray:
    return bytearray(_PATTERN[:n])


def packet(a: int, b: int, size: int) -> bytes:
    p = pattern(size)
    p[0:16] = struct.pack("<QQ", a & M64, b & M64)
    return bytes(p)


def xdp_image_len(size: int) -> int:
    return size if size >= 24 else size + 8


def xdp_packet(a: int, b: int, size: int) -> bytes:
    """The packet whose xdp_md image [ctx][packet] is xdp_image_len(size) long, patterned by image
    position, a and b at image bytes 8 and 16."""
    img = pattern(xdp_image_len(size))
    img[8:24] = struct.pack("<QQ", a & M64, b & M64)
    return bytes(img[8:])


def xdp_image(pkt: bytes) -> bytes:
    return struct.pack("<II", 8, 8 + len(pkt)) + pkt


def _rot(xs, i):
    return xs[i % len(xs)]


def _edge_lanes(groups, full_len_edges, sink):
    """For every offset group: the addresses a = e - off of the edge lists, with lengths chosen by
    rotation (not a cross product): E_FIXED once, E_WINDOW with a short, a 64-byte and a long
    packet, and len-9 .. len+1 for every length (full_len_edges) or one per length class."""
    r = 0
    for g, offs in enumerate(groups):
        def put(e, size):
            for off in offs:
                sink((e - off) & M64, size)
        for e in E_FIXED:
            put(e, _rot(LENGTHS, r))
            r += 1
        for e in E_WINDOW:
            put(e, 64 if r % 3 == 0 else _rot(LEN_CLASSES[0] + LEN_CLASSES[1], r))
            put(e, _rot(LEN_CLASSES[3][-1:] + LEN_CLASSES[4], r))
            r += 1
        lens = [_rot(c, g + r + j) for c in LEN_CLASSES for j in range(2 if full_len_edges(g) else 1)]
        for size in lens:
            for e in range(size - 9, size + 2):
                put(e, size)


def reg_lanes() -> list[tuple[int, int, int]]:
    """(a, b, len) of the register-address forward batch."""
    seen, out = set(), []

    def sink(a, size):
        if (a, size) not in seen:
            seen.add((a, size))
            out.append((a, size))
    _edge_lanes(OFF_GROUPS, lambda g: g == 0, sink)
    # the stack forms' addresses: mostly in packets that reach past the window, so that the
    # image's bytes there are pattern bytes and differ from the stored ones (a's high bytes and
    # the gap are zero, as is the image past a short packet: a missed or a spurious overlay would
    # not show)
    for i, e in enumerate(STACK_E):
        for off in STACK_OFFSETS:
            sink((e - off) & M64, _rot(LENGTHS, i) if i % 4 == 3 else 1024 - i % 2)
    rng = random.Random(SEED)
    lanes = []
    for i, (a, size) in enumerate(out):
        b = B_FIXED[i % 6] if i % 6 < 3 else rng.getrandbits(64)
        lanes.append((a, b, size))
    random.Random(SHUFFLE_SEED).shuffle(lanes)
    return lanes


def loop_lanes() -> list[tuple[int, int, int]]:
    """(a, stride, len) of the loop batch: the edge addresses as first addresses, walks that cross
    byte 64 in both directions and leave the packet, and the stack window's neighbourhood."""
    seen, out = set(), []
    k = [0]

    def sink(a, size):
        if (a, size) not in seen:
            seen.add((a, size))
            out.append((a, _rot(STRIDES, k[0]), size))
            k[0] += 1
    _edge_lanes([[0, -1], [65]], lambda g: False, sink)
    starts = [0, 16, 40, 56, 60, 62, 63, 64, 66, 70, 100, 126, 130, 190]
    for i, s in enumerate(starts):
        for j, st in enumerate(STRIDES):
            size = _rot([64, 100, 128, 200, 1024, 48, 72, 129], i + j)
            if (s, size, st) not in seen:
                seen.add((s, size, st))
                out.append((s, st, size))
    for i, e in enumerate(range(478, 523)):
        for st in (_rot([0, 1, 2, 3, 4, 7, 8, M64, M64 - 15], i), _rot([1, M64, 4, 8], i)):
            out.append((e, st, _rot(LENGTHS, i) if i % 4 == 3 else 1024 - i % 2))
    random.Random(SHUFFLE_SEED).shuffle(out)
    return out


CONST_LENGTHS = list(range(0, 81)) + [100, 127, 128, 129, 200, 1023, 1024]
CONST_KS = [0, 1, 2, 3, 5, 7] + list(range(56, 68)) + [70, 100, 127, 128]
CONST_MEM_KS = list(range(MEM - 9, MEM + 2))


def const_lanes() -> list[tuple[int, int, int]]:
    """One lane per packet length (a, b: pattern bytes like the rest)."""
    return [(None, None, n) for n in CONST_LENGTHS]


@dataclass
class Prog:
    name: str
    group: str             # the GPU tests' parametrisation
    family: str            # the coverage test's unit: the programs sharing an offset / a kind
    kind: str              # "fwd" | "loop" | "const"
    body: str              # assembly after the head (and the stack stores)
    loads: list            # (width, dst register, base register, offset) in program order
    off: int = 0
    rebase: int = 0        # const: r1 is set to this before the loads
    has_stack_form: bool = False
    mul: bool = True       # loop: r0 = r0 * 31 + the loads (False: r0 += the loads)
    byte_head: bool = False  # a and b read with one-byte loads: a & 0xFFFF, b & 0xFF (r4: a & 0xFF00)
    slots: list = field(default_factory=list)   # (opmatrix.mismatch reads it; none here)

    @property
    def batch(self) -> str:
        return {"fwd": "reg", "loop": "loop", "const": "const"}[self.kind]

    def src(self, form: str = "plain") -> str:
        if self.kind == "const":
            return self.body
        head = XDP_HEAD if form in XDP_FORMS else HEAD
        if self.byte_head:
            k = 8 if form in XDP_FORMS else 0
            head = (f"ldxb r6, [r1+{k}]\nldxb r4, [r1+{k + 1}]\nlsh r4, 8\nor r6, r4\n"
                    f"ldxb r7, [r1+{k + 8}]\n")
        return head + (STACK_STORES if form in STACK_FORMS else "") + self.body

    def image(self, form: str = "plain") -> bytes:
        return assemble(self.src(form))

    @property
    def what(self) -> str:
        ws = ",".join(str(w) for w, _d, _b, _o in self.loads)
        return f"{self.kind} load width {ws} offset {self.off:#x}"


def _mem(base, off):
    return f"[r{base}{'+' if off >= 0 else '-'}{abs(off):#x}]"


_DST = [2, 3, 4, 5]


def _fwd(name, off, widths) -> Prog:
    loads = [(w, _DST[i], 6, off) for i, w in enumerate(widths)]
    s = "".join(f"mov r{d}, r7\n" for _w, d, _b, _o in loads)
    s += "".join(f"{LDX[w]} r{d}, {_mem(b, o)}\n" for w, d, b, o in loads)
    s += f"mov r0, r{loads[0][1]}\n" + "".join(f"xor r0, r{d}\n" for _w, d, _b, _o in loads[1:])
    return Prog(name, f"reg{off:+#x}", f"reg{off:+#x}", "fwd", s + "exit\n", loads, off=off,
                has_stack_form=len(widths) == 4 and off in STACK_OFFSETS)


def _const(name, k, widths, rebase) -> Prog:
    loads = [(w, _DST[i], 1, k - rebase) for i, w in enumerate(widths)]
    s = "".join(f"mov r{d}, -1\n" for _w, d, _b, _o in loads)
    s += f"mov r1, {rebase}\n" if rebase else ""
    s += "".join(f"{LDX[w]} r{d}, {_mem(b, o)}\n" for w, d, b, o in loads)
    s += f"mov r0, r{loads[0][1]}\n" + "".join(f"xor r0, r{d}\n" for _w, d, _b, _o in loads[1:])
    group = "const-mem" if k in CONST_MEM_KS else f"const-{'lo' if k < 60 else 'hi'}"
    return Prog(name, group, "const", "const", s + "exit\n", loads, off=k, rebase=rebase)


def _loop(name, off, widths) -> Prog:
    loads = [(w, 3 + i, 6, off) for i, w in enumerate(widths)]
    s = "mov r0, 0\nmov r9, 0\nL:\n"
    s += "".join(f"{LDX[w]} r{d}, {_mem(b, o)}\n" for w, d, b, o in loads)
    s += "mul r0, 31\n" + "".join(f"add r0, r{d}\n" for _w, d, _b, _o in loads)
    s += f"add r6, r7\nadd r9, 1\njlt r9, {ROUNDS}, L\nexit\n"
    return Prog(name, f"loop{off:+#x}", f"loop{off:+#x}", "loop", s, loads, off=off,
                has_stack_form=off == 0 and widths in ([1], [4], [8]))


def programs() -> list[Prog]:
    out = []
    for off in OFFSETS:
        out.append(_fwd(f"reg.asc.{off:+#x}", off, [1, 2, 4, 8]))
        out.append(_fwd(f"reg.desc.{off:+#x}", off, [8, 4, 2, 1]))
    for off in (0, 65):     # the all-one-byte and one-load specialisations
        for w in WIDTHS:
            out.append(_fwd(f"reg.single{w}.{off:+#x}", off, [w]))
    for k in CONST_KS + CONST_MEM_KS:
        out.append(_const(f"const.asc.{k}", k, [1, 2, 4, 8], 0))
        out.append(_const(f"const.asc.{k}.rebased", k, [1, 2, 4, 8], 8))
    for k in CONST_MEM_KS:
        out.append(_const(f"const.desc.{k}", k, [8, 4, 2, 1], 0))
    for off in LOOP_OFFSETS:
        for w in WIDTHS:
            out.append(_loop(f"loop.w{w}.{off:+#x}", off, [w]))
        out.append(_loop(f"loop.mixed.{off:+#x}", off, [1, 4]))   # (a 4-byte load: no zwin)
    # every load one byte wide, the head's too: the loop compiler's zero-past-len windows and
    # qword cache (jit.cpp zwin, qcache) need that. Not a coverage family.
    for off in LOOP_OFFSETS:
        q = _loop(f"loop.bytes.{off:+#x}", off, [1])
        q.family, q.byte_head, q.has_stack_form = "", True, False
        if off == 65:   # (the multiply's temporaries are the qword cache's registers: no qcache)
            q.mul, q.body = False, q.body.replace("mul r0, 31\n", "")
        out.append(q)
    # one long forward program (83 micro-ops: past the tile interpreter's 62, so EBPF_BATCH_NO_JIT
    # runs it on dag_kernel): every offset's asc and desc loads in a row. Not a coverage family.
    loads = [(w, _DST[i], 6, off) for off in OFFSETS for ws in ([1, 2, 4, 8], [8, 4, 2, 1])
             for i, w in enumerate(ws)]
    s = "".join(f"mov r{d}, r7\n" for d in _DST)
    s += "".join(f"{LDX[w]} r{d}, {_mem(b, o)}\n" for w, d, b, o in loads)
    s += "mov r0, r2\nxor r0, r3\nxor r0, r4\nxor r0, r5\nexit\n"
    out.append(Prog("reg.chain", "reg-chain", "", "fwd", s, loads))
    names = [p.name for p in out]
    assert len(set(names)) == len(names)
    return out


def groups() -> list[str]:
    return list(dict.fromkeys(p.group for p in programs()))


FORMS = ("plain", "stack", "xdp", "xstack")   # xstack: the stack-window form under xdp_md


def forms(p: Prog) -> list[str]:
    return (["plain"] + (["stack"] if p.has_stack_form else []) + ["xdp"] +
            (["xstack"] if p.has_stack_form else []))


_LANES = {}


def lanes(batch: str):
    if batch not in _LANES:
        _LANES[batch] = {"reg": reg_lanes, "loop": loop_lanes, "const": const_lanes}[batch]()
    return _LANES[batch]


def lane_packet(lane, form: str = "plain", size=None) -> bytes:
    """The packet of a lane; size overrides its length (the fixed-slot routes: len = stride)."""
    a, b, n = lane
    n = n if size is None else size
    if a is None:           # a constant-address lane: pattern bytes only (size: the image's length)
        if form in XDP_FORMS:
            return bytes(pattern(8 + n if size is None else size)[8:])
        return bytes(pattern(n))
    return xdp_packet(a, b, n) if form in XDP_FORMS else packet(a, b, n)


def lane_image(lane, form: str = "plain", size=None) -> bytes:
    """What the oracle runs on: the packet, or the ctx-prefixed image of the xdp_md form."""
    p = lane_packet(lane, form, size)
    return xdp_image(p) if form in XDP_FORMS else p


def fmt_lane(lane) -> str:
    a, b, n = lane
    return f"len = {n}" if a is None else f"(a, b, len) = ({a:#x}, {b:#x}, {n})"


# ---------------------------------------------------------------------------------------------
# The closed form's vocabulary, shared with the failure messages: the classes of one access.
def classify(base: int, off: int, w: int, size: int, mem: int = MEM, stack: bool = False,
             r10: int = R10) -> set:
    """The classes of a width-w load at base + off (base: u64 register value) from an image whose
    packet is `size` bytes, as the coverage test names them."""
    sb = base - (1 << 64) if base >> 63 else base
    s = sb + off
    if not -(1 << 63) <= s < (1 << 63):
        return {"mem-overflow"}
    a = s & M64
    if a >= mem:
        if a >> 32 and (a & 0xFFFFFFFF) < 64:
            return {"mem-highword"}
        return {"mem-at-mem"} if a == mem else {"mem-past"}
    if a + w > mem:
        return {f"ub-{mem - a}"}
    c = set()
    if sb < 0:
        c.add("wrap")
    if a + w <= 64:
        c.add("win")
    elif a < 64:
        c.add(f"split64-{64 - a}")
    else:
        c.add("far")
    if a + w <= size:
        c.add("in-len")
        if a >= 64:
            c.add("far-in-len")
    elif a < size:
        c.add(f"lensplit-{size - a}")
    else:
        c.add("past-len")
    if stack:
        lo, hi = r10 - STACK_K, r10
        n = max(0, min(a + w, hi) - max(a, lo))
        if n and a <= lo:
            c.add(f"stk-lo-{n}")
        if n and a + w >= hi:
            c.add(f"stk-hi-{n}")
        if a + w == lo:
            c.add("stk-miss-lo")
        if a == hi:
            c.add("stk-miss-hi")
        if max(a, r10 - 12) < min(a + w, r10 - 8):
            c.add("stk-gap")
    return c


# ---------------------------------------------------------------------------------------------
# The GPU side, shared by test_loadmatrix.py and its child process (loadmatrix_child.py).
def stage_fixed(pkts, stride, dev):
    import numpy as np
    import torch

    assert all(len(p) == stride for p in pkts)
    frames = torch.tensor(np.frombuffer(b"".join(pkts), dtype=np.uint8).copy(), device=dev)
    return frames, dict(n=len(pkts), stride=stride)


def stage_offsets(pkts, dev, first=0, gap=0, align=16):
    """Offsets + lens: packet i at the next address that is `first` mod `align`, at least `gap`
    bytes past the one before (gap 16 at 8 mod 16: a capture's record headers)."""
    import numpy as np
    import torch

    offs, pos, chunks = [], 0, []
    for p in pkts:
        pad = gap + (first - (pos + gap)) % align
        chunks.append(bytes(pad))
        pos += pad
        offs.append(pos)
        chunks.append(p)
        pos += len(p)
    buf = b"".join(chunks) + bytes(64)
    frames = torch.tensor(np.frombuffer(buf, dtype=np.uint8).copy(), device=dev)
    o = torch.tensor(np.array(offs, dtype=np.uint32).view(np.int32), device=dev)
    ln = torch.tensor(np.array([len(p) for p in pkts], dtype=np.uint16).view(np.int16), device=dev)
    return frames, dict(n=len(pkts), offsets=o, lens=ln)


def stage_stride_lens(pkts, dev):
    import numpy as np
    import torch

    stride = (max(len(p) for p in pkts) + 15) // 16 * 16
    buf = np.zeros(len(pkts) * stride + 64, dtype=np.uint8)
    for i, p in enumerate(pkts):
        buf[i * stride:i * stride + len(p)] = np.frombuffer(p, dtype=np.uint8)
    ln = torch.tensor(np.array([len(p) for p in pkts], dtype=np.uint16).view(np.int16), device=dev)
    return torch.tensor(buf, device=dev), dict(n=len(pkts), stride=stride, lens=ln)
