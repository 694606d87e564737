"""EBPF_BATCH_WRITEBACK: the rewritten packets written back in place (include/ebpf_emu.h).

The expected buffer is built on the CPU from the oracle alone: the input buffer, and for every
packet whose oracle status is OK the oracle's final memory bytes [0, len) (xdp_md: the image
[8][8 + len][packet]'s bytes [8, 8 + len)) over the packet. The WHOLE device buffer is compared
with it -- the sentinel-filled gaps between offsets-layout packets and the slot bytes past a
packet's length included -- so a write outside a packet, a write for a faulted packet and a
missing write all show.

CPU: the flag's value, make_batch's bit, and the write-back variant (ebpf_prog_jit_asm variant 7)
of the store workloads and of random store programs compiles and assembles without a GPU, leaving
variant 1's text as it was.
GPU: NAT on six layouts (routes asserted, deopt lanes rewritten too), the MAC swap, the responder's
trailer at byte 1500, random store programs (compiled == general interpreter == expected, packed
packets with no gap), a program without stores, a loop program and a packet atomic on the general
interpreter, xdp_md with ctx stores, a binding step budget, the unknown flag bit.
"""
import random
import struct
import zlib

import numpy as np
import pytest

from fuzzgen import gen_store_program

SENT = 0xA5
STEPS = 20000
PACKED_LENS = [1, 3, 15, 16, 17, 60, 63, 64, 65, 130]
LAYOUTS = ["fixed64", "fixed128", "offsets16", "offsets_mis3", "stride_lens", "xdp_offsets"]


# ---------------------------------------------------------------- CPU
def test_flag_value(product_lib):
    import os
    import re

    from ebpf_emu import _lib

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                            "ebpf_emu.h")).read()
    m = re.search(r"#define\s+EBPF_BATCH_WRITEBACK\s+(\d+)u", hdr)
    assert m and int(m.group(1)) == 8
    assert _lib.BATCH_WRITEBACK == 8


def test_make_batch_sets_the_bit(product_lib):
    import torch

    from ebpf_emu import Program, _lib
    from ebpf_emu import workloads as W

    p = Program(W.program("nat"))
    fr = torch.zeros(128, dtype=torch.uint8)
    assert p.make_batch(fr, n=2, stride=64, writeback=True).flags & _lib.BATCH_WRITEBACK
    assert not p.make_batch(fr, n=2, stride=64).flags & _lib.BATCH_WRITEBACK
    assert p.make_batch(fr, n=2, stride=64, writeback=True, xdp_md=True).flags == 10
    p.close()


def _wb_variant_checked(img):
    from ebpf_emu import Program, _lib

    p = Program(img)
    try:
        if not p.stack_window or not p.compile():
            return False
        before = p.jit_asm(1)
        try:
            a = p.jit_asm(7)
        except _lib.EbpfError:
            # (a stack program without packet stores has no write-back variant: nothing to write)
            assert not p.store_mode, img.hex()
            return False
        assert a and "write-back" in a and "global_store_" in a
        assert p.jit_asm(1) == before, "variant 1 changed by the write-back variant's compile"
        return True
    finally:
        p.close()


def test_writeback_variant_compiles(product_lib):
    from ebpf_emu import workloads as W

    for name in ("nat", "mac_swap_tx", "responder"):
        assert _wb_variant_checked(W.program(name)), name
    rng = random.Random(4242)
    n = 0
    for _ in range(60):
        img = gen_store_program(rng)
        try:
            n += _wb_variant_checked(img)
        except Exception as e:  # (a program the loader rejects)
            if type(e).__name__ != "DecodeError":
                raise
    assert n >= 35, n


def test_run_refuses_frames_it_cannot_write(product_lib):
    """writeback=True: a non-contiguous view and an inference tensor (torch's only read-only kind)
    are refused before anything is launched (no GPU needed: CPU tensors)."""
    import torch

    from ebpf_emu import Program
    from ebpf_emu import workloads as W

    p = Program(W.program("nat"))
    fr = torch.zeros(4 * 64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="contiguous"):
        p.run(fr.reshape(4, 64)[:, :32], n=4, stride=32, writeback=True)
    with torch.inference_mode():
        ro = torch.zeros(4 * 64, dtype=torch.uint8)
    assert ro.is_inference()
    with pytest.raises(ValueError, match="writable"):
        p.run(ro, n=4, stride=64, writeback=True)
    p.close()


# ---------------------------------------------------------------- helpers (GPU)
def _lay(pkts, layout, rng=None):
    """-> (buf u8 numpy, run kwargs as numpy, [(start, len)], xdp, packets as the kernel sees them)"""
    xdp = layout.startswith("xdp")
    if layout.startswith("fixed"):
        stride = int(layout[5:])
        pk = [p[:stride].ljust(stride, b"\0") for p in pkts]
        buf = np.frombuffer(b"".join(pk), dtype=np.uint8).copy()
        return buf, dict(n=len(pk), stride=stride), [(i * stride, stride) for i in range(len(pk))], xdp, pk
    if layout == "stride_lens":
        stride = (max(64, max(len(p) for p in pkts)) + 15) // 16 * 16
        buf = np.full(len(pkts) * stride, SENT, dtype=np.uint8)
        for i, p in enumerate(pkts):
            buf[i * stride:i * stride + len(p)] = np.frombuffer(p, dtype=np.uint8)
        lens = np.array([len(p) for p in pkts], dtype=np.uint16)
        return buf, dict(n=len(pkts), stride=stride, lens=lens), [(i * stride, len(p)) for i, p in enumerate(pkts)], xdp, pkts
    align, mis = {"offsets16": (16, 0), "xdp_offsets": (16, 0), "offsets_mis3": (1, 3),
                  "packed": (1, 0)}[layout]
    offs, pos = [], 16 if layout != "packed" else 0
    for p in pkts:
        pos += mis + (-(pos + mis)) % align
        offs.append(pos)
        pos += len(p)
    buf = np.full(pos + 32, SENT, dtype=np.uint8)
    for o, p in zip(offs, pkts):
        buf[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
    kw = dict(n=len(pkts), offsets=np.array(offs, dtype=np.uint32),
              lens=np.array([len(p) for p in pkts], dtype=np.uint16))
    return buf, kw, [(o, len(p)) for o, p in zip(offs, pkts)], xdp, pkts


def _expected(oracle_mod, img, buf, spans, xdp, mem_size=1024, r10=512, max_steps=STEPS):
    """-> (expected buffer, oracle statuses)"""
    op = oracle_mod.Program(img)
    exp = buf.copy()
    sts = []
    for o, ln in spans:
        pkt = bytes(buf[o:o + ln])
        if xdp:
            if 8 + ln > mem_size:
                sts.append(7)
                continue
            image = (struct.pack("<II", 8, 8 + ln) + pkt).ljust(mem_size, b"\0")
            regs = [0] * 11
            regs[2], regs[10] = 8 + ln, r10
            st, _, mem, _, _ = op.run_image(image, regs, (), max_steps)
            mem = mem[8:8 + ln]
        else:
            st, _, mem, _ = op.run_full(pkt, mem_size, r10, max_steps)
            mem = mem[:ln]
        sts.append(st)
        if st == 0:
            exp[o:o + ln] = np.frombuffer(mem, dtype=np.uint8)
    return exp, np.array(sts, dtype=np.uint8)


def _dev_kw(kw, dev):
    import torch

    out = dict(kw)
    if "offsets" in kw:
        out["offsets"] = torch.tensor(kw["offsets"].view(np.int32), device=dev)
    if "lens" in kw:
        out["lens"] = torch.tensor(kw["lens"].view(np.int16), device=dev)
    return out


def _run(prog, buf, kw, dev, writeback, xdp=False, ws=None, fp=False, **extra):
    """One run over a fresh device copy of buf -> (outputs dict, final buffer, kernel id)."""
    import torch

    from ebpf_emu import _lib

    fr = torch.from_numpy(buf.copy()).to(dev)
    dkw = _dev_kw(kw, dev)
    cnt = torch.zeros(8, dtype=torch.int64, device=dev)
    b = prog.make_batch(fr, xdp_md=xdp, writeback=writeback, workspace=ws, **dkw, **extra)
    kid = prog.batch_kernel(b)
    n = b.n
    t = dict(verdict=torch.zeros(n, dtype=torch.uint8, device=dev),
             r0=torch.zeros(n, dtype=torch.int64, device=dev),
             status=torch.zeros(n, dtype=torch.uint8, device=dev),
             regs=torch.zeros((n, 11), dtype=torch.int64, device=dev))
    out = _lib.BatchOut()
    if fp:  # (the final frame stacks: the same route with and without them for these programs)
        t["fp"] = torch.zeros((n, _lib.MAX_CALL_DEPTH), dtype=torch.int32, device=dev)
        t["fp_len"] = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        out.fp, out.fp_len = t["fp"].data_ptr(), t["fp_len"].data_ptr()
    out.verdict, out.r0, out.status = t["verdict"].data_ptr(), t["r0"].data_ptr(), t["status"].data_ptr()
    out.regs, out.counters = t["regs"].data_ptr(), cnt.data_ptr()
    kid = prog.batch_kernel(b, out)
    prog.launch(b, out, torch.cuda.current_stream())
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in t.items()}
    res["counters"] = cnt.cpu().numpy()
    return res, fr.cpu().numpy(), kid


def _identical_outputs(a, b, tag):
    """Flag on against flag off (the same kernel route): every output, every lane, bit for bit."""
    assert set(a) == set(b) and "fp" in a and "fp_len" in a, tag
    for k in a:
        assert np.array_equal(a[k], b[k]), (k, tag)


def _same_outputs(a, b, tag):
    """A compiled route against the general interpreter: r0 and the registers of a faulted lane
    are the values at the fault, which the routes need not share (include/ebpf_emu.h r0)."""
    ok = a["status"] == 0
    for k in ("status", "verdict", "counters"):
        assert np.array_equal(a[k], b[k]), (k, tag)
    for k in ("r0", "regs"):
        assert np.array_equal(a[k][ok], b[k][ok]), (k, tag)


def _buf_eq(got, exp, tag):
    if not np.array_equal(got, exp):
        d = np.nonzero(got != exp)[0]
        raise AssertionError((tag, "first differing bytes", d[:8].tolist(), got[d[:8]].tolist(),
                              exp[d[:8]].tolist(), "count", len(d)))


def _changed(exp, buf, spans):
    return sum(1 for o, ln in spans if not np.array_equal(exp[o:o + ln], buf[o:o + ln]))


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_nat(cuda, oracle_mod, layout):
    import torch

    from ebpf_emu import Program, _lib
    from ebpf_emu import workloads as W
    from test_store_mode import _nat_packets

    img = W.program("nat")
    n = 130
    pkts = _nat_packets(random.Random(31), n, long_options=0.3)
    buf, kw, spans, xdp, pk = _lay(pkts, layout)
    exp, sts = _expected(oracle_mod, img, buf, spans, xdp)
    if not xdp:  # (under xdp_md NAT reads the ctx-prefixed image: parity only, as test_store_mode)
        assert _changed(exp, buf, spans) >= n // 4, _changed(exp, buf, spans)
    prog = Program(img)
    b0 = prog.make_batch(torch.from_numpy(buf.copy()).to(cuda), xdp_md=xdp, **_dev_kw(kw, cuda))
    ws = torch.zeros(prog.workspace_bytes(b0, 0), dtype=torch.uint8, device=cuda)
    ws[8:12] = 0xFF
    got, fin, kid = _run(prog, buf, kw, cuda, True, xdp, ws=ws, fp=True)
    if layout.startswith("fixed"):
        assert kid == _lib.EBPF_KERNEL_JIT_STACK, kid
    elif layout in ("offsets16", "xdp_offsets"):
        assert kid == _lib.EBPF_KERNEL_JIT_VARL_STACK, kid
    else:
        assert kid in (_lib.EBPF_KERNEL_JIT_VARL_STACK, _lib.EBPF_KERNEL_GENERAL_T1), kid
    _buf_eq(fin, exp, f"nat {layout}")
    assert np.array_equal(got["status"], sts)
    # (the IHL >= 13 lanes, whose port lies past the 64-byte window, are rewritten too -- through
    # the overflow image since NAT is proven deopt-free; test_deopt_lanes covers the deopt pass)
    far = [i for i, p in enumerate(pk) if len(p) > 14 and (p[14] & 15) >= 13]
    assert far
    if not xdp and layout != "fixed64":
        assert any(not np.array_equal(exp[o:o + ln], buf[o:o + ln]) for o, ln in (spans[i] for i in far))
    if kid != _lib.EBPF_KERNEL_GENERAL_T1:
        # no lane left for the general interpreter: the list's count is 0 and the deopt pass, NAT
        # being proven deopt-free, was not launched (+8 keeps the 0xFFFFFFFF set above), as
        # test_store_mode._assert_no_deopt reads it
        w = ws[:12].cpu().numpy().view(np.uint32)
        assert w[0] == 0 and w[2] == (0xFFFFFFFF if prog.store_mode_no_deopt else 0), w
    off, fin0, kid0 = _run(prog, buf, kw, cuda, False, xdp, fp=True)
    assert kid0 == kid
    _identical_outputs(got, off, f"nat {layout} flag off")
    _buf_eq(fin0, buf, f"nat {layout}: a flag-off run wrote the packets")
    prog.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [130, 1])
def test_mac_swap(cuda, oracle_mod, n):
    from ebpf_emu import Program, _lib
    from ebpf_emu import workloads as W

    img = W.program("mac_swap_tx")
    rng = random.Random(9)
    pkts = [bytes(rng.getrandbits(8) for _ in range(64)) for _ in range(n)]
    buf, kw, spans, xdp, pk = _lay(pkts, "fixed64")
    exp, sts = _expected(oracle_mod, img, buf, spans, False)
    prog = Program(img)
    got, fin, kid = _run(prog, buf, kw, cuda, True, fp=True)
    assert kid == _lib.EBPF_KERNEL_JIT_STACK
    _buf_eq(fin, exp, "mac_swap")
    f, b = fin.reshape(n, 64), buf.reshape(n, 64)
    assert np.array_equal(f[:, 0:6], b[:, 6:12]) and np.array_equal(f[:, 6:12], b[:, 0:6])
    assert np.array_equal(f[:, 12:], b[:, 12:])
    off, _, _ = _run(prog, buf, kw, cuda, False, fp=True)
    _identical_outputs(got, off, "mac_swap flag off")
    prog.close()


@pytest.mark.gpu
def test_responder_trailer(cuda, oracle_mod):
    import torch

    from ebpf_emu import Program, _lib
    from ebpf_emu import workloads as W
    from test_store_far import _ipv4

    img = W.program("responder")
    rng = random.Random(12)
    n = 130
    pkts = [_ipv4(rng, 1504, 1, rng.choice([5, 6, 15]), 8) if i % 3 == 0
            else _ipv4(rng, 1504, rng.choice([6, 17]), 5) for i in range(n)]
    buf, kw, spans, xdp, pk = _lay(pkts, "fixed1504")
    exp, sts = _expected(oracle_mod, img, buf, spans, False, mem_size=2048, r10=2048)
    e, b = exp.reshape(n, 1504), buf.reshape(n, 1504)
    assert (e[:, 1500:] != b[:, 1500:]).any(axis=1).sum() >= n // 2   # trailers
    assert (e[:, :64] != b[:, :64]).any(axis=1).sum() >= n // 4       # header rewrites
    prog = Program(img)
    b0 = prog.make_batch(torch.from_numpy(buf.copy()).to(cuda), mem_size=2048, r10=2048, **kw)
    ws = torch.zeros(prog.workspace_bytes(b0, 0), dtype=torch.uint8, device=cuda)
    got, fin, kid = _run(prog, buf, kw, cuda, True, ws=ws, fp=True, mem_size=2048, r10=2048)
    assert kid == _lib.EBPF_KERNEL_JIT_STACK
    _buf_eq(fin, exp, "responder")
    w = ws[:12].cpu().numpy().view(np.uint32)
    assert w[0] == 0 and w[2] == 0, w  # zero deopts
    off, _, _ = _run(prog, buf, kw, cuda, False, fp=True, mem_size=2048, r10=2048)
    _identical_outputs(got, off, "responder flag off")
    prog.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["fixed128", "offsets_mis3"])
def test_deopt_lanes(cuda, oracle_mod, layout):
    """Lanes that deoptimize (r10 = 128: a store ending past the stack window's start) are listed
    with their packets untouched, re-run by the deopt pass and written back by it."""
    import torch

    from ebpf_emu import Program, _lib
    from ebpf_emu.asm import assemble
    from test_store_mode import DEOPT_PROG

    img = assemble(DEOPT_PROG)
    rng = random.Random(77)
    pkts = [bytes(rng.getrandbits(8) for _ in range(rng.choice([10, 15, 21, 60, 64, 100, 128])))
            for _ in range(130)]
    buf, kw, spans, xdp, pk = _lay(pkts, layout)
    exp, sts = _expected(oracle_mod, img, buf, spans, False, r10=128)
    prog = Program(img)
    s0 = 128 - prog.stack_window
    want = sum(1 for p in pk if len(p) > 14 and 2 * p[14] + 1 > s0)
    assert want >= 20 and _changed(exp, buf, spans) >= 30
    b0 = prog.make_batch(torch.from_numpy(buf.copy()).to(cuda), r10=128, **_dev_kw(kw, cuda))
    ws = torch.zeros(prog.workspace_bytes(b0, 0), dtype=torch.uint8, device=cuda)
    got, fin, kid = _run(prog, buf, kw, cuda, True, ws=ws, r10=128)
    assert kid in (_lib.EBPF_KERNEL_JIT_STACK, _lib.EBPF_KERNEL_JIT_VARL_STACK), kid
    assert int(ws[:12].cpu().numpy().view(np.uint32)[2]) == want
    _buf_eq(fin, exp, f"deopt {layout}")
    assert np.array_equal(got["status"], sts)
    prog.close()


def _packed_packets(rng, n):
    return [bytes(rng.getrandbits(8) for _ in range(rng.choice(PACKED_LENS))) for _ in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS + ["packed"])
def test_store_fuzz(cuda, oracle_mod, layout):
    from ebpf_emu import Program, _lib
    from test_stack_tier import _var_packets

    rng = random.Random(zlib.crc32(b"wb" + layout.encode()))
    ran = faulted = changed = compiled = 0
    while ran < 12:
        img = gen_store_program(rng)
        try:
            oracle_mod.Program(img)
            prog = Program(img)
        except Exception:
            continue
        if not prog.stack_window:
            prog.close()
            continue
        n = 130
        pkts = _packed_packets(rng, n) if layout == "packed" else _var_packets(rng, n)
        buf, kw, spans, xdp, pk = _lay(pkts, layout)
        exp, sts = _expected(oracle_mod, img, buf, spans, xdp)
        faulted += int((sts != 0).sum())
        changed += _changed(exp, buf, spans)
        got, fin, kid = _run(prog, buf, kw, cuda, True, xdp, max_steps=STEPS)
        compiled += kid in (_lib.EBPF_KERNEL_JIT_STACK, _lib.EBPF_KERNEL_JIT_VARL_STACK)
        _buf_eq(fin, exp, f"fuzz {layout} compiled {img.hex()}")
        assert np.array_equal(got["status"], sts), (layout, img.hex())
        gen, fing, kidg = _run(prog, buf, kw, cuda, True, xdp, max_steps=STEPS, generic=True)
        assert kidg == _lib.EBPF_KERNEL_GENERAL_T1
        _buf_eq(fing, exp, f"fuzz {layout} generic {img.hex()}")
        _same_outputs(got, gen, f"fuzz {layout} {img.hex()}")
        for i, (o, ln) in enumerate(spans):  # faulted packets: their input bytes
            if sts[i] != 0:
                assert np.array_equal(fin[o:o + ln], buf[o:o + ln]), (layout, i)
        prog.close()
        ran += 1
    assert faulted >= 1 and changed >= 1, (faulted, changed)
    if layout in ("fixed64", "fixed128", "offsets16", "xdp_offsets", "packed"):
        assert compiled >= 6, compiled


@pytest.mark.gpu
def test_tier0_program_unchanged(cuda):
    from ebpf_emu import Program
    from ebpf_emu import workloads as W

    n = 130
    buf = W.frames_fixed(n, 64, 3)
    prog = Program(W.program("5tuple"))
    kw = dict(n=n, stride=64)
    got, fin, kid = _run(prog, buf, kw, cuda, True, fp=True)
    off, _, kid0 = _run(prog, buf, kw, cuda, False, fp=True)
    assert kid == kid0
    _buf_eq(fin, buf, "5tuple")
    _identical_outputs(got, off, "5tuple")
    prog.close()


LOOP_STORE = """
    mov r3, 0
    mov r4, r1
loop:
    jge r3, r2, done
    jge r3, 24, done
    ldxb r5, [r4+0]
    xor r5, 0x5a
    stxb [r4+0], r5
    add r4, 1
    add r3, 1
    ja loop
done:
    mov r0, 2
    exit
"""
PACKET_ATOMIC = """
    jlt r2, 16, out
    mov r3, 7
    lock add [r1+8], r3
    stb [r1+1], 0x11
out:
    mov r0, 3
    exit
"""


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["loop_store", "packet_atomic"])
@pytest.mark.parametrize("layout", ["fixed64", "packed"])
def test_general_interpreter_programs(cuda, oracle_mod, name, layout):
    from ebpf_emu import Program, _lib
    from ebpf_emu.asm import assemble

    img = assemble(LOOP_STORE if name == "loop_store" else PACKET_ATOMIC)
    rng = random.Random(3)
    pkts = _packed_packets(rng, 130)
    buf, kw, spans, xdp, pk = _lay(pkts, layout)
    exp, sts = _expected(oracle_mod, img, buf, spans, False)
    assert _changed(exp, buf, spans) >= 30
    prog = Program(img)
    got, fin, kid = _run(prog, buf, kw, cuda, True, max_steps=STEPS)
    assert kid == _lib.EBPF_KERNEL_GENERAL_T1
    _buf_eq(fin, exp, f"{name} {layout}")
    assert np.array_equal(got["status"], sts)
    prog.close()


XDP_CTX_STORE = """
    ldxw r6, [r1+0]
    ldxw r7, [r1+4]
    stw [r1+0], 0x11223344
    sth [r1+6], 0x5566
    mov r3, r6
    add r3, 4
    jgt r3, r7, out
    stb [r6+0], 0xee
    sth [r6+2], 0xbeef
out:
    mov r0, 2
    exit
"""


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["xdp_offsets", "xdp_fixed64"])
def test_xdp_md_ctx_stores(cuda, oracle_mod, layout):
    import torch

    from ebpf_emu import Program, _lib
    from ebpf_emu.asm import assemble

    img = assemble(XDP_CTX_STORE)
    rng = random.Random(8)
    pkts = _packed_packets(rng, 130)
    lay = "fixed64" if layout == "xdp_fixed64" else layout
    buf, kw, spans, _, pk = _lay(pkts, lay)
    exp, sts = _expected(oracle_mod, img, buf, spans, True)
    assert _changed(exp, buf, spans) >= 60
    prog = Program(img)
    got, fin, kid = _run(prog, buf, kw, cuda, True, True)
    # the compiled write-back variant under xdp_md, in place (the ctx dwords skipped)
    assert kid == (_lib.EBPF_KERNEL_JIT_STACK if lay == "fixed64" else _lib.EBPF_KERNEL_JIT_VARL_STACK), kid
    assert not prog.batch_staged(prog.make_batch(torch.zeros(64, dtype=torch.uint8, device=cuda),
                                                 n=1, stride=64, xdp_md=True, writeback=True))
    _buf_eq(fin, exp, layout)
    assert np.array_equal(got["status"], sts)
    gen, fing, _ = _run(prog, buf, kw, cuda, True, True, generic=True)
    _buf_eq(fing, exp, layout + " generic")
    prog.close()


@pytest.mark.gpu
def test_step_budget_lanes_untouched(cuda, oracle_mod):
    from ebpf_emu import Program
    from ebpf_emu.asm import assemble

    img = assemble(LOOP_STORE)
    pkts = _packed_packets(random.Random(5), 130)
    buf, kw, spans, xdp, pk = _lay(pkts, "packed")
    steps = 60  # (a 24-byte loop needs ~170 steps: the longer packets run out, the short ones finish)
    exp, sts = _expected(oracle_mod, img, buf, spans, False, max_steps=steps)
    assert (sts == 5).sum() >= 10 and (sts == 0).sum() >= 10
    prog = Program(img)
    got, fin, kid = _run(prog, buf, kw, cuda, True, max_steps=steps)
    assert np.array_equal(got["status"], sts)
    _buf_eq(fin, exp, "ST_STEPS")
    for i, (o, ln) in enumerate(spans):
        if sts[i] == 5:
            assert np.array_equal(fin[o:o + ln], buf[o:o + ln])
    prog.close()


@pytest.mark.gpu
def test_writeback_with_mem_output(cuda, oracle_mod):
    import torch

    from ebpf_emu import Program
    from ebpf_emu import workloads as W

    img = W.program("mac_swap_tx")
    rng = random.Random(2)
    pkts = [bytes(rng.getrandbits(8) for _ in range(64)) for _ in range(130)]
    buf, kw, spans, _, _ = _lay(pkts, "fixed64")
    exp, _ = _expected(oracle_mod, img, buf, spans, False)
    prog = Program(img)
    fr = torch.from_numpy(buf.copy()).to(cuda)
    res = prog.run(fr, mem=True, writeback=True, **kw)
    torch.cuda.synchronize()
    _buf_eq(fr.cpu().numpy(), exp, "mem + writeback")
    assert np.array_equal(res.mem.cpu().numpy()[:, :64].reshape(-1), exp)
    with pytest.raises(ValueError):
        prog.run(fr.reshape(130, 64)[:, :32], n=130, stride=32, writeback=True)
    prog.close()


@pytest.mark.gpu
def test_unknown_flag_bit(cuda):
    import ctypes

    import torch

    from ebpf_emu import Program, _lib
    from ebpf_emu import workloads as W

    prog = Program(W.program("nat"))
    fr = torch.zeros(64 * 4, dtype=torch.uint8, device=cuda)
    b = prog.make_batch(fr, n=4, stride=64, writeback=True)
    b.flags |= 16
    o = _lib.BatchOut()
    L = _lib.lib()
    assert L.ebpf_batch_kernel(prog._h, ctypes.byref(b), ctypes.byref(o), 0) == -1
    assert L.ebpf_run_batch(prog._h, ctypes.byref(b), ctypes.byref(o), None) == -1
    prog.close()
