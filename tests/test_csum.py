"""ebpf_csum_verify / ebpf_csum_fill on the GPU against the Python model (tests/csum_ref.py), exactly.
Every status array is pre-filled with a sentinel and compared whole, and `frames` is compared byte
for byte with the model's output, filler between and behind the packets included: verify must
leave it as it was, fill may change the two-byte fields and nothing else. Sizes come from the
kernel's constants (ebpf_emu.csum)."""
import functools

import numpy as np
import pytest

import csum_ref as C

pytestmark = pytest.mark.gpu

SENT8 = 0xA5
WHATS = range(1, 8)
R = C.R


def _run(dev, fill, frames, n, what, verdict=None, queue_mask=0x7F, **kw):
    """One call into a sentinel-filled status -> (status u8[n], frames after the call as numpy, or
    the device tensor when one was passed)."""
    import torch

    from ebpf_emu import csum

    st = torch.full((n + 8,), SENT8, dtype=torch.uint8, device=dev)
    lay = {}
    for name, dt in (("offsets", np.int32), ("lens", np.int16)):
        if name in kw:
            lay[name] = torch.from_numpy(kw[name].view(dt)).to(dev)
    if "stride" in kw:
        lay["stride"] = kw["stride"]
    given = isinstance(frames, torch.Tensor)
    fr = frames if given else torch.from_numpy(frames).to(dev)
    dv = None if verdict is None else torch.from_numpy(np.asarray(verdict, dtype=np.uint8)).to(dev)
    (csum.csum_fill if fill else csum.csum_verify)(fr, what, n=n, verdict=dv, queue_mask=queue_mask,
                                                   status=st[:n], **lay)
    torch.cuda.synchronize()
    got = st.cpu().numpy()
    assert np.all(got[n:] == SENT8), "status written past n"
    return got[:n], fr if given else fr.cpu().numpy()


def _same(got, exp, tag, names=None):
    if not np.array_equal(got, exp):
        d = np.flatnonzero(got != exp)
        raise AssertionError((tag, "first wrong", int(d[0]), names[d[0]] if names else "",
                              "got", [hex(int(x)) for x in got[d[:4]]],
                              "expected", [hex(int(x)) for x in exp[d[:4]]], "wrong", len(d)))


def _frames_same(got, exp, offsets, tag, names=None):
    """Byte for byte; a difference is reported by the packet it lies in or behind."""
    if not np.array_equal(got, exp):
        d = np.flatnonzero(got != exp)
        k = int(np.searchsorted(offsets, d[0], side="right")) - 1
        raise AssertionError((tag, "first wrong byte", int(d[0]), "packet", k, names[k] if names else "",
                              "at", int(d[0] - offsets[k]), "got", hex(int(got[d[0]])),
                              "expected", hex(int(exp[d[0]])), "wrong bytes", len(d)))


def _abutting(pkts, aligns=range(16)):
    """The packets laid end to end with no gap, the whole list once at each start alignment ->
    (buf, offsets u32, lens u16) of len(aligns) * len(pkts) packets."""
    one = b"".join(pkts)
    lens1 = np.array([len(p) for p in pkts], dtype=np.int64)
    offs1 = np.concatenate([[0], np.cumsum(lens1)[:-1]])
    parts, offs, pos = [], [], 0
    for s in aligns:
        pad = (s - pos) % 16
        parts.append(bytes([0xEE]) * pad + one)
        offs.append(offs1 + pos + pad)
        pos += pad + len(one)
    reps = len(list(aligns))
    return (np.frombuffer(b"".join(parts), dtype=np.uint8).copy(),
            np.concatenate(offs).astype(np.uint32), np.tile(lens1, reps).astype(np.uint16))


def _put(buf, offsets, pkts):
    """A copy of buf with the packets written at the offsets (the model's fill, placed)."""
    out = buf.copy()
    for o, p in zip(offsets.tolist(), pkts):
        out[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return out


def _check(dev, pkts, buf, kw, offsets, tag, names=None, reps=1, whats=(C.ALL,), verdict=None,
           queue_mask=0x7F, expect=None):
    """verify, then fill, of one layout of `pkts` (tiled reps times) under every mask of whats,
    against the model (expect: a cache (what, fill) -> model answer). -> {what: the device's verify
    statuses}."""
    import torch

    seen = {}

    n = len(pkts) * reps
    dbuf = torch.from_numpy(buf).to(dev)  # (exactly the packets' bytes: no slack behind the last)
    v1 = None if verdict is None else np.asarray(verdict)[:len(pkts)]
    for what in whats:
        ev = expect(what, False) if expect else C.verify_batch(pkts, what, v1, queue_mask)
        gs, gf = _run(dev, False, dbuf.clone(), n, what, verdict, queue_mask, **kw)
        _same(gs, np.tile(ev, reps), f"{tag} what={what} verify status", names)
        seen[what] = gs
        assert torch.equal(gf, dbuf), f"{tag} what={what}: verify wrote frames"
        ep, es = expect(what, True) if expect else C.fill_batch(pkts, what, v1, queue_mask)
        gs, gf = _run(dev, True, dbuf.clone(), n, what, verdict, queue_mask, **kw)
        _same(gs, np.tile(es, reps), f"{tag} what={what} fill status", names)
        _frames_same(gf.cpu().numpy(), _put(buf, offsets, list(ep) * reps), offsets,
                     f"{tag} what={what} fill frames", names)
    return seen


def test_known_answers(cuda):
    """The two published vectors inside frames: the IPv4 header example verifies GOOD, a wiped field
    is filled back to the published b861; the RFC 1071 bytes as a UDP payload give the field the
    published sum ddf2 determines."""
    v = C.vectors()
    hdr = bytes.fromhex(v["ipv4_header"]["bytes"])
    good = R.eth(0x0800) + hdr + bytes(0x73 - 20)
    wiped = C.set_be16(good, 14 + 10, 0x1234)
    pay = bytes.fromhex(v["rfc1071"]["bytes"])
    udp = C.frame4(17, C.udp(53, 60000, pay), valid_sums=False)
    pkts = [good, wiped, udp]
    buf = np.zeros((3, 160), dtype=np.uint8)
    for i, p in enumerate(pkts):
        buf[i, :len(p)] = np.frombuffer(p, dtype=np.uint8)
    lens = np.array([len(p) for p in pkts], dtype=np.uint16)
    st, fr = _run(cuda, False, buf.reshape(-1), 3, C.IPV4_HDR, stride=160, lens=lens)
    assert st.tolist() == [C.L3_GOOD, C.L3_BAD, C.L3_BAD] and np.array_equal(fr, buf.reshape(-1))
    st, fr = _run(cuda, True, buf.reshape(-1), 3, C.IPV4_HDR | C.UDP, stride=160, lens=lens)
    fr = fr.reshape(3, 160)
    assert st.tolist() == [C.L3_GOOD, C.L3_GOOD, C.L3_GOOD | C.L4_GOOD]
    assert fr[0, 24:26].tobytes().hex() == fr[1, 24:26].tobytes().hex() == v["ipv4_header"]["field"]
    assert np.array_equal(fr[1], buf[0])
    words = [0x0A01, 0x0203, 0xC0A8, 0x4D09, 17, 16, 53, 60000, 16, int(v["rfc1071"]["sum"], 16)]
    assert fr[2, 40:42].tobytes().hex() == f"{~C.fold(sum(words)) & 0xFFFF:04x}"
    st, _ = _run(cuda, False, fr.reshape(-1).copy(), 3, C.ALL, stride=160, lens=lens)
    assert st.tolist() == [C.L3_GOOD, C.L3_GOOD, C.L3_GOOD | C.L4_GOOD]


@functools.lru_cache(maxsize=None)
def _matrix():
    """Every parser kind truncated at every length 0..full: [(name, full frame, length)]."""
    out = []
    for name, frame in C.parser_kinds().items():
        out += [(f"{name}[:{ln}]", frame, ln) for ln in range(len(frame) + 1)]
    return out


def _slot(frame, ln):
    """A 128-byte slot with no length of its own: the truncated frame, then a filler."""
    s = np.full(128, 0xEE, dtype=np.uint8)
    s[:ln] = np.frombuffer(frame[:ln], dtype=np.uint8)
    return s.tobytes()


@functools.lru_cache(maxsize=None)
def _matrix_expected(layout, what, fill):
    """The model's answers for a layout of the matrix, computed once per mask."""
    pkts = [_slot(f, ln) if layout == "slots" else f[:ln] for _, f, ln in _matrix()]
    return C.fill_batch(pkts, what) if fill else C.verify_batch(pkts, what)


@pytest.mark.parametrize("layout", ["slots", "slots+lens", "abutting"])
def test_parser_matrix(cuda, layout):
    """slots: 128-byte fixed slots without lens (the packet IS the slot: the truncated frame plus
    a filler, which is Ethernet padding wherever the datagram still fits). slots+lens: the length
    truncates, and the bytes behind the packet continue the untruncated frame, so a read past len
    changes the answer and a write past it shows. abutting: offsets + lens, packet after packet with
    no gap, the whole matrix once at every start alignment 0..15. Every what mask, verify and fill."""
    mat = _matrix()
    names = [m[0] for m in mat]
    n = len(mat)
    cut = [f[:ln] for _, f, ln in mat]
    reps = 1
    if layout == "slots":
        pkts = [_slot(f, ln) for _, f, ln in mat]
        buf = np.frombuffer(b"".join(pkts), dtype=np.uint8).copy()
        kw = dict(stride=128)
        offsets = np.arange(n, dtype=np.int64) * 128
    elif layout == "slots+lens":
        pkts = cut
        buf = np.zeros((n, 128), dtype=np.uint8)
        for i, (_, f, _) in enumerate(mat):
            buf[i, :len(f)] = np.frombuffer(f, dtype=np.uint8)
        buf = buf.reshape(-1)
        kw = dict(stride=128, lens=np.array([ln for _, _, ln in mat], dtype=np.uint16))
        offsets = np.arange(n, dtype=np.int64) * 128
    else:
        pkts = cut
        buf, offs, lens = _abutting(cut)
        kw = dict(offsets=offs, lens=lens)
        offsets = offs.astype(np.int64)
        reps = 16
        starts = offs.reshape(16, n) % 16
        assert all(len(set(starts[:, j].tolist())) == 16 for j in (0, n // 2, n - 1))
        names = names * 16
    key = "slots" if layout == "slots" else "cut"
    got = _check(cuda, pkts, buf, kw, offsets, layout, names, reps, WHATS,
                 expect=lambda what, fill: _matrix_expected(key, what, fill))
    if layout != "slots":  # the device's own answers reach every value of the status byte
        assert set(got[C.ALL].tolist()) == {0, 1, 2, 4, 8, 5, 9, 17, 6, 10, 18}


def _edge_frame(kind, L, fillbyte, seed):
    """Ethernet + IP + an L4 segment of exactly L bytes (below the L4 header's size: what there is
    of it), valid checksums; payload bytes random or all fillbyte."""
    pay = C.body(max(L, 20), seed) if fillbyte is None else bytes([fillbyte]) * max(L, 20)
    if kind == "tcp4":
        return C.frame4(6, (C.tcp(80, 4000 + L) + pay)[:L])
    if kind == "udp4":
        return C.frame4(17, (C.udp(53, 4000 + L, length=L) + pay)[:L], tags=(0x8100,))
    return C.frame6(17, (C.udp(53, 4000 + L, length=L) + pay)[:L])


@functools.lru_cache(maxsize=None)
def _edge_packets():
    lengths = list(range(0, 81)) + list(range(1440, 1501))
    pk, names = [], []
    for kind, fb in (("udp4", None), ("tcp4", None), ("udp6", None), ("udp4", 0xFF), ("tcp4", 0x00)):
        for L in lengths:
            f = _edge_frame(kind, L, fb, L)
            if L % 3 == 1:  # a third of them wrong: GOOD must not be the only answer asked for
                f = C.flip(f, -1 - (L % 7 if L > 8 else 0))
            pk.append(f)
            names.append(f"{kind} L={L} fill={fb}")
    return pk, names


def test_sum_edges(cuda):
    """L4 lengths 0..80 and 1440..1500 at all 16 start alignments (odd and even span starts, spans
    inside one 16-byte block, tails of 1..15 bytes), payloads random, all 0xFF and all 0x00; a wave
    of 64 packets whose lengths are drawn from 0..1500, so one block list mixes owners."""
    pk, names = _edge_packets()
    buf, offs, lens = _abutting(pk)
    ev = C.verify_batch(pk, C.ALL)
    ef = C.fill_batch(pk, C.ALL)
    assert {5, 9} <= set(ev.tolist()) and {4, 8} <= set(ev.tolist())
    _check(cuda, pk, buf, dict(offsets=offs, lens=lens), offs.astype(np.int64), "edges", names * 16, 16,
           expect=lambda what, fill: ef if fill else ev)
    rng = np.random.default_rng(7)
    wave = []
    for i, L in enumerate(rng.integers(0, 1501, 64).tolist()):
        L = min(L, 1500 - 14 - 40)
        f = _edge_frame(("udp4", "tcp4", "udp6")[i % 3], L, None, i)
        wave.append(C.flip(f, -1) if i % 4 == 0 else f)
    for s in (0, 5):
        buf, offs, lens = _abutting(wave, aligns=(s,))
        _check(cuda, wave, buf, dict(offsets=offs, lens=lens), offs.astype(np.int64), f"wave@{s}")


def test_longest_packet(cuda):
    """65535-byte packets whose L4 bytes are all 0xFF: the accumulator's worst case (4095 blocks of
    eight 0xFFFF words in one slot), over IPv4 and over IPv6, at an even and an odd start."""
    seg4, seg6 = bytes([0xFF]) * (65535 - 34), bytes([0xFF]) * (65535 - 54)
    p4 = R.eth(0x0800) + R.ipv4("10.1.2.3", "192.168.77.9", 6, seg4)
    p6 = R.eth(0x86DD) + R.ipv6("2001:db8::1:2", "2001:db8:ffff::9", 6, seg6)
    assert len(p4) == len(p6) == 65535
    pkts = [p4, p6, C.valid(p4), C.valid(p6)]
    buf, offs, lens = _abutting(pkts, aligns=(0,))
    assert set((offs % 2).tolist()) == {0, 1}
    ev = C.verify_batch(pkts, C.ALL)
    assert ev.tolist() == [C.L3_BAD | C.L4_BAD, C.L4_BAD, C.L3_GOOD | C.L4_GOOD, C.L4_GOOD]
    _check(cuda, pkts, buf, dict(offsets=offs, lens=lens), offs.astype(np.int64), "65535")


def test_selection(cuda):
    """A verdict array holding every class (bytes 5..0xFD are class 5, 0xFF class 6) under several
    masks: unselected packets get status 0 and fill leaves their bytes as they were."""
    kinds = C.parser_kinds()
    base = [kinds[k] for k in ("bad_both", "untagged", "bad_udp_payload", "v6udp", "bad_v6tcp", "udp_none",
                               "bad_l3", "arp", "udp_sum0", "ihl15", "bad_opts", "padded", "tcp_l20")]
    classes = [0, 1, 2, 3, 4, 5, 6, 0x7F, 0xFD, 0xFE, 0xFF]
    pkts = [base[i % len(base)] for i in range(len(base) * len(classes))]
    verdict = np.array([classes[i % len(classes)] for i in range(len(pkts))], dtype=np.uint8)
    buf, offs, lens = _abutting(pkts, aligns=(3,))
    for mask in (0, 0x7F, 1 << 3, (1 << 5) | (1 << 6), 0x2A, 1 << 0):
        _check(cuda, pkts, buf, dict(offsets=offs, lens=lens), offs.astype(np.int64), f"mask={mask:#x}",
               verdict=verdict, queue_mask=mask)
    ev = C.verify_batch(pkts, C.ALL, verdict, 1 << 5)
    assert np.all(ev[(verdict < 5) | (verdict == 0xFF)] == 0) and np.any(ev != 0)


def _distinct_packets(count):
    """`count` distinct 64-byte packets of every family, a third with a wrong checksum; the bytes
    behind a datagram are padding."""
    rng = np.random.default_rng(43)
    pk = []
    for i in range(count):
        sp, dp = (int(x) for x in rng.integers(1, 65536, 2))
        pay = bytes(rng.integers(0, 256, 24, dtype=np.uint8))
        kind = i % 7
        if kind == 0:
            f = C.frame4(6, C.tcp(sp, dp, pay[:i % 11]))
        elif kind == 1:
            f = C.frame4(17, C.udp(sp, dp, pay[:i % 23]))
        elif kind == 2:
            f = C.frame4(17, C.udp(sp, dp, pay[:i % 19]), ihl=6)
        elif kind == 3:
            f = C.frame6(17, C.udp(sp, dp, pay[:i % 3]))
        elif kind == 4:
            f = C.frame4(17, C.udp(sp, dp, pay[:i % 13]), tags=(0x8100,))
        elif kind == 5:
            f = C.frame4(1, pay[:8 + i % 9])
        else:
            f = R.eth(0x0806) + pay
        if i % 3 == 0 and len(f) > 24:
            f = C.flip(f, 23 + (i % (len(f) - 23)), 1 << (i % 8))
        assert len(f) <= 64
        pk.append(f + bytes(rng.integers(0, 256, 64 - len(f), dtype=np.uint8)))
    return pk


def test_sizes(cuda):
    """n around a wave, a workgroup's pass and one packet past a full pass of the capped grid: a
    few hundred distinct 64-byte packets tiled on the device, compared there."""
    import torch

    from ebpf_emu import csum

    pk = _distinct_packets(300)
    ev = C.verify_batch(pk, C.ALL)
    ep, es = C.fill_batch(pk, C.ALL)
    assert {0, 1, 2, 4, 8, 5, 6, 9, 10} <= set(ev.tolist())
    dbase = torch.from_numpy(np.frombuffer(b"".join(pk), dtype=np.uint8).reshape(300, 64).copy()).to(cuda)
    dfill = torch.from_numpy(np.frombuffer(b"".join(ep), dtype=np.uint8).reshape(300, 64).copy()).to(cuda)
    blk = csum.CSUM_BLOCK
    for n in (0, 1, 63, 64, 65, blk - 1, blk, blk + 1, blk * csum.CSUM_MAX_WGS + 1):
        sel = torch.arange(n, device=cuda) % 300
        src = dbase[sel].reshape(-1) if n else dbase.reshape(-1).clone()
        tile = np.arange(n) % 300
        gs, gf = _run(cuda, False, src.clone(), n, C.ALL, stride=64)
        _same(gs, ev[tile], f"n={n} verify status")
        assert torch.equal(gf, src), f"n={n}: verify wrote frames"
        gs, gf = _run(cuda, True, src.clone(), n, C.ALL, stride=64)
        _same(gs, es[tile], f"n={n} fill status")
        assert torch.equal(gf, dfill[sel].reshape(-1) if n else src), f"n={n}: fill frames"


def test_nat_end_to_end(cuda):
    """Frames with valid checksums through the `nat` workload with write-back: every IPv4 header
    still verifies (the program's RFC 1624 step, checked independently), the L4 checksum is BAD
    exactly on the XDP_TX verdicts (the rewritten ports); a fill of the TX queue alone makes every
    packet good again and leaves the PASS / DROP packets byte-identical."""
    import torch

    from ebpf_emu import Program
    from ebpf_emu import workloads as W

    rng = np.random.default_rng(5)
    n, S = 700, 128
    buf = rng.integers(0, 256, (n, S), dtype=np.uint8)
    for i in range(n):
        dp = (53, 80, int(rng.integers(1, 65536)))[i % 3]
        pay = bytes(rng.integers(0, 256, int(rng.integers(0, 30)), dtype=np.uint8))
        seg = C.tcp(1000 + i, dp, pay) if i % 2 else C.udp(1000 + i, dp, pay)
        f = bytearray(R.eth(0x0800) + R.ipv4(f"10.{i % 256}.2.3", "192.168.77.9", 6 if i % 2 else 17, seg,
                                             ihl=5 + (i % 5 == 0)))
        f[22] = (1, 2, 64, 255)[i % 4] if i % 7 == 0 else 64  # TTL 1: DROP
        f = C.valid(bytes(f))
        buf[i, :len(f)] = np.frombuffer(f, dtype=np.uint8)
    fr = torch.from_numpy(buf.reshape(-1)).to(cuda)
    st0, _ = _run(cuda, False, fr, n, C.ALL, stride=S)
    assert np.all(st0 == C.L3_GOOD | C.L4_GOOD)
    res = Program(W.program("nat")).run(fr, n=n, stride=S, writeback=True)
    torch.cuda.synchronize()
    v = res.verdict.cpu().numpy()
    assert {1, 2, 3} == set(v.tolist())
    after = fr.cpu().numpy().reshape(n, S)
    assert np.any(after != buf)
    st1, _ = _run(cuda, False, fr, n, C.ALL, stride=S)
    _same(st1, C.verify_batch([r.tobytes() for r in after], C.ALL), "after nat, against the model")
    assert np.all(st1 & C.L3_GOOD) and not np.any(st1 & C.L3_BAD)
    assert np.array_equal((st1 & C.L4_BAD) != 0, v == 3)
    assert np.all((st1 & (C.L4_GOOD | C.L4_BAD)) != 0) and not np.any(st1 & C.L4_NONE)
    st2, _ = _run(cuda, True, fr, n, C.TCP | C.UDP, verdict=v, queue_mask=1 << 3, stride=S)
    assert np.array_equal(st2, np.where(v == 3, C.L4_GOOD, 0))
    fixed = fr.cpu().numpy().reshape(n, S)
    assert np.array_equal(fixed[v != 3], after[v != 3])
    exp, _ = C.fill_batch([r.tobytes() for r in after], C.TCP | C.UDP, v, 1 << 3)
    assert fixed.tobytes() == b"".join(exp)
    st3, _ = _run(cuda, False, fr, n, C.ALL, stride=S)
    assert np.all(st3 == C.L3_GOOD | C.L4_GOOD)


def test_pcap_csum_tool(cuda, tmp_path, capsys):
    """tools/pcap_csum.py over a capture of the parser kinds: the report's counts are the model's,
    and --fix writes the capture back with every packet the model's fill of it, the global header
    and every record header byte-identical; the fixed capture then reports nothing BAD or NONE."""
    import importlib.util
    import os
    import re

    from ebpf_emu import pcap

    pkts = list(C.parser_kinds().values())
    src, dst = tmp_path / "in.pcap", tmp_path / "out.pcap"
    src.write_bytes(pcap.to_bytes(pkts))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("pcap_csum", os.path.join(root, "tools", "pcap_csum.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)

    def counts(line):
        return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", line)}

    def model_counts(ps, what):
        st = C.verify_batch(ps, what)
        out = {"unchecked": int((st == 0).sum())}
        for name, bit in (("L3_GOOD", 1), ("L3_BAD", 2), ("L4_GOOD", 4), ("L4_BAD", 8), ("L4_NONE", 16)):
            out[name] = int(((st & bit) != 0).sum())
        return out

    tool.main([str(src)])
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1 and f"{len(pkts)} packets" in lines[0]
    assert counts(lines[0]) == model_counts(pkts, C.ALL)
    assert not dst.exists()
    tool.main([str(src), "--what", "ipv4,udp", "--fix", str(dst)])
    lines = capsys.readouterr().out.strip().splitlines()
    what = C.IPV4_HDR | C.UDP
    fixed = [C.fill(p, what)[0] for p in pkts]
    assert counts(lines[0]) == model_counts(pkts, what)
    assert counts(lines[1]) == model_counts(fixed, what)
    assert counts(lines[1])["L3_BAD"] == counts(lines[1])["L4_BAD"] == counts(lines[1])["L4_NONE"] == 0
    a, b = src.read_bytes(), dst.read_bytes()
    assert len(a) == len(b) and a[:24] == b[:24] and a != b
    offs, lens, _ = pcap.index(np.frombuffer(b, dtype=np.uint8))
    assert len(offs) == len(pkts)
    for o, ln, p, q in zip(offs.tolist(), lens.tolist(), pkts, fixed):
        assert b[o:o + ln] == q and b[o - 16:o] == a[o - 16:o] and ln == len(p)
