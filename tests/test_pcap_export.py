"""ebpf_pcap_gather on the GPU against the numpy model (tests/pcap_export_ref.py), exactly: the
output buffer, out_offsets, out_lens and out_total are pre-filled with sentinels and compared
WHOLE, slack past their ends included, so every byte and entry the header promises to leave
untouched is checked too. Sizes come from the kernel's constants (ebpf_emu.queues). The last test
is the chain the call exists for, checked against the oracle alone: a capture in place -> 5-tuple
-> PASS queue -> NAT with write-back -> a capture of the passed packets again."""
import random

import numpy as np
import pytest

import pcap_export_ref as R
import queues_ref as QR

pytestmark = pytest.mark.gpu

SENT = 0xA5
SLACK = 48  # bytes / entries past every array's end: untouched
LENS = [0, 1, 15, 16, 17, 31, 33, 63, 64, 65, 1500]
HDR = bytes(range(0x40, 0x58))  # any 24 bytes: the kernel writes them verbatim


def _first_diff(got, exp, tag):
    if not np.array_equal(got, exp):
        d = np.flatnonzero(got != exp)
        raise AssertionError((tag, "first wrong position", int(d[0]), "got", got[d[:4]].tolist(),
                              "expected", exp[d[:4]].tolist(), "wrong", len(d)))


def _u32(a, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(dev)


def _u16(a, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(dev)


def _lens_mix(rng, n):
    return np.array([LENS[rng.randrange(len(LENS))] for _ in range(n)], dtype=np.uint16)


def _layout(kind, lens, rng):
    """The source batch of len(lens) packets -> (frames u8 numpy, layout kwargs as numpy)."""
    n = len(lens)
    nr = np.random.default_rng(rng.randrange(1 << 30))
    if kind == "fixed64":  # no lens: every packet is its 64-byte slot
        return nr.integers(0, 256, n * 64, dtype=np.uint8), dict(stride=64)
    if kind == "stride_lens":
        return nr.integers(0, 256, n * 1520, dtype=np.uint8), dict(stride=1520, lens=lens)
    offs, pos = [], 0
    for i in range(n):
        if kind == "residues":  # every residue mod 16, with gaps
            pos += (i % 16 - pos) % 16 if i % 3 else (i * 7) % 16
        else:
            assert kind == "abut"  # no gap: the source tensor is exactly the packets' size
        offs.append(pos)
        pos += int(lens[i])
    offs = np.array(offs, dtype=np.uint32)
    if kind == "residues" and n >= 64:
        assert len(set((offs % 16).tolist())) == 16
    return nr.integers(0, 256, max(pos, 1), dtype=np.uint8), dict(offsets=offs, lens=lens)


def _verdicts(n, queue_size, queue=2, seed=0):
    """n verdict bytes with exactly queue_size of `queue`, spread; the rest DROP / TX / fault."""
    rng = np.random.default_rng(100 + seed)
    v = rng.choice(np.array([1, 3, 0xFF], dtype=np.uint8), n)
    v[rng.permutation(n)[:queue_size]] = queue
    return v


def _check(dev, tag, frames, index, count, queue, n, kw, *, hdr=HDR, flags=0, snaplen=0, ts=None,
           out_bytes=None, exact=False, with_index=True, dev_index=None, dev_count=None):
    """One pcap_gather into sentinel-filled device arrays against the model. out_bytes: None =
    room for the whole batch; exact: the output tensor is out_bytes long and not one byte more
    (else a view of a longer, sentinel-filled one). -> (records, end, data) of the model."""
    import torch

    from ebpf_emu import queues as Q

    if out_bytes is None:
        out_bytes = Q.pcap_out_bytes(len(frames), n, kw.get("stride", 0), "lens" in kw)
    w, end, oo, ol, data = R.pcap_gather(frames, index, count, queue, n, hdr, flags=flags,
                                         snaplen=snaplen, ts=ts, out_bytes=out_bytes, **kw)
    size = out_bytes if exact else out_bytes + SLACK
    e_out = np.full(size, SENT, dtype=np.uint8)
    e_out[:end] = np.frombuffer(data, dtype=np.uint8)
    e_offs = np.full(n + SLACK, 0xA5A5A5A5, dtype=np.uint32)
    e_lens = np.full(n + SLACK, 0xA5A5, dtype=np.uint16)
    e_offs[:w], e_lens[:w] = oo, ol
    e_tot = np.full(2 + SLACK, 0xA5A5A5A5, dtype=np.uint32)
    e_tot[:2] = (w, end)
    # ---- the device
    d_out = torch.full((size,), SENT, dtype=torch.uint8, device=dev)
    d_offs = torch.full((n + SLACK,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device=dev)
    d_lens = torch.full((n + SLACK,), 0xA5A5 - (1 << 16), dtype=torch.int16, device=dev)
    d_tot = torch.full((2 + SLACK,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device=dev)
    dkw = {k: v for k, v in kw.items() if k == "stride"}
    if "offsets" in kw:
        dkw["offsets"] = _u32(kw["offsets"], dev)
    if "lens" in kw:
        dkw["lens"] = _u16(kw["lens"], dev)
    d_frames = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    assert d_frames.numel() == len(frames)
    extra = dict(out_offsets=d_offs[:n], out_lens=d_lens[:n]) if with_index else {}
    res = Q.pcap_gather(d_frames, dev_index if dev_index is not None else _u32(index, dev),
                        dev_count if dev_count is not None else _u32(count, dev), queue, hdr,
                        flags=flags, snaplen=snaplen, n=n,
                        ts=_u32(ts, dev) if ts is not None else None,
                        out=d_out[:out_bytes], total=d_tot[:2], **extra, **dkw)
    torch.cuda.synchronize()
    assert len(res) == (4 if with_index else 2)
    _first_diff(d_tot.cpu().numpy().view(np.uint32), e_tot, tag + " total")
    _first_diff(d_out.cpu().numpy(), e_out, tag + " out")
    if not with_index:
        e_offs[:], e_lens[:] = 0xA5A5A5A5, 0xA5A5
    _first_diff(d_offs.cpu().numpy().view(np.uint32), e_offs, tag + " out_offsets")
    _first_diff(d_lens.cpu().numpy().view(np.uint16), e_lens, tag + " out_lens")
    return w, end, data


def _tile():
    from ebpf_emu import queues as Q

    return Q.GATHER_TILE


def test_queue_sizes_around_the_tile(cuda):
    """Queue sizes 0, 1, 63, 64, 65, 255, 256, 257, 1025, mixed lengths, abutting packets; ts
    given and NULL."""
    assert _tile() == 256
    rng = random.Random(1)
    for m in (0, 1, 63, 64, 65, 255, 256, 257, 1025):
        n = m + m // 3 + 5
        v = _verdicts(n, m, seed=m)
        index, count = QR.queues(v)
        lens = _lens_mix(rng, n)
        frames, kw = _layout("abut", lens, rng)
        ts = np.random.default_rng(m).integers(0, 1 << 32, (n, 2), dtype=np.uint64).astype(np.uint32)
        for t in (None, ts):
            w, end, _ = _check(cuda, f"sizes m={m} ts={t is not None}", frames, index, count, 2, n,
                               kw, ts=t)
            assert w == m and end == 24 + 16 * m + int(lens[QR.queue_of(index, count, 2)].sum())


def test_past_the_grid_cap(cuda):
    """More queue positions than one pass of the capped grid: 262,437 packets of 64 bytes."""
    from ebpf_emu import queues as Q

    n = Q.GATHER_TILE * Q.GATHER_MAX_WGS + Q.GATHER_TILE + 37
    assert n == 262437
    v = np.full(n, 2, dtype=np.uint8)
    v[::1001] = 1
    index, count = QR.queues(v)
    m = int(count[2])
    frames, kw = _layout("fixed64", np.zeros(n, np.uint16), random.Random(2))
    w, end, _ = _check(cuda, "past the cap", frames, index, count, 2, n, kw)
    assert w == m > Q.GATHER_TILE * Q.GATHER_MAX_WGS and end == 24 + 80 * m


@pytest.mark.parametrize("layout", ["fixed64", "abut", "residues", "stride_lens"])
def test_layouts_headers_and_snaplens(cuda, layout):
    """Every source layout; lengths 0..1500 mixed and one 65,535-byte packet; snaplen 0, 1, 60 and
    above every length (orig_len kept: the model's headers are compared byte for byte); the
    synthesised header little-endian and SWAPPED, with ts and without."""
    rng = random.Random(len(layout))
    n = 700
    lens = _lens_mix(rng, n)
    if layout in ("abut", "residues"):
        lens[333] = 65535
    frames, kw = _layout(layout, lens, rng)
    v = _verdicts(n, 520, seed=len(layout))
    v[333] = 2
    index, count = QR.queues(v)
    m = int(count[2])
    ts = np.random.default_rng(3).integers(0, 1 << 32, (n, 2), dtype=np.uint64).astype(np.uint32)
    for snaplen in (0, 1, 60, 70000):
        for flags, t in ((0, None), (R.SWAPPED, ts), (0, ts), (R.SWAPPED, None)):
            if snaplen not in (0, 60) and flags:
                continue
            w, end, data = _check(cuda, f"{layout} snap={snaplen} f={flags} ts={t is not None}",
                                  frames, index, count, 2, n, kw, flags=flags, snaplen=snaplen, ts=t)
            assert w == m
            if snaplen == 60 and t is None:  # not vacuous: cut and uncut records, orig_len kept
                magic = b"\xa1\xb2\xc3\xd4" if flags else b"\xd4\xc3\xb2\xa1"
                recs = R.parse(magic + data[4:])[3]
                mine = QR.queue_of(index, count, 2)
                assert [r[0] for r in recs] == mine.tolist()
                want = [int(kw["lens"][i]) if "lens" in kw else 64 for i in mine]
                assert [r[3] for r in recs] == want and [r[2] for r in recs] == [min(x, 60) for x in want]
                assert any(r[2] < r[3] for r in recs) and (layout == "fixed64" or any(r[2] == r[3] for r in recs))


@pytest.mark.parametrize("big_endian", [False, True])
def test_capture_in_place(cuda, big_endian):
    """The source is a capture as it lies in memory (ebpf_pcap_index), either byte order: with
    SRC_RECORDS its record headers survive verbatim (nanosecond timestamps made distinct first);
    with the whole batch in one queue the output IS the source capture; without the flag the
    headers are synthesised; with a snaplen only incl_len changes. A packet at offset < 16 under
    the flag (the batch based 32 bytes into the capture: packet 0 at offset 8) gets the
    synthesised header and nothing before `frames` is read."""
    import struct

    from ebpf_emu import pcap

    rng = random.Random(4)
    n = 300
    pkts = [bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 16, 48, 61, 64, 128, 1504])))
            for _ in range(n)]
    cap = np.frombuffer(pcap.to_bytes(pkts, nanos=True, big_endian=big_endian), dtype=np.uint8).copy()
    offs, lens, _ = pcap.index(cap)
    e = ">" if big_endian else "<"
    for i, o in enumerate(offs):  # real-looking timestamps, and orig_len above incl_len for some
        cap[int(o) - 16:int(o) - 8] = np.frombuffer(
            struct.pack(e + "II", 1700000000 + i // 7, (i * 123456789) % 1000000000), dtype=np.uint8)
        if i % 5 == 0:
            cap[int(o) - 4:int(o)] = np.frombuffer(struct.pack(e + "I", len(pkts[i]) + 100), dtype=np.uint8)
    swapped = R.SWAPPED if big_endian else 0
    assert pcap.header_flag(cap[:24]) == swapped
    kw = dict(offsets=offs, lens=lens)
    hdr = cap[:24].tobytes()
    one = np.zeros(7, dtype=np.uint32)
    one[0] = n
    w, end, data = _check(cuda, "whole capture", cap, np.arange(n, dtype=np.uint32), one, 0, n, kw,
                          hdr=hdr, flags=R.SRC_RECORDS | swapped, out_bytes=len(cap), exact=True)
    assert w == n and data == cap.tobytes()
    v = _verdicts(n, 200, seed=4)
    index, count = QR.queues(v)
    for flags in (R.SRC_RECORDS | swapped, swapped):
        for snaplen in (0, 60):
            w, end, data = _check(cuda, f"pcap flags={flags} snap={snaplen}", cap, index, count, 2,
                                  n, kw, hdr=hdr, flags=flags, snaplen=snaplen)
            assert w == 200
            recs = R.parse(data)[3]
            mine = QR.queue_of(index, count, 2)
            if flags & R.SRC_RECORDS:
                assert [r[0] for r in recs] == [1700000000 + int(i) // 7 for i in mine]
                assert [r[3] for r in recs] == [len(pkts[i]) + (100 if i % 5 == 0 else 0) for i in mine]
            else:
                assert [(r[0], r[3]) for r in recs] == [(int(i), len(pkts[i])) for i in mine]
    # the batch based 32 bytes into the capture: packet 0 lies at offset 8 < 16
    sub = cap[32:]
    v0 = v.copy()
    v0[0] = 2
    index0, count0 = QR.queues(v0)
    w, end, data = _check(cuda, "offset below 16", sub, index0, count0, 2, n,
                          dict(offsets=offs - np.uint32(32), lens=lens), hdr=hdr,
                          flags=R.SRC_RECORDS | swapped)
    recs = R.parse(data)[3]
    assert recs[0][:4] == (0, 0, len(pkts[0]), len(pkts[0])) and recs[1][0] >= 1700000000


def test_capacity(cuda):
    """out_bytes of 0, 23, 24, one byte short of a record's end, exactly a record's end, and an
    output tensor of exactly the needed size; the written records are a prefix."""
    rng = random.Random(5)
    n = 900
    lens = _lens_mix(rng, n)
    frames, kw = _layout("residues", lens, rng)
    v = _verdicts(n, 700, seed=5)
    index, count = QR.queues(v)
    mine = QR.queue_of(index, count, 2)
    ends = 24 + np.cumsum(16 + lens[mine].astype(np.int64))
    full = int(ends[-1])
    for out_bytes, want in ((0, (0, 0)), (23, (0, 0)), (24, (0, 24)), (39, (0, 24)),
                            (int(ends[0]) - 1, (0, 24)), (int(ends[0]), (1, int(ends[0]))),
                            (int(ends[255]), (256, int(ends[255]))),
                            (int(ends[256]) - 1, (256, int(ends[255]))),
                            (int(ends[300]) - 1, (300, int(ends[299]))),
                            (int(ends[511]), (512, int(ends[511]))),
                            (full - 1, (699, int(ends[698]))), (full, (700, full))):
        for exact in (False, True):
            w, end, _ = _check(cuda, f"capacity {out_bytes} exact={exact}", frames, index, count, 2,
                               n, kw, out_bytes=out_bytes, exact=exact)
            assert (w, end) == want, (out_bytes, w, end, want)
    # out_offsets / out_lens are optional
    _check(cuda, "no index arrays", frames, index, count, 2, n, kw, with_index=False)


def test_queues_first_last_and_empty(cuda):
    """Queue 0, the last non-empty queue, and empty queues (the global header and {0, 24})."""
    rng = random.Random(6)
    n = 900
    v = np.random.default_rng(6).choice(np.array([0, 1, 2, 0xFE], dtype=np.uint8), n)  # no TX, no fault
    index, count = QR.queues(v)
    lens = _lens_mix(rng, n)
    frames, kw = _layout("abut", lens, rng)
    for queue in (0, 2, 5, 3, 4, 6):
        m = int(count[queue])
        assert (m == 0) == (queue in (3, 4, 6))
        w, end, _ = _check(cuda, f"queue {queue}", frames, index, count, queue, n, kw)
        assert w == m and (m or end == 24)


def test_wrong_index_produces_no_record(cuda):
    """Two entries outside the batch (n and 0xFFFFFFF0): no record, no byte; the records after
    them move up, in out_offsets / out_lens too."""
    rng = random.Random(7)
    n = 600
    v = _verdicts(n, 400, seed=7)
    index, count = QR.queues(v)
    lens = _lens_mix(rng, n)
    frames, kw = _layout("residues", lens, rng)
    start = int(count[:2].sum())
    index = index.copy()
    index[start + 5] = n            # the first number outside the batch
    index[start + 300] = 0xFFFFFFF0
    for flags in (0, R.SRC_RECORDS):
        w, end, data = _check(cuda, f"wrong entries f={flags}", frames, index, count, 2, n, kw,
                              flags=flags)
        assert w == 398
    # ... and a queue of nothing but such entries writes the global header alone
    index[start:start + 400] = n
    w, end, _ = _check(cuda, "all wrong", frames, index, count, 2, n, kw)
    assert (w, end) == (0, 24)


def test_verdict_pointer_at_1_mod_4_upstream(cuda):
    """The queues come from ebpf_verdict_queues on the device, its verdict pointer at 1 mod 4."""
    import torch

    from ebpf_emu import queues as Q

    rng = random.Random(8)
    n = 1300
    v = _verdicts(n, 800, seed=8)
    buf = torch.zeros(n + 8, dtype=torch.uint8, device=cuda)
    view = buf[1:1 + n]
    assert view.data_ptr() % 4 == 1
    view.copy_(torch.from_numpy(v).to(cuda))
    d_index, d_count = Q.verdict_queues(view)
    index, count = QR.queues(v)
    lens = _lens_mix(rng, n)
    frames, kw = _layout("abut", lens, rng)
    w, _, _ = _check(cuda, "upstream", frames, index, count, 2, n, kw, dev_index=d_index,
                     dev_count=d_count)
    assert w == 800


# ---------------------------------------------------------------- composition
_ORACLE = {}


def _oracle_chain(oracle_mod):
    """The chain by the oracle alone, on the CPU, once -> (capture bytes, the expected records
    [(source record number, NAT's final bytes)])."""
    if _ORACLE:
        return _ORACLE["chain"]
    from ebpf_emu import pcap
    from ebpf_emu import workloads as W
    from test_scatter import _two_stage_packets
    from test_writeback import _expected

    n = 600
    pkts = _two_stage_packets(random.Random(39), n)
    cap = np.frombuffer(pcap.to_bytes(pkts), dtype=np.uint8).copy()
    offs, lens, _ = pcap.index(cap)
    spans = [(int(o), int(ln)) for o, ln in zip(offs, lens)]
    r1, s1, _ = oracle_mod.Program(W.program("5tuple")).run_batch(cap, n, offsets=offs, lens=lens)
    passed = (s1 == 0) & (r1 == 2)
    nat_buf, _ = _expected(oracle_mod, W.program("nat"), cap, spans, False)  # (NAT over every packet)
    want = [(i, nat_buf[o:o + ln].tobytes()) for i, (o, ln) in enumerate(spans) if passed[i]]
    changed = sum(1 for i, b in want if b != pkts[i])
    # the test is not vacuous, by the oracle alone
    assert passed.sum() >= n // 8 and (~passed).sum() >= n // 8, (passed.sum(), n)
    assert changed >= n // 8, changed
    assert (int(passed.sum()), int((~passed).sum())) == (379, 221)
    _ORACLE["chain"] = (cap, want)
    return _ORACLE["chain"]


def _assert_records(data, cap, want, tag):
    big, nanos, linktype, recs = R.parse(data)
    assert bytes(data[:24]) == cap[:24].tobytes(), tag
    assert len(recs) == len(want), (tag, len(recs), len(want))
    for (ts, frac, incl, orig, body), (i, exp) in zip(recs, want):
        assert (ts, frac, incl, orig) == (i, 0, len(exp), len(exp)), (tag, i)
        assert body == exp, (tag, i)


def test_chain_matches_the_oracle(cuda, oracle_mod):
    """A capture in place -> 5-tuple -> PASS queue -> NAT with write-back on the source ->
    pcap_gather with SRC_RECORDS: exactly the oracle's passed packets, in order, each with its
    source record number as timestamp and NAT's final image bytes; then the same through
    Capture.filter with two chunk sizes."""
    import torch

    import ebpf_emu
    from ebpf_emu import Program, _lib, pcap
    from ebpf_emu import workloads as W

    cap, want = _oracle_chain(oracle_mod)
    offs, lens, _ = pcap.index(cap)
    n = len(offs)
    first, second = Program(W.program("5tuple")), Program(W.program("nat"))
    fr = torch.from_numpy(cap.copy()).to(cuda)
    d_offs, d_lens = _u32(offs, cuda), _u16(lens, cuda)
    res = ebpf_emu.two_stage(first, second, fr, offsets=d_offs, lens=d_lens, writeback=True)
    out, total = ebpf_emu.pcap_gather(fr, res.first.queue_index, res.first.queue_count, 2,
                                      cap[:24].tobytes(), flags=_lib.PCAP_SRC_RECORDS,
                                      offsets=d_offs, lens=d_lens, n=n)
    tot = total.cpu().numpy().view(np.uint32)
    assert int(tot[0]) == len(want)
    _assert_records(out[:int(tot[1])].cpu().numpy().tobytes(), cap, want, "raw chain")
    c = pcap.Capture(cap)
    for per in (1 << 20, 177):
        data = c.filter(first, 2, writeback=True, packets_per_chunk=per, second=second)
        _assert_records(data, cap, want, f"Capture.filter chunk={per}")
    # one program alone: the 5-tuple's PASS queue, the packets as they were
    data = c.filter(first, 2, packets_per_chunk=250)
    recs = R.parse(data)[3]
    assert [(r[0], r[4]) for r in recs] == [(i, cap[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes())
                                            for i, _ in want]
    assert np.array_equal(c.host.numpy(), cap)  # the source capture is not changed
    first.close()
    second.close()
