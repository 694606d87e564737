"""ebpf_pcap_gather without a GPU: the exports, the struct against the header, every validation
error of include/ebpf_emu.h (each returned before any device call), the valid call that launches
nothing, the Python wrapper's own argument checks, and the numpy model's invariants
(tests/pcap_export_ref.py is what tests/test_pcap_export.py compares the kernel with)."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import pcap_export_ref as R
import queues_ref as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000  # (never dereferenced on the host; no call below reaches a device)


def test_exports_flags_and_workspace_query(product_lib):
    from ebpf_emu import _lib

    for name in ("ebpf_pcap_gather_workspace_bytes", "ebpf_pcap_gather"):
        assert hasattr(product_lib, name), name
        assert name in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "ebpf_emu.h")).read()
    for name, mirror, model in (("EBPF_PCAP_SRC_RECORDS", _lib.PCAP_SRC_RECORDS, R.SRC_RECORDS),
                                ("EBPF_PCAP_SWAPPED", _lib.PCAP_SWAPPED, R.SWAPPED)):
        m = re.search(r"#define\s+%s\s+(\d+)u" % name, hdr)
        assert m and int(m.group(1)) == mirror == model, name
    need = product_lib.ebpf_pcap_gather_workspace_bytes(1 << 20)
    assert need > 0 and need % 8 == 0
    for n in (0, 1, (1 << 32) - 1):  # the grid is capped: one size
        assert product_lib.ebpf_pcap_gather_workspace_bytes(n) == need


def test_struct_matches_header():
    """The ctypes mirror has the header's fields, in its order, with its sizes and offsets."""
    from ebpf_emu import _lib

    hdr = open(os.path.join(ROOT, "include", "ebpf_emu.h")).read()
    body = re.search(r"typedef struct ebpf_pcap_gather_desc \{(.*?)\} ebpf_pcap_gather_desc;", hdr,
                     re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"^\s*([\w ]+?\*?)\s*(\w+)(\[\d+\])?;", body, re.M)  # (type, name, array)
    D = _lib.PcapGatherDesc
    assert [f[1] for f in fields] == [f[0] for f in D._fields_]
    at = 0
    for (ctype, name, arr), (_, mirror) in zip(fields, D._fields_):
        size = int(arr[1:-1]) if arr else 4 if ctype == "uint32_t" else 8
        align = 1 if arr else size
        at = (at + align - 1) // align * align
        assert ctypes.sizeof(mirror) == size, (ctype, name)
        assert getattr(D, name).offset == at, (name, at)
        at += size
    assert ctypes.sizeof(D) == at == 160
    assert D.file_header.offset == 64 and D.snaplen.offset == 88 and D.ts.offset == 96


def test_package_exports():
    import ebpf_emu
    from ebpf_emu import pcap, queues

    assert ebpf_emu.pcap_gather is queues.pcap_gather
    assert callable(pcap.header) and callable(pcap.Capture.filter)


def test_header_helper_matches_to_bytes():
    from ebpf_emu import _lib, pcap

    for nanos in (False, True):
        for big in (False, True):
            h, flag = pcap.header(linktype=101, snaplen=1234, nanos=nanos, big_endian=big)
            assert h == pcap.to_bytes([], linktype=101, snaplen=1234, nanos=nanos, big_endian=big)
            assert flag == (_lib.PCAP_SWAPPED if big else 0) == pcap.header_flag(h)
            assert R.parse(h) == (big, nanos, 101, [])
    with pytest.raises(ValueError):
        pcap.header_flag(b"\x00" * 24)


def _desc():
    from ebpf_emu import _lib

    p = _lib.PcapGatherDesc()
    p.frames, p.stride, p.n = P, 64, 16
    p.index, p.count, p.queue, p.flags = P, P, 2, 3
    p.snaplen, p.ts = 60, P
    p.out, p.out_bytes = P, 4096
    p.out_offsets, p.out_lens, p.out_total = P, P, P
    return p


def test_invalid_arguments_fail_before_any_device_call(product_lib):
    from ebpf_emu import _lib

    L = product_lib
    assert L.ebpf_pcap_gather(None, None) == _lib.EBPF_EINVAL
    for field in ("frames", "index", "count", "out", "out_total"):
        p = _desc()
        setattr(p, field, None)
        assert L.ebpf_pcap_gather(ctypes.byref(p), None) == _lib.EBPF_EINVAL, field
    for queue in (_lib.NQUEUES, 8, (1 << 32) - 1):
        p = _desc()
        p.queue = queue
        assert L.ebpf_pcap_gather(ctypes.byref(p), None) == _lib.EBPF_EINVAL, queue
    for flags in (4, 8, 7, 1 << 31):  # unknown flag bits
        p = _desc()
        p.flags = flags
        assert L.ebpf_pcap_gather(ctypes.byref(p), None) == _lib.EBPF_EINVAL, flags
    p = _desc()
    p.stride = 0  # no packet layout
    assert L.ebpf_pcap_gather(ctypes.byref(p), None) == _lib.EBPF_EINVAL
    p = _desc()
    p.stride = 65536  # no lens: the stride is the length, and incl_len is a u16 here
    assert L.ebpf_pcap_gather(ctypes.byref(p), None) == _lib.EBPF_EINVAL
    need = L.ebpf_pcap_gather_workspace_bytes(16)
    p = _desc()
    p.workspace, p.workspace_bytes = P, need - 1
    assert L.ebpf_pcap_gather(ctypes.byref(p), None) == _lib.EBPF_EINVAL
    p = _desc()
    p.workspace, p.workspace_bytes = P + 4, need  # not 8-byte aligned
    assert L.ebpf_pcap_gather(ctypes.byref(p), None) == _lib.EBPF_EINVAL


def test_too_big_fails_before_any_device_call(product_lib):
    from ebpf_emu import _lib

    L = product_lib
    for field, value in (("n", 1 << 32), ("out_bytes", (1 << 32) + 1)):
        p = _desc()
        setattr(p, field, value)
        assert L.ebpf_pcap_gather(ctypes.byref(p), None) == _lib.EBPF_ETOOBIG, field


def test_empty_batch_is_valid_and_launches_nothing(product_lib):
    """n == 0 returns 0 without a device (this test has none): with every optional pointer, with
    none of them, with a workspace, with out_bytes 0 and no out."""
    from ebpf_emu import _lib

    L = product_lib
    p = _desc()
    p.n = 0
    assert L.ebpf_pcap_gather(ctypes.byref(p), None) == _lib.EBPF_OK
    p.frames = p.ts = p.out_offsets = p.out_lens = None
    assert L.ebpf_pcap_gather(ctypes.byref(p), None) == _lib.EBPF_OK
    p.out, p.out_bytes = None, 0
    p.workspace, p.workspace_bytes = P, L.ebpf_pcap_gather_workspace_bytes(0)
    assert L.ebpf_pcap_gather(ctypes.byref(p), None) == _lib.EBPF_OK
    p.out_bytes = 1 << 32  # exactly 4 GiB is allowed
    p.out = P
    assert L.ebpf_pcap_gather(ctypes.byref(p), None) == _lib.EBPF_OK
    # ... and the checks still come first
    p.flags = 4
    assert L.ebpf_pcap_gather(ctypes.byref(p), None) == _lib.EBPF_EINVAL


def test_python_wrapper_checks_its_arguments(product_lib):
    import torch

    from ebpf_emu import pcap
    from ebpf_emu import queues as Q

    n = 8
    index = torch.zeros(n, dtype=torch.int32)
    count = torch.zeros(7, dtype=torch.int32)
    frames = torch.zeros(n * 64, dtype=torch.uint8)
    h, _ = pcap.header()
    ok = dict(stride=64)

    def bad(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            Q.pcap_gather(*a, **kw)

    bad("queue", frames, index, count, 7, h, **ok)
    bad("queue", frames, index, count, -1, h, **ok)
    bad("int32", frames, index.long(), count, 2, h, **ok)
    bad("int32", frames, index, count[:6], 2, h, **ok)
    bad("uint8", frames.int(), index, count, 2, h, **ok)
    bad("contiguous", frames.view(n, 64)[:, :32], index, count, 2, h, **ok)
    bad("24-byte", frames, index, count, 2, h[:23], **ok)
    bad("24-byte", frames, index, count, 2, h + b"\0", **ok)
    bad("flags", frames, index, count, 2, h, flags=4, **ok)
    bad("snaplen", frames, index, count, 2, h, snaplen=-1, **ok)
    bad("snaplen", frames, index, count, 2, h, snaplen=1 << 32, **ok)
    bad("layout", frames, index, count, 2, h)
    bad("n passes", frames, index, count, 2, h, n=n + 1, **ok)
    bad("n passes", frames, index, count, 2, h, offsets=torch.zeros(n - 1, dtype=torch.int32),
        lens=torch.zeros(n, dtype=torch.int16))
    bad("ts", frames, index, count, 2, h, ts=torch.zeros(n, 2, dtype=torch.int64), **ok)
    bad("ts", frames, index, count, 2, h, ts=torch.zeros(n - 1, 2, dtype=torch.int32), **ok)
    bad("out must", frames, index, count, 2, h, out=torch.zeros(64, dtype=torch.int32), **ok)
    bad("out_offsets", frames, index, count, 2, h, out_offsets=torch.zeros(n, dtype=torch.int64), **ok)
    bad("out_offsets", frames, index, count, 2, h, out_lens=torch.zeros(n - 1, dtype=torch.int16), **ok)
    # the default room: the global header, a record header per packet, the packets
    assert Q.pcap_out_bytes(n * 64, n, 64, False) == 24 + n * (16 + 64)
    assert Q.pcap_out_bytes(1000, n, 0, True) == 24 + 16 * n + 1000 + n
    assert Q.pcap_out_bytes(1 << 33, 1 << 26, 64, False) == Q.MAX_OUT_BYTES


def _batch(rng, n):
    v = rng.choice(np.array([0, 1, 2, 3, 0xFE, 0xFF], dtype=np.uint8), n)
    index, count = QR.queues(v)
    lens = rng.choice(np.array([0, 1, 15, 16, 17, 60, 64, 65, 1500], dtype=np.uint16), n)
    pkts = [rng.integers(0, 256, int(ln), dtype=np.uint8).tobytes() for ln in lens]
    return index, count, lens, pkts


def test_model_undoes_to_bytes_and_agrees_with_pcap_index(product_lib):
    """On a capture in place: with SRC_RECORDS and the whole batch in one queue the model's output
    IS the source capture (either byte order); without it, and without ts, the synthesised headers
    are to_bytes' own convention, so the model's output of a queue is to_bytes of that queue's
    packets but for the timestamps, which are the source record numbers; ebpf_pcap_index on the
    model's output returns the model's out_offsets / out_lens."""
    from ebpf_emu import pcap

    rng = np.random.default_rng(11)
    for n in (1, 7, 300):
        index, count, lens, pkts = _batch(rng, n)
        for big in (False, True):
            cap = np.frombuffer(pcap.to_bytes(pkts, big_endian=big), dtype=np.uint8)
            offs, ilens, _ = pcap.index(cap)
            assert np.array_equal(ilens, lens)
            flag = R.SWAPPED if big else 0
            one = np.zeros(7, dtype=np.uint32)
            one[4] = n
            every = np.arange(n, dtype=np.uint32)
            w, end, oo, ol, data = R.pcap_gather(cap, every, one, 4, n, cap[:24].tobytes(),
                                                 offsets=offs, lens=lens, out_bytes=1 << 30,
                                                 flags=R.SRC_RECORDS | flag)
            assert w == n and end == len(cap) and data == cap.tobytes()  # undoes to_bytes
            assert np.array_equal(oo, offs) and np.array_equal(ol, lens)
            for queue in (1, 2, 6):
                mine = QR.queue_of(index, count, queue)
                for flags in (flag, flag | R.SRC_RECORDS):
                    w, end, oo, ol, data = R.pcap_gather(cap, index, count, queue, n,
                                                         cap[:24].tobytes(), offsets=offs,
                                                         lens=lens, flags=flags, out_bytes=1 << 30)
                    assert w == len(mine) and end == len(data)
                    io, il, _ = pcap.index(np.frombuffer(data, dtype=np.uint8))
                    assert np.array_equal(io, oo) and np.array_equal(il, ol)
                    be, _, lt, recs = R.parse(data)
                    assert be == big and lt == 1
                    assert [r[0] for r in recs] == mine.tolist()  # the source record numbers
                    assert [r[4] for r in recs] == [pkts[i] for i in mine]
                    # the same bytes as to_bytes of the queue, timestamps aside
                    again = bytearray(pcap.to_bytes([pkts[i] for i in mine], big_endian=big))
                    for r, o in enumerate(oo):
                        again[int(o) - 16:int(o) - 12] = struct.pack(">I" if big else "<I", int(mine[r]))
                    assert bytes(again) == data


def test_model_capacity_snaplen_and_bad_index():
    rng = np.random.default_rng(12)
    n = 200
    index, count, lens, pkts = _batch(rng, n)
    offs = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])[:n].astype(np.uint32)
    frames = np.frombuffer(b"".join(pkts), dtype=np.uint8)
    h = bytes(range(24))
    ts = rng.integers(0, 1 << 32, (n, 2), dtype=np.uint64).astype(np.uint32)
    mine = QR.queue_of(index, count, 2)
    full = 24 + sum(16 + int(lens[i]) for i in mine)
    w, end, oo, ol, data = R.pcap_gather(frames, index, count, 2, n, h, offsets=offs, lens=lens,
                                         ts=ts, out_bytes=full)
    assert (w, end) == (len(mine), full) and data[:24] == h
    be, _, _, recs = R.parse(b"\xd4\xc3\xb2\xa1" + data[4:])
    assert [(r[0], r[1]) for r in recs] == [(int(ts[i][0]), int(ts[i][1])) for i in mine]
    # capacity: a prefix; the first record left out would end past out_bytes
    for out_bytes in (0, 23):
        assert R.pcap_gather(frames, index, count, 2, n, h, offsets=offs, lens=lens,
                             out_bytes=out_bytes)[:2] == (0, 0)
    assert R.pcap_gather(frames, index, count, 2, n, h, offsets=offs, lens=lens, out_bytes=24)[:2] == (0, 24)
    for k in (1, len(mine) // 2, len(mine)):
        end_k = 24 + sum(16 + int(lens[i]) for i in mine[:k])
        assert R.pcap_gather(frames, index, count, 2, n, h, offsets=offs, lens=lens,
                             out_bytes=end_k)[:2] == (k, end_k)
        w1, e1 = R.pcap_gather(frames, index, count, 2, n, h, offsets=offs, lens=lens,
                               out_bytes=end_k - 1)[:2]
        assert w1 == k - 1 and e1 == end_k - 16 - int(lens[mine[k - 1]])
    # snaplen: incl is cut, orig_len kept
    for snap in (1, 60, 70000):
        w, end, oo, ol, data = R.pcap_gather(frames, index, count, 2, n, h, offsets=offs, lens=lens,
                                             snaplen=snap, out_bytes=1 << 30)
        recs = R.parse(b"\xd4\xc3\xb2\xa1" + data[4:])[3]
        assert [r[2] for r in recs] == [min(int(lens[i]), snap) for i in mine] == ol.tolist()
        assert [r[3] for r in recs] == [int(lens[i]) for i in mine]
    # a packet number outside the batch is no record
    start = int(count[:2].sum())
    bad = index.copy()
    bad[start + 3] = n
    bad[start + 9] = 0xFFFFFFF0
    w, end, oo, ol, data = R.pcap_gather(frames, bad, count, 2, n, h, offsets=offs, lens=lens,
                                         out_bytes=1 << 30)
    keep = [int(i) for k, i in enumerate(mine) if k not in (3, 9)]
    assert w == len(mine) - 2 and [r[0] for r in R.parse(b"\xd4\xc3\xb2\xa1" + data[4:])[3]] == keep
