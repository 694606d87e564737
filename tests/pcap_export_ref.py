"""The numpy / struct model of ebpf_pcap_gather (include/ebpf_emu.h): the definition the tests
compare the kernel with, written from the header alone (plain loops, no kernel structure), and a
parser of classic pcap bytes that owes nothing to ebpf_pcap_index."""
import struct

import numpy as np

SRC_RECORDS, SWAPPED = 1, 2
MAX_END = (1 << 32) - 1  # offsets and the end byte are u32


def positions(index, count, queue, n):
    """The queue's entries of index, start and size clamped into index[0, n)."""
    start = min(int(np.sum(count[:queue], dtype=np.int64)), n)
    m = min(int(count[queue]), n - start)
    return [int(x) for x in index[start:start + m]]


def pcap_gather(frames, index, count, queue, n, file_header, *, stride=0, offsets=None, lens=None,
                flags=0, snaplen=0, ts=None, out_bytes=0):
    """-> (records, end, out_offsets[records], out_lens[records], data): data = the bytes
    out[0:end] (b"" when not even the global header fits). Everything else is untouched."""
    if out_bytes < 24:
        return 0, 0, np.zeros(0, np.uint32), np.zeros(0, np.uint16), b""
    e = ">" if flags & SWAPPED else "<"  # (the device is little-endian)
    data = bytearray(bytes(file_header))
    assert len(data) == 24
    offs, lns = [], []
    for s in positions(index, count, queue, n):
        if s >= n:
            continue  # no record
        o = int(offsets[s]) if offsets is not None else s * stride
        ln = int(lens[s]) if lens is not None else stride
        incl = snaplen if snaplen and snaplen < ln else ln
        if len(data) + 16 + incl > min(out_bytes, MAX_END):
            break
        if flags & SRC_RECORDS and o >= 16:
            hdr = bytearray(frames[o - 16:o].tobytes())
            if incl < ln:
                hdr[8:12] = struct.pack(e + "I", incl)
        elif ts is not None:
            hdr = struct.pack(e + "IIII", int(ts[s][0]), int(ts[s][1]), incl, ln)
        else:
            hdr = struct.pack(e + "IIII", s, 0, incl, ln)
        data += hdr
        offs.append(len(data))
        lns.append(incl)
        data += frames[o:o + incl].tobytes()
    return (len(offs), len(data), np.array(offs, dtype=np.uint32), np.array(lns, dtype=np.uint16),
            bytes(data))


def parse(buf):
    """Classic pcap bytes -> (big_endian, nanos, linktype, [(ts, ts_frac, incl, orig, bytes)])."""
    buf = bytes(buf)
    magic = buf[:4]
    kinds = {b"\xd4\xc3\xb2\xa1": ("<", False), b"\x4d\x3c\xb2\xa1": ("<", True),
             b"\xa1\xb2\xc3\xd4": (">", False), b"\xa1\xb2\x3c\x4d": (">", True)}
    assert len(buf) >= 24 and magic in kinds, "not a classic pcap capture"
    e, nanos = kinds[magic]
    linktype = struct.unpack(e + "I", buf[20:24])[0]
    recs, at = [], 24
    while at < len(buf):
        assert at + 16 <= len(buf), "truncated record header"
        ts, frac, incl, orig = struct.unpack(e + "IIII", buf[at:at + 16])
        assert at + 16 + incl <= len(buf), "truncated record"
        recs.append((ts, frac, incl, orig, buf[at + 16:at + 16 + incl]))
        at += 16 + incl
    return e == ">", nanos, linktype, recs
