"""Host ingestion: classic pcap captures -> the GPU interpreter -> verdicts in host memory.

The north star's path "starts and ends in host memory (a pcap buffer or NIC ring)". A capture is
used as it is: `index()` (C ABI `ebpf_pcap_index`) returns each record's packet offset and length
within the capture bytes, so a device copy of the capture plus those two arrays is an offsets +
lens batch -- no repacking, and the 16-byte record headers simply sit between the frames.

`Capture.run()` streams a capture through one GPU in record-aligned chunks: pinned staging of the
chunk's bytes (offsets rebased to the chunk), H2D on one stream, the interpreter on a second,
the verdict D2H on a third, with events so that chunk i+1's copy and chunk i-1's verdicts
overlap chunk i's kernel. The reference reads one packet per process from argv (main.rs:14-22);
this is its batched replacement for whole captures.

`Capture.filter()` is the way back out: the records a program puts in one verdict queue, written
on the device as a capture again (`queues.pcap_gather`, C ABI `ebpf_pcap_gather`) with their own
record headers, one D2H copy per chunk.
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np

from . import _lib

LINKTYPE_ETHERNET = 1


def to_bytes(packets, linktype: int = LINKTYPE_ETHERNET, snaplen: int = 65535,
             nanos: bool = False, big_endian: bool = False) -> bytes:
    """A classic pcap capture of `packets` (bytes objects); timestamps are the record index."""
    e = ">" if big_endian else "<"
    magic = 0xA1B23C4D if nanos else 0xA1B2C3D4
    out = [struct.pack(e + "IHHiIII", magic, 2, 4, 0, 0, snaplen, linktype)]
    for i, p in enumerate(packets):
        out.append(struct.pack(e + "IIII", i, 0, len(p), len(p)))
        out.append(bytes(p))
    return b"".join(out)


def header(linktype: int = LINKTYPE_ETHERNET, snaplen: int = 65535, nanos: bool = False,
           big_endian: bool = False) -> tuple[bytes, int]:
    """(the 24-byte global header, the matching queues.pcap_gather flag): to_bytes' header, and
    _lib.PCAP_SWAPPED when its byte order is not the (little-endian) device's."""
    e = ">" if big_endian else "<"
    magic = 0xA1B23C4D if nanos else 0xA1B2C3D4
    return (struct.pack(e + "IHHiIII", magic, 2, 4, 0, 0, snaplen, linktype),
            _lib.PCAP_SWAPPED if big_endian else 0)


def header_flag(file_header) -> int:
    """The pcap_gather flag for a capture's own global header: PCAP_SWAPPED when its magic reads
    as a1b2c3d4 / a1b23c4d big-endian."""
    magic = bytes(file_header[:4])
    if magic in (b"\xd4\xc3\xb2\xa1", b"\x4d\x3c\xb2\xa1"):
        return 0
    if magic in (b"\xa1\xb2\xc3\xd4", b"\xa1\xb2\x3c\x4d"):
        return _lib.PCAP_SWAPPED
    raise ValueError("not a classic pcap global header")


def write(path: str, packets, **kw) -> None:
    with open(path, "wb") as f:
        f.write(to_bytes(packets, **kw))


def index(buf) -> tuple[np.ndarray, np.ndarray, int]:
    """(offsets u32[n], lens u16[n], linktype) of the records of a capture held in `buf`
    (bytes, bytearray, or a uint8 numpy array / pinned tensor's numpy view)."""
    L = _lib.lib()
    arr = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf
    arr = np.ascontiguousarray(arr)
    n = ctypes.c_size_t(0)
    lt = ctypes.c_uint32(0)
    rc = L.ebpf_pcap_index(arr.ctypes.data, arr.nbytes, None, None, 0, ctypes.byref(n),
                           ctypes.byref(lt))
    if rc != 0:
        raise _lib.EbpfError(rc, "ebpf_pcap_index")
    offs = np.zeros(n.value, dtype=np.uint32)
    lens = np.zeros(n.value, dtype=np.uint16)
    if n.value:
        rc = L.ebpf_pcap_index(arr.ctypes.data, arr.nbytes, offs.ctypes.data, lens.ctypes.data,
                               n.value, ctypes.byref(n), ctypes.byref(lt))
        if rc != 0:
            raise _lib.EbpfError(rc, "ebpf_pcap_index")
    return offs, lens, lt.value


class Capture:
    """A capture staged in pinned host memory, indexed once, run chunk by chunk on one GPU."""

    def __init__(self, data, device: int = 0):
        import torch

        src = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        self.device = torch.device("cuda", device)
        self.host = torch.empty(src.nbytes, dtype=torch.uint8, pin_memory=True)
        self.host.numpy()[:] = src
        self.offsets, self.lens, self.linktype = index(self.host.numpy())
        self.n = len(self.offsets)
        # per-record metadata in pinned memory: lengths once, chunk-rebased offsets per chunking
        self._lens_host = torch.from_numpy(self.lens.view(np.int16)).pin_memory()
        self._offs_host = {}

    def _rebased_offsets(self, chunks):
        import torch

        key = tuple(c[:2] for c in chunks)
        if key not in self._offs_host:
            t = torch.empty(self.n, dtype=torch.int32, pin_memory=True)
            ov = t.numpy().view(np.uint32)
            for i, c, b, _ in chunks:
                ov[i:i + c] = self.offsets[i:i + c] - np.uint32(b)
            self._offs_host = {key: t}
        return self._offs_host[key]

    def chunks(self, packets_per_chunk: int):
        """Record-aligned chunks: (first record, count, byte begin, byte end) of the capture."""
        out = []
        for i in range(0, self.n, packets_per_chunk):
            j = min(self.n, i + packets_per_chunk)
            b = int(self.offsets[i])
            e = int(self.offsets[j - 1]) + int(self.lens[j - 1])
            out.append((i, j - i, b, e))
        return out

    def run(self, prog, packets_per_chunk: int = 1 << 20, mem_size: int = 1024, r10: int = 512,
            counters=None, nbuf: int = 3):
        """Verdicts of every record (host uint8 tensor, pinned) and the device counters; the
        H2D / kernel / D2H of consecutive chunks overlap on three streams."""
        import torch

        dev = self.device
        chunks = self.chunks(packets_per_chunk)
        verdict = torch.empty(self.n, dtype=torch.uint8, pin_memory=True)
        if counters is None:
            counters = torch.zeros(8, dtype=torch.int64, device=dev)
        if not chunks:
            return verdict, counters
        max_bytes = max(e - b for _, _, b, e in chunks)
        max_pk = max(c for _, c, _, _ in chunks)
        offs_host = self._rebased_offsets(chunks)
        lens_host = self._lens_host
        dframes = [torch.empty(max_bytes + 16, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        doffs = [torch.empty(max_pk, dtype=torch.int32, device=dev) for _ in range(nbuf)]
        dlens = [torch.empty(max_pk, dtype=torch.int16, device=dev) for _ in range(nbuf)]
        dverd = [torch.empty(max_pk, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        outs = []
        for s in range(nbuf):
            o = _lib.BatchOut()
            o.verdict = dverd[s].data_ptr()
            o.counters = counters.data_ptr()
            outs.append(o)
        s_in, s_k, s_out = (torch.cuda.Stream(dev) for _ in range(3))
        # the buffers and the counters were allocated / zeroed on the current stream: the side
        # streams start after that work (the caching allocator may also have handed back memory
        # that pending current-stream work still uses)
        cur = torch.cuda.current_stream(dev)
        for st in (s_in, s_k, s_out):
            st.wait_stream(cur)
        ev_in = [torch.cuda.Event() for _ in chunks]
        ev_k = [torch.cuda.Event() for _ in chunks]
        ev_out = [torch.cuda.Event() for _ in chunks]
        for k, (i, c, b, e) in enumerate(chunks):
            s = k % nbuf
            with torch.cuda.stream(s_in):
                if k >= nbuf:
                    s_in.wait_event(ev_k[k - nbuf])  # buffers s consumed by kernel k - nbuf
                dframes[s][:e - b].copy_(self.host[b:e], non_blocking=True)
                doffs[s][:c].copy_(offs_host[i:i + c], non_blocking=True)
                dlens[s][:c].copy_(lens_host[i:i + c], non_blocking=True)
                ev_in[k].record(s_in)
            s_k.wait_event(ev_in[k])
            if k >= nbuf:
                s_k.wait_event(ev_out[k - nbuf])  # verdict buffer s drained
            batch = prog.make_batch(dframes[s], n=c, offsets=doffs[s], lens=dlens[s],
                                    mem_size=mem_size, r10=r10)
            prog.launch(batch, outs[s], s_k)
            ev_k[k].record(s_k)
            with torch.cuda.stream(s_out):
                s_out.wait_event(ev_k[k])
                verdict[i:i + c].copy_(dverd[s][:c], non_blocking=True)
                ev_out[k].record(s_out)
        torch.cuda.synchronize(dev)
        return verdict, counters

    def filter(self, prog, queue: int = 2, writeback: bool = False, snaplen: int = 0,
               packets_per_chunk: int = 1 << 20, mem_size: int = 1024, r10: int = 512,
               second=None) -> bytes:
        """The records `prog` puts in verdict queue `queue` (default XDP_PASS), as a new capture
        in host bytes: the source's own global header, then each such record with its own header
        (timestamps kept) in file order. writeback=True: the packets as `prog` rewrote them
        (EBPF_BATCH_WRITEBACK on the device copy; the source capture is not changed). snaplen: cut
        the records (0: no cut; orig_len is kept). second: a Program run over the queue's packets
        before they are written out (queues.two_stage; with writeback=True its rewrites are what
        the new capture holds, and `prog`'s own run does not write).

        Chunked like run(): per chunk the bytes from its first record header on go to the device,
        prog.run(queues=True) and ONE queues.pcap_gather with PCAP_SRC_RECORDS follow on the
        current stream, and after one read of the chunk's out_total its records are appended; the
        global header is kept from the first chunk only."""
        import torch

        from .queues import pcap_gather, pcap_out_bytes, two_stage

        dev = self.device
        file_header = bytes(self.host.numpy()[:24])
        flags = _lib.PCAP_SRC_RECORDS | header_flag(file_header)
        parts = [file_header]
        chunks = self.chunks(packets_per_chunk)
        if not chunks:
            return file_header
        max_bytes = max(e - b for _, _, b, e in chunks) + 16
        max_pk = max(c for _, c, _, _ in chunks)
        with torch.cuda.device(dev):
            dframes = torch.empty(max_bytes, dtype=torch.uint8, device=dev)
            out = torch.empty(pcap_out_bytes(max_bytes, max_pk, 0, True), dtype=torch.uint8, device=dev)
            total = torch.empty(2, dtype=torch.int32, device=dev)
            for i, c, b, e in chunks:
                b -= 16  # the first record's header comes along: every packet offset is >= 16
                dframes[:e - b].copy_(self.host[b:e], non_blocking=True)
                offs = torch.from_numpy((self.offsets[i:i + c] - np.uint32(b)).view(np.int32)).to(dev)
                lens = torch.from_numpy(self.lens[i:i + c].view(np.int16)).to(dev)
                if second is not None:
                    res = two_stage(prog, second, dframes, n=c, offsets=offs, lens=lens,
                                    queue=queue, writeback=writeback, mem_size=mem_size, r10=r10).first
                else:
                    res = prog.run(dframes, n=c, offsets=offs, lens=lens, mem_size=mem_size,
                                   r10=r10, queues=True, writeback=writeback)
                pcap_gather(dframes, res.queue_index, res.queue_count, queue, file_header,
                            flags=flags, snaplen=snaplen, offsets=offs, lens=lens, n=c, out=out,
                            total=total)
                end = int(total[1]) & 0xFFFFFFFF  # the one host read
                parts.append(out[24:end].cpu().numpy().tobytes())
        return b"".join(parts)
