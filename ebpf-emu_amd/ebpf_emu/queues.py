"""Verdict queues, the packet gather, the scatter back and the pcap gather (ebpf_verdict_queues /
ebpf_gather / ebpf_scatter / ebpf_pcap_gather, include/ebpf_emu.h).

What a datapath does with a batch's verdicts: `verdict_queues` is the stable partition of the
packet numbers by XDP action (xdp.rs:3-9 order, then other / fault), `gather` copies one queue's
packets into a dense offsets + lens batch -- itself the input of a next `Program.run` -- and
`scatter` puts that batch's packets and results back at the packets' own numbers; `two_stage` is
the whole chain; `pcap_gather` writes one queue out as a classic pcap capture. All are launches of
the gfx950 kernels in libebpfemu.so (csrc/queues.hip) on the caller's stream, with no host
synchronisation: the queue's size is read on the device. Device memory and streams come from
PyTorch (plumbing only).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

from . import _lib

# the kernels' ranges (csrc/launch.h kQRange, kQMaxWgs, kGTile, kGMaxWgs): a queues workgroup owns
# a whole number of QUEUES_RANGE packets (one while n <= QUEUES_RANGE * QUEUES_MAX_WGS), a gather
# workgroup a whole number of GATHER_TILE queue positions
QUEUES_RANGE, QUEUES_MAX_WGS = 4096, 1024
GATHER_TILE, GATHER_MAX_WGS = 256, 1024
SCATTER_TILE, SCATTER_MAX_WGS = GATHER_TILE, GATHER_MAX_WGS  # the scatter walks the same tiles
MAX_OUT_BYTES = 1 << 32


@dataclass
class GatherResult:
    frames: object = None   # torch.uint8 [out_bytes]
    offsets: object = None  # torch.int32 [n] (u32 bits); entries [0, total[0]) are written
    lens: object = None     # torch.int16 [n] (u16 bits); entries [0, total[0]) are written
    total: object = None    # torch.int32 [2] (u32 bits): packets written, end byte of the last one


def _stream_ptr(stream):
    import torch

    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def verdict_queues(verdict, stream=None, index=None, count=None):
    """-> (index, count): torch.int32 [n] (u32 bits) and [NQUEUES]. Queue q is
    index[count[:q].sum() : count[:q + 1].sum()], its packet numbers ascending. `verdict`: a
    torch.uint8 CUDA tensor (any alignment, contiguous). Asynchronous on `stream` (None = current).
    index / count: optional tensors to write into."""
    import torch

    if verdict.dtype != torch.uint8 or not verdict.is_contiguous():
        raise ValueError("verdict: a contiguous torch.uint8 tensor")
    n = verdict.numel()
    dev = verdict.device
    if index is None:
        index = torch.empty(n, dtype=torch.int32, device=dev)
    if count is None:
        count = torch.empty(_lib.NQUEUES, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().ebpf_verdict_queues(verdict.data_ptr() if n else None, n,
                                            index.data_ptr() if n else None, count.data_ptr(),
                                            None, 0, _stream_ptr(stream))
    if rc:
        raise _lib.EbpfError(rc, "ebpf_verdict_queues")
    return index, count


def _alignup(v: int, a: int) -> int:
    return (v + a - 1) // a * a


def default_out_bytes(frames_bytes: int, n: int, stride: int, has_lens: bool, align: int) -> int:
    """n * alignup(the longest possible packet, align), capped at 4 GiB -- and, for a batch with
    lengths (up to 65535 bytes each), at the source buffer's size plus n paddings, which holds
    every packet of a batch whose packets do not overlap."""
    longest = stride if not has_lens else (min(stride, 0xFFFF) if stride else 0xFFFF)
    b = n * _alignup(longest, align)
    if has_lens:
        b = min(b, _alignup(frames_bytes, align) + n * align)
    return min(b, MAX_OUT_BYTES)


def gather(frames, index, count, queue: int, *, stride: int = 0, offsets=None, lens=None,
           align: int = 16, out_bytes: int | None = None, stream=None, n: int | None = None,
           out: GatherResult | None = None) -> GatherResult:
    """Copy queue `queue` of (index, count) out of the batch (frames, stride / offsets / lens: as
    Program.run takes them) into a dense batch: packet j of the queue at res.frames[res.offsets[j]:]
    with length res.lens[j], offsets multiples of `align`. res.total = [packets written, end byte]:
    the packets that fit out_bytes, a prefix of the queue. Run the result with
    prog.run(res.frames, n=int(res.total[0]), offsets=res.offsets, lens=res.lens).
    out: an optional GatherResult whose tensors are written into (sentinels, reuse)."""
    import torch

    dev = frames.device
    if n is None:
        n = index.numel()
    if out_bytes is None:
        out_bytes = (out.frames.numel() if out is not None else
                     default_out_bytes(frames.numel(), n, stride, lens is not None, align))
    res = out if out is not None else GatherResult(
        frames=torch.empty(out_bytes, dtype=torch.uint8, device=dev),
        offsets=torch.empty(n, dtype=torch.int32, device=dev),
        lens=torch.empty(n, dtype=torch.int16, device=dev),
        total=torch.empty(2, dtype=torch.int32, device=dev))
    g = _lib.GatherDesc()
    g.frames = frames.data_ptr()
    g.offsets = offsets.data_ptr() if offsets is not None else None
    g.lens = lens.data_ptr() if lens is not None else None
    g.stride = stride
    g.n = n
    g.index = index.data_ptr()
    g.count = count.data_ptr()
    g.queue = queue
    g.align = align
    g.out_frames = res.frames.data_ptr() if out_bytes else None
    g.out_bytes = out_bytes
    # (an empty tensor has no storage: the entries of an empty batch are never written)
    g.out_offsets = res.offsets.data_ptr() or res.total.data_ptr()
    g.out_lens = res.lens.data_ptr() or res.total.data_ptr()
    g.out_total = res.total.data_ptr()
    if not g.index:
        g.index = res.total.data_ptr()
    with torch.cuda.device(dev):
        rc = _lib.lib().ebpf_gather(ctypes.byref(g), _stream_ptr(stream))
    if rc:
        raise _lib.EbpfError(rc, "ebpf_gather")
    return res


_RESULTS = (("verdict", "uint8"), ("status", "uint8"), ("r0", "int64"))


def scatter(gathered, index, count, queue: int, *, frames=None, stride: int = 0, offsets=None,
            lens=None, n: int | None = None, src=None, dst=None, cap: int | None = None,
            stream=None) -> None:
    """Put a gathered queue back (ebpf_scatter): queue position j of queue `queue` of (index,
    count) is packet d = index[start + j] of the original batch.

    gathered: the GatherResult the queue was gathered into (and a second Program.run perhaps
    rewrote with writeback=True); its `total`, when set, bounds the positions scattered.
    frames (+ stride / offsets / lens, n: the ORIGINAL batch as Program.run takes it): written --
    bytes [0, min(gathered.lens[j], len(d))) of packet d become the dense packet's, and no other
    byte changes. frames=None: results only.
    src / dst: BatchResult-like objects (the second run's result, the merged result); for each of
    verdict, status and r0 that BOTH hold, dst.x[d] = src.x[j]; every other entry of dst is
    untouched. cap: entries present in the dense arrays (default: the shortest of them).
    Asynchronous on `stream` (None = current), no host synchronisation: the queue's size is read
    on the device. The d values are distinct for verdict_queues' index; the dense and the original
    buffers must not overlap."""
    import torch

    if gathered is None:
        raise ValueError("scatter: `gathered` is the GatherResult of the queue (gather's result)")
    if not 0 <= queue < _lib.NQUEUES:
        raise ValueError(f"scatter: queue must be in 0..{_lib.NQUEUES - 1}")
    if index.dtype != torch.int32 or count.dtype != torch.int32 or count.numel() < _lib.NQUEUES:
        raise ValueError("scatter: index / count are verdict_queues' torch.int32 tensors")
    dev = index.device
    s = _lib.ScatterDesc()
    present = []  # the dense arrays: cap may not pass the shortest of them
    if frames is not None:
        if frames.dtype != torch.uint8 or not frames.is_contiguous() or frames.is_inference():
            raise ValueError("scatter: frames must be a writable, contiguous torch.uint8 tensor")
        if gathered.frames is None or gathered.offsets is None or gathered.lens is None:
            raise ValueError("scatter: frames needs gathered.frames, .offsets and .lens")
        if offsets is None and stride == 0:
            raise ValueError("scatter: frames needs a packet layout (offsets or a stride)")
        if gathered.offsets.dtype != torch.int32 or gathered.lens.dtype != torch.int16:
            raise ValueError("scatter: gathered.offsets / .lens are torch.int32 / torch.int16")
        s.frames = frames.data_ptr()
        s.offsets = offsets.data_ptr() if offsets is not None else None
        s.lens = lens.data_ptr() if lens is not None else None
        s.stride = stride
        # (an empty tensor has no storage; nothing of it is read)
        s.src_frames = gathered.frames.data_ptr() or count.data_ptr()
        s.src_bytes = gathered.frames.numel()
        s.src_offsets = gathered.offsets.data_ptr() or count.data_ptr()
        s.src_lens = gathered.lens.data_ptr() or count.data_ptr()
        present += [gathered.offsets, gathered.lens]
    pairs = []
    for name, dt in _RESULTS:
        a = getattr(src, name, None) if src is not None else None
        b = getattr(dst, name, None) if dst is not None else None
        if a is None or b is None:
            continue
        want = getattr(torch, dt)
        if a.dtype != want or b.dtype != want or not a.is_contiguous() or not b.is_contiguous():
            raise ValueError(f"scatter: src.{name} / dst.{name} must be contiguous torch.{dt}")
        setattr(s, "src_" + name, a.data_ptr())
        setattr(s, name, b.data_ptr())
        present.append(a)
        pairs.append(b)
    if n is None:
        n = (pairs[0].numel() if pairs else offsets.numel() if offsets is not None
             else index.numel())
    if n > index.numel() or any(b.numel() < n for b in pairs) or \
            (frames is not None and offsets is not None and offsets.numel() < n) or \
            (frames is not None and lens is not None and lens.numel() < n):
        raise ValueError("scatter: n passes index, a dst array, offsets or lens")
    room = min((t.numel() for t in present), default=0)
    if cap is None:
        cap = room
    if not 0 <= cap <= room:
        raise ValueError("scatter: cap passes the shortest dense array")
    s.index = index.data_ptr() or count.data_ptr()  # (an empty tensor has no storage)
    s.count = count.data_ptr()
    s.total = gathered.total.data_ptr() if gathered.total is not None else None
    s.queue = queue
    s.cap = cap
    s.n = n
    with torch.cuda.device(dev):
        rc = _lib.lib().ebpf_scatter(ctypes.byref(s), _stream_ptr(stream))
    if rc:
        raise _lib.EbpfError(rc, "ebpf_scatter")


@dataclass
class TwoStageResult:
    merged: object = None    # BatchResult: verdict / status / r0 per ORIGINAL packet
    first: object = None     # the first stage's BatchResult (queue_index / queue_count included)
    second: object = None    # the second stage's BatchResult, numbered by queue position
    gathered: object = None  # the GatherResult the second stage ran on
    m: int = 0               # packets the second stage ran


def two_stage(first, second, frames, *, n: int | None = None, stride: int = 0, offsets=None,
              lens=None, queue: int = 2, writeback: bool = False, align: int = 16, stream=None,
              **run_kw) -> TwoStageResult:
    """Run `first` over the batch, `second` over the packets `first` put in `queue` (default
    XDP_PASS), and merge: res.merged.verdict / .status / .r0 hold the second stage's result for
    the packets of the queue and the first stage's for every other packet; with writeback=True the
    second stage's rewrites (EBPF_BATCH_WRITEBACK) land in `frames`, in the packets' own places.

    The steps, on one stream: first.run(queues=True) -> gather -> ONE HOST READ of total[0], the
    size of the second batch -> second.run on the dense batch -> scatter into a clone of the first
    run's verdict / status / r0 (and into `frames`). That read of total[0] (8 bytes, which waits
    for the first run and the gather) is this chain's only synchronisation; nothing else here
    waits for the device. run_kw (mem_size, max_steps, ...) goes to both runs."""
    import torch

    from .program import BatchResult

    r1 = first.run(frames, n=n, stride=stride, offsets=offsets, lens=lens, verdict=True, r0=True,
                   status=True, queues=True, stream=stream, **run_kw)
    n = r1.verdict.numel()
    g = gather(frames, r1.queue_index, r1.queue_count, queue, stride=stride, offsets=offsets,
               lens=lens, align=align, stream=stream, n=n)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        m = int(g.total[0]) & 0xFFFFFFFF  # the one host read
        merged = BatchResult(verdict=r1.verdict.clone(), status=r1.status.clone(),
                             r0=r1.r0.clone())
    r2 = BatchResult()
    if m:
        r2 = second.run(g.frames, n=m, offsets=g.offsets, lens=g.lens, verdict=True, r0=True,
                        status=True, writeback=writeback, stream=stream, **run_kw)
        scatter(g, r1.queue_index, r1.queue_count, queue, frames=frames if writeback else None,
                stride=stride, offsets=offsets, lens=lens, n=n, src=r2, dst=merged, cap=m,
                stream=stream)
    return TwoStageResult(merged=merged, first=r1, second=r2, gathered=g, m=m)


def pcap_out_bytes(frames_bytes: int, n: int, stride: int, has_lens: bool) -> int:
    """Room for every packet of the batch as a record: the global header, n record headers and
    the gather's bound on the packets' bytes at align 1, capped at 4 GiB."""
    return min(24 + 16 * n + default_out_bytes(frames_bytes, n, stride, has_lens, 1), MAX_OUT_BYTES)


def pcap_gather(frames, index, count, queue: int, file_header, *, flags: int = 0, snaplen: int = 0,
                ts=None, stride: int = 0, offsets=None, lens=None, n: int | None = None,
                out=None, total=None, out_offsets=None, out_lens=None, with_index: bool = False,
                stream=None):
    """Write queue `queue` of (index, count) out of the batch (frames, stride / offsets / lens: as
    Program.run takes them) as a classic libpcap byte stream (ebpf_pcap_gather): file_header (24
    bytes, pcap.header's or the source capture's own) at out[0:24], then one record per packet of
    the queue. -> (out, total), total = [records written, end byte]: out[:total[1]] is the
    capture. With with_index=True (or out_offsets / out_lens given) -> (out, total, out_offsets,
    out_lens): each record's packet offset in `out` and its captured length, entries [0, total[0]).

    flags: _lib.PCAP_SRC_RECORDS (the batch is a capture in place: copy its record headers),
    _lib.PCAP_SWAPPED (a big-endian capture). snaplen: 0 = no cut. ts: optional torch.int32 [n, 2]
    (u32 bits) seconds and fraction by source packet number; without it (and without SRC_RECORDS)
    the timestamp is the source packet number. out / total / out_offsets / out_lens: optional
    tensors to write into (sentinels, reuse); `out` defaults to room for the whole batch.
    Asynchronous on `stream` (None = current), no host synchronisation."""
    import torch

    if not 0 <= queue < _lib.NQUEUES:
        raise ValueError(f"pcap_gather: queue must be in 0..{_lib.NQUEUES - 1}")
    if index.dtype != torch.int32 or count.dtype != torch.int32 or count.numel() < _lib.NQUEUES:
        raise ValueError("pcap_gather: index / count are verdict_queues' torch.int32 tensors")
    if frames.dtype != torch.uint8 or not frames.is_contiguous():
        raise ValueError("pcap_gather: frames must be a contiguous torch.uint8 tensor")
    hdr = bytes(file_header)
    if len(hdr) != 24:
        raise ValueError("pcap_gather: file_header is the 24-byte global header")
    if flags & ~(_lib.PCAP_SRC_RECORDS | _lib.PCAP_SWAPPED):
        raise ValueError("pcap_gather: flags are PCAP_SRC_RECORDS | PCAP_SWAPPED")
    if not 0 <= snaplen <= 0xFFFFFFFF:
        raise ValueError("pcap_gather: snaplen is a u32 (0: no cut)")
    if offsets is None and lens is None and stride == 0:
        raise ValueError("pcap_gather: needs a packet layout (offsets, lens or a stride)")
    if n is None:
        n = index.numel()
    if n > index.numel() or (offsets is not None and offsets.numel() < n) or \
            (lens is not None and lens.numel() < n):
        raise ValueError("pcap_gather: n passes index, offsets or lens")
    if ts is not None and (ts.dtype != torch.int32 or not ts.is_contiguous() or ts.numel() < 2 * n):
        raise ValueError("pcap_gather: ts must be a contiguous torch.int32 [n, 2] tensor")
    dev = frames.device
    if out is None:
        out = torch.empty(pcap_out_bytes(frames.numel(), n, stride, lens is not None),
                          dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() > MAX_OUT_BYTES:
        raise ValueError("pcap_gather: out must be a contiguous torch.uint8 tensor of at most 4 GiB")
    if total is None:
        total = torch.empty(2, dtype=torch.int32, device=dev)
    if with_index or out_offsets is not None or out_lens is not None:
        if out_offsets is None:
            out_offsets = torch.empty(n, dtype=torch.int32, device=dev)
        if out_lens is None:
            out_lens = torch.empty(n, dtype=torch.int16, device=dev)
        if out_offsets.dtype != torch.int32 or out_lens.dtype != torch.int16 or \
                out_offsets.numel() < n or out_lens.numel() < n:
            raise ValueError("pcap_gather: out_offsets / out_lens are torch.int32 / torch.int16 [n]")
        with_index = True
    p = _lib.PcapGatherDesc()
    p.frames = frames.data_ptr() or total.data_ptr()  # (an empty tensor has no storage)
    p.offsets = offsets.data_ptr() if offsets is not None else None
    p.lens = lens.data_ptr() if lens is not None else None
    p.stride = stride
    p.n = n
    p.index = index.data_ptr() or total.data_ptr()
    p.count = count.data_ptr()
    p.queue = queue
    p.flags = flags
    p.file_header[:] = hdr
    p.snaplen = snaplen
    p.ts = ts.data_ptr() if ts is not None else None
    p.out = out.data_ptr() if out.numel() else None
    p.out_bytes = out.numel()
    p.out_offsets = (out_offsets.data_ptr() or None) if with_index else None
    p.out_lens = (out_lens.data_ptr() or None) if with_index else None
    p.out_total = total.data_ptr()
    with torch.cuda.device(dev):
        rc = _lib.lib().ebpf_pcap_gather(ctypes.byref(p), _stream_ptr(stream))
    if rc:
        raise _lib.EbpfError(rc, "ebpf_pcap_gather")
    return (out, total, out_offsets, out_lens) if with_index else (out, total)
