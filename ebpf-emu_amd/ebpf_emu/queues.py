"""Verdict queues and the packet gather (ebpf_verdict_queues / ebpf_gather, include/ebpf_emu.h).

What a datapath does with a batch's verdicts: `verdict_queues` is the stable partition of the
packet numbers by XDP action (xdp.rs:3-9 order, then other / fault), `gather` copies one queue's
packets into a dense offsets + lens batch -- itself the input of a next `Program.run`. Both are
launches of the gfx950 kernels in libebpfemu.so (csrc/queues.hip) on the caller's stream, with no
host synchronisation: the queue's size is read on the device. Device memory and streams come from
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
