"""Checksum offload (ebpf_csum_verify / ebpf_csum_fill, include/ebpf_emu.h): the Internet checksum
of a whole batch.

A NIC's RX descriptor says whether a packet's IPv4 header checksum and its TCP / UDP checksum were
good; its TX side writes them into packets whose headers a program rewrote. `csum_verify` is the
first, `csum_fill` the second (the `nat` workload adjusts only the IPv4 header checksum: a fill of
its XDP_TX queue is what makes the redirected packets valid again). Both are one launch of the
gfx950 kernel in libebpfemu.so (csrc/csum.hip) on the caller's stream, with no host synchronisation
and no scratch. Device memory and streams come from PyTorch (plumbing only).
"""
from __future__ import annotations

import ctypes

from . import _lib
from ._lib import (CSUM_ALL, CSUM_IPV4_HDR, CSUM_L3_BAD, CSUM_L3_GOOD, CSUM_L4_BAD,  # noqa: F401
                   CSUM_L4_GOOD, CSUM_L4_NONE, CSUM_TCP, CSUM_UDP)
from .queues import _stream_ptr

# the kernel's ranges (csrc/launch.h kCsBlock, kCsMaxWgs): a workgroup is one wave and takes
# CSUM_BLOCK packets a pass (one pass while n <= CSUM_BLOCK * CSUM_MAX_WGS)
CSUM_BLOCK, CSUM_MAX_WGS = 64, 8192
STATUS_BITS = (("L3_GOOD", CSUM_L3_GOOD), ("L3_BAD", CSUM_L3_BAD), ("L4_GOOD", CSUM_L4_GOOD),
               ("L4_BAD", CSUM_L4_BAD), ("L4_NONE", CSUM_L4_NONE))


def _call(name, frames, what, stride, offsets, lens, n, verdict, queue_mask, stream, status):
    import torch

    if frames.dtype != torch.uint8 or not frames.is_contiguous():
        raise ValueError(f"{name}: frames must be a contiguous torch.uint8 tensor")
    if offsets is None and lens is None and stride == 0:
        raise ValueError(f"{name}: needs a packet layout (offsets, lens or a stride)")
    if n is None:
        n = (offsets.numel() if offsets is not None else lens.numel() if lens is not None
             else frames.numel() // stride)
    if (offsets is not None and offsets.numel() < n) or (lens is not None and lens.numel() < n):
        raise ValueError(f"{name}: n passes offsets or lens")
    dev = frames.device
    # (the kernel reads these as u32 / u16 / u8 words: a tensor of another type, a strided view or
    # one on another device would be read as something it is not)
    for what_, t, dt in (("offsets", offsets, torch.int32), ("lens", lens, torch.int16),
                         ("verdict", verdict, torch.uint8)):
        if t is not None and (t.dtype != dt or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"{name}: {what_} is a contiguous {dt} tensor on frames' device")
    if verdict is not None and verdict.numel() < n:
        raise ValueError(f"{name}: n passes verdict")
    if status is None:
        status = torch.empty(n, dtype=torch.uint8, device=dev)
    if status.dtype != torch.uint8 or status.numel() < n or not status.is_contiguous() or \
            status.device != dev:
        raise ValueError(f"{name}: status is a contiguous torch.uint8 [n] on frames' device")
    if n == 0:  # (empty tensors have no storage; the call launches nothing for n == 0)
        return status
    c = _lib.CsumDesc()
    c.frames = frames.data_ptr() or None
    c.offsets = offsets.data_ptr() if offsets is not None else None
    c.lens = lens.data_ptr() if lens is not None else None
    c.stride = stride
    c.n = n
    c.what = what
    c.verdict = verdict.data_ptr() if verdict is not None else None
    c.queue_mask = queue_mask
    c.status = status.data_ptr()
    with torch.cuda.device(dev):
        rc = getattr(_lib.lib(), "ebpf_" + name)(ctypes.byref(c), _stream_ptr(stream))
    if rc:
        raise _lib.EbpfError(rc, "ebpf_" + name)
    return status


def csum_verify(frames, what: int = CSUM_ALL, *, stride: int = 0, offsets=None, lens=None,
                n: int | None = None, verdict=None, queue_mask: int = 0x7F, stream=None,
                status=None):
    """-> status: torch.uint8 [n], per packet the CSUM_L3_GOOD / _L3_BAD bit of its IPv4 header
    checksum and the CSUM_L4_GOOD / _L4_BAD / _L4_NONE bit of its TCP / UDP checksum (0: nothing
    was checked). frames, stride / offsets / lens, n: the batch as Program.run takes it. what: the
    CSUM_* checksums looked at. verdict (torch.uint8 [n]) and queue_mask select the packets by
    verdict queue class; the others get status 0. The parse is the contract in include/ebpf_emu.h.
    status: an optional tensor to write into. Asynchronous on `stream` (None = current)."""
    return _call("csum_verify", frames, what, stride, offsets, lens, n, verdict, queue_mask, stream,
                 status)


def csum_fill(frames, what: int = CSUM_ALL, *, stride: int = 0, offsets=None, lens=None,
              n: int | None = None, verdict=None, queue_mask: int = 0x7F, stream=None,
              status=None):
    """Writes the checksums csum_verify would check INTO frames (the two-byte fields and no other
    byte) -> status: torch.uint8 [n], CSUM_L3_GOOD / CSUM_L4_GOOD for each field written. Arguments
    as csum_verify's."""
    return _call("csum_fill", frames, what, stride, offsets, lens, n, verdict, queue_mask, stream,
                 status)
