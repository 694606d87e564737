"""RSS flow steering (ebpf_rss_hash / ebpf_steer, include/ebpf_emu.h): which receive queue a packet
arrives on.

A NIC fills its RX queues by receive-side scaling: a Toeplitz hash of the packet's address and
port tuple, looked up in an indirection table. `rss_hash` is that hash for a whole batch, `steer`
the stable partition of the packet numbers into up to 64 queues by the table, so a flow's packets
stay in one queue, in arrival order. `SteerResult.queue(k)` is what `queues.gather`, `scatter` and
`pcap_gather` take as (index, count, queue): those kernels run unchanged on a steering queue. All
are launches of the gfx950 kernels in libebpfemu.so (csrc/steer.hip) on the caller's stream, with
no host synchronisation. Device memory and streams come from PyTorch (plumbing only).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

from . import _lib
from ._lib import (RSS_ALL, RSS_IPV4, RSS_IPV4_TCP, RSS_IPV4_UDP, RSS_IPV6,  # noqa: F401
                   RSS_IPV6_TCP, RSS_IPV6_UDP, STEER_MAX_QUEUES, STEER_MAX_RETA)
from .queues import _stream_ptr

# the key of the Microsoft RSS specification's verification suite (and many drivers' default)
MSFT_KEY = bytes.fromhex("6d5a56da255b0ec24167253d43a38fb0d0ca2bcbae7b30b477cb2da38030f20c"
                         "6a42b73bbeac01fa")
# 6d5a repeated: a 16-bit period, so swapping source and destination leaves the hash unchanged
SYMMETRIC_KEY = bytes.fromhex("6d5a" * 20)

# the kernels' ranges (csrc/launch.h kRssBlock, kRssMaxWgs, kSRange, kSMaxWgs): a hash workgroup
# takes RSS_BLOCK packets a pass (one pass while n <= RSS_BLOCK * RSS_MAX_WGS); a steer workgroup
# owns a whole number of STEER_RANGE keys (one while n <= STEER_RANGE * STEER_MAX_WGS)
RSS_BLOCK, RSS_MAX_WGS = 256, 2048
STEER_RANGE, STEER_MAX_WGS = 4096, 1024
# words behind bounds[2 * nq]: queues.scatter / pcap_gather want count.numel() >= NQUEUES of every
# view bounds[2 * k:] (the kernels read two words)
BOUNDS_PAD = _lib.NQUEUES - 2


def rss_hash(frames, key=MSFT_KEY, types: int = RSS_ALL, *, stride: int = 0, offsets=None,
             lens=None, n: int | None = None, stream=None, hash=None, type=None):
    """-> (hash, type): torch.int32 [n] (u32 bits), the Toeplitz hash of each packet's addresses
    (and ports) under `key` (40 bytes), and torch.uint8 [n], the one RSS_* bit of the input used
    (0: not hashed, hash 0). frames, stride / offsets / lens, n: the batch as Program.run takes it.
    types: the RSS_* inputs enabled. The parse (VLAN tags, fragments, IPv4 options; IPv6 extension
    headers are not walked) is the contract in include/ebpf_emu.h. hash / type: optional tensors
    to write into. Asynchronous on `stream` (None = current)."""
    import torch

    if frames.dtype != torch.uint8 or not frames.is_contiguous():
        raise ValueError("rss_hash: frames must be a contiguous torch.uint8 tensor")
    key = bytes(key)
    if len(key) != 40:
        raise ValueError("rss_hash: key is 40 bytes")
    if offsets is None and lens is None and stride == 0:
        raise ValueError("rss_hash: needs a packet layout (offsets, lens or a stride)")
    if n is None:
        n = (offsets.numel() if offsets is not None else lens.numel() if lens is not None
             else frames.numel() // stride)
    if (offsets is not None and offsets.numel() < n) or (lens is not None and lens.numel() < n):
        raise ValueError("rss_hash: n passes offsets or lens")
    dev = frames.device
    if hash is None:
        hash = torch.empty(n, dtype=torch.int32, device=dev)
    if type is None:
        type = torch.empty(n, dtype=torch.uint8, device=dev)
    if hash.dtype != torch.int32 or type.dtype != torch.uint8 or hash.numel() < n or \
            type.numel() < n or not hash.is_contiguous() or not type.is_contiguous():
        raise ValueError("rss_hash: hash / type are contiguous torch.int32 / torch.uint8 [n]")
    if n == 0:  # (empty tensors have no storage; the call launches nothing for n == 0)
        return hash, type
    r = _lib.RssDesc()
    r.frames = frames.data_ptr() or None
    r.offsets = offsets.data_ptr() if offsets is not None else None
    r.lens = lens.data_ptr() if lens is not None else None
    r.stride = stride
    r.n = n
    r.key[:] = key
    r.types = types
    r.hash = hash.data_ptr()
    r.type = type.data_ptr()
    with torch.cuda.device(dev):
        rc = _lib.lib().ebpf_rss_hash(ctypes.byref(r), _stream_ptr(stream))
    if rc:
        raise _lib.EbpfError(rc, "ebpf_rss_hash")
    return hash, type


@dataclass
class SteerResult:
    index: object = None   # torch.int32 [n] (u32 bits): the packet numbers, queue after queue
    bounds: object = None  # torch.int32 [>= 2 * nq] (u32 bits): {start_k, count_k} per queue
    nq: int = 0

    def queue(self, k: int):
        """(index, count, queue) of steering queue k for queues.gather / scatter / pcap_gather:
        their kernels read start = count[0] and m = count[1] of the view bounds[2 * k:]."""
        if not 0 <= k < self.nq:
            raise ValueError(f"queue must be in 0..{self.nq - 1}")
        return self.index, self.bounds[2 * k:], 1

    def counts(self):
        """torch.int32 [nq]: the queues' sizes (a view of bounds)."""
        return self.bounds[:2 * self.nq].view(self.nq, 2)[:, 1]


def default_reta(nq: int) -> list[int]:
    """Linux's default indirection table: 128 entries, reta[j] = j % nq."""
    return [j % nq for j in range(STEER_MAX_RETA)]


def steer(key, nq: int, reta=None, stream=None, index=None, bounds=None) -> SteerResult:
    """The stable partition of the packet numbers into nq (1..64) receive queues: queue(i) =
    reta[key[i] & (len(reta) - 1)]. key: a contiguous torch.int32 CUDA tensor (u32 bits; rss_hash's
    hash, or any flow key). reta: a sequence of 1..128 (a power of two) queue numbers < nq; None:
    default_reta(nq). -> SteerResult: queue k is index[bounds[2k] : bounds[2k] + bounds[2k + 1]],
    its packet numbers ascending. index / bounds: optional torch.int32 tensors to write into ([n]
    and [>= 2 * nq]; the default bounds carries BOUNDS_PAD words of padding so that every
    queue(k) view also passes scatter's and pcap_gather's size check). Asynchronous on `stream`
    (None = current), no host synchronisation."""
    import torch

    if key.dtype != torch.int32 or not key.is_contiguous():
        raise ValueError("steer: key must be a contiguous torch.int32 tensor")
    n = key.numel()
    dev = key.device
    if index is None:
        index = torch.empty(n, dtype=torch.int32, device=dev)
    if bounds is None:
        bounds = torch.zeros(2 * max(nq, 0) + BOUNDS_PAD, dtype=torch.int32, device=dev)
    if index.dtype != torch.int32 or bounds.dtype != torch.int32 or index.numel() < n or \
            bounds.numel() < 2 * nq or not index.is_contiguous() or not bounds.is_contiguous():
        raise ValueError("steer: index / bounds are contiguous torch.int32 [n] / [>= 2 * nq]")
    table, table_len = None, 0
    if reta is not None:
        table_len = len(reta)
        table = (ctypes.c_uint16 * max(table_len, 1))(*[int(x) for x in reta])
    with torch.cuda.device(dev):
        rc = _lib.lib().ebpf_steer(key.data_ptr() if n else None, n, nq,
                                   ctypes.cast(table, ctypes.c_void_p) if table is not None else None,
                                   table_len, index.data_ptr() if n else None, bounds.data_ptr(),
                                   None, 0, _stream_ptr(stream))
    if rc:
        raise _lib.EbpfError(rc, "ebpf_steer")
    return SteerResult(index=index, bounds=bounds, nq=nq)
