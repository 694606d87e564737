"""The numpy model of ebpf_verdict_queues / ebpf_gather (include/ebpf_emu.h): the definition the
tests compare the kernels with, written from the header alone (plain loops, no kernel structure)."""
import numpy as np

NQUEUES = 7
MAX_END = (1 << 32) - 1  # offsets and the end byte are u32


def classes(verdict):
    v = np.asarray(verdict, dtype=np.uint8).astype(np.int64)
    return np.where(v < 5, v, np.where(v == 0xFF, 6, 5))


def queues(verdict):
    """-> (index u32[n], count u32[7]): the stable partition by class."""
    q = classes(verdict)
    index = np.argsort(q, kind="stable").astype(np.uint32)
    count = np.bincount(q, minlength=NQUEUES).astype(np.uint32)
    return index, count


def queue_of(index, count, q):
    start = int(np.sum(count[:q], dtype=np.int64))
    return index[start:start + int(count[q])]


def alignup(v, a):
    return (v + a - 1) // a * a


def packet(frames, i, stride=0, offsets=None, lens=None):
    o = int(offsets[i]) if offsets is not None else i * stride
    ln = int(lens[i]) if lens is not None else stride
    return frames[o:o + ln]


def gather(frames, index, count, queue, *, stride=0, offsets=None, lens=None, align=16,
           out_bytes=0):
    """-> (written, end, out_offsets[written], out_lens[written], spans): spans = [(offset, bytes)]
    of the written packets. Everything else of the outputs is untouched."""
    src = queue_of(index, count, queue)
    off = 0
    offs, lns, spans = [], [], []
    for i in src:
        p = packet(frames, int(i), stride, offsets, lens)
        if off + len(p) > min(out_bytes, MAX_END):
            break
        offs.append(off)
        lns.append(len(p))
        spans.append((off, np.asarray(p, dtype=np.uint8)))
        off += alignup(len(p), align)
    end = offs[-1] + lns[-1] if offs else 0
    return len(offs), end, np.array(offs, dtype=np.uint32), np.array(lns, dtype=np.uint16), spans


def expected_frames(size, out_bytes, sentinel, align, end, spans):
    """-> (expected u8[size], mask of the bytes that are specified), size >= out_bytes: the
    packets' bytes over the sentinel; the padding below alignup(end, align) and below out_bytes is
    unspecified, every other byte is the sentinel (untouched)."""
    exp = np.full(size, sentinel, dtype=np.uint8)
    known = np.ones(size, dtype=bool)
    known[:min(alignup(end, align), out_bytes)] = False
    for o, b in spans:
        exp[o:o + len(b)] = b
        known[o:o + len(b)] = True
    return exp, known
