"""The numpy model of ebpf_scatter (include/ebpf_emu.h): the definition tests/test_scatter.py
compares the kernel with, written from the header's text alone (plain loops, no kernel structure).
Every array is modified in place, so whatever the header leaves untouched keeps the caller's
sentinel and the test compares the arrays whole."""
import numpy as np

NQUEUES = 7
U32_MAX = (1 << 32) - 1


def positions(index, count, queue, n, cap, total=None):
    """-> (start, m): the queue positions scattered are index[start : start + m]."""
    start = int(np.sum(count[:queue], dtype=np.int64))
    m = int(count[queue])
    start = min(start, n)          # (index is read inside index[0, n) only)
    m = min(m, n - start)
    m = min(m, cap, int(total[0]) if total is not None else U32_MAX)
    return start, m


def scatter(index, count, queue, n, cap, *, total=None,
            src_frames=None, src_offsets=None, src_lens=None,
            src_verdict=None, src_status=None, src_r0=None,
            frames=None, offsets=None, lens=None, stride=0,
            verdict=None, status=None, r0=None):
    """Applies the call to frames / verdict / status / r0 (numpy arrays, in place). -> the list of
    (j, d, L) of the valid entries."""
    start, m = positions(index, count, queue, n, cap, total)
    done = []
    for j in range(m):
        d = int(index[start + j])
        if d >= n:
            continue
        L = 0
        if frames is not None:
            so, sl = int(src_offsets[j]), int(src_lens[j])
            if so + sl > len(src_frames):
                continue
            dlen = int(lens[d]) if lens is not None else stride
            L = min(sl, dlen)
            at = int(offsets[d]) if offsets is not None else d * stride
            frames[at:at + L] = src_frames[so:so + L]
        for dst, src in ((verdict, src_verdict), (status, src_status), (r0, src_r0)):
            if dst is not None and src is not None:
                dst[d] = src[j]
        done.append((j, d, L))
    return done
