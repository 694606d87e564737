"""ebpf_scatter without a GPU: the exports, every validation error of include/ebpf_emu.h (each
returned before any device call), the calls that are valid and launch nothing, the Python
wrapper's own argument checks, and the numpy model's invariants (tests/scatter_ref.py is what
tests/test_scatter.py compares the kernel with)."""
import ctypes
import os
import re

import numpy as np
import pytest

import queues_ref as QR
import scatter_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000  # (never dereferenced on the host; no call below reaches a device)


def test_exports_and_workspace_query(product_lib):
    from ebpf_emu import _lib

    for name in ("ebpf_scatter_workspace_bytes", "ebpf_scatter"):
        assert hasattr(product_lib, name), name
        assert name in _lib.EXPORTS
    # the one launch needs no scratch: the query answers, for any cap
    for cap in (0, 1, 1 << 20, (1 << 32) - 1):
        assert product_lib.ebpf_scatter_workspace_bytes(cap) == 0


def test_struct_matches_header():
    """The ctypes mirror has the header's fields, in its order, with its sizes."""
    from ebpf_emu import _lib

    hdr = open(os.path.join(ROOT, "include", "ebpf_emu.h")).read()
    body = re.search(r"typedef struct ebpf_scatter_desc \{(.*?)\} ebpf_scatter_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"^\s*([\w ]+?\*?)\s*(\w+);", body, re.M)  # (type, name)
    assert [f[1] for f in fields] == [f[0] for f in _lib.ScatterDesc._fields_]
    for (ctype, name), (_, mirror) in zip(fields, _lib.ScatterDesc._fields_):
        want = 4 if ctype == "uint32_t" else 8  # (the one u32; everything else a pointer or u64)
        assert ctypes.sizeof(mirror) == want, (ctype, name)
    assert ctypes.sizeof(_lib.ScatterDesc) == 8 * 22  # 21 8-byte words + one u32 and its padding


def test_package_exports():
    import ebpf_emu
    from ebpf_emu import queues

    assert ebpf_emu.scatter is queues.scatter
    assert ebpf_emu.two_stage is queues.two_stage
    assert ebpf_emu.TwoStageResult is queues.TwoStageResult
    assert queues.SCATTER_TILE == queues.GATHER_TILE


def _desc():
    from ebpf_emu import _lib

    s = _lib.ScatterDesc()
    s.index, s.count, s.total, s.queue, s.cap = P, P, P, 2, 16
    s.src_frames, s.src_bytes, s.src_offsets, s.src_lens = P, 1024, P, P
    s.src_verdict, s.src_status, s.src_r0 = P, P, P
    s.frames, s.stride, s.n = P, 64, 16
    s.verdict, s.status, s.r0 = P, P, P
    return s


def test_invalid_arguments_fail_before_any_device_call(product_lib):
    from ebpf_emu import _lib

    L = product_lib
    assert L.ebpf_scatter(None, None) == _lib.EBPF_EINVAL
    for field in ("index", "count", "src_frames", "src_offsets", "src_lens"):
        s = _desc()
        setattr(s, field, None)
        assert L.ebpf_scatter(ctypes.byref(s), None) == _lib.EBPF_EINVAL, field
    for queue in (_lib.NQUEUES, 8, (1 << 32) - 1):
        s = _desc()
        s.queue = queue
        assert L.ebpf_scatter(ctypes.byref(s), None) == _lib.EBPF_EINVAL, queue
    s = _desc()
    s.stride = 0  # frames with neither offsets nor a stride
    assert L.ebpf_scatter(ctypes.byref(s), None) == _lib.EBPF_EINVAL
    # a workspace below the query's answer: the query answers 0 today, so none is too small --
    # and the check is there (a passed workspace is accepted at any size and never used)
    s = _desc()
    s.cap, s.workspace, s.workspace_bytes = 0, P, 0
    assert L.ebpf_scatter_workspace_bytes(0) == 0
    assert L.ebpf_scatter(ctypes.byref(s), None) == _lib.EBPF_OK


def test_too_big_fails_before_any_device_call(product_lib):
    from ebpf_emu import _lib

    L = product_lib
    for field, value in (("n", 1 << 32), ("cap", 1 << 32), ("src_bytes", (1 << 32) + 1)):
        s = _desc()
        setattr(s, field, value)
        assert L.ebpf_scatter(ctypes.byref(s), None) == _lib.EBPF_ETOOBIG, field


def test_nothing_to_do_is_valid_and_launches_nothing(product_lib):
    """cap == 0, n == 0 and no array to write return 0 without a device (this test has none)."""
    from ebpf_emu import _lib

    L = product_lib
    s = _desc()
    s.cap = 0
    assert L.ebpf_scatter(ctypes.byref(s), None) == _lib.EBPF_OK
    s = _desc()
    s.n = 0
    assert L.ebpf_scatter(ctypes.byref(s), None) == _lib.EBPF_OK
    s = _desc()
    s.frames = None
    s.src_verdict = s.status = s.r0 = None  # no pair is whole: nothing to write
    assert L.ebpf_scatter(ctypes.byref(s), None) == _lib.EBPF_OK
    # results only needs none of the dense packet arrays
    s = _desc()
    s.frames = s.src_frames = s.src_offsets = s.src_lens = None
    s.cap = 0
    assert L.ebpf_scatter(ctypes.byref(s), None) == _lib.EBPF_OK


def test_python_wrapper_checks_its_arguments(product_lib):
    import torch

    from ebpf_emu import queues as Q
    from ebpf_emu.program import BatchResult

    n, m = 8, 4
    index = torch.zeros(n, dtype=torch.int32)
    count = torch.zeros(7, dtype=torch.int32)
    g = Q.GatherResult(frames=torch.zeros(m * 64, dtype=torch.uint8),
                       offsets=torch.zeros(m, dtype=torch.int32),
                       lens=torch.zeros(m, dtype=torch.int16),
                       total=torch.zeros(2, dtype=torch.int32))
    frames = torch.zeros(n * 64, dtype=torch.uint8)
    src = BatchResult(verdict=torch.zeros(m, dtype=torch.uint8))
    dst = BatchResult(verdict=torch.zeros(n, dtype=torch.uint8))
    ok = dict(frames=frames, stride=64, src=src, dst=dst)

    def bad(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            Q.scatter(*a, **kw)

    bad("gathered", None, index, count, 2, **ok)
    bad("queue", g, index, count, 7, **ok)
    bad("queue", g, index, count, -1, **ok)
    bad("int32", g, index.long(), count, 2, **ok)
    bad("int32", g, index, count[:6], 2, **ok)
    bad("layout", g, index, count, 2, frames=frames, src=src, dst=dst)
    bad("contiguous", g, index, count, 2, frames=frames.view(n, 64)[:, :32], stride=64)
    bad("uint8", g, index, count, 2, frames=frames.int(), stride=64)
    bad("gathered.frames", Q.GatherResult(total=g.total), index, count, 2, frames=frames, stride=64)
    bad("src.verdict", g, index, count, 2, src=BatchResult(verdict=torch.zeros(m, dtype=torch.int32)), dst=dst)
    bad("src.r0", g, index, count, 2, src=BatchResult(r0=torch.zeros(m, dtype=torch.int32)),
        dst=BatchResult(r0=torch.zeros(n, dtype=torch.int64)))
    bad("cap", g, index, count, 2, cap=m + 1, **ok)
    bad("cap", g, index, count, 2, cap=-1, **ok)
    bad("n passes", g, index, count, 2, n=n + 1, **ok)
    bad("n passes", g, index, count, 2, frames=frames, stride=64, src=src,
        dst=BatchResult(verdict=torch.zeros(n - 1, dtype=torch.uint8)), n=n)


def test_model_invariants():
    """scatter_ref undoes queues_ref.gather: a gathered queue scattered back over a wiped copy
    restores exactly that queue's packets; results land at the packets' numbers; the bounds cut."""
    rng = np.random.default_rng(7)
    for n in (0, 1, 7, 300):
        v = rng.choice(np.array([0, 1, 2, 3, 0xFE, 0xFF], dtype=np.uint8), n)
        index, count = QR.queues(v)
        lens = rng.choice(np.array([0, 1, 15, 16, 17, 60, 64, 65], dtype=np.uint16), n)
        offs = np.concatenate([[0], np.cumsum(lens.astype(np.int64) + 3)])[:n].astype(np.uint32)
        frames = rng.integers(0, 256, int(offs[-1]) + 80 if n else 1, dtype=np.uint8)
        for queue in (1, 2, 6):
            mine = QR.queue_of(index, count, queue)
            w, end, oo, ol, spans = QR.gather(frames, index, count, queue, offsets=offs, lens=lens,
                                              align=4, out_bytes=1 << 20)
            assert w == len(mine)
            dense = np.zeros(max(end, 1), dtype=np.uint8)
            for o, b in spans:
                dense[o:o + len(b)] = b
            wiped = frames.copy()
            for i in mine:
                wiped[int(offs[i]):int(offs[i]) + int(lens[i])] = 0xEE
            sv = rng.integers(0, 256, w, dtype=np.uint8)
            verdict = np.full(n, 0xA5, dtype=np.uint8)
            done = R.scatter(index, count, queue, n, w, src_frames=dense[:end], src_offsets=oo,
                             src_lens=ol, src_verdict=sv, frames=wiped, offsets=offs, lens=lens,
                             verdict=verdict)
            assert np.array_equal(wiped, frames)
            assert [d for _, d, _ in done] == mine.tolist()
            assert np.array_equal(verdict[mine], sv)
            rest = np.setdiff1d(np.arange(n), mine)
            assert np.all(verdict[rest] == 0xA5)
            # the bounds: cap and total[0] cut the positions, whichever is lower
            for cap, tot in ((w // 2, None), (w, [w // 3, 0]), (w // 3, [w // 2, 0]), (0, None)):
                _, m = R.positions(index, count, queue, n, cap, tot)
                assert m == min(w, cap, tot[0] if tot else w)
