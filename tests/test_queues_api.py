"""ebpf_verdict_queues / ebpf_gather without a GPU: the exports, every validation error of
include/ebpf_emu.h (each returned before any device call), and the numpy model's own invariants
(tests/queues_ref.py is what tests/test_queues.py compares the kernels with)."""
import ctypes
import os
import re

import numpy as np
import pytest

import queues_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_and_constants(product_lib):
    from ebpf_emu import _lib

    for name in ("ebpf_queues_workspace_bytes", "ebpf_verdict_queues",
                 "ebpf_gather_workspace_bytes", "ebpf_gather"):
        assert hasattr(product_lib, name), name
        assert name in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "ebpf_emu.h")).read()
    m = re.search(r"#define\s+EBPF_NQUEUES\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 7 == _lib.NQUEUES == R.NQUEUES
    assert product_lib.ebpf_queues_workspace_bytes(1 << 20) > 0
    assert product_lib.ebpf_gather_workspace_bytes(1 << 20) > 0


def test_struct_matches_header():
    """The ctypes mirror has the header's fields, in its order."""
    from ebpf_emu import _lib

    hdr = open(os.path.join(ROOT, "include", "ebpf_emu.h")).read()
    body = re.search(r"typedef struct ebpf_gather_desc \{(.*?)\} ebpf_gather_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*;", body)
    assert names == [f[0] for f in _lib.GatherDesc._fields_]
    assert ctypes.sizeof(_lib.GatherDesc) == 8 * 16 - 8  # 14 8-byte words + two u32


def test_package_exports():
    import ebpf_emu
    from ebpf_emu import queues

    assert ebpf_emu.verdict_queues is queues.verdict_queues
    assert ebpf_emu.gather is queues.gather
    assert ebpf_emu.GatherResult is queues.GatherResult


def test_queues_invalid_arguments_fail_before_any_device_call(product_lib):
    from ebpf_emu import _lib

    L = product_lib
    p = 0x1000  # (never dereferenced on the host; no call below reaches a device)
    need = L.ebpf_queues_workspace_bytes(64)
    assert L.ebpf_verdict_queues(None, 64, p, p, None, 0, None) == _lib.EBPF_EINVAL
    assert L.ebpf_verdict_queues(p, 64, None, p, None, 0, None) == _lib.EBPF_EINVAL
    assert L.ebpf_verdict_queues(p, 64, p, None, None, 0, None) == _lib.EBPF_EINVAL
    assert L.ebpf_verdict_queues(p, (1 << 32), p, p, None, 0, None) == _lib.EBPF_ETOOBIG
    assert L.ebpf_verdict_queues(p, 64, p, p, p, need - 1, None) == _lib.EBPF_EINVAL


def _desc():
    from ebpf_emu import _lib

    g = _lib.GatherDesc()
    p = 0x1000
    g.frames, g.stride, g.n = p, 64, 16
    g.index, g.count, g.queue, g.align = p, p, 2, 16
    g.out_frames, g.out_bytes = p, 1024
    g.out_offsets, g.out_lens, g.out_total = p, p, p
    return g


def test_gather_invalid_arguments_fail_before_any_device_call(product_lib):
    from ebpf_emu import _lib

    L = product_lib
    assert L.ebpf_gather(None, None) == _lib.EBPF_EINVAL
    for field in ("frames", "index", "count", "out_frames", "out_offsets", "out_lens", "out_total"):
        g = _desc()
        setattr(g, field, None)
        assert L.ebpf_gather(ctypes.byref(g), None) == _lib.EBPF_EINVAL, field
    g = _desc()
    g.queue = _lib.NQUEUES
    assert L.ebpf_gather(ctypes.byref(g), None) == _lib.EBPF_EINVAL
    for align in (0, 3, 24, 512, 1 << 31):
        g = _desc()
        g.align = align
        assert L.ebpf_gather(ctypes.byref(g), None) == _lib.EBPF_EINVAL, align
    g = _desc()
    g.out_bytes = (1 << 32) + 1
    assert L.ebpf_gather(ctypes.byref(g), None) == _lib.EBPF_ETOOBIG
    g = _desc()
    g.stride = 0  # no packet layout
    assert L.ebpf_gather(ctypes.byref(g), None) == _lib.EBPF_EINVAL
    g = _desc()
    g.workspace, g.workspace_bytes = 0x1000, L.ebpf_gather_workspace_bytes(16) - 1
    assert L.ebpf_gather(ctypes.byref(g), None) == _lib.EBPF_EINVAL


def test_run_queues_requires_verdict(product_lib):
    import torch

    from ebpf_emu import Program
    from ebpf_emu import workloads as W

    p = Program(W.program("5tuple"))
    with pytest.raises(ValueError, match="verdict"):
        p.run(torch.zeros(128, dtype=torch.uint8), n=2, stride=64, verdict=False, queues=True)
    p.close()


def test_model_invariants():
    rng = np.random.default_rng(5)
    for n in (0, 1, 7, 300, 5000):
        v = rng.choice(np.array([0, 1, 2, 3, 4, 5, 77, 0xFD, 0xFE, 0xFF], dtype=np.uint8), n)
        index, count = R.queues(v)
        assert int(count.sum()) == n and len(count) == 7
        assert sorted(index.tolist()) == list(range(n))
        q = R.classes(v)
        for c in range(7):
            mine = R.queue_of(index, count, c)
            assert np.all(np.diff(mine.astype(np.int64)) > 0)          # ascending: stable
            assert np.array_equal(mine, np.flatnonzero(q == c))
        assert int(count[5]) == int(((v >= 5) & (v != 0xFF)).sum())
        # gather: offsets follow the formula, the written packets are a prefix
        lens = rng.choice(np.array([0, 1, 15, 16, 17, 60, 64, 65], dtype=np.uint16), n)
        offs = np.concatenate([[0], np.cumsum(lens.astype(np.int64) + 3)])[:n].astype(np.uint32)
        frames = rng.integers(0, 256, int(offs[-1]) + 80 if n else 1, dtype=np.uint8)
        for align in (1, 4, 16, 64):
            for c in (1, 2):
                src = R.queue_of(index, count, c)
                full = sum(R.alignup(int(lens[i]), align) for i in src)
                for out_bytes in (0, full // 2, full):
                    w, end, oo, ol, spans = R.gather(frames, index, count, c, offsets=offs,
                                                     lens=lens, align=align, out_bytes=out_bytes)
                    assert w <= len(src) and (out_bytes < full or w == len(src))
                    acc = 0
                    for j in range(w):
                        assert oo[j] == acc and oo[j] % align == 0 and ol[j] == lens[src[j]]
                        assert oo[j] + ol[j] <= out_bytes
                        acc += R.alignup(int(ol[j]), align)
                    if w < len(src):
                        assert acc + int(lens[src[w]]) > out_bytes
                    assert end == (int(oo[-1]) + int(ol[-1]) if w else 0)
