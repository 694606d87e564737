"""ebpf_csum_verify / ebpf_csum_fill: the C ABI surface without a GPU. The symbols, the constants
and the descriptor against include/ebpf_emu.h, and every invalid argument refused before any
device call (no call below reaches a device: this machine may have none)."""
import ctypes
import os
import re

import pytest

import csum_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ebpf_csum_verify", "ebpf_csum_fill")


def test_exports_constants_and_struct(product_lib):
    import ebpf_emu
    from ebpf_emu import _lib, csum

    for name in CALLS:
        assert hasattr(product_lib, name), name
        assert name in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "ebpf_emu.h")).read()
    for name, val in (("IPV4_HDR", 1), ("TCP", 2), ("UDP", 4), ("L3_GOOD", 1), ("L3_BAD", 2),
                      ("L4_GOOD", 4), ("L4_BAD", 8), ("L4_NONE", 16)):
        m = re.search(r"#define\s+EBPF_CSUM_%s\s+(\d+)u" % name, hdr)
        assert m and int(m.group(1)) == val == getattr(_lib, "CSUM_" + name) == getattr(C, name)
    assert _lib.CSUM_ALL == C.ALL == 7 and _lib.NQUEUES == C.NQUEUES
    body = re.search(r"typedef struct ebpf_csum_desc \{(.*?)\} ebpf_csum_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*;", body)
    assert names == [f[0] for f in _lib.CsumDesc._fields_]
    assert ctypes.sizeof(_lib.CsumDesc) == 9 * 8
    assert ebpf_emu.csum_verify is csum.csum_verify and ebpf_emu.csum_fill is csum.csum_fill
    assert csum.CSUM_BLOCK % 64 == 0 and csum.CSUM_MAX_WGS >= 1
    launch = open(os.path.join(ROOT, "ebpf-emu_amd", "csrc", "launch.h")).read()
    assert int(re.search(r"kCsBlock = (\d+);", launch).group(1)) == csum.CSUM_BLOCK
    assert int(re.search(r"kCsMaxWgs = (\d+);", launch).group(1)) == csum.CSUM_MAX_WGS


def _desc():
    from ebpf_emu import _lib

    c = _lib.CsumDesc()
    p = 0x1000  # (never dereferenced on the host; no call below reaches a device)
    c.frames, c.stride, c.n = p, 64, 16
    c.what = C.ALL
    c.verdict, c.queue_mask = p, 0x7F
    c.status = p
    return c


@pytest.mark.parametrize("call", CALLS)
def test_invalid_arguments_fail_before_any_device_call(product_lib, call):
    from ebpf_emu import _lib

    fn = getattr(product_lib, call)
    assert fn(None, None) == _lib.EBPF_EINVAL
    c = _desc()
    c.frames = None
    assert fn(ctypes.byref(c), None) == _lib.EBPF_EINVAL
    c = _desc()
    c.stride = 0  # no packet layout
    assert fn(ctypes.byref(c), None) == _lib.EBPF_EINVAL
    c = _desc()
    c.stride = 65536  # without lens
    assert fn(ctypes.byref(c), None) == _lib.EBPF_EINVAL
    for what in (0, 8, C.ALL | 16, 1 << 31):
        c = _desc()
        c.what = what
        assert fn(ctypes.byref(c), None) == _lib.EBPF_EINVAL, what
    for mask in (1 << C.NQUEUES, 0x7F | (1 << 8), 1 << 31):
        c = _desc()
        c.queue_mask = mask
        assert fn(ctypes.byref(c), None) == _lib.EBPF_EINVAL, mask
        c.verdict = None
        assert fn(ctypes.byref(c), None) == _lib.EBPF_EINVAL, mask
    c = _desc()
    c.n = 1 << 32
    assert fn(ctypes.byref(c), None) == _lib.EBPF_ETOOBIG
    # n == 0 launches nothing: valid without a device, frames may be NULL
    c = _desc()
    c.n, c.frames = 0, None
    assert fn(ctypes.byref(c), None) == _lib.EBPF_OK


def test_status_is_required_by_verify_only(product_lib):
    from ebpf_emu import _lib

    c = _desc()
    c.status = None
    assert product_lib.ebpf_csum_verify(ctypes.byref(c), None) == _lib.EBPF_EINVAL
    c.n = 0  # (still refused: the check comes before the empty batch)
    assert product_lib.ebpf_csum_verify(ctypes.byref(c), None) == _lib.EBPF_EINVAL
    assert product_lib.ebpf_csum_fill(ctypes.byref(c), None) == _lib.EBPF_OK  # n == 0, no status


def test_wrongly_typed_tensors_are_refused_before_any_call():
    """offsets / lens / verdict / status of another dtype, a strided view or another length would be
    read by the kernel as something they are not: ValueError, with no library call (CPU tensors)."""
    import torch

    from ebpf_emu import csum

    fr = torch.zeros(4 * 64, dtype=torch.uint8)
    offs = torch.arange(4, dtype=torch.int32) * 64
    lens = torch.full((4,), 64, dtype=torch.int16)
    bad = [dict(offsets=offs.to(torch.int64), lens=lens), dict(offsets=offs, lens=lens.to(torch.int32)),
           dict(offsets=torch.arange(8, dtype=torch.int32)[::2], lens=lens),
           dict(offsets=offs, lens=torch.zeros(8, dtype=torch.int16)[::2]),
           dict(offsets=offs, lens=lens, n=5), dict(stride=0),
           dict(stride=64, verdict=torch.zeros(4, dtype=torch.int8)),
           dict(stride=64, verdict=torch.zeros(3, dtype=torch.uint8)),
           dict(stride=64, status=torch.zeros(4, dtype=torch.int32)),
           dict(stride=64, status=torch.zeros(3, dtype=torch.uint8))]
    for fn in (csum.csum_verify, csum.csum_fill):
        for kw in bad:
            with pytest.raises(ValueError):
                fn(fr, **kw)
        with pytest.raises(ValueError):
            fn(fr.to(torch.int8), stride=64)
        # n == 0 is valid and calls nothing
        assert fn(fr, stride=64, n=0).numel() == 0
