"""ebpf_rss_hash / ebpf_steer without a GPU: the model (tests/rss_ref.py) against the Microsoft RSS
specification's verification vectors, the symmetric key, the default indirection table, the exports
and every validation error of include/ebpf_emu.h (each returned before any device call)."""
import ctypes
import os
import re

import numpy as np

import rss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_reproduces_the_specification_vectors():
    key, vectors = R.msft()
    assert len(key) == 40 and len(vectors) == 8
    seen = 0
    for v in vectors:
        frame = R.flow_frame(v["src"], v["dst"], v["sport"], v["dport"])
        v6 = ":" in v["src"]
        assert R.rss(frame, key, R.ALL) == (int(v["tcp"], 16), R.IPV6_TCP if v6 else R.IPV4_TCP), v
        assert R.rss(frame, key, R.IPV4 | R.IPV6) == (int(v["ip"], 16), R.IPV6 if v6 else R.IPV4), v
        # the input itself, as the specification lays it out
        a = R._addr(v["src"]) + R._addr(v["dst"])
        assert R.toeplitz(key, a) == int(v["ip"], 16)
        assert R.toeplitz(key, a + v["sport"].to_bytes(2, "big") + v["dport"].to_bytes(2, "big")) == \
            int(v["tcp"], 16)
        seen += 2
    assert seen == 16


def test_symmetric_key_ignores_direction():
    _, vectors = R.msft()
    for v in vectors:
        for proto in (6, 17):
            fwd = R.flow_frame(v["src"], v["dst"], v["sport"], v["dport"], proto)
            rev = R.flow_frame(v["dst"], v["src"], v["dport"], v["sport"], proto)
            for types in (R.ALL, R.IPV4 | R.IPV6):
                h, t = R.rss(fwd, R.SYMMETRIC_KEY, types)
                assert t != 0 and h != 0 and (h, t) == R.rss(rev, R.SYMMETRIC_KEY, types)
    key, _ = R.msft()
    v = vectors[0]  # (the specification's key is not symmetric)
    assert R.rss(R.flow_frame(v["src"], v["dst"], v["sport"], v["dport"]), key) != \
        R.rss(R.flow_frame(v["dst"], v["src"], v["dport"], v["sport"]), key)


def test_parser_kinds_take_their_branches():
    key, _ = R.msft()
    want = {"untagged": R.IPV4_TCP, "tag1": R.IPV4_TCP, "tag2": R.IPV4_UDP, "tag3": 0,
            "ihl5": R.IPV4_TCP, "ihl6": R.IPV4_TCP, "ihl15": R.IPV4_UDP, "mf": R.IPV4,
            "fragoff": R.IPV4, "df": R.IPV4_TCP, "tcp": R.IPV4_TCP, "udp": R.IPV4_UDP,
            "icmp": R.IPV4, "badver4": 0, "ihl4": 0, "v6tcp": R.IPV6_TCP, "v6udp": R.IPV6_UDP,
            "v6hbh": R.IPV6, "badver6": 0, "arp": 0}
    kinds = R.parser_kinds()
    assert set(kinds) == set(want)
    for name, frame in kinds.items():
        h, t = R.rss(frame, key)
        assert t == want[name] and (h != 0) == (t != 0), name
    # options move the ports: IHL 6 hashes the bytes 4 further on
    data, _ = R.rss_input(kinds["ihl6"], R.ALL)
    assert data[8:] == kinds["ihl6"][14 + 24:14 + 28]
    # a truncated packet falls back branch by branch
    f = kinds["untagged"]
    assert R.rss(f[:38], key)[1] == R.IPV4_TCP and R.rss(f[:37], key)[1] == R.IPV4
    assert R.rss(f[:34], key)[1] == R.IPV4 and R.rss(f[:33], key)[1] == 0
    assert R.rss(f[:37], key, R.IPV4_TCP) == (0, 0)


def test_default_reta_and_steer_model():
    from ebpf_emu import rss

    for nq in (1, 2, 3, 7, 8, 33, 64):
        table = R.default_reta(nq)
        assert table == [j % nq for j in range(128)] == rss.default_reta(nq)
    rng = np.random.default_rng(3)
    for n in (0, 1, 500):
        keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        for nq in (1, 7, 64):
            index, bounds, q = R.steer(keys, nq)
            assert sorted(index.tolist()) == list(range(n)) and bounds.shape == (nq, 2)
            assert int(bounds[:, 1].sum()) == n
            for k in range(nq):
                s, c = int(bounds[k, 0]), int(bounds[k, 1])
                assert s == int(bounds[:k, 1].sum())
                assert np.array_equal(index[s:s + c], np.flatnonzero(q == k))


def test_exports_constants_and_struct(product_lib):
    import ebpf_emu
    from ebpf_emu import _lib, rss

    for name in ("ebpf_rss_hash", "ebpf_steer_workspace_bytes", "ebpf_steer"):
        assert hasattr(product_lib, name), name
        assert name in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "ebpf_emu.h")).read()
    for name, val in (("IPV4", 1), ("IPV4_TCP", 2), ("IPV4_UDP", 4), ("IPV6", 8), ("IPV6_TCP", 16),
                      ("IPV6_UDP", 32)):
        m = re.search(r"#define\s+EBPF_RSS_%s\s+(\d+)u" % name, hdr)
        assert m and int(m.group(1)) == val == getattr(_lib, "RSS_" + name) == getattr(R, name)
    for name, val in (("QUEUES", 64), ("RETA", 128)):
        m = re.search(r"#define\s+EBPF_STEER_MAX_%s\s+(\d+)" % name, hdr)
        assert m and int(m.group(1)) == val == getattr(_lib, "STEER_MAX_" + name)
    body = re.search(r"typedef struct ebpf_rss_desc \{(.*?)\} ebpf_rss_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*;", body)
    assert names == [f[0] for f in _lib.RssDesc._fields_]
    assert ctypes.sizeof(_lib.RssDesc) == 5 * 8 + 40 + 8 + 2 * 8
    assert product_lib.ebpf_steer_workspace_bytes(1 << 20, 64) > 0
    assert rss.MSFT_KEY == R.msft()[0] and rss.SYMMETRIC_KEY == R.SYMMETRIC_KEY
    assert ebpf_emu.rss_hash is rss.rss_hash and ebpf_emu.steer is rss.steer
    assert ebpf_emu.SteerResult is rss.SteerResult and ebpf_emu.MSFT_KEY == rss.MSFT_KEY
    assert rss.BOUNDS_PAD >= 5


def _desc():
    from ebpf_emu import _lib

    r = _lib.RssDesc()
    p = 0x1000  # (never dereferenced on the host; no call below reaches a device)
    r.frames, r.stride, r.n = p, 64, 16
    r.key[:] = R.msft()[0]
    r.types = R.ALL
    r.hash, r.type = p, p
    return r


def test_rss_hash_invalid_arguments_fail_before_any_device_call(product_lib):
    from ebpf_emu import _lib

    L = product_lib
    assert L.ebpf_rss_hash(None, None) == _lib.EBPF_EINVAL
    for field in ("hash", "frames"):
        r = _desc()
        setattr(r, field, None)
        assert L.ebpf_rss_hash(ctypes.byref(r), None) == _lib.EBPF_EINVAL, field
    r = _desc()
    r.stride = 0  # no packet layout
    assert L.ebpf_rss_hash(ctypes.byref(r), None) == _lib.EBPF_EINVAL
    r = _desc()
    r.stride = 65536  # without lens
    assert L.ebpf_rss_hash(ctypes.byref(r), None) == _lib.EBPF_EINVAL
    for types in (0, 64, R.ALL | 128, 1 << 31):
        r = _desc()
        r.types = types
        assert L.ebpf_rss_hash(ctypes.byref(r), None) == _lib.EBPF_EINVAL, types
    r = _desc()
    r.n = 1 << 32
    assert L.ebpf_rss_hash(ctypes.byref(r), None) == _lib.EBPF_ETOOBIG
    # n == 0 launches nothing: valid without a device, frames may be NULL
    r = _desc()
    r.n, r.frames = 0, None
    assert L.ebpf_rss_hash(ctypes.byref(r), None) == _lib.EBPF_OK


def test_steer_invalid_arguments_fail_before_any_device_call(product_lib):
    from ebpf_emu import _lib

    L = product_lib
    p = 0x1000  # (never dereferenced on the host; no call below reaches a device)
    need = L.ebpf_steer_workspace_bytes(64, 8)

    def table(vals):
        return ctypes.cast((ctypes.c_uint16 * len(vals))(*vals), ctypes.c_void_p)

    for nq in (0, 65, 1 << 16):
        assert L.ebpf_steer(p, 64, nq, None, 0, p, p, None, 0, None) == _lib.EBPF_EINVAL, nq
    for reta_len in (0, 3, 6, 129, 256):
        t = table([0] * max(reta_len, 1))
        assert L.ebpf_steer(p, 64, 8, t, reta_len, p, p, None, 0, None) == _lib.EBPF_EINVAL, reta_len
    assert L.ebpf_steer(p, 64, 8, table([0, 7, 8, 1]), 4, p, p, None, 0, None) == _lib.EBPF_EINVAL
    assert L.ebpf_steer(p, 64, 1, table([1]), 1, p, p, None, 0, None) == _lib.EBPF_EINVAL
    assert L.ebpf_steer(p, 64, 8, None, 0, p, None, None, 0, None) == _lib.EBPF_EINVAL   # bounds
    assert L.ebpf_steer(None, 64, 8, None, 0, p, p, None, 0, None) == _lib.EBPF_EINVAL   # key
    assert L.ebpf_steer(p, 64, 8, None, 0, None, p, None, 0, None) == _lib.EBPF_EINVAL   # index
    assert L.ebpf_steer(None, 0, 8, None, 0, None, None, None, 0, None) == _lib.EBPF_EINVAL
    assert L.ebpf_steer(p, 64, 8, None, 0, p, p, p, need - 1, None) == _lib.EBPF_EINVAL  # too small
    assert L.ebpf_steer(p, 64, 8, None, 0, p, p, p + 4, need, None) == _lib.EBPF_EINVAL  # alignment
    assert L.ebpf_steer(p, 1 << 32, 8, None, 0, p, p, None, 0, None) == _lib.EBPF_ETOOBIG
