"""ebpf_rss_hash on the GPU: the Microsoft RSS specification's known answers, then the Python model
(tests/rss_ref.py), exactly. Every output is pre-filled with a sentinel, so what the header promises
to leave untouched is compared too. Sizes come from the kernel's constants (ebpf_emu.rss)."""
import functools

import numpy as np
import pytest

import rss_ref as R

pytestmark = pytest.mark.gpu

SENT32 = 0x5A5A5A5A
SENT8 = 0xA5
MASKS = [1, 2, 4, 8, 16, 32, R.ALL]


def _run(dev, frames, n, key, types, **kw):
    """rss_hash into sentinel-filled outputs -> (hash u32[n], type u8[n]); nothing past n is
    written."""
    import torch

    from ebpf_emu import rss

    h = torch.full((n + 8,), SENT32, dtype=torch.int32, device=dev)
    t = torch.full((n + 8,), SENT8, dtype=torch.uint8, device=dev)
    lay = {}
    for name, dt in (("offsets", np.int32), ("lens", np.int16)):
        if name in kw:
            lay[name] = torch.from_numpy(kw[name].view(dt)).to(dev)
    if "stride" in kw:
        lay["stride"] = kw["stride"]
    fr = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(frames).to(dev)
    rss.rss_hash(fr, key, types, n=n, hash=h[:n], type=t[:n], **lay)
    torch.cuda.synchronize()
    gh, gt = h.cpu().numpy().view(np.uint32), t.cpu().numpy()
    assert np.all(gh[n:] == SENT32) and np.all(gt[n:] == SENT8), "written past n"
    return gh[:n], gt[:n]


def _same(got, exp, tag, names=None):
    if not np.array_equal(got, exp):
        d = np.flatnonzero(got != exp)
        raise AssertionError((tag, "first wrong packet", int(d[0]), names[d[0]] if names else "",
                              "got", [hex(int(x)) for x in got[d[:4]]],
                              "expected", [hex(int(x)) for x in exp[d[:4]]], "wrong", len(d)))


def test_known_answers(cuda):
    """The specification's 8 flows as Ethernet + IP + TCP frames in 128-byte slots: the "with
    ports" column under every type, the "addresses only" column under the two IP types."""
    key, vectors = R.msft()
    buf = np.zeros((len(vectors), 128), dtype=np.uint8)
    for i, v in enumerate(vectors):
        f = R.flow_frame(v["src"], v["dst"], v["sport"], v["dport"])
        buf[i, :len(f)] = np.frombuffer(f, dtype=np.uint8)
    v6 = np.array([":" in v["src"] for v in vectors])
    gh, gt = _run(cuda, buf.reshape(-1), len(vectors), key, R.ALL, stride=128)
    assert [f"{x:08x}" for x in gh] == [v["tcp"] for v in vectors]
    assert np.array_equal(gt, np.where(v6, R.IPV6_TCP, R.IPV4_TCP))
    gh, gt = _run(cuda, buf.reshape(-1), len(vectors), key, R.IPV4 | R.IPV6, stride=128)
    assert [f"{x:08x}" for x in gh] == [v["ip"] for v in vectors]
    assert np.array_equal(gt, np.where(v6, R.IPV6, R.IPV4))


@functools.lru_cache(maxsize=None)
def _matrix():
    """Every parser kind truncated at every length 0..full: [(name, full frame, length)]."""
    out = []
    for name, frame in R.parser_kinds().items():
        out += [(f"{name}[:{ln}]", frame, ln) for ln in range(len(frame) + 1)]
    return out


@functools.lru_cache(maxsize=None)
def _expected(layout, types):
    """The model's answers for a layout of the matrix, computed once per mask."""
    key, _ = R.msft()
    if layout == "slots":
        pkts = [_slot(f, ln).tobytes() for _, f, ln in _matrix()]
    else:
        pkts = [f[:ln] for _, f, ln in _matrix()]
    return R.rss_batch(pkts, key, types)


def _slot(frame, ln):
    """A 128-byte slot with no length of its own: the truncated frame, then a filler."""
    s = np.full(128, 0xEE, dtype=np.uint8)
    s[:ln] = np.frombuffer(frame[:ln], dtype=np.uint8)
    return s


@pytest.mark.parametrize("layout", ["slots", "slots+lens", "abutting"])
def test_parser_matrix(cuda, layout):
    """slots: 128-byte fixed slots without lens (the packet IS the slot: the truncated frame plus
    a filler). slots+lens: 128-byte slots, the length truncates, and the bytes behind the packet
    continue the untruncated frame, so a read past len changes the answer. abutting: offsets +
    lens, packet after packet with no gap (the bytes behind a packet are the next one's), the
    whole matrix once at every start alignment 0..15."""
    import torch

    key, _ = R.msft()
    mat = _matrix()
    names = [m[0] for m in mat]
    n = len(mat)
    if layout == "slots":
        buf = np.concatenate([_slot(f, ln) for _, f, ln in mat])
        kw = dict(stride=128)
        reps = 1
    elif layout == "slots+lens":
        buf = np.zeros((n, 128), dtype=np.uint8)
        for i, (_, f, _) in enumerate(mat):
            buf[i, :len(f)] = np.frombuffer(f, dtype=np.uint8)
        buf = buf.reshape(-1)
        kw = dict(stride=128, lens=np.array([ln for _, _, ln in mat], dtype=np.uint16))
        reps = 1
    else:
        one = b"".join(f[:ln] for _, f, ln in mat)
        lens1 = np.array([ln for _, _, ln in mat], dtype=np.int64)
        offs1 = np.concatenate([[0], np.cumsum(lens1)[:-1]])
        parts, offs, pos = [], [], 0
        for s in range(16):  # copy s of the matrix starts at s mod 16
            pad = (s - pos) % 16
            parts.append(bytes([0xEE]) * pad + one)
            offs.append(offs1 + pos + pad)
            pos += pad + len(one)
        buf = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
        kw = dict(offsets=np.concatenate(offs).astype(np.uint32),
                  lens=np.tile(lens1, 16).astype(np.uint16))
        reps = 16
        starts = kw["offsets"].reshape(16, n) % 16
        assert all(len(set(starts[:, j].tolist())) == 16 for j in (0, n // 2, n - 1))
        names = names * 16
    fr = torch.from_numpy(buf).to(cuda)  # (exactly the packets' bytes: no slack behind the last)
    for types in MASKS:
        eh, et = _expected("slots" if layout == "slots" else "cut", types)
        gh, gt = _run(cuda, fr, n * reps, key, types, **kw)
        _same(gt, np.tile(et, reps), f"{layout} types={types} type", names)
        _same(gh, np.tile(eh, reps), f"{layout} types={types} hash", names)
    if layout != "slots":  # the matrix reaches every outcome
        _, et = _expected("cut", R.ALL)
        assert set(et.tolist()) == {0, 1, 2, 4, 8, 16, 32}


def _distinct_packets(count):
    """`count` distinct 64-byte packets of every family (IPv6 ones cut at 64 bytes keep their
    ports), and the model's answers."""
    rng = np.random.default_rng(41)
    pk = []
    for i in range(count):
        a = rng.integers(0, 256, 40, dtype=np.uint8)
        sp, dp = (int(x) for x in rng.integers(1, 65536, 2))
        v4 = (".".join(str(x) for x in a[0:4]), ".".join(str(x) for x in a[4:8]))
        v6 = (":".join(f"{a[8 + 2 * j]:02x}{a[9 + 2 * j]:02x}" for j in range(8)),
              ":".join(f"{a[24 + 2 * j]:02x}{a[25 + 2 * j]:02x}" for j in range(8)))
        kind = i % 8
        if kind < 3:
            f = R.flow_frame(*v4, sp, dp, 6 if kind else 17)
        elif kind < 5:
            f = R.flow_frame(*v6, sp, dp, 6 if kind == 3 else 17)
        elif kind == 5:
            f = R.flow_frame(*v4, sp, dp, 6, tags=(0x8100,))
        elif kind == 6:
            f = R.eth(0x0800) + R.ipv4(*v4, 1, R.l4(sp, dp))
        else:
            f = R.eth(0x0806) + bytes(a[:28])
        pk.append((f + bytes(64))[:64])
    key, _ = R.msft()
    eh, et = R.rss_batch(pk, key, R.ALL)
    assert len(set(eh.tolist())) > count * 3 // 4 and set(et.tolist()) == {0, 1, 2, 4, 16, 32}
    return np.frombuffer(b"".join(pk), dtype=np.uint8).reshape(count, 64).copy(), eh, et


def test_sizes(cuda):
    """n around a wave, a workgroup's pass and one packet past a full pass of the capped grid:
    a few hundred distinct 64-byte packets tiled on the device."""
    import torch

    from ebpf_emu import rss

    key, _ = R.msft()
    base, eh, et = _distinct_packets(300)
    dbase = torch.from_numpy(base).to(cuda)
    blk = rss.RSS_BLOCK
    for n in (0, 1, 63, 64, 65, blk - 1, blk, blk + 1, blk * rss.RSS_MAX_WGS + 1):
        sel = torch.arange(n, device=cuda) % len(base)
        fr = dbase[sel].reshape(-1)
        if n == 0:
            fr = dbase.reshape(-1)
        gh, gt = _run(cuda, fr, n, key, R.ALL, stride=64)
        tile = np.arange(n) % len(base)
        _same(gt, et[tile], f"n={n} type")
        _same(gh, eh[tile], f"n={n} hash")
