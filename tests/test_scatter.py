"""ebpf_scatter on the GPU against the numpy model (tests/scatter_ref.py), exactly: the destination
buffer and every result array are pre-filled with sentinels and compared WHOLE, slack past their
ends included, so every byte and entry the header promises to leave untouched is checked too.
Sizes come from the kernel's constants (ebpf_emu.queues). The last two tests are the chain the
call exists for, checked against the oracle alone: 5-tuple -> PASS queue -> NAT with write-back
-> scatter, through two_stage and through the raw calls."""
import random
import struct
from types import SimpleNamespace

import numpy as np
import pytest

import queues_ref as QR
import scatter_ref as R

pytestmark = pytest.mark.gpu

SENT = 0xA5
SENT64 = 0x5A5A5A5A5A5A5A5A
SLACK = 48  # bytes / entries past every array's end: untouched
LENS = [0, 1, 15, 16, 17, 31, 33, 63, 64, 65, 1500]


def _first_diff(got, exp, tag):
    if not np.array_equal(got, exp):
        d = np.flatnonzero(got != exp)
        raise AssertionError((tag, "first wrong position", int(d[0]), "got", got[d[:4]].tolist(),
                              "expected", exp[d[:4]].tolist(), "wrong", len(d)))


def _u32(a, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(dev)


def _u16(a, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(dev)


def _lens_mix(rng, n):
    return np.array([LENS[rng.randrange(len(LENS))] for _ in range(n)], dtype=np.uint16)


def _layout(kind, lens):
    """The destination batch of len(lens) packets -> (buffer size, layout kwargs as numpy)."""
    n = len(lens)
    if kind == "fixed64":  # no lens: every packet is its 64-byte slot
        return n * 64, dict(stride=64)
    if kind == "stride_lens":  # slots longer than the packets: a slot's tail keeps its sentinel
        return n * 1520, dict(stride=1520, lens=lens)
    offs, pos = [], 0
    for i in range(n):
        if kind == "residues":  # every residue mod 16, with gaps
            pos += (i % 16 - pos) % 16 if i % 3 else (i * 7) % 16
        else:
            assert kind == "abut"  # align 1, no gap: every edge has a neighbour
        offs.append(pos)
        pos += int(lens[i])
    offs = np.array(offs, dtype=np.uint32)
    if kind == "residues" and n >= 64:
        assert len(set((offs % 16).tolist())) == 16
    return pos, dict(offsets=offs, lens=lens)


def _dense(rng, dlens, align, vary=False):
    """The dense side for the queue's packets (dlens: their destination lengths, by position): the
    source tensor is exactly the packets' size (the first packet at byte 0, the last one ending at
    its last byte). vary: every third src_lens[j] is shorter than len(d), every fifth longer."""
    m = len(dlens)
    sl = np.array(dlens, dtype=np.int64)
    if vary:
        j = np.arange(m)
        sl = np.where(j % 3 == 1, sl // 2, np.where(j % 5 == 2, sl + 1 + j % 40, sl))
    offs, pos, end = [], 0, 0
    for j in range(m):
        offs.append(pos)
        end = pos + int(sl[j])
        pos += QR.alignup(int(sl[j]), align)
    nr = np.random.default_rng(rng.randrange(1 << 30))
    return SimpleNamespace(
        frames=nr.integers(0, 256, end, dtype=np.uint8),
        offsets=np.array(offs, dtype=np.uint32), lens=sl.astype(np.uint16),
        verdict=nr.integers(0, 256, m, dtype=np.uint8),
        status=nr.integers(0, 9, m, dtype=np.uint8),
        r0=nr.integers(0, 1 << 63, m, dtype=np.uint64))


def _check(dev, tag, index, count, queue, n, *, size=0, kw=None, src=None, cap=None,
           total="count", results=("verdict", "status", "r0"), shift=0, src_pad=0):
    """One scatter into sentinel-filled device arrays against the model. kw: the destination's
    layout (None: results only); src: _dense's; total: "count" (the queue's own size), None (no
    total) or a number; shift: the verdict / status pointers' address mod 4, both sides; src_pad:
    entries of the dense arrays past cap. -> the model's valid entries."""
    import torch

    from ebpf_emu import queues as Q

    m_all = len(src.lens)
    if cap is None:
        cap = m_all
    tot = None
    if total is not None:
        tot = np.array([int(count[queue]) if total == "count" else total, 12345], dtype=np.uint32)
    # ---- the model, on numpy copies
    e_frames = np.full(size + SLACK, SENT, dtype=np.uint8) if kw is not None else None
    e_res = {"verdict": np.full(n + SLACK, SENT, dtype=np.uint8),
             "status": np.full(n + SLACK, SENT, dtype=np.uint8),
             "r0": np.full(n + SLACK, SENT64, dtype=np.uint64)}
    lay = {k: v for k, v in (kw or {}).items()}
    done = R.scatter(index, count, queue, n, cap, total=tot,
                     src_frames=src.frames if kw is not None else None,
                     src_offsets=src.offsets, src_lens=src.lens,
                     frames=e_frames, **lay,
                     **{"src_" + r: getattr(src, r) for r in results},
                     **{r: e_res[r] for r in results})
    # ---- the device
    def byte_array(init, length):  # a u8 tensor whose pointer is `shift` mod 4, in a larger buffer
        buf = torch.full((length + 8,), SENT, dtype=torch.uint8, device=dev)
        view = buf[shift:shift + length]
        assert view.data_ptr() % 4 == shift
        if init is not None:
            view.copy_(torch.from_numpy(init).to(dev))
        return buf, view

    d_frames = torch.full((size + SLACK,), SENT, dtype=torch.uint8, device=dev) if kw is not None else None
    g = Q.GatherResult(total=_u32(tot, dev) if tot is not None else None)
    if kw is not None:
        g.frames = torch.from_numpy(src.frames).to(dev)
        assert g.frames.numel() == len(src.frames)  # exactly the packets' size
        g.offsets, g.lens = _u32(src.offsets, dev), _u16(src.lens, dev)
    dkw = {}
    if kw is not None:
        dkw = {k: v for k, v in kw.items() if k == "stride"}
        if "offsets" in kw:
            dkw["offsets"] = _u32(kw["offsets"], dev)
        if "lens" in kw:
            dkw["lens"] = _u16(kw["lens"], dev)
    s_ns, d_ns, bufs = SimpleNamespace(), SimpleNamespace(), {}
    for r in results:
        if r == "r0":
            s_ns.r0 = torch.from_numpy(src.r0.view(np.int64)).to(dev)
            bufs[r] = torch.from_numpy(np.full(n + SLACK, SENT64, dtype=np.uint64).view(np.int64)).to(dev)
            d_ns.r0 = bufs[r][:n]
        else:
            _, sv = byte_array(getattr(src, r), m_all)
            setattr(s_ns, r, sv)
            bufs[r], dv = byte_array(None, n + SLACK)
            setattr(d_ns, r, dv[:n])
    Q.scatter(g, _u32(index, dev), _u32(count, dev), queue, frames=d_frames[:size] if kw is not None else None,
              n=n, src=s_ns, dst=d_ns, cap=cap, **dkw)
    torch.cuda.synchronize()
    if kw is not None:
        _first_diff(d_frames.cpu().numpy(), e_frames, tag + " frames")
    for r in ("verdict", "status", "r0"):
        if r not in results:
            continue
        got = bufs[r].cpu().numpy()
        if r == "r0":
            _first_diff(got.view(np.uint64), e_res[r], tag + " r0")
        else:
            assert np.all(got[:shift] == SENT) and np.all(got[shift + n + SLACK:] == SENT), (tag, r)
            _first_diff(got[shift:shift + n + SLACK], e_res[r], tag + " " + r)
    return done


def _verdicts(n, queue_size, queue=2, seed=0):
    """n verdict bytes with exactly queue_size of `queue`, spread; the rest DROP / TX / fault."""
    rng = np.random.default_rng(100 + seed)
    v = rng.choice(np.array([1, 3, 0xFF], dtype=np.uint8), n)
    v[rng.permutation(n)[:queue_size]] = queue
    return v


def _queue_lens(index, count, queue, kw, n):
    mine = QR.queue_of(index, count, queue)
    return [int(kw["lens"][i]) if "lens" in kw else int(kw["stride"]) for i in mine]


def _tile():
    from ebpf_emu import queues as Q

    return Q.SCATTER_TILE


def test_queue_sizes_around_the_tile(cuda):
    """Queue sizes 0, 1, 63, 64, 65, T-1, T, T+1, 4T+1 (T: the kernel's tile), mixed lengths,
    abutting packets."""
    T = _tile()
    rng = random.Random(1)
    for m in (0, 1, 63, 64, 65, T - 1, T, T + 1, 4 * T + 1):
        n = m + m // 3 + 5
        v = _verdicts(n, m, seed=m)
        index, count = QR.queues(v)
        lens = _lens_mix(rng, n)
        size, kw = _layout("abut", lens)
        src = _dense(rng, _queue_lens(index, count, 2, kw, n), 16)
        done = _check(cuda, f"sizes m={m}", index, count, 2, n, size=size, kw=kw, src=src)
        assert len(done) == m


def test_past_the_grid_cap(cuda):
    """More queue positions than one pass of the capped grid: 262,437 packets of 64 bytes."""
    from ebpf_emu import queues as Q

    n = Q.SCATTER_TILE * Q.SCATTER_MAX_WGS + Q.SCATTER_TILE + 37
    assert n == 262437
    v = np.full(n, 2, dtype=np.uint8)
    v[::1001] = 1
    index, count = QR.queues(v)
    m = int(count[2])
    src = _dense(random.Random(2), [64] * m, 16)
    done = _check(cuda, "past the cap", index, count, 2, n, size=n * 64, kw=dict(stride=64), src=src)
    assert len(done) == m > Q.SCATTER_TILE * Q.SCATTER_MAX_WGS


@pytest.mark.parametrize("layout", ["fixed64", "abut", "residues", "stride_lens"])
@pytest.mark.parametrize("align", [1, 4, 16, 64])
def test_layouts_and_source_aligns(cuda, layout, align):
    """Every destination layout against every source align; src_lens shorter and longer than
    len(d) in the same batch (the longer ones copy len(d) bytes and no more); the source tensor
    is exactly the packets' size."""
    rng = random.Random(align * 7 + len(layout))
    n = 700
    lens = _lens_mix(rng, n)
    size, kw = _layout(layout, lens)
    v = _verdicts(n, 520, seed=align)
    index, count = QR.queues(v)
    dl = _queue_lens(index, count, 2, kw, n)
    for vary in (False, True):
        src = _dense(rng, dl, align, vary=vary)
        done = _check(cuda, f"{layout} a={align} vary={vary}", index, count, 2, n, size=size,
                      kw=kw, src=src)
        assert len(done) == 520
        if vary:
            cut = [(j, L) for j, d, L in done if L < int(src.lens[j])]
            assert len(cut) > 50 and all(L == dl[j] for j, L in cut)  # len(d) bytes and no more
            assert sum(1 for j, d, L in done if L < dl[j]) > 50       # and shorter ones


def test_pcap_capture_in_place(cuda):
    """The destination is a capture as it lies in memory (ebpf_pcap_index): the record headers
    between the packets keep their bytes."""
    from ebpf_emu import pcap

    rng = random.Random(4)
    pkts = [bytes(rng.getrandbits(8) for _ in range(rng.choice([16, 48, 64, 128, 1504])))
            for _ in range(300)]
    cap_bytes = np.frombuffer(pcap.to_bytes(pkts), dtype=np.uint8).copy()
    offs, lens, _ = pcap.index(cap_bytes)
    assert np.all(offs % 16 == 8)
    n = len(pkts)
    v = _verdicts(n, 200, seed=4)
    index, count = QR.queues(v)
    kw = dict(offsets=offs, lens=lens)
    src = _dense(rng, _queue_lens(index, count, 2, kw, n), 16)
    done = _check(cuda, "pcap", index, count, 2, n, size=len(cap_bytes), kw=kw, src=src)
    assert len(done) == 200
    # (the model wrote the packets only: what it expects of the headers is the sentinel fill)
    covered = np.zeros(len(cap_bytes), dtype=bool)
    for o, ln in zip(offs, lens):
        covered[int(o):int(o) + int(ln)] = True
    assert (~covered).sum() >= 24 + 16 * n


def test_bounds_total_cap_and_queues(cuda):
    """total[0] below count[queue]; cap below both; no total; queue 0, the last non-empty queue,
    an empty queue (writes nothing)."""
    rng = random.Random(5)
    n = 900
    v = np.random.default_rng(5).choice(np.array([0, 1, 2, 0xFE], dtype=np.uint8), n)  # no TX, no fault
    index, count = QR.queues(v)
    lens = _lens_mix(rng, n)
    size, kw = _layout("abut", lens)
    for queue in (0, 2, 5, 3, 6):
        m = int(count[queue])
        assert (m == 0) == (queue in (3, 6))
        dl = _queue_lens(index, count, queue, kw, n)
        src = _dense(rng, dl if m else [64] * 8, 4)
        room = len(src.lens)
        cases = [("count", None), (None, None)]
        if m:
            cases += [(m - 7, None), (m // 2, m // 3), (m // 3, m // 2), (m + 50, m - 1), (0, None),
                      (None, 1)]
        for total, cap in cases:
            done = _check(cuda, f"bounds q={queue} total={total} cap={cap}", index, count, queue, n,
                          size=size, kw=kw, src=src, total=total, cap=cap)
            want = min(m, room if cap is None else cap, m if total in ("count", None) else total)
            assert len(done) == want, (queue, total, cap, len(done), want)


def test_wrong_index_and_source_span_write_nothing(cuda):
    """One entry with d >= n and one whose source span passes src_bytes: neither writes anything
    (bounds the kernel checks), every other entry is correct."""
    rng = random.Random(6)
    n = 600
    v = _verdicts(n, 400, seed=6)
    index, count = QR.queues(v)
    lens = _lens_mix(rng, n)
    size, kw = _layout("residues", lens)
    src = _dense(rng, _queue_lens(index, count, 2, kw, n), 16)
    start = int(count[:2].sum())
    index = index.copy()
    index[start + 5] = n            # the first number outside the batch
    index[start + 300] = 0xFFFFFFF0
    j = next(j for j in range(100, 300) if src.lens[j] >= 16)
    src.offsets[j] = len(src.frames) - int(src.lens[j]) + 1  # ends one byte past the dense buffer
    done = _check(cuda, "wrong entries", index, count, 2, n, size=size, kw=kw, src=src)
    assert len(done) == 400 - 3 and not {5, 300, j} & {e[0] for e in done}


def test_results_only(cuda):
    """frames == NULL: verdict / status pointers at 1, 2 and 3 mod 4 on both sides, each of the
    three pairs alone and all together, queue sizes around the tile."""
    T = _tile()
    rng = random.Random(8)
    for m in (1, 65, T + 1, 4 * T + 1):
        n = m + m // 2 + 3
        v = _verdicts(n, m, seed=m + 1)
        index, count = QR.queues(v)
        src = _dense(rng, [0] * m, 1)
        for shift in (1, 2, 3):
            done = _check(cuda, f"results m={m} shift={shift}", index, count, 2, n, src=src, shift=shift)
            assert len(done) == m
        for pair in ("verdict", "status", "r0"):
            _check(cuda, f"results m={m} only {pair}", index, count, 2, n, src=src, results=(pair,),
                   shift=0 if pair == "r0" else 3)


# ---------------------------------------------------------------- composition
def _two_stage_packets(rng, n):
    """test_store_mode's NAT frames, three in ten of them made DNS over UDP/IPv4 so the 5-tuple
    drops a good share."""
    from test_store_mode import _nat_packets

    out = []
    for p in _nat_packets(rng, n, long_options=0.3):
        b = bytearray(p)
        l4 = 14 + 4 * (b[14] & 15)
        if rng.random() < 0.3 and l4 + 4 <= len(b):
            b[12:14] = b"\x08\x00"
            b[23] = 17
            b[l4 + 2:l4 + 4] = struct.pack(">H", 53)
        out.append(bytes(b))
    return out


_ORACLE_CHAIN = {}


def _oracle_chain(oracle_mod, layout):
    """The chain by the oracle alone, on the CPU, once per layout -> (input buffer, layout kwargs,
    final buffer, merged verdict / status / r0, first-stage verdicts)."""
    if layout in _ORACLE_CHAIN:
        return _ORACLE_CHAIN[layout]
    from ebpf_emu import workloads as W
    from test_writeback import _expected, _lay

    n = 600
    pkts = _two_stage_packets(random.Random(39), n)
    buf, kw, spans, xdp, _ = _lay(pkts, layout)
    lay = dict(offsets=kw["offsets"], lens=kw["lens"])
    r1, s1, _ = oracle_mod.Program(W.program("5tuple")).run_batch(buf, n, **lay)
    v1 = np.where(s1 != 0, 0xFF, np.where(r1 < 5, r1, 0xFE)).astype(np.uint8)
    nat_buf, _ = _expected(oracle_mod, W.program("nat"), buf, spans, xdp)  # (NAT over every packet)
    r2, s2, _ = oracle_mod.Program(W.program("nat")).run_batch(buf, n, **lay)
    v2 = np.where(s2 != 0, 0xFF, np.where(r2 < 5, r2, 0xFE)).astype(np.uint8)
    passed = v1 == 2
    final = buf.copy()
    changed = 0
    for i, (o, ln) in enumerate(spans):
        if passed[i] and s2[i] == 0:  # NAT's final image bytes [0, len); input bytes elsewhere
            final[o:o + ln] = nat_buf[o:o + ln]
            changed += not np.array_equal(final[o:o + ln], buf[o:o + ln])
    # the test is not vacuous, by the oracle alone
    assert passed.sum() >= n // 8 and (~passed).sum() >= n // 8, (passed.sum(), n)
    assert changed >= n // 8, changed
    merged = dict(verdict=np.where(passed, v2, v1), status=np.where(passed, s2, s1).astype(np.uint8),
                  r0=np.where(passed, r2, r1).astype(np.uint64))
    _ORACLE_CHAIN[layout] = (buf, lay, final, merged, v1)
    return _ORACLE_CHAIN[layout]


def _assert_chain(fr, merged, oracle_chain, tag):
    buf, lay, final, exp, v1 = oracle_chain
    _first_diff(fr.cpu().numpy(), final, tag + " frames")
    assert np.array_equal(merged.verdict.cpu().numpy(), exp["verdict"]), tag
    assert np.array_equal(merged.status.cpu().numpy(), exp["status"]), tag
    assert np.array_equal(merged.r0.cpu().numpy().view(np.uint64), exp["r0"]), tag


@pytest.mark.parametrize("layout", ["offsets16", "packed"])
def test_two_stage_matches_the_oracle(cuda, oracle_mod, layout):
    """5-tuple -> PASS queue -> NAT with write-back -> scatter, through two_stage: the final
    buffer and the merged results equal the ones built from the oracle alone."""
    import torch

    import ebpf_emu
    from ebpf_emu import Program
    from ebpf_emu import workloads as W

    chain = _oracle_chain(oracle_mod, layout)
    buf, lay = chain[0], chain[1]
    first, second = Program(W.program("5tuple")), Program(W.program("nat"))
    fr = torch.from_numpy(buf.copy()).to(cuda)
    res = ebpf_emu.two_stage(first, second, fr, offsets=_u32(lay["offsets"], cuda),
                             lens=_u16(lay["lens"], cuda), writeback=True)
    torch.cuda.synchronize()
    assert res.m == int((chain[4] == 2).sum())
    assert np.array_equal(res.first.verdict.cpu().numpy(), chain[4])
    _assert_chain(fr, res.merged, chain, f"two_stage {layout}")
    # without write-back the packets keep their input bytes; the results are the same
    fr2 = torch.from_numpy(buf.copy()).to(cuda)
    res2 = ebpf_emu.two_stage(first, second, fr2, offsets=_u32(lay["offsets"], cuda),
                              lens=_u16(lay["lens"], cuda))
    torch.cuda.synchronize()
    assert np.array_equal(fr2.cpu().numpy(), buf)
    assert np.array_equal(res2.merged.verdict.cpu().numpy(), chain[3]["verdict"])
    first.close()
    second.close()


def test_raw_calls_match_the_oracle(cuda, oracle_mod):
    """The same chain through the C ABI's descriptors (run, queues, gather, run, scatter)."""
    import ctypes

    import torch

    from ebpf_emu import Program, _lib
    from ebpf_emu import queues as Q
    from ebpf_emu import workloads as W

    chain = _oracle_chain(oracle_mod, "packed")
    buf, lay = chain[0], chain[1]
    n = len(lay["lens"])
    first, second = Program(W.program("5tuple")), Program(W.program("nat"))
    fr = torch.from_numpy(buf.copy()).to(cuda)
    offs, lens = _u32(lay["offsets"], cuda), _u16(lay["lens"], cuda)
    r1 = first.run(fr, n=n, offsets=offs, lens=lens, r0=True, status=True, queues=True)
    g = Q.gather(fr, r1.queue_index, r1.queue_count, 2, offsets=offs, lens=lens, align=16)
    m = int(g.total[0])
    r2 = second.run(g.frames, n=m, offsets=g.offsets, lens=g.lens, r0=True, status=True, writeback=True)
    merged = SimpleNamespace(verdict=r1.verdict.clone(), status=r1.status.clone(), r0=r1.r0.clone())
    s = _lib.ScatterDesc()
    s.index, s.count, s.total = r1.queue_index.data_ptr(), r1.queue_count.data_ptr(), g.total.data_ptr()
    s.queue, s.cap = 2, m
    s.src_frames, s.src_bytes = g.frames.data_ptr(), g.frames.numel()
    s.src_offsets, s.src_lens = g.offsets.data_ptr(), g.lens.data_ptr()
    s.src_verdict, s.src_status, s.src_r0 = r2.verdict.data_ptr(), r2.status.data_ptr(), r2.r0.data_ptr()
    s.frames, s.offsets, s.lens, s.n = fr.data_ptr(), offs.data_ptr(), lens.data_ptr(), n
    s.verdict, s.status, s.r0 = merged.verdict.data_ptr(), merged.status.data_ptr(), merged.r0.data_ptr()
    rc = _lib.lib().ebpf_scatter(ctypes.byref(s), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    _assert_chain(fr, merged, chain, "raw calls")
    first.close()
    second.close()
