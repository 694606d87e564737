"""ebpf_verdict_queues / ebpf_gather on the GPU against the numpy model (tests/queues_ref.py),
exactly: every output is pre-filled with a sentinel, so the entries and bytes the header promises
to leave untouched are compared too. Sizes come from the kernels' constants (ebpf_emu.queues)."""
import random

import numpy as np
import pytest

import queues_ref as R

pytestmark = pytest.mark.gpu

SENT = 0xA5
SENT32 = 0x5A5A5A5A
SENT16 = 0x5A5A
LENS = [0, 1, 15, 16, 17, 60, 64, 65, 1500, 1514]
ALIGNS = [1, 4, 16, 64, 256]
PATTERNS = ["one_class", "random7", "absent", "period2", "period65", "other_bytes"]


def _sizes():
    from ebpf_emu import queues as Q

    rng = Q.QUEUES_RANGE  # one workgroup's range; its waves take a quarter each
    return [0, 1, 63, 64, 65, rng // 4 + 1, rng - 1, rng, rng + 1, 2 * rng + 1,
            rng * Q.QUEUES_MAX_WGS + rng + 65]  # the last: past a full pass of the capped grid


def _pattern(name, n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    i = np.arange(n)
    if name == "one_class":
        return np.full(n, 2, dtype=np.uint8)
    if name == "random7":
        return rng.choice(np.array([0, 1, 2, 3, 4, 0xFE, 0xFF], dtype=np.uint8), n)
    if name == "absent":  # no TX, no fault
        return rng.choice(np.array([0, 1, 2, 4, 0xFE], dtype=np.uint8), n)
    if name == "period2":
        return np.where(i % 2 == 0, 1, 2).astype(np.uint8)
    if name == "period65":  # runs of 65: class runs straddle wave and workgroup edges
        return np.where((i // 65) % 2 == 0, 3, 0xFF).astype(np.uint8)
    if name == "other_bytes":
        return rng.choice(np.array([1, 2, 5, 6, 0x7F, 0xFD, 0xFE, 0xFF], dtype=np.uint8), n)
    raise KeyError(name)


def _first_diff(got, exp, tag):
    if not np.array_equal(got, exp):
        d = np.flatnonzero(got != exp)
        raise AssertionError((tag, "first wrong position", int(d[0]), "got", got[d[:4]].tolist(),
                              "expected", exp[d[:4]].tolist(), "wrong", len(d)))


def _dev_queues(v_dev, n):
    """verdict_queues into sentinel-filled outputs -> (index u32[n + 8] numpy, count u32[7] numpy,
    index tensor, count tensor)."""
    import torch

    from ebpf_emu import queues as Q

    idx = torch.full((n + 8,), SENT32, dtype=torch.int32, device=v_dev.device)
    cnt = torch.full((7,), SENT32, dtype=torch.int32, device=v_dev.device)
    Q.verdict_queues(v_dev, index=idx[:n], count=cnt)
    torch.cuda.synchronize()
    return idx.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32), idx[:n], cnt


def _check_queues(v, v_dev, tag):
    n = len(v)
    gi, gc, ti, tc = _dev_queues(v_dev, n)
    ei, ec = R.queues(v)
    assert np.array_equal(gc, ec), (tag, gc.tolist(), ec.tolist())
    _first_diff(gi[:n], ei, tag)
    assert np.all(gi[n:] == SENT32), (tag, "index written past n")
    return ti, tc, ei, ec


@pytest.mark.parametrize("pattern", PATTERNS)
def test_queues_match_the_model(cuda, pattern):
    import torch

    for n in _sizes():
        v = _pattern(pattern, n, n % 97)
        _check_queues(v, torch.from_numpy(v).to(cuda), f"{pattern} n={n}")


@pytest.mark.parametrize("pattern", ["random7", "period65"])
def test_queues_misaligned_verdicts(cuda, pattern):
    """A verdict pointer at odd addresses: the wide loads at every misalignment."""
    import torch

    from ebpf_emu import queues as Q

    for shift in (1, 2, 3):
        for n in (1, 3, 65, Q.QUEUES_RANGE + 1, 2 * Q.QUEUES_RANGE + 7):
            v = _pattern(pattern, n, shift)
            buf = torch.full((n + shift + 5,), 3, dtype=torch.uint8, device=cuda)
            buf[shift:shift + n] = torch.from_numpy(v).to(cuda)
            vd = buf[shift:shift + n]
            assert vd.data_ptr() % 4 == shift
            _check_queues(v, vd, f"{pattern} n={n} shift={shift}")


FAULTY = """
    ldxb r3, [r1+0]
    and r3, 3
    lsh r3, 4
    add r3, r1
    ldxb r4, [r3+1000]
    ldxb r0, [r1+1]
    and r0, 7
    exit
"""


@pytest.mark.parametrize("name", ["5tuple", "faulty"])
def test_queues_match_counters_and_oracle(cuda, oracle_mod, name):
    import torch

    from ebpf_emu import Program
    from ebpf_emu import workloads as W
    from ebpf_emu.asm import assemble

    n = 4096 + 17
    buf = W.frames_fixed(n, 64, 3)
    img = W.program("5tuple") if name == "5tuple" else assemble(FAULTY)
    prog = Program(img)
    cnt = torch.zeros(8, dtype=torch.int64, device=cuda)
    res = prog.run(torch.from_numpy(buf).to(cuda), n=n, stride=64, counters=cnt, queues=True)
    torch.cuda.synchronize()
    r0, st, ocnt = oracle_mod.Program(img).run_batch(buf, n, stride=64, threads=4)
    ov = np.where(st != 0, 0xFF, np.where(r0 < 5, r0, 0xFE)).astype(np.uint8)
    if name == "faulty":
        assert (st != 0).sum() >= n // 8 and (ov == 0xFE).sum() >= n // 8
    qc = res.queue_count.cpu().numpy().view(np.uint32)
    qi = res.queue_index.cpu().numpy().view(np.uint32)
    assert np.array_equal(qc.astype(np.uint64), cnt.cpu().numpy().view(np.uint64)[:7])
    assert np.array_equal(qc.astype(np.uint64), ocnt[:7])
    oq = R.classes(ov)
    for q in range(7):
        assert np.array_equal(R.queue_of(qi, qc, q), np.flatnonzero(oq == q)), q
    prog.close()


# ---------------------------------------------------------------- gather
def _dev_layout(kw, dev):
    import torch

    out = {k: v for k, v in kw.items() if k == "stride"}
    if "offsets" in kw:
        out["offsets"] = torch.from_numpy(kw["offsets"].view(np.int32)).to(dev)
    if "lens" in kw:
        out["lens"] = torch.from_numpy(kw["lens"].view(np.int16)).to(dev)
    return out


def _check_gather(dev, frames, kw, v, queue, align, out_bytes, tag, fr_dev=None, qs=None):
    """One gather into sentinel-filled outputs against the model; -> packets written."""
    import torch

    from ebpf_emu import queues as Q

    n = len(v)
    if fr_dev is None:
        fr_dev = torch.from_numpy(frames).to(dev)
    ti, tc, ei, ec = qs if qs is not None else _check_queues(v, torch.from_numpy(v).to(dev), tag)
    slack = 272  # (past out_bytes: untouched)
    out = Q.GatherResult(frames=torch.full((out_bytes + slack,), SENT, dtype=torch.uint8, device=dev),
                         offsets=torch.full((n + 4,), SENT32, dtype=torch.int32, device=dev),
                         lens=torch.full((n + 4,), SENT16, dtype=torch.int16, device=dev),
                         total=torch.full((2,), SENT32, dtype=torch.int32, device=dev))
    Q.gather(fr_dev, ti, tc, queue, align=align, out_bytes=out_bytes, n=n, out=out,
             **_dev_layout(kw, dev))
    torch.cuda.synchronize()
    w, end, eo, el, spans = R.gather(frames, ei, ec, queue, align=align, out_bytes=out_bytes, **kw)
    total = out.total.cpu().numpy().view(np.uint32)
    assert total.tolist() == [w, end], (tag, total.tolist(), [w, end])
    go = out.offsets.cpu().numpy().view(np.uint32)
    gl = out.lens.cpu().numpy().view(np.uint16)
    _first_diff(go[:w], eo, tag + " offsets")
    _first_diff(gl[:w], el, tag + " lens")
    assert np.all(go[w:] == SENT32) and np.all(gl[w:] == SENT16), (tag, "entries past the prefix")
    gf = out.frames.cpu().numpy()
    exp, known = R.expected_frames(out_bytes + slack, out_bytes, SENT, align, end, spans)
    if not np.array_equal(gf[known], exp[known]):
        d = np.flatnonzero(known & (gf != exp))
        raise AssertionError((tag, "first wrong byte", int(d[0]), "got", gf[d[:4]].tolist(),
                              "expected", exp[d[:4]].tolist(), "wrong", len(d),
                              "untouched" if d[0] >= R.alignup(end, align) else "packet"))
    return w, (ti, tc, ei, ec)


def _full_bytes(kw, v, queue, align, n):
    q = R.classes(v)
    lens = kw["lens"] if "lens" in kw else np.full(n, kw["stride"])
    return int(sum(R.alignup(int(lens[i]), align) for i in np.flatnonzero(q == queue)))


def _var_batch(rng, n, exact=False):
    """Offsets + lens: lengths from LENS, source offsets at every residue mod 16; exact: the first
    packet at byte 0 and the last ending at the buffer's last byte."""
    lens = np.array([LENS[rng.randrange(len(LENS))] for _ in range(n)], dtype=np.uint16)
    if exact:
        lens[0], lens[-1] = 17, 65
    offs, pos = [], 0
    for i in range(n):
        if not (exact and i == 0):
            pos += (i % 16 - pos) % 16 if i % 3 else (i * 7) % 16  # residues 0..15, and gaps
        if exact and i == n - 1:
            pos += (5 - pos) % 16
        offs.append(pos)
        pos += int(lens[i])
    size = pos if exact else pos + 40
    frames = np.random.default_rng(n).integers(0, 256, size, dtype=np.uint8)
    offs = np.array(offs, dtype=np.uint32)
    assert len(set((offs % 16).tolist())) == 16
    return frames, dict(offsets=offs, lens=lens)


@pytest.mark.parametrize("align", ALIGNS)
def test_gather_fixed_slots(cuda, align):
    n = 600
    frames = np.random.default_rng(2).integers(0, 256, n * 64, dtype=np.uint8)
    v = _pattern("random7", n)
    kw = dict(stride=64)
    qs = None
    for queue in (2, 6):
        full = _full_bytes(kw, v, queue, align, n)
        w, qs = _check_gather(cuda, frames, kw, v, queue, align, full, f"fixed64 a={align} q={queue}", qs=qs)
        assert w == int((R.classes(v) == queue).sum()) and w > 50


@pytest.mark.parametrize("align", ALIGNS)
def test_gather_offsets_lens(cuda, align):
    n = 700
    frames, kw = _var_batch(random.Random(align), n)
    v = _pattern("random7", n, 3)
    full = _full_bytes(kw, v, 2, align, n)
    w, qs = _check_gather(cuda, frames, kw, v, 2, align, full, f"var a={align}")
    assert w == int((v == 2).sum())
    # a stride layout with lens (len = lens[i] inside fixed slots)
    kw2 = dict(stride=1520, lens=kw["lens"])
    fr2 = np.random.default_rng(9).integers(0, 256, n * 1520, dtype=np.uint8)
    _check_gather(cuda, fr2, kw2, v, 1, align, _full_bytes(kw2, v, 1, align, n),
                  f"stride+lens a={align}", qs=qs)


@pytest.mark.parametrize("align", [1, 16])
def test_gather_exact_allocation(cuda, align):
    """The first packet begins at byte 0 of the source tensor and the last ends at its last byte:
    a read outside the packets' own 16-byte blocks would leave the tensor."""
    n = 300
    frames, kw = _var_batch(random.Random(77), n, exact=True)
    assert kw["offsets"][0] == 0 and int(kw["offsets"][-1]) + int(kw["lens"][-1]) == len(frames)
    v = np.full(n, 2, dtype=np.uint8)
    w, _ = _check_gather(cuda, frames, kw, v, 2, align, _full_bytes(kw, v, 2, align, n), f"exact a={align}")
    assert w == n


def test_gather_pcap_layout(cuda):
    """A capture as it lies in memory (ebpf_pcap_index): packets at 8 mod 16."""
    from ebpf_emu import pcap

    rng = random.Random(4)
    pkts = [bytes(rng.getrandbits(8) for _ in range(rng.choice([16, 48, 64, 128, 1504])))
            for _ in range(300)]
    cap = np.frombuffer(pcap.to_bytes(pkts), dtype=np.uint8).copy()
    offs, lens, _ = pcap.index(cap)
    assert np.all(offs % 16 == 8)
    v = _pattern("random7", len(pkts), 8)
    kw = dict(offsets=offs, lens=lens)
    for align in (16, 1):
        w, _ = _check_gather(cuda, cap, kw, v, 2, align, _full_bytes(kw, v, 2, align, len(pkts)), f"pcap a={align}")
        assert w == int((v == 2).sum())


def test_gather_empty_and_whole_queue(cuda):
    n = 520
    frames, kw = _var_batch(random.Random(5), n)
    v = _pattern("absent", n, 1)
    w, _ = _check_gather(cuda, frames, kw, v, 3, 16, 4096, "empty queue")   # no TX in the pattern
    assert w == 0
    w, _ = _check_gather(cuda, frames, kw, v, 6, 1, 0, "empty queue, no output bytes")
    assert w == 0
    v = np.full(n, 1, dtype=np.uint8)
    for align in (1, 16):
        w, _ = _check_gather(cuda, frames, kw, v, 1, align, _full_bytes(kw, v, 1, align, n), f"whole a={align}")
        assert w == n
    # n == 0: nothing but the totals
    e = np.zeros(0, dtype=np.uint8)
    _check_gather(cuda, np.zeros(16, dtype=np.uint8), dict(stride=64), e, 2, 16, 64, "n=0")


@pytest.mark.parametrize("align", [1, 4, 16, 64])
def test_gather_capacity_cuts(cuda, align):
    """out_bytes at a packet's end, one byte short of it, inside the first packet, 0."""
    n = 600
    frames, kw = _var_batch(random.Random(11 + align), n)
    kw["lens"][0] = 60  # (the queue's first packet has bytes to cut into)
    v = np.full(n, 2, dtype=np.uint8)
    v[1::7] = 1
    ei, ec = R.queues(v)
    _, _, eo, el, _ = R.gather(frames, ei, ec, 2, align=align, out_bytes=1 << 30, **kw)
    k = next(j for j in range(300, len(eo)) if el[j] not in (0, 16, 64))  # a packet with a tail
    at = int(eo[k]) + int(el[k])
    qs = None
    for out_bytes, want in ((at, k + 1), (at - 1, k), (int(el[0]) - 1, 0), (0, 0)):
        w, qs = _check_gather(cuda, frames, kw, v, 2, align, out_bytes, f"cut a={align} out={out_bytes}", qs=qs)
        assert w == want, (out_bytes, w, want)


def test_gather_past_the_grid_cap(cuda):
    """More queue positions than one pass of the capped grid: workgroups take several tiles."""
    from ebpf_emu import queues as Q

    n = Q.GATHER_TILE * Q.GATHER_MAX_WGS + Q.GATHER_TILE + 37
    frames = np.random.default_rng(6).integers(0, 256, n * 16, dtype=np.uint8)
    lens = np.where(np.arange(n) % 5 == 0, 9, 16).astype(np.uint16)
    kw = dict(stride=16, lens=lens)
    v = np.full(n, 2, dtype=np.uint8)
    v[::1001] = 1
    w, _ = _check_gather(cuda, frames, kw, v, 2, 4, _full_bytes(kw, v, 2, 4, n), "past the cap")
    assert w == int((v == 2).sum())


# ---------------------------------------------------------------- composition
def test_nat_writeback_then_gather(cuda, oracle_mod):
    """NAT rewrites in place; the gathered queues hold the oracle's final image bytes [0, len)."""
    import torch

    from ebpf_emu import Program
    from ebpf_emu import workloads as W
    from test_store_mode import _nat_packets
    from test_writeback import _dev_kw, _expected, _lay

    img = W.program("nat")
    n = 300
    pkts = _nat_packets(random.Random(31), n, long_options=0.3)
    buf, kw, spans, xdp, _ = _lay(pkts, "offsets16")
    exp, sts = _expected(oracle_mod, img, buf, spans, xdp)
    assert not np.array_equal(exp, buf)
    r0, st, _ = oracle_mod.Program(img).run_batch(buf, n, offsets=kw["offsets"], lens=kw["lens"])
    assert np.array_equal(st, sts)
    ov = np.where(st != 0, 0xFF, np.where(r0 < 5, r0, 0xFE)).astype(np.uint8)
    prog = Program(img)
    fr = torch.from_numpy(buf.copy()).to(cuda)
    res = prog.run(fr, writeback=True, queues=True, **_dev_kw(kw, cuda))
    torch.cuda.synchronize()
    assert np.array_equal(res.verdict.cpu().numpy(), ov)
    ei, ec = R.queues(ov)
    assert np.array_equal(res.queue_index.cpu().numpy().view(np.uint32), ei)
    lay = dict(offsets=kw["offsets"], lens=kw["lens"])
    seen = 0
    for queue in range(6):  # the non-fault queues
        if ec[queue] == 0:
            continue
        w, _ = _check_gather(cuda, exp, lay, ov, queue, 16, _full_bytes(lay, ov, queue, 16, n),
                             f"nat q={queue}", fr_dev=fr,
                             qs=(res.queue_index, res.queue_count, ei, ec))
        assert w == ec[queue]
        seen += w
    assert seen == int((st == 0).sum()) and seen >= n // 4
    prog.close()


def test_gathered_queue_runs_as_a_batch(cuda, oracle_mod):
    """5-tuple -> gather of PASS -> the ACL on the gathered offsets + lens batch (the var tile
    loop): r0 / status equal the oracle over the numpy-compacted packets."""
    import torch

    from ebpf_emu import Program, _lib
    from ebpf_emu import queues as Q
    from ebpf_emu import workloads as W

    n = 4096 + 17
    buf = W.frames_fixed(n, 64, 3)
    first, second = Program(W.program("5tuple")), Program(W.program("acl"))
    fr = torch.from_numpy(buf).to(cuda)
    res = first.run(fr, n=n, stride=64, queues=True)
    g = Q.gather(fr, res.queue_index, res.queue_count, 2, stride=64, align=16)
    m = int(g.total[0])  # (the test reads it; a pipeline sizes the next batch from its capacity)
    r0, st, _ = oracle_mod.Program(W.program("5tuple")).run_batch(buf, n, stride=64, threads=4)
    keep = np.flatnonzero((st == 0) & (r0 == 2))
    assert m == len(keep) and m > 100
    compact = buf.reshape(n, 64)[keep].reshape(-1)
    assert np.array_equal(g.frames.cpu().numpy()[:m * 64], compact)
    b = second.make_batch(g.frames, n=m, offsets=g.offsets, lens=g.lens)
    assert second.batch_kernel(b) == _lib.EBPF_KERNEL_JIT_VARL
    out = second.run(g.frames, n=m, offsets=g.offsets, lens=g.lens, r0=True, status=True)
    torch.cuda.synchronize()
    er0, est, _ = oracle_mod.Program(W.program("acl")).run_batch(compact, m, stride=64, threads=4)
    assert np.array_equal(out.status.cpu().numpy(), est)
    assert np.array_equal(out.r0.cpu().numpy().view(np.uint64), er0)
    first.close()
    second.close()
