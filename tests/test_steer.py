"""ebpf_steer on the GPU against the model (tests/rss_ref.py: a stable argsort), exactly; the pair
contract (a steering queue handed to ebpf_gather / ebpf_pcap_gather / ebpf_scatter as count =
bounds + 2k, queue = 1) against those calls' own models; and the chain rss_hash -> steer -> gather
-> run, end to end. Every output is pre-filled with a sentinel, so what the header promises to
leave untouched is compared too. Sizes come from the kernel's constants (ebpf_emu.rss)."""
import importlib.util
import os
import random
import struct
import types

import numpy as np
import pytest

import pcap_export_ref as PR
import queues_ref as QR
import rss_ref as R
import scatter_ref as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0xA5
SENT32 = 0x5A5A5A5A
SENT16 = 0x5A5A
NQS = [1, 2, 3, 7, 8, 33, 64]
PATTERNS = ["one_queue", "random", "absent", "period2", "runs65", "high_bits"]
RETAS = ["default", "len1", "len2", "shuffled128"]


def _sizes():
    from ebpf_emu import rss

    rng = rss.STEER_RANGE  # one workgroup's range; its waves take a quarter each
    return [0, 1, 63, 64, 65, rng // 4 + 1, rng - 1, rng, rng + 1, 2 * rng + 1,
            rng * rss.STEER_MAX_WGS + rng + 65]  # the last: past a full pass of the capped grid


def _keys(name, n, seed=0):
    rng = np.random.default_rng(2000 + seed)
    i = np.arange(n, dtype=np.int64)
    if name == "one_queue":
        k = np.full(n, 0x1234567B, dtype=np.int64)
    elif name == "random":
        k = rng.integers(0, 1 << 32, n, dtype=np.int64)
    elif name == "absent":  # a few table slots only
        k = rng.choice(np.array([0, 3, 5, 64, 77, 127, 0x80, 0x1FF], dtype=np.int64), n)
    elif name == "period2":
        k = np.where(i % 2 == 0, 0x10, 0x2F)
    elif name == "runs65":  # runs of 65: queue runs straddle wave and workgroup edges
        k = np.where((i // 65) % 2 == 0, 1, 126)
    elif name == "high_bits":
        k = rng.integers(0, 1 << 32, n, dtype=np.int64) | 0xFFFF0000
    else:
        raise KeyError(name)
    return k.astype(np.uint32)


def _reta(name, nq, seed=0):
    rng = np.random.default_rng(3000 + seed)
    if name == "default":
        return None
    if name == "len1":
        return [nq - 1]
    if name == "len2":
        return [nq // 2, 0]
    t = np.arange(128) % nq
    if nq > 2:
        t[t == 1] = nq - 1  # queue 1 stays empty
    rng.shuffle(t)
    return t.tolist()


def _first_diff(got, exp, tag):
    if not np.array_equal(got, exp):
        d = np.flatnonzero(got != exp)
        raise AssertionError((tag, "first wrong position", int(d[0]), "got", got[d[:4]].tolist(),
                              "expected", exp[d[:4]].tolist(), "wrong", len(d)))


def _dev_steer(k_dev, n, nq, reta):
    """steer into sentinel-filled outputs -> (SteerResult, index u32[n + 8], bounds u32[2nq + 8])."""
    import torch

    from ebpf_emu import rss

    idx = torch.full((n + 8,), SENT32, dtype=torch.int32, device=k_dev.device)
    bnd = torch.full((2 * nq + 8,), SENT32, dtype=torch.int32, device=k_dev.device)
    res = rss.steer(k_dev, nq, reta=reta, index=idx[:n], bounds=bnd)
    torch.cuda.synchronize()
    return res, idx.cpu().numpy().view(np.uint32), bnd.cpu().numpy().view(np.uint32)


def _check(keys, k_dev, nq, reta, tag):
    n = len(keys)
    res, gi, gb = _dev_steer(k_dev, n, nq, reta)
    ei, eb, _ = R.steer(keys, nq, reta)
    assert np.array_equal(gb[:2 * nq], eb.reshape(-1)), (tag, gb[:2 * nq].tolist(), eb.tolist())
    assert np.all(gb[2 * nq:] == SENT32), (tag, "bounds written past 2 * nq")
    _first_diff(gi[:n], ei, tag)
    assert np.all(gi[n:] == SENT32), (tag, "index written past n")
    return res, ei, eb


@pytest.mark.parametrize("nq", NQS)
def test_steer_matches_the_model(cuda, nq):
    """Every pattern x table x size below the grid cap; the size past the cap (4 Mi keys) once per
    nq, its pattern and table rotating with nq so that the seven cases cover them all."""
    import torch

    sizes = _sizes()
    for pi, pattern in enumerate(PATTERNS):
        for n in sizes[:-1]:
            keys = _keys(pattern, n, n % 89)
            kd = torch.from_numpy(keys.view(np.int32)).to(cuda)
            for ri, rname in enumerate(RETAS):
                _check(keys, kd, nq, _reta(rname, nq, pi), f"nq={nq} {pattern} {rname} n={n}")
    n, j = sizes[-1], NQS.index(nq)
    pattern, rname = PATTERNS[j % len(PATTERNS)], RETAS[j % len(RETAS)]
    keys = _keys(pattern, n, j)
    kd = torch.from_numpy(keys.view(np.int32)).to(cuda)
    _check(keys, kd, nq, _reta(rname, nq, j), f"nq={nq} {pattern} {rname} n={n}")


def test_steer_key_at_any_dword(cuda):
    """A key pointer that is 4-byte but not 8- or 16-byte aligned."""
    import torch

    from ebpf_emu import rss

    for shift in (1, 2, 3):
        for n in (1, 65, rss.STEER_RANGE + 1):
            keys = _keys("random", n, shift)
            buf = torch.zeros(n + shift + 3, dtype=torch.int32, device=cuda)
            buf[shift:shift + n] = torch.from_numpy(keys.view(np.int32)).to(cuda)
            kd = buf[shift:shift + n]
            assert kd.data_ptr() % 16 == 4 * shift
            _check(keys, kd, 7, None, f"shift={shift} n={n}")


# ---------------------------------------------------------------- the pair contract
def _var_batch(n):
    """Offsets + lens, source offsets at every residue mod 16."""
    rng = random.Random(n)
    lens = np.array([rng.choice([0, 1, 15, 16, 17, 60, 64, 65, 300]) for _ in range(n)], dtype=np.uint16)
    offs, pos = [], 16
    for i in range(n):
        pos += (i % 16 - pos) % 16 if i % 3 else (i * 7) % 16
        offs.append(pos)
        pos += int(lens[i])
    frames = np.random.default_rng(n).integers(0, 256, pos + 40, dtype=np.uint8)
    return frames, np.array(offs, dtype=np.uint32), lens


@pytest.fixture(scope="module")
def steered(cuda):
    """One batch, steered into 8 queues of which queue 1 is empty: the device result and the
    model's."""
    import torch

    n, nq = 700, 8
    frames, offs, lens = _var_batch(n)
    keys = _keys("random", n, 5)
    reta = _reta("shuffled128", nq, 1)
    res, ei, eb = _check(keys, torch.from_numpy(keys.view(np.int32)).to(cuda), nq, reta, "steered")
    assert eb[1, 1] == 0 and all(eb[k, 1] > 20 for k in (0, 3, 7))
    dev = dict(frames=torch.from_numpy(frames).to(cuda),
               offsets=torch.from_numpy(offs.view(np.int32)).to(cuda),
               lens=torch.from_numpy(lens.view(np.int16)).to(cuda))
    return types.SimpleNamespace(n=n, nq=nq, frames=frames, offs=offs, lens=lens, res=res, ei=ei,
                                 eb=eb, dev=dev)


QUEUES = [0, 3, 7, 1]  # first, middle, last, empty


@pytest.mark.parametrize("k", QUEUES)
def test_pair_contract_gather(cuda, steered, k):
    import torch

    from ebpf_emu import queues as Q

    s = steered
    n, align = s.n, 16
    out_bytes = int(sum(QR.alignup(int(s.lens[i]), align) for i in QR.queue_of(s.ei, s.eb[k], 1)))
    slack = 272
    out = Q.GatherResult(frames=torch.full((out_bytes + slack,), SENT, dtype=torch.uint8, device=cuda),
                         offsets=torch.full((n + 4,), SENT32, dtype=torch.int32, device=cuda),
                         lens=torch.full((n + 4,), SENT16, dtype=torch.int16, device=cuda),
                         total=torch.full((2,), SENT32, dtype=torch.int32, device=cuda))
    index, count, queue = s.res.queue(k)
    assert queue == 1 and count.data_ptr() == s.res.bounds.data_ptr() + 8 * k
    Q.gather(s.dev["frames"], index, count, queue, offsets=s.dev["offsets"], lens=s.dev["lens"],
             align=align, out_bytes=out_bytes, n=n, out=out)
    torch.cuda.synchronize()
    w, end, eo, el, spans = QR.gather(s.frames, s.ei, s.eb[k], 1, offsets=s.offs, lens=s.lens,
                                      align=align, out_bytes=out_bytes)
    assert w == int(s.eb[k, 1])
    assert out.total.cpu().numpy().view(np.uint32).tolist() == [w, end]
    go = out.offsets.cpu().numpy().view(np.uint32)
    gl = out.lens.cpu().numpy().view(np.uint16)
    _first_diff(go[:w], eo, f"gather k={k} offsets")
    _first_diff(gl[:w], el, f"gather k={k} lens")
    assert np.all(go[w:] == SENT32) and np.all(gl[w:] == SENT16)
    gf = out.frames.cpu().numpy()
    exp, known = QR.expected_frames(out_bytes + slack, out_bytes, SENT, align, end, spans)
    assert np.array_equal(gf[known], exp[known]), f"gather k={k} bytes"


@pytest.mark.parametrize("k", QUEUES)
def test_pair_contract_pcap_gather(cuda, steered, k):
    import torch

    from ebpf_emu import pcap
    from ebpf_emu import queues as Q

    s = steered
    hdr, flags = pcap.header()
    rn, end, eo, el, data = PR.pcap_gather(s.frames, s.ei, s.eb[k], 1, s.n, hdr, offsets=s.offs,
                                           lens=s.lens, flags=flags, out_bytes=1 << 30)
    assert rn == int(s.eb[k, 1])
    out = torch.full((end + 64,), SENT, dtype=torch.uint8, device=cuda)
    total = torch.full((2,), SENT32, dtype=torch.int32, device=cuda)
    oo = torch.full((s.n + 4,), SENT32, dtype=torch.int32, device=cuda)
    ol = torch.full((s.n + 4,), SENT16, dtype=torch.int16, device=cuda)
    Q.pcap_gather(s.dev["frames"], *s.res.queue(k), hdr, flags=flags, offsets=s.dev["offsets"],
                  lens=s.dev["lens"], n=s.n, out=out, total=total, out_offsets=oo, out_lens=ol)
    torch.cuda.synchronize()
    assert total.cpu().numpy().view(np.uint32).tolist() == [rn, end]
    got = out.cpu().numpy()
    assert got[:end].tobytes() == data and np.all(got[end:] == SENT), f"pcap k={k}"
    go, gl = oo.cpu().numpy().view(np.uint32), ol.cpu().numpy().view(np.uint16)
    assert np.array_equal(go[:rn], eo) and np.array_equal(gl[:rn], el)
    assert np.all(go[rn:] == SENT32) and np.all(gl[rn:] == SENT16)


@pytest.mark.parametrize("k", QUEUES)
def test_pair_contract_scatter_results(cuda, steered, k):
    """Results only: the dense side's verdict / status / r0 land at the queue's packet numbers."""
    import torch

    from ebpf_emu import queues as Q

    s = steered
    n = s.n
    m = int(s.eb[k, 1])
    rng = np.random.default_rng(50 + k)
    sv = rng.integers(0, 256, n, dtype=np.uint8)
    ss = rng.integers(0, 9, n, dtype=np.uint8)
    sr = rng.integers(0, 1 << 62, n, dtype=np.int64)
    ev, es, er = (np.full(n, SENT, dtype=np.uint8), np.full(n, SENT, dtype=np.uint8),
                  np.full(n, -7, dtype=np.int64))
    done = SR.scatter(s.ei, s.eb[k], 1, n, n, src_verdict=sv, src_status=ss, src_r0=sr,
                      verdict=ev, status=es, r0=er)
    assert len(done) == m
    src = types.SimpleNamespace(verdict=torch.from_numpy(sv).to(cuda), status=torch.from_numpy(ss).to(cuda),
                                r0=torch.from_numpy(sr).to(cuda))
    dst = types.SimpleNamespace(verdict=torch.full((n,), SENT, dtype=torch.uint8, device=cuda),
                                status=torch.full((n,), SENT, dtype=torch.uint8, device=cuda),
                                r0=torch.full((n,), -7, dtype=torch.int64, device=cuda))
    Q.scatter(Q.GatherResult(), *s.res.queue(k), n=n, src=src, dst=dst)
    torch.cuda.synchronize()
    assert np.array_equal(dst.verdict.cpu().numpy(), ev)
    assert np.array_equal(dst.status.cpu().numpy(), es)
    assert np.array_equal(dst.r0.cpu().numpy(), er)
    assert int((ev != SENT).sum()) <= m and (m == 0 or np.any(er != -7))


# ---------------------------------------------------------------- end to end
def test_hash_steer_gather_run(cuda):
    """rss_hash -> steer(nq = 8) over a batch of several packets per flow: a flow's packets sit in
    one queue, ascending, and the 5-tuple program run per gathered queue gives the whole-batch
    verdicts at index."""
    import torch

    from ebpf_emu import Program, rss
    from ebpf_emu import queues as Q
    from ebpf_emu import workloads as W

    flows, n, nq = 60, 900, 8
    base = W.frames_fixed(flows, 64, 3).reshape(flows, 64)
    flow = np.random.default_rng(8).integers(0, flows, n)
    buf = base[flow].reshape(-1).copy()
    key, _ = R.msft()
    eh, et = R.rss_batch([bytes(base[f]) for f in range(flows)], key)
    assert (et != 0).sum() > flows // 2
    fr = torch.from_numpy(buf).to(cuda)
    h, t = rss.rss_hash(fr, key, R.ALL, stride=64, n=n)
    st = rss.steer(h, nq)
    prog = Program(W.program("5tuple"))
    whole = prog.run(fr, n=n, stride=64).verdict
    torch.cuda.synchronize()
    assert np.array_equal(h.cpu().numpy().view(np.uint32), eh[flow])
    assert np.array_equal(t.cpu().numpy(), et[flow])
    ei, eb, q = R.steer(eh[flow], nq)
    gi = st.index.cpu().numpy().view(np.uint32)
    gb = st.bounds.cpu().numpy().view(np.uint32)[:2 * nq].reshape(nq, 2)
    assert np.array_equal(gi, ei) and np.array_equal(gb, eb)
    assert np.array_equal(st.counts().cpu().numpy().view(np.uint32), eb[:, 1])
    for f in range(flows):  # one queue per flow, in arrival order
        mine = np.flatnonzero(flow == f)
        k = int(q[mine[0]])
        inq = gi[gb[k, 0]:gb[k, 0] + gb[k, 1]]
        assert np.array_equal(inq[np.isin(inq, mine)], mine), f
    wv = whole.cpu().numpy()
    seen = 0
    for k in range(nq):
        g = Q.gather(fr, *st.queue(k), stride=64, align=16, n=n)
        m = int(g.total[0])
        assert m == int(eb[k, 1])
        if m == 0:
            continue
        v = prog.run(g.frames, n=m, offsets=g.offsets, lens=g.lens).verdict
        torch.cuda.synchronize()
        assert np.array_equal(v.cpu().numpy(), wv[gi[gb[k, 0]:gb[k, 0] + m]]), k
        seen += m
    assert seen == n
    prog.close()


def test_pcap_steer_tool(cuda, tmp_path):
    """tools/pcap_steer.py over a 200-packet capture: each PREFIX.q<k>.pcap, indexed again with
    ebpf_pcap_index, holds exactly the model's packets with their own record headers."""
    from ebpf_emu import pcap

    rng = random.Random(12)
    key, vectors = R.msft()
    flows = [R.flow_frame(v["src"], v["dst"], v["sport"] + j, v["dport"], 6 if j % 2 else 17)
             for v in vectors for j in range(4)] + [R.eth(0x0806) + bytes(28)]
    pkts = [flows[rng.randrange(len(flows))] + bytes(rng.randrange(0, 40)) for _ in range(200)]
    src = tmp_path / "in.pcap"
    src.write_bytes(pcap.to_bytes(pkts))
    spec = importlib.util.spec_from_file_location("pcap_steer", os.path.join(ROOT, "tools", "pcap_steer.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    nq = 4
    tool.main([str(src), "--queues", str(nq), "--out", str(tmp_path / "rx")])
    eh, _ = R.rss_batch(pkts, key)
    ei, eb, q = R.steer(eh, nq)
    assert (eb[:, 1] > 0).sum() >= 3
    total = 0
    for k in range(nq):
        data = (tmp_path / f"rx.q{k}.pcap").read_bytes()
        assert data[:24] == src.read_bytes()[:24]
        offs, lens, _ = pcap.index(data)
        want = np.flatnonzero(q == k)
        assert len(offs) == len(want) == int(eb[k, 1])
        for o, ln, i in zip(offs, lens, want):
            assert data[o:o + ln] == pkts[i], (k, i)
            # the source's own record header: the timestamp is the source record number
            assert data[o - 16:o] == struct.pack("<IIII", int(i), 0, len(pkts[i]), len(pkts[i]))
        total += len(want)
    assert total == len(pkts)
