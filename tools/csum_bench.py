#!/usr/bin/env python3
"""ebpf_csum_verify / ebpf_csum_fill timed over the benchmark's own batches, next to
the one thing here that already sums packet bytes, the compiled `checksum` program:

  verify_mixed / fill_mixed    1 Mi mixed 64 / 1500-byte packets (workloads.frames_mixed)
  verify_64 / fill_64          1 Mi x 64-byte fixed slots (workloads.frames_fixed)
  checksum_prog_mixed          the compiled `checksum` program's batch over the same mixed batch

The workloads' frames carry random length fields, so first the IPv4 total length, the fragment
word, the UDP length and the IPv6 payload length / next header are made to describe the packet
(numpy), the checksums are filled on the device, and a sample of the packets is checked against
the tests' Python model (tests/csum_ref.py): every timed verify then sums a whole datagram.

steer_bench.py's method: RUNS runs, interleaved side by side, each WARMUP warm-up calls and then
HIP events around --steps back-to-back calls on one stream (time per call). The floor is the
batch's packet bytes over 8 TB/s. One JSON document to <out>/csum_bench.json.

  python tools/csum_bench.py [--n 1048576] [--steps 20] [--out profiles]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebpf-emu_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
RUNS, WARMUP = 5, 5
HBM_PEAK = 8e12  # bytes / s


def timed(fn, steps):
    import torch

    for _ in range(WARMUP):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps  # us per call


def describe_packets(buf, offsets, lens):
    """Length fields that describe the packet, in place (numpy): IPv4 total length = len - 14,
    no fragment, UDP length = what is left; IPv6 payload length = len - 54, next header TCP."""
    import numpy as np

    o = offsets.astype(np.int64)
    ln = lens.astype(np.int64)

    def put16(sel, at, val):
        buf[o[sel] + at] = (val[sel] >> 8).astype(np.uint8)
        buf[o[sel] + at + 1] = (val[sel] & 0xFF).astype(np.uint8)

    et = (buf[o + 12].astype(np.int64) << 8) | buf[o + 13]
    v4, v6 = et == 0x0800, et == 0x86DD
    put16(v4, 16, ln - 14)
    put16(v4, 20, np.zeros_like(ln))
    ihl = (buf[o + 14] & 15).astype(np.int64)
    udp = v4 & (buf[o + 23] == 17)
    for i in (5, 6):  # the workloads' two header sizes
        sel = udp & (ihl == i)
        put16(sel, 14 + 4 * i + 4, ln - 14 - 4 * i)
    put16(v6, 18, ln - 54)
    buf[o[v6] + 20] = 6
    buf[o[v6] + 14] = 0x60 | (buf[o[v6] + 14] & 15)


def main():
    import numpy as np
    import torch

    import csum_ref as C
    from ebpf_emu import Program, _lib, csum
    from ebpf_emu import workloads as W

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.n
    os.makedirs(args.out, exist_ok=True)

    mbuf, moffs, mlens = W.frames_mixed(n)
    fbuf = W.frames_fixed(n, 64, 3)
    foffs, flens = np.arange(n, dtype=np.int64) * 64, np.full(n, 64, dtype=np.int64)
    describe_packets(mbuf, moffs, mlens)
    describe_packets(fbuf, foffs, flens)
    batches = {}
    for name, buf, offs, lens in (("mixed", mbuf, moffs, mlens), ("64", fbuf, foffs, flens)):
        fr = torch.from_numpy(buf).to(dev)
        kw = (dict(offsets=torch.from_numpy(offs.view(np.int32)).to(dev),
                   lens=torch.from_numpy(lens.view(np.int16)).to(dev)) if name == "mixed"
              else dict(stride=64))
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        csum.csum_fill(fr, n=n, status=st, **kw)
        filled = st.cpu().numpy().copy()
        csum.csum_verify(fr, n=n, status=st, **kw)
        torch.cuda.synchronize()
        got = st.cpu().numpy()
        host = fr.cpu().numpy()
        # the device's answers against the model on a sample; nothing BAD after the fill
        assert np.array_equal(got, filled) and not np.any(got & (C.L3_BAD | C.L4_BAD))
        for i in np.random.default_rng(1).integers(0, n, 1500).tolist():
            p = host[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes()
            assert C.verify(p) == got[i] and C.fill(p)[0] == p, (name, i)
        batches[name] = dict(fr=fr, kw=kw, st=st, bytes=int(lens.astype(np.int64).sum()),
                             l3=int(((got & C.L3_GOOD) != 0).sum()), l4=int(((got & C.L4_GOOD) != 0).sum()))

    prog = Program(W.program("checksum"))
    m = batches["mixed"]
    # (bench.py's configuration of this batch: a 1500-byte packet needs a 2 KiB memory image)
    batch = prog.make_batch(m["fr"], n=n, mem_size=2048, r10=2048, **m["kw"])
    out = _lib.BatchOut()
    dv = torch.empty(n, dtype=torch.uint8, device=dev)
    ds = torch.empty(n, dtype=torch.uint8, device=dev)
    out.verdict, out.status = dv.data_ptr(), ds.data_ptr()
    stream = torch.cuda.current_stream()
    prog.launch(batch, out, stream)  # (compiles the program)
    torch.cuda.synchronize()
    assert int((ds != _lib.ST_OK).sum()) == 0, "the checksum program did not run every packet to its end"
    out.status = None
    kernel = _lib.KERNEL_NAMES[prog.batch_kernel(batch, out, 0)]

    def call(fn, b):
        return lambda: fn(b["fr"], n=n, status=b["st"], **b["kw"])

    sides = {
        "verify_mixed": call(csum.csum_verify, batches["mixed"]),
        "fill_mixed": call(csum.csum_fill, batches["mixed"]),
        "checksum_prog_mixed": lambda: prog.launch(batch, out, stream),
        "verify_64": call(csum.csum_verify, batches["64"]),
        "fill_64": call(csum.csum_fill, batches["64"]),
    }
    times = {s: [] for s in sides}
    for _ in range(RUNS):
        for s, fn in sides.items():
            times[s].append(timed(fn, args.steps))
    doc = dict(packets=n, steps=args.steps, warmup=WARMUP, runs=RUNS, device=torch.cuda.get_device_name(0),
               checksum_prog_kernel=kernel, sides={})
    for s, ts in times.items():
        o = sorted(ts)
        b = batches["64" if s.endswith("_64") else "mixed"]
        doc["sides"][s] = dict(us_runs=[round(x, 2) for x in ts], us_median=round(o[len(o) // 2], 2),
                               us_min=round(o[0], 2), us_max=round(o[-1], 2), packet_bytes=b["bytes"],
                               floor_us_at_8TBps=round(b["bytes"] / HBM_PEAK * 1e6, 2),
                               l3_checked=b["l3"], l4_checked=b["l4"])
    med = {s: d["us_median"] for s, d in doc["sides"].items()}
    doc["verify_mixed_over_checksum_prog"] = round(med["verify_mixed"] / med["checksum_prog_mixed"], 3)
    for s in sides:
        doc["sides"][s]["over_floor"] = round(med[s] / doc["sides"][s]["floor_us_at_8TBps"], 2)
    with open(os.path.join(args.out, "csum_bench.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)
    prog.close()


if __name__ == "__main__":
    main()
