#!/usr/bin/env python3
"""ebpf_pcap_gather against the path a caller uses without it:

  pass64    the 5-tuple's PASS queue from 1 Mi 64-byte slots
  mixed     the PASS queue of the mixed 64/1500-byte offsets + lens batch
  capture   the PASS queue of a capture in place (64-byte packets behind their record headers),
            with EBPF_PCAP_SRC_RECORDS

each against (a) this library's own ebpf_gather at align 1 on the same queue -- what a caller runs
today before building the record headers on the host; it writes 16 fewer bytes per packet, so the
line states the byte ratio beside the time -- and (b) tools/sol_copy.hip's plain copy of as many
bytes as the pcap gather writes (`--sol-copy PATH`, built with
`hipcc --offload-arch=gfx950 -O3 tools/sol_copy.hip -o tools/bin/sol_copy`). tools/queues_bench.py's
method: RUNS runs a side, interleaved, each 5 warm-up calls and then HIP events around --steps
back-to-back calls on one stream. One JSON line per case and side to <out>/pcap_export_<case>.jsonl.

  python tools/pcap_export_bench.py [--n 1048576] [--steps 20] [--out profiles] [--sol-copy PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebpf-emu_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from queues_bench import RUNS, WARMUP, sol_copy_us, timed  # noqa: E402


def main():
    import numpy as np
    import torch

    from ebpf_emu import Program, _lib, pcap
    from ebpf_emu import queues as Q
    from ebpf_emu import workloads as W

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--sol-copy", default=os.path.join(ROOT, "tools", "bin", "sol_copy"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.n
    sol = args.sol_copy if os.path.exists(args.sol_copy) else None
    prog = Program(W.program("5tuple"))
    os.makedirs(args.out, exist_ok=True)
    hdr, _ = pcap.header()

    def case(name, fr, kw, run_kw, flags):
        res = prog.run(fr, n=n, queues=True, **kw, **run_kw)
        torch.cuda.synchronize()
        qi, qc = res.queue_index, res.queue_count
        out, total, oo, ol = Q.pcap_gather(fr, qi, qc, 2, hdr, flags=flags, n=n, with_index=True, **kw)
        g = Q.gather(fr, qi, qc, 2, align=1, n=n, **kw)
        torch.cuda.synchronize()
        m, end = (int(x) & 0xFFFFFFFF for x in total.tolist())
        gm, gend = (int(x) & 0xFFFFFFFF for x in g.total.tolist())
        assert m == gm == int(qc[2]) and end == 24 + 16 * m + gend
        # the two agree on the packets' bytes (spot check: the first and the last record)
        for r in (0, m - 1):
            o, ln = int(oo[r]) & 0xFFFFFFFF, int(ol[r]) & 0xFFFF
            go = int(g.offsets[r]) & 0xFFFFFFFF
            assert torch.equal(out[o:o + ln], g.frames[go:go + ln])
        sides = {"pcap_gather": lambda: timed(lambda: Q.pcap_gather(
                     fr, qi, qc, 2, hdr, flags=flags, n=n, out=out, total=total, out_offsets=oo,
                     out_lens=ol, **kw), args.steps),
                 "gather_align1": lambda: timed(lambda: Q.gather(fr, qi, qc, 2, align=1, n=n, out=g,
                                                                 **kw), args.steps)}
        if sol:
            sides["sol_copy"] = lambda: sol_copy_us(sol, end)
        times = {s: [] for s in sides}
        for _ in range(RUNS):
            for s, fn in sides.items():
                times[s].append(fn())
        med = {s: sorted(ts)[len(ts) // 2] for s, ts in times.items()}
        with open(os.path.join(args.out, f"pcap_export_{name}.jsonl"), "w") as f:
            for s, ts in times.items():
                o = sorted(ts)
                nbytes = gend if s == "gather_align1" else end
                line = dict(case=name, side=s, packets=n, queue_packets=m, bytes_written=nbytes,
                            steps=args.steps, warmup=WARMUP, us_runs=[round(t, 2) for t in ts],
                            us_median=round(med[s], 2), us_min=round(o[0], 2), us_max=round(o[-1], 2),
                            time_vs_pcap_gather=round(med[s] / med["pcap_gather"], 3),
                            bytes_vs_pcap_gather=round(nbytes / end, 3))
                f.write(json.dumps(line) + "\n")
                print(json.dumps(line), flush=True)

    fr = torch.from_numpy(W.frames_fixed(n, 64, 3)).to(dev)
    case("pass64", fr, dict(stride=64), {}, 0)
    # the same packets as a capture in place
    host = W.frames_fixed(n, 64, 3).reshape(n, 64)
    cap = np.frombuffer(pcap.to_bytes([host[i].tobytes() for i in range(n)]), dtype=np.uint8)
    offs, lens, _ = pcap.index(cap)
    del fr
    fr = torch.from_numpy(cap.copy()).to(dev)
    kw = dict(offsets=torch.from_numpy(offs.view(np.int32)).to(dev),
              lens=torch.from_numpy(lens.view(np.int16)).to(dev))
    case("capture", fr, kw, {}, _lib.PCAP_SRC_RECORDS)
    del fr
    buf, offs, lens = W.frames_mixed(n)
    fr = torch.from_numpy(buf).to(dev)
    kw = dict(offsets=torch.from_numpy(offs.view(np.int32)).to(dev),
              lens=torch.from_numpy(lens.view(np.int16)).to(dev))
    # (mem_size 2048: the default 1 KiB image faults every 1500-byte packet ST_BADPKT)
    case("mixed", fr, kw, dict(mem_size=2048), 0)
    prog.close()


if __name__ == "__main__":
    main()
