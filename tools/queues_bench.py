#!/usr/bin/env python3
"""ebpf_verdict_queues / ebpf_gather against what a caller does without them:

  queues_5tuple   1 Mi verdicts of the 5-tuple's own output: verdict_queues vs the class map +
                  torch.sort(stable=True) + torch.bincount on the same tensor
  gather_pass64   that batch's PASS queue (64-byte slots): gather (align 16) vs torch.index_select
                  with the queue's indices already sliced and widened (the host sync and the
                  conversion a torch caller pays are NOT timed) vs a plain copy of as many bytes
  gather_mixed    the PASS queue of a mixed 64/1500-byte offsets + lens batch: gather vs the plain
                  copy (torch cannot express it)

The plain copy is tools/sol_copy.hip's best line (`--sol-copy PATH`, built with
`hipcc --offload-arch=gfx950 -O3 tools/sol_copy.hip -o tools/bin/sol_copy`). Every side: RUNS runs,
interleaved side by side, each 5 warm-up calls and then HIP events around --steps back-to-back
calls on one stream (time per call). One JSON line per case and side to <out>/queues_<case>.jsonl.

  python tools/queues_bench.py [--n 1048576] [--steps 20] [--out profiles] [--sol-copy PATH]
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebpf-emu_amd"))
RUNS, WARMUP = 5, 5


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


def sol_copy_us(path, nbytes):
    """The best of sol_copy's lines for nbytes -> us (read nbytes + write nbytes)."""
    r = subprocess.run(["timeout", "-k", "10", "120", path, str(nbytes)], capture_output=True,
                       text=True, check=True)
    return min(float(m) for m in re.findall(r": ([0-9.]+) us", r.stdout))


def main():
    import numpy as np
    import torch

    from ebpf_emu import Program
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

    def report(case, sides, extra):
        """sides: {name: fn() -> us}; RUNS interleaved rounds."""
        times = {s: [] for s in sides}
        for _ in range(RUNS):
            for s, fn in sides.items():
                times[s].append(fn())
        with open(os.path.join(args.out, f"queues_{case}.jsonl"), "w") as f:
            for s, ts in times.items():
                o = sorted(ts)
                line = dict(case=case, side=s, packets=n, steps=args.steps, warmup=WARMUP,
                            us_runs=[round(t, 2) for t in ts], us_median=round(o[len(o) // 2], 2),
                            us_min=round(o[0], 2), us_max=round(o[-1], 2), **extra)
                if "bytes" in extra:  # read + write of the packets' bytes
                    line["tb_s"] = round(2 * extra["bytes"] / (line["us_median"] * 1e-6) / 1e12, 3)
                f.write(json.dumps(line) + "\n")
                print(json.dumps(line), flush=True)

    # ---- queues: the 5-tuple's own verdicts
    fr = torch.from_numpy(W.frames_fixed(n, 64, 3)).to(dev)
    res = prog.run(fr, n=n, stride=64, queues=True)
    torch.cuda.synchronize()
    v = res.verdict
    index = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty(7, dtype=torch.int32, device=dev)

    def torch_queues():
        q = torch.where(v < 5, v, torch.where(v == 0xFF, 6, 5).to(torch.uint8))
        _, idx = torch.sort(q, stable=True)
        return idx, torch.bincount(q.int(), minlength=7)

    ti, tc = torch_queues()
    assert torch.equal(ti.to(torch.int32), res.queue_index) and torch.equal(tc.to(torch.int32), res.queue_count)
    report("5tuple", {"verdict_queues": lambda: timed(lambda: Q.verdict_queues(v, index=index, count=count), args.steps),
                      "torch_sort_bincount": lambda: timed(torch_queues, args.steps)},
           dict(counts=res.queue_count.tolist()))

    # ---- gather: the PASS queue, 64-byte slots
    cnt = res.queue_count.cpu().numpy()
    start, m = int(cnt[:2].sum()), int(cnt[2])
    out = Q.GatherResult(frames=torch.empty(n * 64, dtype=torch.uint8, device=dev),
                         offsets=torch.empty(n, dtype=torch.int32, device=dev),
                         lens=torch.empty(n, dtype=torch.int16, device=dev),
                         total=torch.empty(2, dtype=torch.int32, device=dev))
    rows = fr.view(n, 64)
    sel = res.queue_index[start:start + m].to(torch.int64)
    dst = torch.empty((m, 64), dtype=torch.uint8, device=dev)
    Q.gather(fr, res.queue_index, res.queue_count, 2, stride=64, out=out)
    torch.index_select(rows, 0, sel, out=dst)
    torch.cuda.synchronize()
    assert out.total.tolist() == [m, m * 64] and torch.equal(out.frames[:m * 64].view(m, 64), dst)
    sides = {"gather": lambda: timed(lambda: Q.gather(fr, res.queue_index, res.queue_count, 2,
                                                      stride=64, out=out), args.steps),
             "torch_index_select": lambda: timed(lambda: torch.index_select(rows, 0, sel, out=dst),
                                                 args.steps)}
    if sol:
        sides["sol_copy"] = lambda: sol_copy_us(sol, m * 64)
    report("gather_pass64", sides, dict(queue_packets=m, bytes=m * 64))
    del out, dst, rows, fr

    # ---- gather: the PASS queue of a mixed 64/1500-byte offsets + lens batch
    buf, offs, lens = W.frames_mixed(n)
    fr = torch.from_numpy(buf).to(dev)
    doffs = torch.from_numpy(offs.view(np.int32)).to(dev)
    dlens = torch.from_numpy(lens.view(np.int16)).to(dev)
    # (mem_size 2048: the default 1 KiB image faults every 1500-byte packet ST_BADPKT)
    res = prog.run(fr, n=n, offsets=doffs, lens=dlens, mem_size=2048, queues=True)
    torch.cuda.synchronize()
    qi = res.queue_index.cpu().numpy().view(np.uint32)
    cnt = res.queue_count.cpu().numpy()
    mine = qi[int(cnt[:2].sum()):int(cnt[:3].sum())]
    nbytes = int(lens[mine].astype(np.int64).sum())
    g = Q.gather(fr, res.queue_index, res.queue_count, 2, offsets=doffs, lens=dlens)
    torch.cuda.synchronize()
    assert int(g.total[0]) == len(mine) and len(set(lens[mine].tolist())) == 2
    sides = {"gather": lambda: timed(lambda: Q.gather(fr, res.queue_index, res.queue_count, 2,
                                                      offsets=doffs, lens=dlens, out=g), args.steps)}
    if sol:
        sides["sol_copy"] = lambda: sol_copy_us(sol, nbytes)
    report("gather_mixed", sides, dict(queue_packets=len(mine), bytes=nbytes))
    prog.close()


if __name__ == "__main__":
    main()
