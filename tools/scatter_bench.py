#!/usr/bin/env python3
"""ebpf_scatter against what a caller does without it, tools/queues_bench.py's
method:

  scatter_pass64   the 5-tuple's PASS queue of 1 Mi 64-byte slots, gathered (align 16) and
                   scattered back, packets and the three result arrays: scatter vs
                   torch.index_copy_ on an [n, 64] view with the queue's indices already sliced
                   and widened (the host sync and the conversion a torch caller pays are NOT timed;
                   its three result arrays are not copied either) vs a plain copy of as many bytes
  scatter_mixed    the PASS queue of a mixed 64/1500-byte offsets + lens batch: scatter vs the
                   plain copy (torch cannot express it)

The plain copy is tools/sol_copy.hip's best line (`--sol-copy PATH`, built with
`hipcc --offload-arch=gfx950 -O3 tools/sol_copy.hip -o tools/bin/sol_copy`). Every side: RUNS runs,
interleaved side by side, each 5 warm-up calls and then HIP events around --steps back-to-back
calls on one stream (time per call). One JSON line per case and side to <out>/scatter_<case>.jsonl.

  python tools/scatter_bench.py [--n 1048576] [--steps 20] [--out profiles] [--sol-copy PATH]
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

    from ebpf_emu import Program
    from ebpf_emu import queues as Q
    from ebpf_emu import workloads as W
    from ebpf_emu.program import BatchResult

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
        with open(os.path.join(args.out, f"scatter_{case}.jsonl"), "w") as f:
            for s, ts in times.items():
                o = sorted(ts)
                line = dict(case=case, side=s, packets=n, steps=args.steps, warmup=WARMUP,
                            us_runs=[round(t, 2) for t in ts], us_median=round(o[len(o) // 2], 2),
                            us_min=round(o[0], 2), us_max=round(o[-1], 2), **extra)
                line["tb_s"] = round(2 * extra["bytes"] / (line["us_median"] * 1e-6) / 1e12, 3)
                f.write(json.dumps(line) + "\n")
                print(json.dumps(line), flush=True)

    def results(m):  # a second run's outputs (their values do not matter to the time)
        return BatchResult(verdict=torch.full((m,), 3, dtype=torch.uint8, device=dev),
                           status=torch.zeros(m, dtype=torch.uint8, device=dev),
                           r0=torch.full((m,), 3, dtype=torch.int64, device=dev))

    # ---- the PASS queue, 64-byte slots
    fr = torch.from_numpy(W.frames_fixed(n, 64, 3)).to(dev)
    res = prog.run(fr, n=n, stride=64, r0=True, status=True, queues=True)
    g = Q.gather(fr, res.queue_index, res.queue_count, 2, stride=64)
    torch.cuda.synchronize()
    cnt = res.queue_count.cpu().numpy()
    start, m = int(cnt[:2].sum()), int(cnt[2])
    assert int(g.total[0]) == m
    src = results(m)
    merged = BatchResult(verdict=res.verdict.clone(), status=res.status.clone(), r0=res.r0.clone())
    back = torch.zeros_like(fr)
    rows = back.view(n, 64)
    sel = res.queue_index[start:start + m].to(torch.int64)
    dense = g.frames[:m * 64].view(m, 64)

    def scatter64():
        Q.scatter(g, res.queue_index, res.queue_count, 2, frames=back, stride=64, n=n, src=src,
                  dst=merged, cap=m)

    scatter64()
    torch.cuda.synchronize()
    passed = res.verdict == 2
    assert torch.equal(rows[passed], fr.view(n, 64)[passed]) and not rows[~passed].any()
    assert torch.equal(merged.verdict[passed], src.verdict) and torch.equal(merged.verdict[~passed], res.verdict[~passed])
    rows.index_copy_(0, sel, dense)
    torch.cuda.synchronize()
    assert torch.equal(rows[passed], fr.view(n, 64)[passed])
    sides = {"scatter": lambda: timed(scatter64, args.steps),
             "torch_index_copy": lambda: timed(lambda: rows.index_copy_(0, sel, dense), args.steps)}
    if sol:
        sides["sol_copy"] = lambda: sol_copy_us(sol, m * 64)
    report("pass64", sides, dict(queue_packets=m, bytes=m * 64))
    del back, rows, dense, g, fr, merged, src

    # ---- the PASS queue of a mixed 64/1500-byte offsets + lens batch
    buf, offs, lens = W.frames_mixed(n)
    fr = torch.from_numpy(buf).to(dev)
    doffs = torch.from_numpy(offs.view(np.int32)).to(dev)
    dlens = torch.from_numpy(lens.view(np.int16)).to(dev)
    # (mem_size 2048: the default 1 KiB image faults every 1500-byte packet ST_BADPKT)
    res = prog.run(fr, n=n, offsets=doffs, lens=dlens, mem_size=2048, r0=True, status=True, queues=True)
    g = Q.gather(fr, res.queue_index, res.queue_count, 2, offsets=doffs, lens=dlens)
    torch.cuda.synchronize()
    qi = res.queue_index.cpu().numpy().view(np.uint32)
    cnt = res.queue_count.cpu().numpy()
    mine = qi[int(cnt[:2].sum()):int(cnt[:3].sum())]
    m = len(mine)
    nbytes = int(lens[mine].astype(np.int64).sum())
    assert int(g.total[0]) == m and len(set(lens[mine].tolist())) == 2
    src = results(m)
    merged = BatchResult(verdict=res.verdict.clone(), status=res.status.clone(), r0=res.r0.clone())
    back = torch.zeros_like(fr)

    def scatter_mixed():
        Q.scatter(g, res.queue_index, res.queue_count, 2, frames=back, offsets=doffs, lens=dlens,
                  n=n, src=src, dst=merged, cap=m)

    scatter_mixed()
    torch.cuda.synchronize()
    got = back.cpu().numpy()
    for i in list(mine[:200]) + list(mine[-200:]):
        o, ln = int(offs[i]), int(lens[i])
        assert np.array_equal(got[o:o + ln], buf[o:o + ln]), i
    assert int(np.count_nonzero(got)) <= nbytes
    sides = {"scatter": lambda: timed(scatter_mixed, args.steps)}
    if sol:
        sides["sol_copy"] = lambda: sol_copy_us(sol, nbytes)
    report("mixed", sides, dict(queue_packets=m, bytes=nbytes))
    prog.close()


if __name__ == "__main__":
    main()
