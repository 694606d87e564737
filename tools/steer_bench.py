#!/usr/bin/env python3
"""ebpf_rss_hash / ebpf_steer against the launches they sit next to, all over the
same 1 Mi x 64-byte fixed slots:

  rss_hash         one launch of ebpf_rss_hash, every type enabled
  drop_all         the drop-all program's batch on the same frames (it reads the same bytes)
  steer_nq8 / 64   ebpf_steer over the 1 Mi hashes, 8 and 64 queues (three launches each)
  verdict_queues   ebpf_verdict_queues over 1 Mi verdicts (the 5-tuple's own output)

queues_bench.py's method: RUNS runs, interleaved side by side, each 5 warm-up calls and then HIP
events around --steps back-to-back calls on one stream (time per call). One JSON line per side to
<out>/steer_bench.jsonl, then one line with the two ratios.

  python tools/steer_bench.py [--n 1048576] [--steps 20] [--out profiles]
"""
import argparse
import json
import os
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


def main():
    import torch

    from ebpf_emu import Program, _lib, rss
    from ebpf_emu import queues as Q
    from ebpf_emu import workloads as W

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.n
    os.makedirs(args.out, exist_ok=True)
    fr = torch.from_numpy(W.frames_fixed(n, 64, 3)).to(dev)
    drop, five = Program(W.program("drop")), Program(W.program("5tuple"))
    v = five.run(fr, n=n, stride=64).verdict
    h = torch.empty(n, dtype=torch.int32, device=dev)
    t = torch.empty(n, dtype=torch.uint8, device=dev)
    rss.rss_hash(fr, rss.MSFT_KEY, rss.RSS_ALL, stride=64, n=n, hash=h, type=t)
    torch.cuda.synchronize()
    hashed = int((t != 0).sum())
    index = torch.empty(n, dtype=torch.int32, device=dev)
    bounds = torch.zeros(2 * 64 + rss.BOUNDS_PAD, dtype=torch.int32, device=dev)
    count = torch.empty(_lib.NQUEUES, dtype=torch.int32, device=dev)
    batch = drop.make_batch(fr, n=n, stride=64)
    out = _lib.BatchOut()
    dv = torch.empty(n, dtype=torch.uint8, device=dev)
    out.verdict = dv.data_ptr()
    stream = torch.cuda.current_stream()
    sides = {
        "rss_hash": lambda: rss.rss_hash(fr, rss.MSFT_KEY, rss.RSS_ALL, stride=64, n=n, hash=h, type=t),
        "drop_all": lambda: drop.launch(batch, out, stream),
        "steer_nq8": lambda: rss.steer(h, 8, index=index, bounds=bounds),
        "steer_nq64": lambda: rss.steer(h, 64, index=index, bounds=bounds),
        "verdict_queues": lambda: Q.verdict_queues(v, index=index, count=count),
    }
    times = {s: [] for s in sides}
    for _ in range(RUNS):
        for s, fn in sides.items():
            times[s].append(timed(fn, args.steps))
    med = {}
    with open(os.path.join(args.out, "steer_bench.jsonl"), "w") as f:
        for s, ts in times.items():
            o = sorted(ts)
            med[s] = o[len(o) // 2]
            line = dict(side=s, packets=n, hashed=hashed, steps=args.steps, warmup=WARMUP,
                        us_runs=[round(x, 2) for x in ts], us_median=round(med[s], 2),
                        us_min=round(o[0], 2), us_max=round(o[-1], 2))
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
        line = dict(rss_hash_over_drop_all=round(med["rss_hash"] / med["drop_all"], 2),
                    steer_nq8_over_verdict_queues=round(med["steer_nq8"] / med["verdict_queues"], 2),
                    steer_nq64_over_verdict_queues=round(med["steer_nq64"] / med["verdict_queues"], 2))
        f.write(json.dumps(line) + "\n")
        print(json.dumps(line), flush=True)
    drop.close()
    five.close()


if __name__ == "__main__":
    main()
