#!/usr/bin/env python3
"""EBPF_BATCH_WRITEBACK's cost: NAT over 1 Mi x 64 B on fixed slots and on
offsets + lens, the responder over 1504-byte slots; per configuration three cases --
  a  the flag off
  b  the flag on (the compiled write-back variant)
  c  generic=True, mem=True (the only way to see the rewritten bytes without the flag)
-- each timed one launch at a time and with two streams (stream events around the launch call of
a batch and outputs built beforehand). An in-place run changes its input (the
TTL decays run over run), so `frames` is restored from a pristine device copy outside the timed
region before every timed launch. The cases are interleaved (a, b, c, a, b, c, ...) so drift hits
all alike. One JSON line per case and stream count goes to profiles/writeback_<config>.jsonl.

  python tools/writeback_bench.py [--n 1048576] [--reps 20] [--out profiles]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebpf-emu_amd"))


def main():
    import numpy as np
    import torch

    from ebpf_emu import Program, _lib
    from ebpf_emu import workloads as W

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.n
    configs = {
        "nat_fixed64": ("nat", 64, False, dict()),
        "nat_offsets": ("nat", 64, True, dict()),
        "responder_fixed1504": ("responder", 1504, False, dict(mem_size=2048, r10=2048)),
    }
    cases = {"a_flag_off": dict(), "b_writeback": dict(writeback=True),
             "c_generic_mem": dict(generic=True, mem=True)}
    for cname, (wl, frame, offsets, extra) in configs.items():
        nn = n if frame == 64 else max(1, n // 8)
        pristine = torch.from_numpy(W.frames_fixed(nn, frame, 3)).to(dev)
        kw = dict(n=nn, **extra)
        if offsets:
            kw["offsets"] = torch.arange(0, nn * frame, frame, dtype=torch.int32, device=dev)
            kw["lens"] = torch.full((nn,), frame, dtype=torch.int16, device=dev)
        else:
            kw["stride"] = frame
        prog = Program(W.program(wl))
        streams = [torch.cuda.Stream(dev) for _ in range(2)]
        bufs = [pristine.clone() for _ in range(2)]
        times = {(c, k): [] for c in cases for k in (1, 2)}
        kernels = {}
        # batches and outputs built once per (case, stream): the timed region is prog.launch alone
        # (the ctypes call and the kernel; the stream is idle at the start event, so one launch's
        # time still holds the host's launch latency -- compare the cases, not the absolute rate)
        verdicts = [torch.empty(nn, dtype=torch.uint8, device=dev) for _ in range(2)]
        mems = [torch.empty((nn, kw.get("mem_size", 1024)), dtype=torch.uint8, device=dev)
                for _ in range(2)]
        built = {}
        for case, ckw in cases.items():
            for q in range(2):
                b = prog.make_batch(bufs[q], **{k: v for k, v in {**kw, **ckw}.items() if k != "mem"})
                o = _lib.BatchOut()
                o.verdict = verdicts[q].data_ptr()
                if ckw.get("mem"):
                    o.mem = mems[q].data_ptr()
                built[(case, q)] = (b, o)
            kernels[case] = _lib.KERNEL_NAMES[prog.batch_kernel(*built[(case, 0)])]
        for rep in range(args.reps + 2):  # (two warm-up rounds, dropped)
            for case, ckw in cases.items():
                for k in (1, 2):
                    for q in range(k):
                        bufs[q].copy_(pristine)
                    torch.cuda.synchronize()
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                          for _ in range(k)]
                    for q in range(k):
                        with torch.cuda.stream(streams[q]):
                            ev[q][0].record()
                            prog.launch(*built[(case, q)], streams[q])
                            ev[q][1].record()
                    torch.cuda.synchronize()
                    t0 = min(e[0].elapsed_time(e[1]) for e in ev)
                    span = max(ev[0][0].elapsed_time(e[1]) for e in ev) if k == 2 else t0
                    if rep >= 2:
                        times[(case, k)].append(span * 1e3)
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, f"writeback_{cname}.jsonl"), "w") as f:
            for (case, k), ts in times.items():
                ts = sorted(ts)
                line = dict(config=cname, case=case, streams=k, packets=nn * k, frame_bytes=frame,
                            kernel=kernels[case], us_median=ts[len(ts) // 2], us_min=ts[0],
                            us_max=ts[-1], reps=len(ts),
                            gpkt_s=nn * k / (ts[len(ts) // 2] * 1e-6) / 1e9)
                f.write(json.dumps(line) + "\n")
                print(json.dumps(line))
        prog.close()


if __name__ == "__main__":
    main()
