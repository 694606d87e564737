#!/usr/bin/env python3
"""Host wall time of 10,000 back-to-back ebpf_run_batch enqueues of the 5-tuple on fixed slots
(4096 packets, so the host and not the kernel sets the pace; no synchronisation inside the loop,
one at the end); prints one JSON line: value = us per enqueue call, with_sync_us = including the
final synchronisation. EBPFEMU_LIB_PATH selects another build of the library (A/B runs)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebpf-emu_amd"))
import torch

from ebpf_emu import Program, _lib
from ebpf_emu import workloads as W

K = 10000
dev = torch.device("cuda", 0)
n = 4096
prog = Program(W.program("5tuple"))
prog.upload(0)
fr = torch.from_numpy(W.frames_fixed(n, 64, 3)).to(dev)
b = prog.make_batch(fr, n=n, stride=64)
verdict = torch.empty(n, dtype=torch.uint8, device=dev)
counters = torch.zeros(8, dtype=torch.int64, device=dev)
out = _lib.BatchOut()
out.verdict = verdict.data_ptr()
out.counters = counters.data_ptr()
stream = torch.cuda.current_stream(dev)
for _ in range(200):
    prog.launch(b, out, stream)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(K):
    prog.launch(b, out, stream)
t1 = time.perf_counter()
torch.cuda.synchronize()
t2 = time.perf_counter()
print(json.dumps({"metric": "host enqueue, 5tuple fixed slots, 4096 packets", "unit": "us/enqueue",
                  "value": (t1 - t0) * 1e6 / K, "with_sync_us": (t2 - t0) * 1e6 / K,
                  "launches": K, "kernel": _lib.KERNEL_NAMES[prog.batch_kernel(b, out, 0)]}))
