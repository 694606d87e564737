#!/usr/bin/env python3
"""Run an XDP program over a capture on the GPU and write the packets of one verdict queue out as
a capture again (ebpf_emu.pcap.Capture.filter: ebpf_pcap_gather with the source's own record
headers, so timestamps and orig_len survive).

  python tools/pcap_filter.py IN.pcap PROG OUT.pcap [--queue PASS] [--writeback] [--snaplen N]

PROG: a workload name of ebpf_emu.workloads (5tuple, nat, acl, ...) or a file of the program's
instructions as hex words, one per line (the reference's input format). --queue: ABORTED, DROP,
PASS, TX, REDIRECT, OTHER, FAULT or 0..6. --writeback: write the packets as the program rewrote
them (EBPF_BATCH_WRITEBACK), e.g. the NATed traffic as a capture tool would see it.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebpf-emu_amd"))

QUEUES = ["ABORTED", "DROP", "PASS", "TX", "REDIRECT", "OTHER", "FAULT"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input")
    ap.add_argument("prog")
    ap.add_argument("output")
    ap.add_argument("--queue", default="PASS")
    ap.add_argument("--writeback", action="store_true")
    ap.add_argument("--snaplen", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=1 << 20, help="packets per device chunk")
    ap.add_argument("--mem-size", type=int, default=2048)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    q = args.queue.upper()
    queue = QUEUES.index(q) if q in QUEUES else int(args.queue)
    if not 0 <= queue < len(QUEUES):
        ap.error("--queue: a name of %s or 0..6" % ", ".join(QUEUES))

    from ebpf_emu import Program, pcap
    from ebpf_emu import workloads as W

    if os.path.exists(args.prog):
        from ebpf_emu import hexs_to_u8s

        image = bytes(hexs_to_u8s(open(args.prog).read()))
    else:
        image = W.program(args.prog)
    with open(args.input, "rb") as f:
        cap = pcap.Capture(f.read(), device=args.device)
    prog = Program(image)
    data = cap.filter(prog, queue, writeback=args.writeback, snaplen=args.snaplen,
                      packets_per_chunk=args.chunk, mem_size=args.mem_size)
    prog.close()
    with open(args.output, "wb") as f:
        f.write(data)
    kept = len(pcap.index(data)[0])
    print(f"{args.output}: {kept} of {cap.n} records (queue {QUEUES[queue]}), {len(data)} bytes")


if __name__ == "__main__":
    main()
