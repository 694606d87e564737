#!/usr/bin/env python3
"""Check a capture's checksums as a NIC's RX side would, and optionally fix them as its TX side
would: ebpf_csum_verify over the capture as it lies (the IPv4 header checksum, TCP and UDP over
IPv4 and IPv6), the counts per status bit, and with --fix OUT an ebpf_csum_fill in place and the
capture written back out, record headers and all. All on the GPU.

  python tools/pcap_csum.py IN.pcap [--what W[,W...]] [--fix OUT.pcap]

--what: the checksums looked at, of ipv4, tcp, udp, or `all` (the default). A capture of the `nat`
workload's XDP_TX queue (tools/pcap_filter.py) shows every redirected packet L4_BAD; --fix is the
checksum offload that makes it what a capture tool accepts.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebpf-emu_amd"))

WHAT = {"ipv4": 1, "tcp": 2, "udp": 4, "all": 7}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input")
    ap.add_argument("--what", default="all")
    ap.add_argument("--fix", metavar="OUT")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    from ebpf_emu import csum, pcap

    what = 0
    for w in args.what.split(","):
        if w not in WHAT:
            ap.error("--what: of " + ", ".join(WHAT))
        what |= WHAT[w]

    with open(args.input, "rb") as f:
        data = np.frombuffer(f.read(), dtype=np.uint8)
    offs, lens, _ = pcap.index(data)
    n = len(offs)
    dev = torch.device("cuda", args.device)
    # the capture as it lies is the batch: fill writes the fields inside the file's own bytes
    frames = torch.from_numpy(data.copy()).to(dev)
    kw = dict(offsets=torch.from_numpy(offs.view(np.int32)).to(dev),
              lens=torch.from_numpy(lens.view(np.int16)).to(dev), n=n)

    def report(tag, st):
        st = st.cpu().numpy()
        parts = [f"{name}={int(((st & bit) != 0).sum())}" for name, bit in csum.STATUS_BITS]
        print(f"{tag}: {n} packets, unchecked={int((st == 0).sum())} " + " ".join(parts))
        return st

    st = report(args.input, csum.csum_verify(frames, what, **kw))
    if args.fix:
        csum.csum_fill(frames, what, **kw)
        after = report(args.fix, csum.csum_verify(frames, what, **kw))
        with open(args.fix, "wb") as f:
            f.write(frames.cpu().numpy().tobytes())
        print(f"{args.fix}: {int((st != after).sum())} packets changed status")


if __name__ == "__main__":
    main()
