#!/usr/bin/env python3
"""Split a capture into one capture per receive queue, as a NIC's RSS would deliver it: the
Toeplitz hash of every packet (ebpf_rss_hash), the stable partition by the default indirection
table (ebpf_steer), then one ebpf_pcap_gather per queue with the source's own record headers, so
timestamps and orig_len survive and a flow's packets stay in one file, in order. All on the GPU.

  python tools/pcap_steer.py IN.pcap --queues N [--key HEX] [--types T[,T...]] --out PREFIX

writes PREFIX.q<k>.pcap for k = 0..N-1. --key: 40 bytes of hex, `msft` (the Microsoft
specification's key, the default) or `symmetric` (6d5a repeated: both directions of a flow in one
queue). --types: the inputs hashed, of ipv4, ipv4-tcp, ipv4-udp, ipv6, ipv6-tcp, ipv6-udp, or `all`
(the default) / `ip` (addresses only).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebpf-emu_amd"))

TYPES = {"ipv4": 1, "ipv4-tcp": 2, "ipv4-udp": 4, "ipv6": 8, "ipv6-tcp": 16, "ipv6-udp": 32,
         "all": 63, "ip": 9}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input")
    ap.add_argument("--queues", type=int, required=True)
    ap.add_argument("--key", default="msft")
    ap.add_argument("--types", default="all")
    ap.add_argument("--out", required=True)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    from ebpf_emu import _lib, pcap, rss
    from ebpf_emu.queues import pcap_gather

    if not 1 <= args.queues <= rss.STEER_MAX_QUEUES:
        ap.error(f"--queues: 1..{rss.STEER_MAX_QUEUES}")
    key = {"msft": rss.MSFT_KEY, "symmetric": rss.SYMMETRIC_KEY}.get(args.key) or bytes.fromhex(args.key)
    if len(key) != 40:
        ap.error("--key: 40 bytes of hex, msft or symmetric")
    types = 0
    for t in args.types.split(","):
        if t not in TYPES:
            ap.error("--types: of " + ", ".join(TYPES))
        types |= TYPES[t]

    with open(args.input, "rb") as f:
        data = np.frombuffer(f.read(), dtype=np.uint8)
    offs, lens, _ = pcap.index(data)
    n = len(offs)
    file_header = bytes(data[:24])
    flags = _lib.PCAP_SRC_RECORDS | pcap.header_flag(file_header)
    dev = torch.device("cuda", args.device)
    # the capture as it lies is the batch: every packet has its record header 16 bytes before it
    frames = torch.from_numpy(data.copy()).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int32)).to(dev)
    d_lens = torch.from_numpy(lens.view(np.int16)).to(dev)
    h, _ = rss.rss_hash(frames, key, types, offsets=d_offs, lens=d_lens, n=n)
    st = rss.steer(h, args.queues)
    out = total = None
    for k in range(args.queues):
        if n == 0:  # (no batch: pcap_gather writes nothing, not even the totals)
            with open(f"{args.out}.q{k}.pcap", "wb") as f:
                f.write(file_header)
            continue
        out, total = pcap_gather(frames, *st.queue(k), file_header, flags=flags, offsets=d_offs,
                                 lens=d_lens, n=n, out=out, total=total)
        records, end = (int(x) & 0xFFFFFFFF for x in total.cpu())
        path = f"{args.out}.q{k}.pcap"
        with open(path, "wb") as f:
            f.write(out[:end].cpu().numpy().tobytes())
        print(f"{path}: {records} of {n} records, {end} bytes")


if __name__ == "__main__":
    main()
