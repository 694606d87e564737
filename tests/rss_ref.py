"""The Python / numpy model of ebpf_rss_hash and ebpf_steer (include/ebpf_emu.h): the definition
the tests compare the kernels with, written from the header's text alone (plain loops, no kernel
structure, nothing shared with ebpf_emu/rss.py), and the builders of the test packets."""
import ipaddress
import json
import os
import struct

import numpy as np

IPV4, IPV4_TCP, IPV4_UDP, IPV6, IPV6_TCP, IPV6_UDP = 1, 2, 4, 8, 16, 32
ALL = 63
MAX_QUEUES, MAX_RETA = 64, 128
SYMMETRIC_KEY = bytes.fromhex("6d5a" * 20)


def msft():
    """-> (key bytes, vectors) of tests/golden/rss_msft_vectors.json."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rss_msft_vectors.json")
    with open(path) as f:
        d = json.load(f)
    return bytes.fromhex(d["key"]), d["vectors"]


def toeplitz(key, data):
    """Bit by bit: for every set bit i of data (MSB of byte 0 first) XOR in key bits [i, i + 32)."""
    kbits = int.from_bytes(bytes(key), "big")
    nk = 8 * len(key)
    h = 0
    for i in range(8 * len(data)):
        if data[i // 8] & (0x80 >> (i % 8)):
            assert i + 32 <= nk
            h ^= (kbits >> (nk - 32 - i)) & 0xFFFFFFFF
    return h


def rss_input(pkt, types):
    """The parse: -> (input bytes, type bit), or (b"", 0) when the packet is not hashed. Only
    pkt[0:len(pkt)] exists: every field is looked at only after the length covers it."""
    pkt = bytes(pkt)
    ln = len(pkt)
    none = (b"", 0)
    o, tags = 14, 0
    while True:
        if ln < o:
            return none
        et = (pkt[o - 2] << 8) | pkt[o - 1]
        if et not in (0x8100, 0x88A8):
            break
        tags += 1
        if tags == 3:
            return none
        o += 4
    if et == 0x0800:
        if ln < o + 20:
            return none
        ihl = pkt[o] & 15
        if pkt[o] >> 4 != 4 or ihl < 5:
            return none
        frag = ((pkt[o + 6] << 8) | pkt[o + 7]) & 0x3FFF
        proto = pkt[o + 9]
        l4 = {6: IPV4_TCP, 17: IPV4_UDP}.get(proto, 0)
        at = o + 4 * ihl
        if frag == 0 and l4 & types and ln >= at + 4:
            return pkt[o + 12:o + 20] + pkt[at:at + 4], l4
        if types & IPV4:
            return pkt[o + 12:o + 20], IPV4
        return none
    if et == 0x86DD:
        if ln < o + 40 or pkt[o] >> 4 != 6:
            return none
        l4 = {6: IPV6_TCP, 17: IPV6_UDP}.get(pkt[o + 6], 0)
        if l4 & types and ln >= o + 44:
            return pkt[o + 8:o + 44], l4
        if types & IPV6:
            return pkt[o + 8:o + 40], IPV6
        return none
    return none


def rss(pkt, key, types=ALL):
    """-> (hash, type) of one packet."""
    data, ty = rss_input(pkt, types)
    return (toeplitz(key, data), ty) if ty else (0, 0)


def rss_batch(pkts, key, types=ALL):
    """-> (hash u32[n], type u8[n])."""
    out = [rss(p, key, types) for p in pkts]
    return (np.array([h for h, _ in out], dtype=np.uint32), np.array([t for _, t in out], dtype=np.uint8))


def default_reta(nq):
    return [j % nq for j in range(MAX_RETA)]


def steer(keys, nq, reta=None):
    """-> (index u32[n], bounds u32[nq][2], queue i64[n]): a stable argsort by queue."""
    reta = np.asarray(default_reta(nq) if reta is None else reta, dtype=np.int64)
    assert len(reta) in (1, 2, 4, 8, 16, 32, 64, 128) and np.all(reta < nq)
    k = np.asarray(keys).view(np.uint32).astype(np.int64)
    q = reta[k & (len(reta) - 1)] if len(k) else np.zeros(0, dtype=np.int64)
    index = np.argsort(q, kind="stable").astype(np.uint32)
    count = np.bincount(q, minlength=nq).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    bounds = np.stack([start, count], axis=1).astype(np.uint32)
    return index, bounds, q


# ---------------------------------------------------------------- packets
def _addr(a):
    return ipaddress.ip_address(a).packed


def eth(ethertype, tags=()):
    """14 bytes of Ethernet plus one 4-byte tag per entry of tags (each a VLAN ethertype)."""
    out = bytes(range(0x10, 0x1C))
    for i, t in enumerate(tags):
        out += struct.pack(">HH", t, 0x0100 + i)
    return out + struct.pack(">H", ethertype)


def ipv4(src, dst, proto, payload, ihl=5, frag=0, ver=4):
    opts = bytes((0x40 + i) & 0xFF for i in range(4 * max(ihl, 5) - 20))
    hdr = struct.pack(">BBHHHBBH", (ver << 4) | ihl, 0, 20 + len(opts) + len(payload), 0x1234, frag,
                      64, proto, 0) + _addr(src) + _addr(dst)
    return hdr + opts + payload


def ipv6(src, dst, nh, payload, ver=6):
    return struct.pack(">IHBB", (ver << 28) | 0x12345, len(payload), nh, 64) + _addr(src) + _addr(dst) + payload


def l4(sport, dport, extra=12):
    return struct.pack(">HH", sport, dport) + bytes((0x80 + i) & 0xFF for i in range(extra))


def flow_frame(src, dst, sport, dport, proto=6, tags=()):
    """Ethernet + IP + TCP/UDP for an address pair of either family."""
    if ":" in src:
        return eth(0x86DD, tags) + ipv6(src, dst, proto, l4(sport, dport))
    return eth(0x0800, tags) + ipv4(src, dst, proto, l4(sport, dport))


def parser_kinds():
    """{name: frame}: every branch of the parse (tests/test_rss.py truncates each at every length)."""
    a4, b4 = "10.1.2.3", "192.168.77.9"
    a6, b6 = "2001:db8::1:2", "2001:db8:ffff::9"
    tcp, udp = l4(4321, 443), l4(53, 60000)
    k = {
        "untagged": eth(0x0800) + ipv4(a4, b4, 6, tcp),
        "tag1": eth(0x0800, (0x8100,)) + ipv4(a4, b4, 6, tcp),
        "tag2": eth(0x0800, (0x88A8, 0x8100)) + ipv4(a4, b4, 17, udp),
        "tag3": eth(0x0800, (0x88A8, 0x8100, 0x8100)) + ipv4(a4, b4, 6, tcp),
        "ihl5": eth(0x0800) + ipv4(b4, a4, 6, tcp, ihl=5),
        "ihl6": eth(0x0800) + ipv4(a4, b4, 6, tcp, ihl=6),
        "ihl15": eth(0x0800) + ipv4(a4, b4, 17, udp, ihl=15),
        "mf": eth(0x0800) + ipv4(a4, b4, 6, tcp, frag=0x2000),
        "fragoff": eth(0x0800) + ipv4(a4, b4, 17, udp, frag=0x0003),
        "df": eth(0x0800) + ipv4(a4, b4, 6, tcp, frag=0x4000),  # DF alone is no fragment
        "tcp": eth(0x0800) + ipv4(a4, b4, 6, tcp),
        "udp": eth(0x0800) + ipv4(a4, b4, 17, udp),
        "icmp": eth(0x0800) + ipv4(a4, b4, 1, tcp),
        "badver4": eth(0x0800) + ipv4(a4, b4, 6, tcp, ver=5),
        "ihl4": eth(0x0800) + ipv4(a4, b4, 6, tcp, ihl=4),
        "v6tcp": eth(0x86DD) + ipv6(a6, b6, 6, tcp),
        "v6udp": eth(0x86DD, (0x8100,)) + ipv6(a6, b6, 17, udp),
        "v6hbh": eth(0x86DD) + ipv6(a6, b6, 0, bytes([6, 0, 0, 0, 0, 0, 0, 0]) + tcp),
        "badver6": eth(0x86DD) + ipv6(a6, b6, 6, tcp, ver=4),
        "arp": eth(0x0806) + bytes(range(28)),
    }
    assert all(len(v) <= 128 for v in k.values())
    return k
