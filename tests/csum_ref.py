"""The Python model of ebpf_csum_verify and ebpf_csum_fill (include/ebpf_emu.h): the definition the
tests compare the kernel with, written from the header's text alone (plain loops over bytes, no
kernel structure, nothing shared with ebpf_emu/csum.py), and the builders of the test packets
(rss_ref's Ethernet / IP builders, with real TCP / UDP headers and valid checksums on top)."""
import json
import os
import struct

import numpy as np

import rss_ref as R

IPV4_HDR, TCP, UDP = 1, 2, 4
ALL = 7
L3_GOOD, L3_BAD, L4_GOOD, L4_BAD, L4_NONE = 1, 2, 4, 8, 16
NQUEUES = 7


def vectors():
    """-> the published answers of tests/golden/csum_vectors.json."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "csum_vectors.json")
    with open(path) as f:
        return json.load(f)


def fold(t):
    while t >> 16:
        t = (t & 0xFFFF) + (t >> 16)
    return t


def sum16(b):
    """The plain integer sum of the big-endian 16-bit words; an odd last byte is a high byte."""
    b = bytes(b)
    if len(b) & 1:
        b += b"\0"
    return sum((b[i] << 8) | b[i + 1] for i in range(0, len(b), 2))


def queue_class(v):
    return v if v < 5 else 6 if v == 0xFF else 5


def selected(v, queue_mask):
    return v is None or bool((queue_mask >> queue_class(v)) & 1)


def parse(pkt, what):
    """-> (l3, l4): l3 = (o, H) when the IPv4 header checksum is looked at, else None; l4 = (p, L,
    field offset inside the packet, pseudo-header sum, is_udp, is_v4) when an L4 checksum is, else
    None. Only pkt[0:len(pkt)] exists: every field is looked at only after the length covers it."""
    pkt = bytes(pkt)
    ln = len(pkt)
    none = (None, None)
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

    def be16(at):
        return (pkt[at] << 8) | pkt[at + 1]

    def l4_of(proto, p, L, addrs, v4):
        if p + L > ln:
            return None
        if proto == 6 and what & TCP and L >= 20:
            at, udp = p + 16, False
        elif proto == 17 and what & UDP and L >= 8 and be16(p + 4) == L:
            at, udp = p + 6, True
        else:
            return None
        return (p, L, at, sum16(addrs) + proto + L, udp, v4)

    if et == 0x0800:
        if ln < o + 20:
            return none
        ihl = pkt[o] & 15
        H = 4 * ihl
        if pkt[o] >> 4 != 4 or ihl < 5 or ln < o + H:
            return none
        l3 = (o, H) if what & IPV4_HDR else None
        T = be16(o + 2)
        l4 = None
        if T >= H and o + T <= ln and be16(o + 6) & 0x3FFF == 0:
            l4 = l4_of(pkt[o + 9], o + H, T - H, pkt[o + 12:o + 20], True)
        return l3, l4
    if et == 0x86DD:
        if ln < o + 40 or pkt[o] >> 4 != 6:
            return none
        return None, l4_of(pkt[o + 6], o + 40, be16(o + 4), pkt[o + 8:o + 40], False)
    return none


def verify(pkt, what=ALL):
    """-> the status byte of one (selected) packet."""
    pkt = bytes(pkt)
    l3, l4 = parse(pkt, what)
    st = 0
    if l3:
        o, H = l3
        st |= L3_GOOD if fold(sum16(pkt[o:o + H])) == 0xFFFF else L3_BAD
    if l4:
        p, L, at, pseudo, udp, v4 = l4
        if udp and v4 and pkt[at] == 0 and pkt[at + 1] == 0:
            st |= L4_NONE
        else:
            st |= L4_GOOD if fold(pseudo + sum16(pkt[p:p + L])) == 0xFFFF else L4_BAD
    return st


def fill(pkt, what=ALL):
    """-> (the packet with its fields filled, the status byte) of one (selected) packet."""
    out = bytearray(pkt)
    l3, l4 = parse(bytes(pkt), what)
    st = 0
    if l3:
        o, H = l3
        out[o + 10:o + 12] = b"\0\0"
        out[o + 10:o + 12] = struct.pack(">H", ~fold(sum16(out[o:o + H])) & 0xFFFF)
        st |= L3_GOOD
    if l4:
        p, L, at, pseudo, udp, _ = l4
        out[at:at + 2] = b"\0\0"
        val = ~fold(pseudo + sum16(out[p:p + L])) & 0xFFFF
        if udp and val == 0:
            val = 0xFFFF
        out[at:at + 2] = struct.pack(">H", val)
        st |= L4_GOOD
    return bytes(out), st


def verify_batch(pkts, what=ALL, verdict=None, queue_mask=0x7F):
    """-> status u8[n]."""
    return np.array([verify(p, what) if selected(None if verdict is None else int(verdict[i]), queue_mask)
                     else 0 for i, p in enumerate(pkts)], dtype=np.uint8)


def fill_batch(pkts, what=ALL, verdict=None, queue_mask=0x7F):
    """-> ([packet bytes], status u8[n])."""
    out, st = [], []
    for i, p in enumerate(pkts):
        if selected(None if verdict is None else int(verdict[i]), queue_mask):
            q, s = fill(p, what)
        else:
            q, s = bytes(p), 0
        out.append(q)
        st.append(s)
    return out, np.array(st, dtype=np.uint8)


# ---------------------------------------------------------------- packets
def tcp(sport, dport, payload=b"", csum=0):
    return struct.pack(">HHIIBBHHH", sport, dport, 0x01020304, 0x0A0B0C0D, 0x50, 0x18, 0x2000, csum,
                       0) + bytes(payload)


def udp(sport, dport, payload=b"", length=None, csum=0):
    return struct.pack(">HHHH", sport, dport, 8 + len(payload) if length is None else length,
                       csum) + bytes(payload)


def body(n, seed=0):
    """n payload bytes, no two neighbours equal."""
    return bytes((seed + 7 * i + (i >> 3)) & 0xFF for i in range(n))


def valid(frame):
    """The frame with every checksum this library knows filled in."""
    return fill(frame, ALL)[0]


def frame4(proto, seg, tags=(), valid_sums=True, **kw):
    f = R.eth(0x0800, tags) + R.ipv4("10.1.2.3", "192.168.77.9", proto, seg, **kw)
    return valid(f) if valid_sums else f


def frame6(nh, seg, tags=(), valid_sums=True, **kw):
    f = R.eth(0x86DD, tags) + R.ipv6("2001:db8::1:2", "2001:db8:ffff::9", nh, seg, **kw)
    return valid(f) if valid_sums else f


def flip(frame, at, bit=0x10):
    """One bit of byte `at` flipped (at < 0: from the end)."""
    f = bytearray(frame)
    f[at] ^= bit
    return bytes(f)


def set_be16(frame, at, val):
    f = bytearray(frame)
    f[at:at + 2] = struct.pack(">H", val & 0xFFFF)
    return bytes(f)


def udp_sum_zero(frame_of):
    """frame_of(payload) -> a UDP frame; -> that frame with a 10-byte payload whose computed checksum
    is 0, so that fill stores 0xFFFF. The payload's last word makes up the difference."""
    pay = bytearray(body(8, 3) + b"\0\0")
    f = frame_of(bytes(pay))
    _, l4 = parse(f, ALL)
    p, L, at, pseudo, is_udp, _ = l4
    z = bytearray(f)
    z[at:at + 2] = b"\0\0"
    c0 = fold(pseudo + sum16(z[p:p + L]))
    assert is_udp and 0 < c0 <= 0xFFFF and (p + L - 2 - p) % 2 == 0
    pay[8:10] = struct.pack(">H", 0xFFFF - c0)
    g = frame_of(bytes(pay))
    assert fill(g, ALL)[0] == g and g[at:at + 2] == b"\xff\xff"
    return g


def parser_kinds():
    """{name: frame}: every branch of the parse and of the sums' conditions (the tests truncate each
    at every length). Frames are at most 128 bytes; checksums are valid unless the name says not."""
    t, u = tcp(4321, 443, body(7)), udp(53, 60000, body(5, 9))
    k = {
        "untagged": frame4(6, t),
        "tag1": frame4(6, t, (0x8100,)),
        "tag2": frame4(17, u, (0x88A8, 0x8100)),
        "tag3": frame4(6, t, (0x88A8, 0x8100, 0x8100)),
        "ihl6": frame4(6, t, ihl=6),
        "ihl15": frame4(17, u, ihl=15),
        "mf": frame4(6, t, frag=0x2000),
        "fragoff": frame4(17, u, frag=0x0003),
        "df": frame4(6, t, frag=0x4000),  # DF alone is no fragment
        "udp": frame4(17, u),
        "icmp": frame4(1, t),
        "badver4": frame4(6, t, ver=5),
        "ihl4": frame4(6, t, ihl=4),
        "v6tcp": frame6(6, t),
        "v6udp": frame6(17, u, (0x8100,)),
        "v6hbh": frame6(0, bytes([6, 0, 0, 0, 0, 0, 0, 0]) + t),
        "badver6": frame6(6, t, ver=4),
        "arp": R.eth(0x0806) + bytes(range(28)),
    }
    # corrupted checksums: the header's, the L4 one, a payload byte, an address (pseudo-header)
    k["bad_l3"] = flip(k["untagged"], 14 + 8)              # TTL
    k["bad_l3_field"] = flip(k["udp"], 14 + 10)
    k["bad_tcp_field"] = flip(k["untagged"], 14 + 20 + 16)
    k["bad_tcp_payload"] = flip(k["untagged"], -1)
    k["bad_udp_payload"] = flip(k["udp"], -2)
    k["bad_both"] = flip(flip(k["tag1"], 18 + 8), -3)
    k["bad_v6tcp"] = flip(k["v6tcp"], -1)
    k["bad_v6udp_addr"] = flip(k["v6udp"], 18 + 8 + 5)
    k["bad_opts"] = flip(k["ihl6"], 14 + 21)               # an option byte: L3 only
    # UDP over IPv4 without a checksum; over IPv6 a zero field is summed like any other
    k["udp_none"] = set_be16(k["udp"], 14 + 20 + 6, 0)
    k["udp_none_opts"] = set_be16(k["ihl15"], 14 + 60 + 6, 0)
    k["udp_none_bad_l3"] = flip(k["udp_none"], 14 + 8)
    k["v6udp_zero_field"] =set_be16(k["v6udp"], 18 + 40 + 6, 0)
    # UDP's own length against L
    k["udp_len_short"] = frame4(17, udp(53, 60000, body(5, 9), length=12))
    k["udp_len_long"] = frame4(17, udp(53, 60000, body(5, 9), length=14))
    k["v6udp_len_short"] = frame6(17, udp(53, 60000, body(5, 9), length=12))
    # the total length: shorter than the header, equal to it, past len; padding behind the datagram
    k["tot_lt_hdr"] = valid(set_be16(k["untagged"], 14 + 2, 19))
    k["tot_eq_hdr"] = valid(set_be16(k["untagged"], 14 + 2, 20))
    k["tot_past_len"] = valid(set_be16(k["untagged"], 14 + 2, 20 + len(t) + 1))
    k["padded"] = frame4(6, t) + bytes([0x5A, 0xA5] * 5)
    k["padded_udp_odd"] = frame4(17, u) + bytes([0xC3] * 7)
    k["v6_padded"] = frame6(17, u) + bytes([0x3C] * 3)
    k["v6_plen_past_len"] = valid(set_be16(k["v6tcp"], 14 + 4, len(t) + 1))
    # L4 lengths around the minimums (UDP 7 / 8, TCP 19 / 20)
    k["udp_l7"] = frame4(17, udp(53, 9, b"")[:7])
    k["udp_l8"] = frame4(17, udp(53, 9, b""))
    k["tcp_l19"] = frame4(6, tcp(80, 9)[:19])
    k["tcp_l20"] = frame4(6, tcp(80, 9))
    k["v6udp_l7"] = frame6(17, udp(53, 9, b"")[:7])
    k["v6udp_l8"] = frame6(17, udp(53, 9, b""))
    k["v6tcp_l19"] = frame6(6, tcp(80, 9)[:19])
    k["v6tcp_l20"] = frame6(6, tcp(80, 9))
    # a computed UDP checksum of 0 is sent as 0xFFFF
    k["udp_sum0"] = udp_sum_zero(lambda pay: frame4(17, udp(53, 60000, pay)))
    k["v6udp_sum0"] = udp_sum_zero(lambda pay: frame6(17, udp(53, 60000, pay)))
    assert all(len(v) <= 128 for v in k.values())
    return k
