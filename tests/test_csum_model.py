"""ebpf_csum_verify / ebpf_csum_fill without a GPU: the model (tests/csum_ref.py) against published
answers that do not come from it, against itself (verify after fill), and over the parser matrix
the GPU tests use, whose statuses must reach every value the status byte can take."""
import functools

import csum_ref as C


def test_published_vectors():
    v = C.vectors()
    r = v["rfc1071"]
    b = bytes.fromhex(r["bytes"])
    assert f"{C.fold(C.sum16(b)):04x}" == r["sum"]
    assert f"{~C.fold(C.sum16(b)) & 0xFFFF:04x}" == r["checksum"]
    assert C.fold(C.sum16(b + bytes.fromhex(r["checksum"]))) == 0xFFFF
    assert C.sum16(b"\x12") == 0x1200 and C.sum16(b"\x12\x34\x56") == 0x1234 + 0x5600
    h = v["ipv4_header"]
    hdr = bytes.fromhex(h["bytes"])
    assert f"{C.fold(C.sum16(hdr)):04x}" == h["folded"] and hdr[10:12].hex() == h["field"]
    # as a frame: the header verifies, and fill puts the published field back
    frame = C.R.eth(0x0800) + hdr + bytes(0x73 - 20)
    assert C.verify(frame, C.IPV4_HDR) == C.L3_GOOD
    assert C.verify(C.flip(frame, 14 + 10), C.IPV4_HDR) == C.L3_BAD
    wiped = C.set_be16(frame, 14 + 10, 0x1234)
    out, st = C.fill(wiped, C.IPV4_HDR)
    assert out == frame and st == C.L3_GOOD


def test_rfc1071_bytes_as_a_udp_payload():
    """The RFC's 8 bytes as a UDP payload: the field is the complement of the published sum plus
    the pseudo-header and UDP header words, added by hand here."""
    pay = bytes.fromhex(C.vectors()["rfc1071"]["bytes"])
    f = C.frame4(17, C.udp(53, 60000, pay), valid_sums=False)
    out, st = C.fill(f, C.UDP)
    words = [0x0A01, 0x0203, 0xC0A8, 0x4D09, 17, 16, 53, 60000, 16, 0, 0xDDF2]
    assert out[14 + 20 + 6:14 + 20 + 8].hex() == f"{~C.fold(sum(words)) & 0xFFFF:04x}"
    assert st == C.L4_GOOD and C.verify(out, C.UDP) == C.L4_GOOD


def test_verify_after_fill_is_all_good():
    for name, f in C.parser_kinds().items():
        for what in range(1, 8):
            out, st = C.fill(f, what)
            again = C.verify(out, what)
            assert again & (C.L3_BAD | C.L4_BAD | C.L4_NONE) == 0, (name, what)
            assert again == st, (name, what)  # GOOD exactly where a field was written
            assert len(out) == len(f)
            assert C.fill(out, what) == (out, st), (name, what, "fill is idempotent")


@functools.lru_cache(maxsize=None)
def _matrix_status():
    return {(name, ln): C.verify(f[:ln], C.ALL)
            for name, f in C.parser_kinds().items() for ln in range(len(f) + 1)}


def test_matrix_reaches_every_status():
    """A matrix that stops reaching a branch fails here instead of passing quietly."""
    st = _matrix_status()
    seen = set(st.values())
    l3 = (C.L3_GOOD, C.L3_BAD)
    l4 = (C.L4_GOOD, C.L4_BAD, C.L4_NONE)
    want = {0} | set(l3) | {a | b for a in l3 for b in l4} | {C.L4_GOOD, C.L4_BAD}
    assert seen == want, (sorted(seen), sorted(want))
    full = {name: C.verify(f, C.ALL) for name, f in C.parser_kinds().items()}
    assert full["untagged"] == full["tag2"] == full["ihl15"] == full["df"] == C.L3_GOOD | C.L4_GOOD
    assert full["tag3"] == full["arp"] == full["badver4"] == full["ihl4"] == full["badver6"] == 0
    assert full["mf"] == full["fragoff"] == full["icmp"] == C.L3_GOOD
    assert full["v6tcp"] == full["v6udp"] == C.L4_GOOD and full["v6hbh"] == 0
    assert full["bad_l3"] == full["bad_l3_field"] == full["bad_opts"] == C.L3_BAD | C.L4_GOOD
    assert full["bad_tcp_field"] == full["bad_tcp_payload"] == full["bad_udp_payload"] == C.L3_GOOD | C.L4_BAD
    assert full["bad_both"] == C.L3_BAD | C.L4_BAD
    assert full["bad_v6tcp"] == full["bad_v6udp_addr"] == full["v6udp_zero_field"] == C.L4_BAD
    assert full["udp_none"] == full["udp_none_opts"] == C.L3_GOOD | C.L4_NONE
    assert full["udp_none_bad_l3"] == C.L3_BAD | C.L4_NONE
    for name in ("udp_len_short", "udp_len_long", "tot_lt_hdr", "tot_eq_hdr", "tot_past_len", "udp_l7",
                 "tcp_l19"):
        assert full[name] == C.L3_GOOD, name
    for name in ("v6udp_len_short", "v6_plen_past_len", "v6udp_l7", "v6tcp_l19"):
        assert full[name] == 0, name
    for name in ("padded", "padded_udp_odd", "udp_l8", "tcp_l20", "udp_sum0"):
        assert full[name] == C.L3_GOOD | C.L4_GOOD, name
    for name in ("v6_padded", "v6udp_l8", "v6tcp_l20", "v6udp_sum0"):
        assert full[name] == C.L4_GOOD, name
    # the bytes behind the datagram are padding: any value gives the same answer
    assert C.verify(C.flip(C.parser_kinds()["padded"], -1), C.ALL) == C.L3_GOOD | C.L4_GOOD


def test_what_masks_and_selection():
    k = C.parser_kinds()
    assert C.verify(k["bad_both"], C.IPV4_HDR) == C.L3_BAD
    assert C.verify(k["bad_both"], C.TCP) == C.L4_BAD
    assert C.verify(k["bad_both"], C.UDP) == 0
    assert C.verify(k["udp"], C.TCP | C.IPV4_HDR) == C.L3_GOOD
    pk = [k["bad_both"]] * 9
    verdict = [0, 1, 2, 3, 4, 5, 0xFD, 0xFE, 0xFF]
    st = C.verify_batch(pk, C.ALL, verdict, (1 << 3) | (1 << 5))
    assert st.tolist() == [0, 0, 0, 10, 0, 10, 10, 10, 0]
    st = C.verify_batch(pk, C.ALL, verdict, 1 << 6)
    assert st.tolist() == [0] * 8 + [10]
    out, st = C.fill_batch(pk, C.ALL, verdict, 1 << 2)
    assert [o == pk[0] for o in out] == [True, True, False] + [True] * 6
    assert st.tolist() == [0, 0, 5, 0, 0, 0, 0, 0, 0]
