"""CPU: the DHCP service's host side (include/halo_rx.h, "DHCP") against tests/dhcp_model.py —
halo_dhcp_decode_host bit for bit into prefilled outputs, every HALO_E_INVAL answer of both decode
entry points and both build entry points, the lease table and state machine on the named cases and
on seeded random traces, halo_dhcp_reply_build_host for every kind, the round trip build -> decode,
and the descriptors through the CPU transmit-build oracle."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import dhcp_cases as C
from tests import dhcp_model as M

FILL = C.FILL
NET24 = dict(ip=0xC0A80101, network_mask=0xFFFFFF00, dns=0x08080808, mac=bytes([2, 0, 0, 0, 0, 1]))


def host_decode(d, msg_cap):
    from halo_amd import _lib

    got = dict(msgs=np.full((msg_cap + 1, 128), FILL, np.uint8), summary=np.full(64 + 8, FILL, np.uint8))
    rc = _lib.lib.halo_dhcp_decode_host(_lib.ptr(d.out), _lib.ptr(d.summary_raw), _lib.ptr(d.index_raw), d.index_cap,
                                        _lib.ptr(got["msgs"]), msg_cap, _lib.ptr(got["summary"]))
    assert rc == 0
    return got


CASES = C.crafted()


def test_crafted_set_covers_every_status_and_type():
    w = C.Delivery(C.dhcp_items(CASES)).want(len(CASES))
    assert (w.summary["status_counts"] > 0).all() and (w.summary["type_counts"] > 0).all()
    assert int(w.summary["msgs"]) == len(CASES) >= 100


def test_crafted_set_in_one_call():
    d = C.Delivery(C.dhcp_items(CASES))
    C.check_outputs(host_decode(d, len(CASES)), d.want(len(CASES)), len(CASES), "all")


@pytest.mark.parametrize("chunk", range(4))
def test_every_crafted_case_alone(chunk):
    for name, payload, ports in CASES[chunk::4]:
        d = C.Delivery([(C.DHCP, ports[0], ports[1], payload)], exact=True)
        C.check_outputs(host_decode(d, 1), d.want(1), 1, name)


def test_named_semantics():
    """What the issue states, read off the model's records (which the calls must equal)."""
    w = {n: m for (n, _, _), m in zip(CASES, C.Delivery(C.dhcp_items(CASES)).want(len(CASES)).msgs)}
    assert [int(w[n]["status"]) for n in ("len0", "len239", "len240_panic", "len241_ff", "len241_one_byte", "len1472")] == \
        [M.SHORT, M.SHORT, M.REF_PANIC, M.OK, M.OK, M.OK]
    assert all(int(w[f"cookie_byte{i}"]["status"]) == M.COOKIE for i in range(4))
    assert int(w["to_server"]["dir"]) == M.TO_SERVER and int(w["to_client"]["dir"]) == M.TO_CLIENT
    assert int(w["to_client"]["yiaddr"]) == 0xC0A80164
    for n in ("ports_68_68", "ports_67_67", "ports_1234_67"):
        assert int(w[n]["status"]) == M.PORTS and not w[n]["xid"].any()
    assert int(w["no_53"]["status"]) == M.OK and not int(w["no_53"]["options"]) & M.OPT_MSG_TYPE
    assert int(w["53_twice"]["msg_type"]) == 3
    assert int(w["53_len0_before"]["status"]) == int(w["53_len0_after"]["status"]) == M.REF_PANIC
    assert int(w["ends_at_end_panic"]["status"]) == M.REF_PANIC and int(w["ends_one_before_end"]["status"]) == M.OK
    assert int(w["one_short_of_end"]["options"]) == M.OPT_MSG_TYPE
    assert int(w["code0_tlv"]["msg_type"]) == 1 and int(w["overrun_hides_53"]["options"]) == M.OPT_HOSTNAME
    assert [int(w[f"opt50_len{n}"]["req_ip"]) for n in (0, 3, 4, 5)] == [0, 0, 0x0A0B0C0D, 0]
    assert [int(w[f"opt1_len{n}"]["mask_n"]) for n in range(6)] == [0, 1, 2, 3, 4, 4]
    assert bytes(w["opt3_len5"]["gateway"]) == bytes([200, 201, 202, 203])
    for n in range(9):
        bits = int(w[f"opt6_len{n}"]["options"])
        assert bits & (M.OPT_DNS | M.OPT_DNS_SHORT) == (M.OPT_DNS if n >= 4 else M.OPT_DNS_SHORT)
    assert bytes(w["opt6_len8"]["dns"]) == bytes([100, 101, 102, 103])
    h = w["hostname_a1_len255"]["hostname"]
    assert int(h[63]) == 63 and bytes(h[:63]) == C.rnd(16 + 255, 255)[:63]
    assert bytes(w["hostname_last_wins"]["hostname"][:4]) == b"2nd\0" and int(w["hostname_last_wins"]["hostname"][63]) == 3
    assert bytes(w["300_empty_options"]["hostname"][:4]) == b"late" and int(w["300_empty_options"]["msg_type"]) == 1


def test_capacity_cuts_and_other_records():
    items = []
    for i, (name, payload, ports) in enumerate(CASES[:40]):
        items.append((C.UDP, 4000, 22102, C.rnd(i, 5 + i)))
        items.append((C.DHCP, ports[0], ports[1], payload))
        items.append((C.TCP, 4000, 67, b"x" * (i % 7)))  # a TCP record to port 67 is not DHCP
    for cap in (0, 1, 17, 39, 40, 41):
        d = C.Delivery(items)
        want = d.want(cap)
        assert int(want.summary["msgs"]) == 40 and int(want.summary["msgs_written"]) == min(cap, 40)
        C.check_outputs(host_decode(d, cap), want, cap, f"cap{cap}")
    # unwritten records, and an index_cap below the record count
    d = C.Delivery(items, unwritten=9)
    C.check_outputs(host_decode(d, 64), d.want(64), 64, "unwritten")
    d = C.Delivery(items, index_cap=50)
    want = d.want(64)
    assert int(want.summary["msgs"]) == 17
    C.check_outputs(host_decode(d, 64), want, 64, "index_cap")
    d = C.Delivery([])
    got = host_decode(d, 4)
    assert got["summary"][:64].tobytes() == bytes(64) and (got["msgs"] == FILL).all()


def test_every_inval_answer():
    from halo_amd import _lib

    buf = np.zeros(4096 + 64, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 64
    _, answers = C.decode_entry_answers(base, send_well_formed=False)
    _, build_answers = C.build_entry_answers(base, send_well_formed=False)
    assert len(answers) >= 16 and len(build_answers) >= 9
    for what, rc in answers + build_answers:
        assert rc == _lib.HALO_E_INVAL, (what, rc)
    L = _lib.lib
    at = dict(stream=base, dsum=base + 64, summary=base + 128, msgs=base + 256, index=base + 1024)
    for kw in (dict(summary=None), dict(dsum=None), dict(stream=None), dict(index=None), dict(msgs=None)):
        a = {**at, **kw}
        assert L.halo_dhcp_decode_host(a["stream"], a["dsum"], a["index"], 300, a["msgs"], 4, a["summary"]) == _lib.HALO_E_INVAL, kw
    cfg = _lib.DhcpConfig()
    for args in ((None, base, 2, base + 256, base + 64), (ctypes.byref(cfg), None, 2, base + 256, base + 64),
                 (ctypes.byref(cfg), base, 2, None, base + 64), (ctypes.byref(cfg), base, 2, base + 256, None),
                 (ctypes.byref(cfg), base, (1 << 23) + 1, base + 256, base + 64)):
        assert L.halo_dhcp_reply_build_host(*args) == _lib.HALO_E_INVAL
    assert not buf.any()


# ---- the lease table and the state machine ----------------------------------------------------
def both(**cfg):
    from halo_amd.dhcp import DhcpServer

    return DhcpServer(**cfg), M.Server(**cfg)


def step(pair, msgs, now, what=""):
    """Handles msgs in both and compares replies, verdicts, events and the lease tables bit for bit."""
    srv, mod = pair
    msgs = np.array(msgs, M.MSG)
    r = srv.handle(msgs, now)
    replies, verdicts, events = mod.handle(msgs, now)
    assert r.verdicts.tolist() == verdicts.tolist(), (what, r.verdicts, verdicts)
    assert r.replies.tobytes() == replies.tobytes(), (what, r.replies, replies)
    assert r.events.tobytes() == events.tobytes(), (what, r.events, events)
    assert srv.leases().tobytes() == mod.leases().tobytes(), what
    return r


def test_ack_then_nak_pair():
    pair = both(**NET24)
    r = step(pair, [C.rec(M.REQUEST, req_ip=0xC0A80132, hostname=b"laptop")], 1000)
    assert r.replies["kind"].tolist() == [M.ACK, M.NAK] and r.verdicts[0] == M.H_ACK_NAK | M.H_F_REPLY
    assert int(r.replies[0]["yiaddr"]) == 0xC0A80132 and int(r.replies[1]["yiaddr"]) == 0
    l = pair[0].leases()
    assert len(l) == 1 and int(l[0]["exp_time"]) == 4600 and bytes(l[0]["hostname"][:6]) == b"laptop" and int(l[0]["hostname"][63]) == 6
    # a renewal with a shorter name keeps the bytes behind it (StaticString64.Set copies, never clears)
    r = step(pair, [C.rec(M.REQUEST, req_ip=0xC0A80132, hostname=b"pc")], 2000)
    assert r.verdicts[0] == M.H_ACK_NAK | M.H_F_REUSED | M.H_F_REPLY
    assert bytes(pair[0].leases()[0]["hostname"][:6]) == b"pcptop"


def test_empty_hostname_panic_and_each_nak_reason_in_order():
    pair = both(capacity=1, **NET24)
    other = bytes([2, 9, 9, 9, 9, 9])
    r = step(pair, [C.rec(M.REQUEST, req_ip=0xC0A80132),                              # no option 12
                    C.rec(M.REQUEST, req_ip=0xC0A80132, hostname=b""),                 # option 12 of length 0
                    C.rec(M.REQUEST, hostname=b"x"),                                  # no option 50: nothing
                    C.rec(M.REQUEST, req_ip=[1, 2, 3], hostname=b"x"),                 # IpAddrToU of 3 bytes = 0
                    C.rec(M.REQUEST, req_ip=0xC0A80232, hostname=b"x"),                # other subnet
                    C.rec(M.REQUEST, req_ip=0xC0A80132, hostname=b"x"),                # ACK + NAK, the table is now full
                    C.rec(M.REQUEST, req_ip=0xC0A80132, hostname=b"x", chaddr=other),  # another MAC's
                    C.rec(M.REQUEST, req_ip=0xC0A80133, hostname=b"x", chaddr=other),  # capacity
                    C.rec(M.REQUEST, req_ip=0xC0A80133, chaddr=other)], 7)            # capacity comes before the panic
    codes = [int(v) & 0x0F for v in r.verdicts]
    assert codes == [M.H_REF_PANIC, M.H_REF_PANIC, M.H_NO_REQ_IP, M.H_NAK_ZERO, M.H_NAK_SUBNET, M.H_ACK_NAK, M.H_NAK_OTHER_MAC,
                     M.H_NAK_FULL, M.H_NAK_FULL]
    assert r.replies["kind"].tolist() == [M.NAK, M.NAK, M.ACK, M.NAK, M.NAK, M.NAK, M.NAK]
    assert len(pair[0].leases()) == 1


def test_discover_scan_reuse_and_full_subnet():
    pair = both(**NET24)
    # no lease yet: every DISCOVER of a batch is offered the same first address, .1 is the server's
    r = step(pair, [C.rec(M.DISCOVER), C.rec(M.DISCOVER, chaddr=bytes(6))], 0)
    assert r.replies["yiaddr"].tolist() == [0xC0A80102, 0xC0A80102]
    step(pair, [C.rec(M.REQUEST, req_ip=0xC0A80102, hostname=b"a"), C.rec(M.REQUEST, req_ip=0xC0A80105, hostname=b"b", chaddr=bytes(6))], 0)
    r = step(pair, [C.rec(M.DISCOVER, req_ip=0xC0A80102),                # reuse: its own lease
                    C.rec(M.DISCOVER, req_ip=0xC0A80105),                # another MAC's lease: the scan
                    C.rec(M.DISCOVER, req_ip=[1, 2, 3, 4, 5])], 0)       # IpAddrToU = 0
    assert r.replies["yiaddr"].tolist() == [0xC0A80102, 0xC0A80103, 0xC0A80103]
    assert int(r.verdicts[0]) == M.H_OFFER | M.H_F_REUSED | M.H_F_REPLY
    # fill the /24: hostBits = 32 - popcount(192.168.1.0) = 26, so the scan runs past it into 192.168.2.x
    fill = [C.rec(M.REQUEST, req_ip=0xC0A80100 + i, hostname=b"f", chaddr=bytes([2, 0, 0, 0, 1, i])) for i in range(2, 255)]
    step(pair, fill, 0)
    r = step(pair, [C.rec(M.DISCOVER, chaddr=bytes([2, 7, 7, 7, 7, 7]))], 0)
    assert r.replies["yiaddr"].tolist() == [0xC0A80201]


def test_host_bits_32_and_a_wrapping_scan():
    pair = both(ip=0x0A000001, network_mask=0, dns=0, mac=bytes(6))  # network address 0: hostBits == 32, nothing is scanned
    r = step(pair, [C.rec(M.DISCOVER)], 0)
    assert int(r.verdicts[0]) == M.H_NO_ADDR and len(r.replies) == 0
    pair = both(ip=0xFFFFFFFE, network_mask=0xFFFFFFFC, dns=0, mac=bytes(6))  # a /30: hostBits == 2; .252 .253 (.254 own) .255
    r = step(pair, [C.rec(M.DISCOVER)], 0)
    assert r.replies["yiaddr"].tolist() == [0xFFFFFFFC | 0]  # last octet 252 is neither 0 nor 255
    step(pair, [C.rec(M.REQUEST, req_ip=0xFFFFFFFC, hostname=b"a"), C.rec(M.REQUEST, req_ip=0xFFFFFFFD, hostname=b"b")], 0)
    assert int(step(pair, [C.rec(M.DISCOVER, chaddr=bytes(6))], 0).verdicts[0]) == M.H_NO_ADDR


def test_release_expiry_and_the_u32_wrap():
    pair = both(**NET24)
    step(pair, [C.rec(M.REQUEST, req_ip=0xC0A80110, hostname=b"a"), C.rec(M.REQUEST, req_ip=0xC0A80111, hostname=b"b")], 100)
    # RELEASE is keyed by the SOURCE address, whatever the MAC
    r = step(pair, [C.rec(M.RELEASE, remote_ip=0xC0A80111, chaddr=bytes(6)), C.rec(M.RELEASE, remote_ip=0xC0A80155)], 100)
    assert [int(v) for v in r.verdicts] == [M.H_RELEASED, M.H_RELEASE_ABSENT] and pair[0].leases()["ip"].tolist() == [0xC0A80110]
    for now, gone in ((3700, 0), (3701, 1)):  # now > ExpTime
        assert pair[0].clear(now) == pair[1].clear(now) == gone
    assert len(pair[0].leases()) == 0
    step(pair, [C.rec(M.REQUEST, req_ip=0xC0A80110, hostname=b"a")], 0xFFFFFFFF - 100)
    assert int(pair[0].leases()[0]["exp_time"]) == 3499  # (now + 3600) mod 2^32
    assert pair[0].clear(3499) == pair[1].clear(3499) == 0 and pair[0].clear(3500) == pair[1].clear(3500) == 1


def test_disabled_sides_and_statuses_do_nothing():
    pair = both(server_enable=False, **NET24)
    assert not step(pair, [C.rec(M.DISCOVER), C.rec(M.REQUEST, req_ip=0xC0A80110, hostname=b"a")], 0).verdicts.any()
    pair = both(**NET24)
    msgs = [C.rec(M.DISCOVER, status=s) for s in (M.PORTS, M.SHORT, M.COOKIE, M.REF_PANIC)] + [C.rec(None), C.rec(4), C.rec(8)]
    msgs.append(C.rec(M.OFFER, dir=M.TO_CLIENT))  # client side disabled
    assert not step(pair, msgs, 0).verdicts.any()


def test_client_offer_and_ack_with_each_option_missing():
    cfg = dict(ip=0, network_mask=0, dns=0, mac=bytes([2, 1, 2, 3, 4, 5]), server_enable=False, client_enable=True)
    pair = both(**cfg)
    offer = C.rec(M.OFFER, dir=M.TO_CLIENT, yiaddr=0xC0A80142, remote_ip=0xC0A80101)
    assert not step(pair, [offer], 0).verdicts.any()  # no transaction id yet: nothing matches nil
    d, dm = pair[0].discover(C.XID), pair[1].discover(C.XID)
    assert d.tobytes() == np.array([dm], M.REPLY).tobytes() and int(d[0]["kind"]) == M.DISCOVER
    r = step(pair, [offer, C.rec(M.OFFER, dir=M.TO_CLIENT, xid=b"\0\0\0\1")], 0)
    assert [int(v) for v in r.verdicts] == [M.H_CLIENT_REQUEST | M.H_F_REPLY, M.H_NONE]
    q = r.replies[0]
    assert (int(q["kind"]), int(q["req_ip"]), int(q["server_id"]), bytes(q["chaddr"])) == (M.REQUEST, 0xC0A80142, 0xC0A80101, cfg["mac"])
    full = dict(mask=[255, 255, 255, 0], gateway=[192, 168, 1, 1], dns=[8, 8, 8, 8])
    acks = [C.rec(M.ACK, dir=M.TO_CLIENT, yiaddr=0xC0A80142, **{k: v for k, v in full.items() if k != drop}) for drop in (None, *full)]
    acks.append(C.rec(M.ACK, dir=M.TO_CLIENT, yiaddr=0xC0A80142, mask=[255, 255], gateway=[10], dns=[1, 2, 3]))
    r = step(pair, acks, 0)
    assert [int(v) for v in r.verdicts] == [M.H_CLIENT_ACK] * 5 and r.events["options"].tolist() == [7, 6, 5, 3, 3]
    assert r.events["msg"].tolist() == [0, 1, 2, 3, 4] and r.events["mask_n"].tolist() == [4, 0, 4, 4, 2]
    # a client that has an address ignores the server's messages
    pair = both(**{**cfg, "ip": 0xC0A80142})
    pair[0].discover(C.XID), pair[1].discover(C.XID)
    assert not step(pair, [offer], 0).verdicts.any()


def random_trace(seed, n, net, prefix_hosts):
    rng = np.random.default_rng(seed)
    macs = [bytes([2, 0, 0, 0, 0, i]) for i in range(12)]
    names = [b"", b"a", b"host-%d" % seed, C.rnd(seed, 63), C.rnd(seed + 1, 70), None]
    out = []
    for i in range(n):
        t = int(rng.choice([M.DISCOVER, M.REQUEST, M.REQUEST, M.RELEASE, M.OFFER, 0]))
        ip = int(rng.choice([net + int(rng.integers(0, prefix_hosts)), net + 256 + int(rng.integers(0, 4)), 0]))
        req = None if rng.random() < 0.1 else (C.rnd(i, 3) if rng.random() < 0.05 else ip)
        out.append(C.rec(t or None, chaddr=macs[int(rng.integers(0, len(macs)))], req_ip=req, hostname=names[int(rng.integers(0, len(names)))],
                         remote_ip=net + int(rng.integers(0, prefix_hosts)), status=M.OK if rng.random() < 0.95 else M.SHORT, index=i))
    return out


@pytest.mark.parametrize("seed,cfg,hosts", [(1, dict(NET24, capacity=6), 16), (2, dict(NET24, capacity=300), 256),
                                            (3, dict(ip=0x0A0000FD, network_mask=0xFFFFFFFC, dns=1, mac=bytes(6), capacity=2), 4),
                                            (4, dict(ip=0x0A0000FD, network_mask=0xFFFFFFFC, dns=1, mac=bytes(6), capacity=64), 4)])
def test_random_traces(seed, cfg, hosts):
    pair = both(**cfg)
    net = cfg["ip"] & cfg["network_mask"]
    trace = random_trace(seed, 3000, net, hosts)
    seen = set()
    for b in range(0, len(trace), 250):
        now = 500 * (b // 250)
        r = step(pair, trace[b:b + 250], now, f"batch{b}")
        seen |= {int(v) & 0x0F for v in r.verdicts}
        if b % 500 == 0:
            assert pair[0].clear(now) == pair[1].clear(now)
    assert {M.H_OFFER, M.H_ACK_NAK, M.H_REF_PANIC, M.H_RELEASED, M.H_NAK_ZERO, M.H_NO_REQ_IP} <= seen
    assert len(pair[0].leases()) <= cfg["capacity"]


def test_handle_msgs_argument_checks():
    from halo_amd import _lib

    L = _lib.lib
    srv, _ = both(**NET24)
    msgs = np.array([C.rec(M.DISCOVER)] * 3, M.MSG)
    replies, events, verdicts = np.zeros(6, M.REPLY), np.zeros(3, M.EVENT), np.zeros(3, np.uint8)
    nr, ne = ctypes.c_uint32(), ctypes.c_uint32()
    p = _lib.ptr

    def call(s=srv._h, m=p(msgs), r=p(replies), rcap=6, nrp=ctypes.byref(nr), e=p(events), ecap=3):
        return L.halo_dhcp_handle_msgs(s, m, 3, 0, r, rcap, p(verdicts), nrp, e, ecap, ctypes.byref(ne))

    assert call() == 0 and nr.value == 3
    assert call(e=None, ecap=0) == 0
    for kw in (dict(s=None), dict(m=None), dict(r=None), dict(rcap=5), dict(nrp=None), dict(ecap=2), dict(e=None, ecap=3)):
        assert call(**kw) == _lib.HALO_E_INVAL, kw


# ---- the reply build -----------------------------------------------------------------------------
def some_replies():
    r = np.zeros(7, M.REPLY)
    r["kind"] = [M.OFFER, M.ACK, M.NAK, M.REQUEST, M.DISCOVER, 4, 0]
    r["xid"] = [list(C.rnd(i, 4)) for i in range(7)]
    r["yiaddr"] = [0xC0A80132, 0xC0A801FE, 0, 0, 0, 5, 0]
    r["chaddr"] = [list(C.rnd(10 + i, 6)) for i in range(7)]
    r["req_ip"], r["server_id"] = 0xC0A80142, 0xC0A80101
    return r


def test_build_replies_host_equals_the_model_for_every_kind():
    from halo_amd.dhcp import DhcpServer, build_replies_host

    srv = DhcpServer(**NET24)
    r = some_replies()
    got = build_replies_host(r, config=srv)
    slots, descs = M.build(r, NET24["ip"], NET24["network_mask"], NET24["dns"])
    assert got.slots().tobytes() == slots.tobytes()
    assert got.descs().tobytes() == descs.tobytes()
    assert descs["payload_len"].tolist() == [286, 286, 250, 270, 258, 0, 0]
    assert [len(p) for p in got.payloads()] == [286, 286, 250, 270, 258, 0, 0]
    srv.set_dns(0x01010101)  # the setter reaches the build
    assert build_replies_host(r[:1], config=srv).payloads()[0][240 + 3 + 12 + 2:][:4] == bytes([1, 1, 1, 1])


def test_round_trip_build_then_decode():
    """build -> decode_host gives back the fields that went in; and with the options parsed as a SET
    (a dict), a check that does not depend on the order this build fixed."""
    from halo_amd.dhcp import DhcpServer, build_replies_host

    srv = DhcpServer(**NET24)
    r = some_replies()[:5]
    got = build_replies_host(r, config=srv)
    payloads, descs = got.payloads(), got.descs()
    items = [(C.DHCP, int(d["src_port"]), int(d["dst_port"]), p) for p, d in zip(payloads, descs)]
    dl = C.Delivery(items)
    out = host_decode(dl, 5)
    C.check_outputs(out, dl.want(5), 5, "round trip")
    m = out["msgs"][:5].reshape(-1).view(M.MSG)
    assert m["status"].tolist() == [M.OK] * 5 and m["msg_type"].tolist() == r["kind"].tolist()
    assert m["dir"].tolist() == [M.TO_CLIENT] * 3 + [M.TO_SERVER] * 2
    assert m["xid"].tobytes() == r["xid"].tobytes() and m["chaddr"].tobytes() == r["chaddr"].tobytes()
    assert m["yiaddr"].tolist() == r["yiaddr"].tolist()
    assert int(m[3]["req_ip"]) == 0xC0A80142
    for i in (0, 1):
        assert bytes(m[i]["mask"]) == M.u_to_ip(NET24["network_mask"]) and bytes(m[i]["gateway"]) == M.u_to_ip(NET24["ip"])
        assert bytes(m[i]["dns"]) == M.u_to_ip(NET24["dns"])
    be = lambda v: v.to_bytes(4, "big")  # noqa: E731
    ip = be(NET24["ip"])
    want_sets = [{53: bytes([k]), 1: be(NET24["network_mask"]), 3: ip, 6: be(NET24["dns"]), 51: be(3600), 59: be(3150), 58: be(1800), 54: ip}
                 for k in (M.OFFER, M.ACK)]
    want_sets.append({53: bytes([M.NAK]), 54: ip})
    want_sets.append({53: bytes([M.REQUEST]), 61: b"\x01" + bytes(r[3]["chaddr"]), 50: be(0xC0A80142), 54: be(0xC0A80101), 55: bytes([1, 3, 6])})
    want_sets.append({53: bytes([M.DISCOVER]), 61: b"\x01" + bytes(r[4]["chaddr"]), 55: bytes([1, 3, 6])})
    for p, want in zip(payloads, want_sets):
        o, i, seen = p[240:], 0, {}
        while o[i] != 0xFF:
            seen[o[i]] = o[i + 2:i + 2 + o[i + 1]]
            i += 2 + o[i + 1]
        assert seen == want and i + 1 == len(o)
        assert p[0] == (2 if want[53][0] in (M.OFFER, M.ACK, M.NAK) else 1) and p[1:4] == bytes([1, 6, 0]) and p[10:12] == b"\x80\0"


def test_descs_through_the_build_oracle():
    """The descriptors and the slots handed to the CPU transmit build (the tx oracle): broadcast
    Ethernet frames whose UDP payload is the message."""
    from halo_amd.dhcp import DhcpServer, build_replies_host
    from oracle import oracle

    srv = DhcpServer(**NET24)
    got = build_replies_host(some_replies()[:5], config=srv)
    desc, payloads = got.descs().view(M.DESC), got.payloads()
    frames, lens, res, _ = oracle.tx_build_batch(desc, got.slots().reshape(-1), NET24["mac"], 1, 1516, 7)
    assert not res.any()
    for j, p in enumerate(payloads):
        f = frames[j].tobytes()
        assert int(lens[j]) == 42 + len(p) and f[42:42 + len(p)] == p
        assert f[:6] == b"\xff" * 6 and f[6:12] == NET24["mac"] and f[23] == 17
        assert int.from_bytes(f[26:30], "big") == NET24["ip"] and f[30:34] == b"\xff" * 4
        assert (int.from_bytes(f[34:36], "big"), int.from_bytes(f[36:38], "big")) == ((67, 68) if j < 3 else (68, 67))
        assert int.from_bytes(f[38:40], "big") == 8 + len(p)


def test_rx_dhcp_is_a_dispatch_consumer():
    """DeliverResult.dispatch(netif, dhcp=server.rx_dhcp): RxDhcp's arguments, one datagram at a time."""
    from halo_amd.deliver import DeliverResult
    from halo_amd.dhcp import DhcpServer

    srv, mod = both(**NET24)
    assert isinstance(srv, DhcpServer)
    items = [(C.DHCP, 68, 67, C.discover()), (C.DHCP, 68, 67, C.request(0xC0A80102, b"box")), (C.DHCP, 68, 68, C.discover()),
             (C.DHCP, 68, 67, C.release())]
    d = C.Delivery(items)
    r = DeliverResult(d.region_bytes, d.index_cap, d.out, d.summary_raw, d.index_raw)
    srv.time_now = 50
    assert r.dispatch(None, dhcp=srv.rx_dhcp) == 4
    msgs = d.want(4).msgs
    replies, _, _ = mod.handle(msgs, 50)
    assert np.array(srv.tx_queue, M.REPLY).tobytes() == replies.tobytes() and replies["kind"].tolist() == [M.OFFER, M.ACK, M.NAK]
    assert srv.leases().tobytes() == mod.leases().tobytes()
