"""TEST INFRASTRUCTURE ONLY: the DHCP service's crafted payloads and the helpers its CPU and GPU
tests share — a message encoder, a delivery stream made by hand from (kind, remote_port, local_port,
payload) items (tests/kcp_cases.Delivery's layout, which fixes the remote port; here it is the
case's), the bit-for-bit comparison of a call's prefilled outputs with tests/dhcp_model.py, and the
argument-check lists."""
from __future__ import annotations

import struct

import numpy as np

from tests import dhcp_model as M
from tests.kcp_cases import DHCP, FILL, TCP, UDP, rnd  # noqa: F401

MAC = bytes([0x02, 0xAA, 0xBB, 0xCC, 0xDD, 0x01])
XID = bytes([0x12, 0x34, 0x56, 0x78])
S, C = (68, 67), (67, 68)  # (remote_port, local_port): to the server, to the client


def tlv(code, data=b"") -> bytes:
    return bytes([code, len(data)]) + bytes(data)


def msg(opts=(), *, xid=XID, yiaddr=0, chaddr=MAC, op=1, end=True, tail=b"", cookie=M.COOKIE_BYTES) -> bytes:
    """A BOOTP header, the cookie, the options ((code, data) pairs or raw bytes), 0xff when ``end``, ``tail``."""
    fixed = bytes([op, 1, 6, 0]) + bytes(xid) + bytes([0, 0, 0x80, 0]) + bytes(4) + M.u_to_ip(yiaddr) + bytes(8) + bytes(chaddr) + bytes(10)
    fixed += bytes(64) + bytes(128) + cookie
    assert len(fixed) == 240
    body = b"".join(o if isinstance(o, (bytes, bytearray)) else tlv(*o) for o in opts)
    return fixed + body + (b"\xff" if end else b"") + tail


def discover(hostname=b"host", req_ip=None, **kw) -> bytes:
    o = [(53, [M.DISCOVER])] + ([(50, M.u_to_ip(req_ip))] if req_ip is not None else []) + ([(12, hostname)] if hostname is not None else [])
    return msg(o, **kw)


def request(req_ip, hostname=b"host", **kw) -> bytes:
    o = [(53, [M.REQUEST])] + ([(50, M.u_to_ip(req_ip))] if req_ip is not None else []) + ([(12, hostname)] if hostname is not None else [])
    return msg(o, **kw)


def release(**kw) -> bytes:
    return msg([(53, [M.RELEASE])], **kw)


def crafted():
    """[(name, payload, (remote_port, local_port))] — the cases the issue names."""
    T = (53, [1])
    out = [("len0", b"", S), ("len239", msg()[:239], S), ("len240_panic", msg(end=False), S), ("len241_ff", msg(), S),
           ("len241_one_byte", msg(end=False, tail=b"\x35"), S), ("len1472", msg([T, (12, b"big")], tail=rnd(1, 1472 - 249)), S)]
    assert len(out[-1][1]) == 1472
    for i in range(4):
        c = bytearray(M.COOKIE_BYTES)
        c[i] ^= 0x40
        out.append((f"cookie_byte{i}", msg([T], cookie=bytes(c)), S))
    out += [("to_server", msg([T]), S), ("to_client", msg([(53, [2])], op=2, yiaddr=0xC0A80164), C)]
    out += [(f"ports_{r}_{l}", msg([T]), (r, l)) for r, l in ((68, 68), (67, 67), (1234, 67))]
    out += [(f"type{t}", msg([(53, [t]), (50, [10, 0, 0, t]), (12, b"n%d" % t)]), S) for t in range(9)]
    out.append(("type_200", msg([(53, [200])]), S))
    out.append(("no_53", msg([(12, b"quiet"), (50, [10, 0, 0, 9])]), S))
    out.append(("53_twice", msg([(53, [1]), (12, b"x"), (53, [3])]), S))
    out.append(("53_len2", msg([(53, [7, 9])]), S))
    out.append(("53_len0_before", msg([(53, []), (53, [1])]), S))
    out.append(("53_len0_after", msg([(53, [1]), (53, [])]), S))
    out.append(("ends_at_end_panic", msg([T, (12, b"abc")], end=False), S))
    out.append(("ends_one_before_end", msg([T, (12, b"abc")], end=False, tail=b"\x07"), S))  # the one-byte break
    out.append(("one_short_of_end", msg([T], end=False, tail=bytes([12, 4]) + b"abc"), S))  # length 4, three bytes: overrun
    out.append(("overrun_255", msg([T], end=False, tail=bytes([12, 255]) + b"abcdefgh"), S))
    out.append(("overrun_hides_53", msg([(12, b"n")], end=False, tail=bytes([50, 9, 1, 2, 3, 4]) + tlv(53, [1]) + b"\xff"), S))
    out.append(("code0_tlv", msg([(0, [53, 1, 3]), T]), S))            # the inner 53 is data
    out.append(("code0_len0", msg([(0, []), (0, []), T]), S))
    out.append(("ff_inside_data", msg([(12, b"\xff\xff"), T]), S))
    out.append(("after_ff_ignored", msg([T], tail=tlv(53, [3]) + tlv(50, [1, 2, 3, 4])), S))
    out += [(f"opt50_len{n}", msg([(53, [3]), (50, bytes(range(10, 10 + n))), (12, b"h")]), S) for n in (0, 3, 4, 5)]
    out.append(("opt50_twice", msg([(53, [3]), (50, [10, 0, 0, 5]), (50, [10, 0, 0])]), S))
    for code in (1, 3):
        out += [(f"opt{code}_len{n}", msg([(53, [5]), (code, bytes(range(200, 200 + n)))], op=2), C) for n in range(6)]
    out += [(f"opt6_len{n}", msg([(53, [5]), (6, bytes(range(100, 100 + n)))], op=2), C) for n in range(9)]
    out.append(("opt6_short_then_ok", msg([(53, [5]), (6, [1, 2]), (6, [8, 8, 4, 4])], op=2), C))
    out.append(("opt6_ok_then_short", msg([(53, [5]), (6, [8, 8, 4, 4]), (6, [1, 2, 3])], op=2), C))
    for a in range(4):  # a leading code-0 option of a data bytes moves the name through the four alignments
        for n in (0, 1, 3, 4, 62, 63, 64, 255):
            out.append((f"hostname_a{a}_len{n}", msg([(0, bytes(a)), (53, [3]), (50, [10, 0, 0, 7]), (12, rnd(16 * a + n, n))]), S))
    out.append(("hostname_last_wins", msg([T, (12, b"first-and-longer"), (12, b"2nd")]), S))
    out.append(("300_empty_options", msg([(7, [])] * 300 + [T, (12, b"late")]), S))
    out.append(("all_options_client", msg([(53, [5]), (1, [255, 255, 255, 0]), (3, [192, 168, 1, 1]), (6, [8, 8, 8, 8]),
                                           (51, [0, 0, 14, 16]), (54, [192, 168, 1, 1])], op=2, yiaddr=0xC0A80142), C))
    return out


class Delivery:
    """A delivery made by hand: what halo_amd.deliver.DeliverResult shows, for the model and the
    calls. items: (kind, remote_port, local_port, payload); ``unwritten`` further records lie beyond
    the region (index offset 0xFFFFFFFF); ``index_cap`` defaults to every record. ``out`` is sized
    exactly to the stream (no byte behind its last word) when ``exact``."""

    def __init__(self, items, *, unwritten=0, index_cap=None, exact=False):
        parts, offs = [], []
        at = 0
        for i, (kind, rport, lport, payload) in enumerate(items):
            offs.append(at)
            rec = struct.pack("<IBBHIHHII", i * 3 + 1, kind, 0x18 if kind == TCP else 0, len(payload), 0x0A000001 + i, rport, lport,
                              i, 2 * i) + payload
            rec += bytes(-len(rec) % 4)
            parts.append(rec)
            at += len(rec)
        self.records_total = len(items) + unwritten
        self.index_cap = self.records_total if index_cap is None else index_cap
        self.region_bytes = at if exact else (at + 15) & ~15
        self.out = np.full(max(self.region_bytes + (0 if exact else 16), 1), 0xEE, np.uint8)  # bytes beyond bytes_written are not the stream's
        self.out[:at] = np.frombuffer(b"".join(parts), np.uint8)
        summary = np.zeros(1, np.dtype([("records", "<u4"), ("records_written", "<u4"), ("bytes", "<u8"), ("bytes_written", "<u8"),
                                        ("kind_counts", "<u4", (3,)), ("skipped", "<u4")]))
        summary["records"], summary["records_written"] = self.records_total, len(items)
        summary["bytes"], summary["bytes_written"] = at + 48 * unwritten, at
        self.summary_raw = summary.view(np.uint8).reshape(-1)
        index = np.zeros((max(self.index_cap, 1), 2), np.uint32)
        n = min(self.index_cap, self.records_total)
        index[:n, 0] = 3 * np.arange(n) + 1
        index[:n, 1] = 0xFFFFFFFF
        m = min(n, len(items))
        index[:m, 1] = offs[:m]
        self.index = index
        self.index_raw = index.view(np.uint8).reshape(-1, 8)
        self.bytes_written = at

    def want(self, msg_cap) -> M.Want:
        return M.decode(self.out, self.records_total, self.index, self.index_cap, msg_cap)


def dhcp_items(cases):
    return [(DHCP, ports[0], ports[1], payload) for _, payload, ports in cases]


def minimal_record_stream(n, dhcp_at, payload):
    """A delivery of n records built with numpy: empty UDP records (24 bytes) to port 9 except at the
    indices ``dhcp_at``, which carry ``payload`` as a 68 -> 67 DHCP record. Returns a Delivery-like
    object."""
    dhcp_at = np.asarray(sorted(dhcp_at))
    plen = len(payload)
    size = np.full(n, 24, np.int64)
    size[dhcp_at] = 24 + ((plen + 3) & ~3)
    offs = np.concatenate([[0], np.cumsum(size)[:-1]])
    total = int(size.sum())
    d = Delivery.__new__(Delivery)
    d.records_total, d.index_cap, d.bytes_written = n, n, total
    d.region_bytes = (total + 15) & ~15
    out = np.zeros(d.region_bytes + 16, np.uint8)
    hdr = np.zeros(n, np.dtype([("frame", "<u4"), ("kind", "u1"), ("flags", "u1"), ("plen", "<u2"), ("rip", "<u4"), ("rport", "<u2"),
                                ("lport", "<u2"), ("seq", "<u4"), ("ack", "<u4")]))
    hdr["frame"], hdr["kind"], hdr["rip"], hdr["rport"], hdr["lport"] = np.arange(n), UDP, 0x0A000001 + np.arange(n), 5000, 9
    hdr["kind"][dhcp_at], hdr["plen"][dhcp_at], hdr["rport"][dhcp_at], hdr["lport"][dhcp_at] = DHCP, plen, 68, 67
    raw = hdr.view(np.uint8).reshape(n, 24)
    idx = (offs[:, None] + np.arange(24)[None, :]).reshape(-1)
    out[idx] = raw.reshape(-1)
    body = np.frombuffer(payload, np.uint8)
    for o in offs[dhcp_at]:
        out[o + 24:o + 24 + plen] = body
    out[total:] = 0xEE
    d.out = out
    summary = np.zeros(1, np.dtype([("records", "<u4"), ("records_written", "<u4"), ("bytes", "<u8"), ("bytes_written", "<u8"),
                                    ("kind_counts", "<u4", (3,)), ("skipped", "<u4")]))
    summary["records"], summary["records_written"], summary["bytes"], summary["bytes_written"] = n, n, total, total
    d.summary_raw = summary.view(np.uint8).reshape(-1)
    index = np.zeros((n, 2), np.uint32)
    index[:, 0], index[:, 1] = np.arange(n), offs
    d.index, d.index_raw = index, index.view(np.uint8).reshape(-1, 8)
    return d


def check_outputs(got, want: M.Want, msg_cap, what=""):
    """got: dict(msgs=[msg_cap + 1, 128] u8, summary=[64 + 8] u8), each 0xA5-prefilled with a
    sentinel element behind it."""
    s = got["summary"][:64].view(M.SUMMARY)[0]
    for f in M.SUMMARY.names:
        assert np.array_equal(s[f], want.summary[f]), (what, f, s[f], want.summary[f])
    assert (got["summary"][64:] == FILL).all(), (what, "summary sentinel")
    n = int(s["msgs_written"])
    assert n == len(want.msgs) <= msg_cap, what
    m = got["msgs"][:n].reshape(-1).view(M.MSG)
    for f in M.MSG.names:
        bad = np.flatnonzero((m[f] != want.msgs[f]).reshape(n, -1).any(axis=1)) if n else []
        assert len(bad) == 0, (what, f, bad[:5], m[f][bad[:5]], want.msgs[f][bad[:5]])
    assert got["msgs"][:n].tobytes() == want.msgs.tobytes(), what
    assert (got["msgs"][n:] == FILL).all(), (what, "written beyond the prefix")


def decode_entry_answers(base: int, send_well_formed: bool = True):
    """halo_dhcp_decode_device's argument checks over 64-byte-aligned addresses from ``base`` (4 KiB of
    zeros: an empty delivery, every array whole and apart): returns (well_formed, [(what, answer)]) —
    the answer of a well-formed call (None when not sent), and of calls that each differ from it in
    one argument and must be HALO_E_INVAL. Nothing is dereferenced before the checks, so host
    addresses serve where there is no device."""
    from halo_amd import _lib

    L = _lib.lib
    wsb = int(L.halo_dhcp_decode_workspace(300))
    assert wsb == 8
    # stream 64 B | delivery summary 40 | summary 64 | workspace 8 | msgs 4 x 128 | index 300 x 8
    at = dict(stream=base, dsum=base + 64, summary=base + 128, ws=base + 192, msgs=base + 256, index=base + 1024)
    assert at["index"] + 8 * 300 <= base + 4096

    def call(msg_cap=4, cap=300, ws_bytes=wsb, **ptr):
        a = {**at, **ptr}
        return L.halo_dhcp_decode_device(a["stream"], a["dsum"], a["index"], cap, a["msgs"], msg_cap, a["summary"], a["ws"], ws_bytes, None)

    bad = [dict(summary=None), dict(dsum=None), dict(stream=None), dict(index=None), dict(msgs=None), dict(ws=None),
           dict(ws_bytes=wsb - 1), dict(ws_bytes=0),
           # one per documented alignment: msgs 16; index, both summaries, workspace 8; stream 4
           dict(msgs=at["msgs"] + 8), dict(msgs=at["msgs"] + 4), dict(index=at["index"] + 4), dict(summary=at["summary"] + 4),
           dict(dsum=at["dsum"] + 4), dict(ws=at["ws"] + 4), dict(stream=base + 2), dict(stream=base + 1)]
    return (call() if send_well_formed else None), [(kw, call(**kw)) for kw in bad]


def build_entry_answers(base: int, send_well_formed: bool = True):
    """The same for halo_dhcp_reply_build_device: replies 2 x 32 at base, descs at base + 64, payload
    at base + 256 (two slots)."""
    import ctypes

    from halo_amd import _lib

    L = _lib.lib
    cfg = _lib.DhcpConfig()
    at = dict(replies=base, descs=base + 64, payload=base + 256)

    def call(n=2, cfg_null=False, **ptr):
        a = {**at, **ptr}
        return L.halo_dhcp_reply_build_device(None if cfg_null else ctypes.byref(cfg), a["replies"], n, a["payload"], a["descs"], None)

    bad = [dict(cfg_null=True), dict(replies=None), dict(descs=None), dict(payload=None), dict(n=(1 << 23) + 1),
           dict(replies=base + 8), dict(descs=base + 68), dict(payload=base + 258), dict(payload=base + 257)]
    return (call() if send_well_formed else None), [(kw, call(**kw)) for kw in bad]


# ---- message records by hand, for the state machine's tests -----------------------------------
def rec(msg_type=None, *, dir=M.TO_SERVER, status=M.OK, xid=XID, chaddr=MAC, req_ip=None, hostname=None, remote_ip=0, yiaddr=0,
        mask=None, gateway=None, dns=None, index=0):
    """One MSG record as the decode would write it for such a message."""
    opts = [] if msg_type is None else [(53, [msg_type])]
    if req_ip is not None:
        opts.append((50, req_ip if isinstance(req_ip, (bytes, list)) else M.u_to_ip(req_ip)))
    for code, v in ((12, hostname), (1, mask), (3, gateway), (6, dns)):
        if v is not None:
            opts.append((code, v))
    ports = S if dir == M.TO_SERVER else C
    m = M.decode_one(index, remote_ip, ports[0], ports[1], msg(opts, xid=xid, chaddr=chaddr, yiaddr=yiaddr))
    if status != M.OK:
        m["status"] = status
    return m
