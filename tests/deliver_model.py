"""Not a test: a from-scratch statement of local delivery (include/halo_rx.h, "local delivery")
that works from frame BYTES, not records. A frame is parsed with the Python restatement of the rx
path (oracle/ref_py.py), the engine branch is taken with the engine restatement there (engine_rx /
engine_lo), and for a frame the reference hands to a service — RxUdp (engine/udp_engine.go:10-21),
RxTcp (engine/tcp_engine.go:10-26), RxUdpBroadcast's DHCP ports (engine/udp_engine.go:35-44) — the
handler's arguments are taken from the parsers' return values: the payload is the slice the parser
returns, never a record's payload_off. `expect` lays the records out as the stream, summary and
index a call must produce for a given region and index cap.
"""
from __future__ import annotations

import struct

import numpy as np

from oracle import ref_py as R

UDP, TCP, DHCP = range(3)
KINDS = 3
HDR = 24
NOT_WRITTEN = 0xFFFFFFFF
DHCP_PORTS = (67, 68)  # DhcpServerPort, DhcpClientPort


class NetIf:
    def __init__(self, mac: bytes, ip: int, nat_enable: bool = False):
        self.mac, self.ip, self.nat_enable = bytes(mac), int(ip), bool(nat_enable)


def delivery_of(buf: bytes, nif: NetIf, *, check_sum_enable=True, jumbo=False, l3=False, udp_ports=(), tcp_ports=(),
                dhcp=False):
    """None, or what the reference hands to a handler for one received frame (or LoChan packet
    with l3): dict(kind, tcp_flags, remote_ip, remote_port, local_port, seq, ack, payload)."""
    c = R.Cfg(check_sum_enable, jumbo)
    if l3:
        act, pkt = R.engine_lo(buf, nif.ip, check_sum_enable, jumbo), buf
    else:
        act, pkt = R.engine_rx(buf, nif.mac, nif.ip, nif.nat_enable, check_sum_enable, jumbo), buf[14:]
    if act not in ("LOCAL_UDP", "LOCAL_TCP", "BCAST_UDP"):
        return None
    ip_payload, _proto, src, dst, _tl, err = R.parse_ipv4_pkt(pkt, c)
    assert not err
    own = nif.ip.to_bytes(4, "big")
    base = dict(tcp_flags=0, remote_ip=R.ip_addr_to_u(src), seq=0, ack=0)
    if act == "LOCAL_TCP":
        pay, sport, dport, seq, ack, flags, err = R.parse_tcp_pkt(ip_payload, src, own, c)
        assert not err
        if dport not in tcp_ports:
            return None
        return dict(base, kind=TCP, tcp_flags=flags, remote_port=sport, local_port=dport, seq=seq, ack=ack, payload=bytes(pay))
    pay, sport, dport, err = R.parse_udp_pkt(ip_payload, src, own if act == "LOCAL_UDP" else dst, c)
    assert not err
    if act == "LOCAL_UDP":
        if dport not in udp_ports:
            return None
        return dict(base, kind=UDP, remote_port=sport, local_port=dport, payload=bytes(pay))
    if not dhcp or dport not in DHCP_PORTS:
        return None
    return dict(base, kind=DHCP, remote_port=sport, local_port=dport, payload=bytes(pay))


def record_bytes(frame: int, d: dict) -> bytes:
    pay = d["payload"]
    hdr = struct.pack("<IBBHIHHII", frame, d["kind"], d["tcp_flags"], len(pay), d["remote_ip"], d["remote_port"],
                      d["local_port"], d["seq"], d["ack"])
    assert len(hdr) == HDR
    return hdr + pay + bytes(-len(pay) % 4)


class Want:
    """The deliveries of a batch: `items` = [(frame, dict)], and what a call must write."""

    def __init__(self, items, skipped=0):
        self.items, self.skipped = items, skipped
        self.recs = [record_bytes(i, d) for i, d in items]
        self.kind_counts = np.bincount([d["kind"] for _, d in items], minlength=KINDS).astype(np.uint32)

    @property
    def total_bytes(self) -> int:
        return sum(map(len, self.recs))

    def expect(self, region: int, index_cap: int):
        """(stream bytes, summary dict, index [(frame, offset)]) for a region and an index cap."""
        stream, index, at, written, cut = bytearray(), [], 0, 0, False
        for (frame, _), rec in zip(self.items, self.recs):
            if not cut and at + len(rec) <= region:
                index.append((frame, at))
                stream += rec
                at += len(rec)
                written += 1
            else:
                cut = True
                index.append((frame, NOT_WRITTEN))
        summary = dict(records=len(self.recs), records_written=written, bytes=self.total_bytes, bytes_written=at,
                       kind_counts=self.kind_counts, skipped=self.skipped)
        return bytes(stream), summary, index[:index_cap]

    def handler_log(self):
        """The calls the reference's handlers see, in order: what recording handlers log."""
        log = []
        for _, d in self.items:
            if d["kind"] == UDP:
                log.append(("udp", d["local_port"], d["remote_ip"], d["remote_port"], d["payload"]))
            elif d["kind"] == TCP:
                log.append(("tcp", d["local_port"], d["remote_ip"], d["remote_port"], d["payload"], d["seq"], d["ack"],
                            d["tcp_flags"]))
            else:
                log.append(("dhcp", d["payload"], d["remote_port"], d["local_port"], d["remote_ip"]))
        return log


def want_of(frames, nif: NetIf, **kw) -> Want:
    items = []
    for i, f in enumerate(frames):
        d = delivery_of(f, nif, **kw)
        if d is not None:
            items.append((i, d))
    return Want(items)
