"""TEST INFRASTRUCTURE ONLY: a from-scratch Python model of the DHCP service (include/halo_rx.h,
"DHCP"), restated from the reference's lines — RxDhcp, ParseDhcpPkt, ParseDhcpOption, BuildDhcpPkt,
BuildDhcpOption, DhcpDiscover, ListDhcp and DhcpLeaseClear (engine/dhcp_engine.go) and
StaticString64.Set (mem/static_allocator.go:213-220). It imports nothing from halo_amd: the record
layouts are written out again here, so that a slip in the package's mirrors shows."""
from __future__ import annotations

import struct

import numpy as np

OK, PORTS, SHORT, COOKIE, REF_PANIC = range(5)
TO_SERVER, TO_CLIENT, DIR_NONE = 0, 1, 2
OPT_MASK, OPT_ROUTER, OPT_DNS, OPT_HOSTNAME, OPT_REQ_IP, OPT_MSG_TYPE, OPT_DNS_SHORT = 1, 2, 4, 8, 16, 32, 64
DISCOVER, OFFER, REQUEST, ACK, NAK, RELEASE = 1, 2, 3, 5, 6, 7
H_NONE, H_OFFER, H_NO_ADDR, H_NO_REQ_IP, H_NAK_ZERO, H_NAK_SUBNET, H_NAK_OTHER_MAC, H_NAK_FULL, H_ACK_NAK, H_REF_PANIC, \
    H_RELEASED, H_RELEASE_ABSENT, H_CLIENT_REQUEST, H_CLIENT_ACK = range(14)
H_F_REUSED, H_F_REPLY = 0x40, 0x80
COOKIE_BYTES = bytes([0x63, 0x82, 0x53, 0x63])
LEASE_TIME = 3600
SLOT = 288

MSG = np.dtype([("index", "<u4"), ("status", "u1"), ("dir", "u1"), ("msg_type", "u1"), ("reserved0", "u1"), ("options", "<u4"),
                ("xid", "u1", (4,)), ("yiaddr", "<u4"), ("chaddr", "u1", (6,)), ("payload_len", "<u2"), ("remote_ip", "<u4"),
                ("req_ip", "<u4"), ("mask", "u1", (4,)), ("gateway", "u1", (4,)), ("dns", "u1", (4,)), ("mask_n", "u1"),
                ("gateway_n", "u1"), ("reserved1", "u1", (2,)), ("reserved2", "<u4", (3,)), ("hostname", "u1", (64,))])
SUMMARY = np.dtype([("msgs", "<u4"), ("msgs_written", "<u4"), ("status_counts", "<u4", (5,)), ("type_counts", "<u4", (9,))])
LEASE = np.dtype([("ip", "<u4"), ("mac", "u1", (6,)), ("reserved", "<u2"), ("exp_time", "<u4"), ("hostname", "u1", (64,))])
REPLY = np.dtype([("kind", "u1"), ("reserved0", "u1", (3,)), ("xid", "u1", (4,)), ("yiaddr", "<u4"), ("chaddr", "u1", (6,)),
                  ("reserved1", "<u2"), ("req_ip", "<u4"), ("server_id", "<u4"), ("reserved2", "<u4")])
EVENT = np.dtype([("msg", "<u4"), ("ip", "<u4"), ("mask", "u1", (4,)), ("gateway", "u1", (4,)), ("dns", "u1", (4,)),
                  ("mask_n", "u1"), ("gateway_n", "u1"), ("options", "u1"), ("reserved", "u1")])
DESC = np.dtype([("payload_off", "<u8"), ("payload_len", "<u2"), ("proto", "u1"), ("aux", "u1"), ("src_port", "<u2"),
                 ("dst_port", "<u2"), ("src_ip", "<u4"), ("dst_ip", "<u4"), ("seq", "<u4"), ("ack", "<u4"),
                 ("dst_mac", "u1", (6,)), ("mode", "u1"), ("pad", "u1")])
assert (MSG.itemsize, SUMMARY.itemsize, LEASE.itemsize, REPLY.itemsize, EVENT.itemsize, DESC.itemsize) == (128, 64, 80, 32, 24, 40)


def ip_to_u(b: bytes) -> int:
    """protocol.IpAddrToU: 0 when the slice is not four bytes."""
    return struct.unpack(">I", b)[0] if len(b) == 4 else 0


def u_to_ip(u: int) -> bytes:
    return struct.pack(">I", u & 0xFFFFFFFF)


class GoPanic(Exception):
    pass


def parse_options(o: bytes) -> dict:
    """ParseDhcpOption (dhcp_engine.go:70-122): {code: data} of the kept codes; GoPanic where the Go
    code indexes out of range. Option 6 shorter than four bytes is kept as it came: ``data[0:4]``
    reslices into the caller's buffer, which the build defines as absent (see decode_one)."""
    kept, i = {}, 0
    while True:
        if i >= len(o):
            raise GoPanic("optionData[i]")
        if o[i] == 0xFF:
            break
        if i + 1 >= len(o):
            break
        code, length = o[i], o[i + 1]
        if i + 2 + length > len(o):
            break
        data = o[i + 2:i + 2 + length]
        if code == 53 and not data:
            raise GoPanic("data[0]")
        if code in (1, 3, 6, 12, 50, 53):
            kept[code] = data
        i += 2 + length
    return kept


def static_string64(name: bytes) -> bytes:
    n = min(len(name), 63)
    return name[:n] + bytes(63 - n) + bytes([n])


def decode_one(k: int, remote_ip: int, remote_port: int, local_port: int, payload: bytes) -> np.void:
    m = np.zeros(1, MSG)[0]
    m["index"], m["remote_ip"], m["payload_len"] = k, remote_ip, len(payload)
    if (remote_port, local_port) == (68, 67):
        m["dir"] = TO_SERVER
    elif (remote_port, local_port) == (67, 68):
        m["dir"] = TO_CLIENT
    else:
        m["dir"], m["status"] = DIR_NONE, PORTS
        return m
    if len(payload) < 240:
        m["status"] = SHORT
        return m
    if payload[236:240] != COOKIE_BYTES:
        m["status"] = COOKIE
        return m
    m["xid"] = list(payload[4:8])
    m["yiaddr"] = ip_to_u(payload[16:20])
    m["chaddr"] = list(payload[28:34])
    try:
        kept = parse_options(payload[240:])
    except GoPanic:
        m["status"] = REF_PANIC
        return m
    bits = 0
    if 53 in kept:
        bits |= OPT_MSG_TYPE
        m["msg_type"] = kept[53][0]
    if 50 in kept:
        bits |= OPT_REQ_IP
        m["req_ip"] = ip_to_u(kept[50])
    for code, bit, field, count in ((1, OPT_MASK, "mask", "mask_n"), (3, OPT_ROUTER, "gateway", "gateway_n")):
        if code in kept:
            bits |= bit
            d = kept[code][:4]
            m[field] = list(d + bytes(4 - len(d)))
            m[count] = len(d)
    if 6 in kept:
        if len(kept[6]) >= 4:
            bits |= OPT_DNS
            m["dns"] = list(kept[6][:4])
        else:
            bits |= OPT_DNS_SHORT
    if 12 in kept:
        bits |= OPT_HOSTNAME
        m["hostname"] = list(static_string64(kept[12]))
    m["options"] = bits
    return m


class Want:
    def __init__(self, msgs, summary):
        self.msgs, self.summary = msgs, summary


def decode(out: np.ndarray, records: int, index: np.ndarray, index_cap: int, msg_cap: int) -> Want:
    """The decode over a delivery: ``out`` the stream's buffer, ``records`` the delivery summary's
    count, ``index`` [(frame, offset)]."""
    raw = out.tobytes()
    msgs, s = [], np.zeros(1, SUMMARY)[0]
    for k in range(min(records, index_cap)):
        off = int(index[k][1])
        if off == 0xFFFFFFFF:
            continue
        _, kind, _, plen, rip, rport, lport = struct.unpack_from("<IBBHIHH", raw, off)
        if kind != 2:
            continue
        s["msgs"] += 1
        if len(msgs) >= msg_cap:
            continue
        m = decode_one(k, rip, rport, lport, raw[off + 24:off + 24 + plen])
        msgs.append(m)
        s["msgs_written"] += 1
        s["status_counts"][int(m["status"])] += 1
        if m["status"] == OK:
            t = int(m["msg_type"])
            s["type_counts"][t if (int(m["options"]) & OPT_MSG_TYPE) and t < 9 else 0] += 1
    return Want(np.array(msgs, MSG) if msgs else np.zeros(0, MSG), s)


# ---- the state machine ---------------------------------------------------------------------------
class Server:
    """RxDhcp's state (dhcp_engine.go:216-434) with a dict lease table: ip -> [mac, exp_time, hostname64]."""

    def __init__(self, *, ip, network_mask, dns=0, mac=bytes(6), server_enable=True, client_enable=False, capacity=1 << 16):
        self.ip, self.network_mask, self.dns, self.mac = ip, network_mask, dns, bytes(mac)
        self.server_enable, self.client_enable, self.capacity = server_enable, client_enable, capacity
        self.table: dict = {}
        self.client_xid = None

    @staticmethod
    def _reply(kind, xid, yiaddr, chaddr, req_ip=0, server_id=0):
        r = np.zeros(1, REPLY)[0]
        r["kind"], r["xid"], r["yiaddr"], r["chaddr"], r["req_ip"], r["server_id"] = kind, list(xid), yiaddr, list(chaddr), req_ip, server_id
        return r

    def discover(self, xid: bytes):
        self.client_xid = bytes(xid)
        return self._reply(DISCOVER, xid, 0, self.mac)

    def handle(self, msgs, now: int):
        replies, verdicts, events = [], [], []
        for i, m in enumerate(msgs):
            verdicts.append(self._one(m, i, now, replies, events))
        return (np.array(replies, REPLY) if replies else np.zeros(0, REPLY), np.array(verdicts, np.uint8),
                np.array(events, EVENT) if events else np.zeros(0, EVENT))

    def _one(self, m, i, now, replies, events) -> int:
        if int(m["status"]) != OK:
            return H_NONE
        bits, mac, xid = int(m["options"]), bytes(m["chaddr"]), bytes(m["xid"])
        if int(m["dir"]) == TO_SERVER:
            if not self.server_enable or not bits & OPT_MSG_TYPE:
                return H_NONE
            t = int(m["msg_type"])
            if t == DISCOVER:
                client, flags = 0, 0
                if bits & OPT_REQ_IP:
                    req = int(m["req_ip"])
                    if req in self.table and self.table[req][0] == mac:
                        client, flags = req, H_F_REUSED
                if client == 0:
                    flags = 0
                    network = self.ip & self.network_mask
                    host_bits = 32 - bin(network).count("1")  # the popcount of the network ADDRESS, as written
                    if host_bits < 32:
                        ii = 0
                        while ii < 1 << host_bits:
                            a = (network + ii) & 0xFFFFFFFF
                            ii += 1
                            if a & 0xFF in (0, 255) or a == self.ip or a in self.table:
                                continue
                            client = a
                            break
                if client == 0:
                    return H_NO_ADDR
                replies.append(self._reply(OFFER, xid, client, mac))
                return H_OFFER | flags | H_F_REPLY
            if t == REQUEST:
                if not bits & OPT_REQ_IP:
                    return H_NO_REQ_IP
                req = int(m["req_ip"])
                code, flags = H_ACK_NAK, 0
                if req == 0:
                    code = H_NAK_ZERO
                elif self.ip & self.network_mask != req & self.network_mask:
                    code = H_NAK_SUBNET
                elif req in self.table and self.table[req][0] != mac:
                    code = H_NAK_OTHER_MAC
                elif req not in self.table and len(self.table) >= self.capacity:
                    code = H_NAK_FULL
                if code == H_ACK_NAK:
                    hn = int(m["hostname"][63]) if bits & OPT_HOSTNAME else 0
                    if hn == 0:
                        return H_REF_PANIC  # StaticString64.Set("")
                    old = self.table[req][2] if req in self.table else bytes(64)
                    if req in self.table:
                        flags = H_F_REUSED
                    name = bytes(m["hostname"][:hn]) + old[hn:63] + bytes([hn])  # Set copies hn bytes and the count
                    self.table[req] = [mac, (now + LEASE_TIME) & 0xFFFFFFFF, name]
                    replies.append(self._reply(ACK, xid, req, mac))
                replies.append(self._reply(NAK, xid, 0, mac))  # the dhcp_nak label follows the ACK's TxDhcp
                return code | flags | H_F_REPLY
            if t == RELEASE:
                return H_RELEASED if self.table.pop(int(m["remote_ip"]), None) is not None else H_RELEASE_ABSENT
            return H_NONE
        if int(m["dir"]) == TO_CLIENT:
            if not self.client_enable or self.ip != 0 or self.client_xid is None or xid != self.client_xid:
                return H_NONE
            if not bits & OPT_MSG_TYPE:
                return H_NONE
            t = int(m["msg_type"])
            if t == OFFER:
                replies.append(self._reply(REQUEST, xid, 0, self.mac, int(m["yiaddr"]), int(m["remote_ip"])))
                return H_CLIENT_REQUEST | H_F_REPLY
            if t == ACK:
                e = np.zeros(1, EVENT)[0]
                e["msg"], e["ip"] = i, m["yiaddr"]
                for f in ("mask", "gateway", "dns", "mask_n", "gateway_n"):
                    e[f] = m[f]
                e["options"] = bits & (OPT_MASK | OPT_ROUTER | OPT_DNS)
                events.append(e)
                return H_CLIENT_ACK
        return H_NONE

    def leases(self) -> np.ndarray:
        out = np.zeros(len(self.table), LEASE)
        for o, ip in zip(out, sorted(self.table)):
            mac, exp, name = self.table[ip]
            o["ip"], o["mac"], o["exp_time"], o["hostname"] = ip, list(mac), exp, list(name)
        return out

    def clear(self, now: int) -> int:
        gone = [ip for ip, l in self.table.items() if (now & 0xFFFFFFFF) > l[1]]
        for ip in gone:
            del self.table[ip]
        return len(gone)


# ---- the builder ---------------------------------------------------------------------------------
def build_options(opts) -> bytes:
    """BuildDhcpOption over an ORDERED list of (code, value) — the order of the map literals."""
    out = b""
    for code, v in opts:
        if code in (1, 3, 6, 50, 54):
            out += bytes([code, 4]) + u_to_ip(v)
        elif code in (51, 58, 59):
            out += bytes([code, 4]) + struct.pack(">I", v)
        elif code == 53:
            out += bytes([53, 1, v])
        elif code == 55:
            out += bytes([55, 3, 1, 3, 6])
        elif code == 61:
            out += bytes([61, 7, 1]) + bytes(v)
    return out + b"\xff"


def reply_options(r, ip, network_mask, dns):
    kind, mac = int(r["kind"]), bytes(r["chaddr"])
    if kind in (OFFER, ACK):
        return [(53, kind), (1, network_mask), (3, ip), (6, dns), (51, LEASE_TIME), (59, int(LEASE_TIME * 0.875)),
                (58, int(LEASE_TIME * 0.5)), (54, ip)]
    if kind == NAK:
        return [(53, kind), (54, ip)]
    if kind == REQUEST:
        return [(53, kind), (61, mac), (50, int(r["req_ip"])), (54, int(r["server_id"])), (55, None)]
    if kind == DISCOVER:
        return [(53, kind), (61, mac), (55, None)]
    return None


def build_one(r, ip, network_mask, dns) -> bytes:
    """TxDhcp + BuildDhcpPkt (dhcp_engine.go:184-213, :437-450); b"" for a kind that is none of the five."""
    opts = reply_options(r, ip, network_mask, dns)
    if opts is None:
        return b""
    boot = 2 if int(r["kind"]) in (OFFER, ACK, NAK) else 1
    pkt = bytes([boot, 1, 6, 0]) + bytes(r["xid"]) + bytes([0, 0, 0x80, 0]) + bytes(4) + u_to_ip(int(r["yiaddr"])) + bytes(8)
    pkt += bytes(r["chaddr"]) + bytes(10) + bytes(64) + bytes(128) + COOKIE_BYTES
    return pkt + build_options(opts)


def build(replies, ip, network_mask, dns):
    """(slots uint8 [n, 288], descs DESC [n])."""
    n = len(replies)
    slots, descs = np.zeros((n, SLOT), np.uint8), np.zeros(n, DESC)
    for i, r in enumerate(replies):
        pkt = build_one(r, ip, network_mask, dns)
        if not pkt:
            continue
        slots[i, :len(pkt)] = np.frombuffer(pkt, np.uint8)
        server = int(r["kind"]) in (OFFER, ACK, NAK)
        d = descs[i]
        d["payload_off"], d["payload_len"], d["proto"] = i * SLOT, len(pkt), 17
        d["src_port"], d["dst_port"] = (67, 68) if server else (68, 67)
        d["src_ip"], d["dst_ip"], d["dst_mac"], d["mode"] = ip, 0xFFFFFFFF, [255] * 6, 0
    return slots, descs
