"""A from-scratch dict model of the ARP neighbour cache (include/halo_rx.h, "ARP neighbour cache"):
the reference's SetArpCache / GetArpCache / HandleArp / ArpTableClear / ArpTableRefresh / ListArp
(engine/arp_engine.go, protocol/arp.go) with Go's wrapping u32 arithmetic, the forward path's L2
step per frame, and the gather's selection. No hashing, no slots: nothing of the implementation."""
from __future__ import annotations

U32 = 0xFFFFFFFF
BCAST = bytes([0xFF] * 6)
# handle verdicts / flags, get results, encap verdicts (the header's numbering)
BAD_OP, SRC_MISMATCH, CONFLICT, ACCEPTED = range(4)
F_NOT_LEARNED, F_REPLY = 0x40, 0x80
GET_ABSENT, GET_FOUND, GET_OWN_IP = range(3)
NONE, NO_ROUTE, ROUTE_PANIC, LOOPBACK, OWN_IP, MISS, HIT = range(7)
ROUTE_NONE, ROUTE_PANIC_ID = 0xFFFFFFFF, 0xFFFFFFFE


def ip_bytes(ip: int) -> bytes:
    return bytes([(ip >> 24) & 255, (ip >> 16) & 255, (ip >> 8) & 255, ip & 255])


def ip_of(b: bytes) -> int:
    return b[0] << 24 | b[1] << 16 | b[2] << 8 | b[3]


def arp_pkt(op: int, sha: bytes, spa: int, tha: bytes, tpa: int, head: bytes = b"\x00\x01\x08\x00\x06\x04") -> bytes:
    """BuildArpPkt (protocol/arp.go:57-77); `head` lets a test put garbage in bytes 0-5."""
    return head + bytes([op >> 8, op & 255]) + sha + ip_bytes(spa) + tha + ip_bytes(tpa)


def eth_frame(dst: bytes, src: bytes, ethertype: int, payload: bytes) -> bytes:
    """BuildEthFrm (protocol/ethernet.go:58-82): zero-padded to 60 bytes."""
    f = dst + src + bytes([ethertype >> 8, ethertype & 255]) + payload
    return f + bytes(max(0, 60 - len(f)))


class NetIf:
    def __init__(self, mac: bytes, ip: int, nat_enable: bool = False):
        self.mac, self.ip, self.nat_enable = bytes(mac), ip, nat_enable


class Model:
    def __init__(self, netifs, capacity: int):
        self.netifs, self.capacity = list(netifs), capacity
        self.cache = {}  # (netif, ip) -> [mac, exp_time]

    def set(self, netif: int, ip: int, mac: bytes, now: int) -> bool:
        k = (netif, ip)
        if k not in self.cache:
            if len(self.cache) >= self.capacity:
                return False
            self.cache[k] = [None, 0]
        self.cache[k] = [bytes(mac), (now + 300) & U32]
        return True

    def get(self, netif: int, ip: int):
        if ip == self.netifs[netif].ip:
            return GET_OWN_IP, None
        e = self.cache.get((netif, ip))
        return (GET_FOUND, e) if e else (GET_ABSENT, None)

    def handle(self, netif: int, payload: bytes, eth_src: bytes, now: int):
        """One HandleArp: (verdict byte, reply frame or None, changed 0/1)."""
        nif = self.netifs[netif]
        op = payload[6] << 8 | payload[7]
        if op not in (1, 2):
            return BAD_OP, None, 0
        sha, spa, tpa = payload[8:14], ip_of(payload[14:18]), ip_of(payload[24:28])
        if sha != eth_src:
            return SRC_MISMATCH, None, 0
        if spa == nif.ip:
            return CONFLICT, None, 0
        old = self.cache.get((netif, spa))
        learned = self.set(netif, spa, sha, now)
        changed = 1 if learned and (old is None or old[0] != sha) else 0
        v, reply = ACCEPTED | (0 if learned else F_NOT_LEARNED), None
        if op == 1 and tpa == nif.ip:
            reply = eth_frame(sha, nif.mac, 0x0806, arp_pkt(2, nif.mac, nif.ip, sha, spa))
            v |= F_REPLY
        return v, reply, changed

    def request(self, netif: int, target: int) -> bytes:
        nif = self.netifs[netif]
        return eth_frame(BCAST, nif.mac, 0x0806, arp_pkt(1, nif.mac, nif.ip, BCAST, target))

    def expire(self, now: int) -> int:
        gone = [k for k, e in self.cache.items() if now > e[1]]
        for k in gone:
            del self.cache[k]
        return len(gone)

    def refresh(self, now: int):
        return sorted(k for k, e in self.cache.items() if now > ((e[1] - 10) & U32))

    def listing(self):
        return sorted((k[0], k[1], e[0], e[1]) for k, e in self.cache.items())

    def lookup(self, netif: int, ip: int):
        """The device's bare GetArpCache: (verdict, mac or None)."""
        if netif >= len(self.netifs):
            return NONE, None
        f, e = self.get(netif, ip)
        return {GET_OWN_IP: (OWN_IP, None), GET_ABSENT: (MISS, None)}.get(f) or (HIT, e[0])

    def encap(self, frame: bytes, route, in_netif: int, selected: bool = True):
        """The L2 step for one frame. `route` is ROUTE_NONE, ROUTE_PANIC_ID, None (an id the device
        copy does not know) or (next_hop, netif). Returns (verdict, out_netif, tx_len, target_ip,
        the frame afterwards)."""
        n = len(frame)
        if not selected or n < 34 or frame[12:14] != b"\x08\x00" or route is None:
            return NONE, 0xFF, 0, 0, frame
        if route == ROUTE_NONE:
            return NO_ROUTE, 0xFF, 0, 0, frame
        if route == ROUTE_PANIC_ID:
            return ROUTE_PANIC, 0xFF, 0, 0, frame
        next_hop, out = route
        if out >= len(self.netifs):
            return NONE, 0xFF, 0, 0, frame
        nif = self.netifs[out]
        dst = ip_of(frame[30:34])
        if dst == nif.ip and not self.netifs[in_netif].nat_enable:
            return LOOPBACK, out, 0, 0, frame
        target = next_hop or dst
        if target == nif.ip:
            return OWN_IP, out, 0, target, frame
        e = self.cache.get((out, target))
        if e is None:
            return MISS, out, 0, target, frame
        return HIT, out, max(n, 60), target, e[0] + nif.mac + frame[12:]


def is_arp_for(frame: bytes, own_mac: bytes) -> bool:
    """RxEthernet's path to HandleArp: ParseEthFrm passes, the destination is ours or the
    broadcast, the EtherType is ARP (engine/ethernet_engine.go:13-31)."""
    return 42 <= len(frame) <= 1514 and frame[12:14] == b"\x08\x06" and frame[:6] in (own_mac, BCAST)
