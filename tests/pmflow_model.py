"""A from-scratch dict model of the port-mapping return-flow table (include/halo_rx.h,
"port-mapping return flows"): the reference's Get / MallocType / Set of
engine/ipv4_engine.go:238-266, the lookup, override and SNAT of :160-186 and :203-207 and
NatPortMappingFlowClear (:497-516), with Go's wrapping u32 arithmetic. It works from frame bytes
through oracle/ref_py.py, restates the override over tests/arp_model.py and the SNAT over
oracle/ref_tx_py.py. No hashing, no slots: nothing of the implementation."""
from __future__ import annotations

from oracle import ref_py as R
from oracle import ref_tx_py as T
from tests import arp_model as AM

U32 = 0xFFFFFFFF
V_NONE, V_MISS, V_HIT, V_OVERRIDE = range(4)
ROUTE_NONE, ROUTE_PANIC_ID = AM.ROUTE_NONE, AM.ROUTE_PANIC_ID
NAT_V_MAPPING = 4
TX_NAT_SRC = 0x04


def five_tuple(frame: bytes, mac: bytes, own_ip: int):
    """(proto, src, dst, sport, dport) as the parsed record holds them; proto 0xFF when
    ParseIpv4Pkt failed (Ipv4RouteForward never runs)."""
    r = R.rx_frame(frame, mac, own_ip)
    return r["ip_proto"], r["src_ip"], r["dst_ip"], r["sport"], r["dport"]


class Model:
    """`netifs`: arp_model.NetIf objects (ip, nat_enable read); `gateways`: IpAddrToU(Gateway), 0 = nil."""

    def __init__(self, netifs, gateways, capacity: int):
        self.netifs, self.gateways, self.capacity = list(netifs), list(gateways), capacity
        self.flows = {}  # (remote_ip, remote_port, lan_ip, lan_port, proto) -> [wan_netif, wan_port, last_alive, id]
        self.next_id = 0

    # ---- :238-266 ----
    def record_one(self, in_netif: int, key, wan_port: int, now: int) -> bool:
        """False: MallocType failed, the frame is not sent."""
        f = self.flows.get(key)
        if f is None:
            if len(self.flows) >= self.capacity:
                return False
            f = self.flows[key] = [0, 0, 0, self.next_id]
            self.next_id += 1
        f[0], f[1], f[2] = in_netif, wan_port, now & U32
        return True

    def record(self, in_netif: int, items, now: int):
        """items: (remote_ip, remote_port, lan_ip, lan_port, proto, wan_port) in frame order.
        Returns (dropped list, inserts)."""
        before = self.next_id
        dropped = [0 if self.record_one(in_netif, tuple(it[:5]), it[5], now) else 1 for it in items]
        return dropped, self.next_id - before

    # ---- :164-179 ----
    def get(self, key, now=None):
        f = self.flows.get(tuple(key))
        if f is not None and now is not None:
            f[2] = now & U32
        return f

    # ---- :497-516 ----
    def expire(self, now: int) -> int:
        gone = [k for k, f in self.flows.items() if ((now - f[2]) & U32) > 60]
        for k in gone:
            del self.flows[k]
        return len(gone)

    def listing(self):
        """(id, remote_ip, remote_port, lan_ip, lan_port, proto, wan_netif, wan_port, last_alive) by id."""
        return sorted((f[3], *k, f[0], f[1], f[2]) for k, f in self.flows.items())

    # ---- the LAN-side half for one frame a non-NAT NetIf received (:160-186, :203-207) ----
    def lookup(self, tup, route, now: int, selected: bool = True, stamp: bool = True):
        """`tup` = five_tuple(...); `route` as arp_model.Model.encap takes it: ROUTE_NONE,
        ROUTE_PANIC_ID, None (an id the device copy does not know) or (next_hop, netif).
        Returns (verdict, wan_netif, wan_port, next_hop, snat) with snat = (src_ip, src_port) or None."""
        proto, src, dst, sport, dport = tup
        if proto == 0xFF or not selected:
            return V_NONE, 0xFF, 0, 0, None
        f = self.flows.get((dst, dport, src, sport, proto))
        if f is None:
            return V_MISS, 0xFF, 0, 0, None
        if stamp:
            f[2] = now & U32
        wan = f[0]
        # outNetIfName != WanNetIf (:182); a panicking FindRoute never gets that far
        same = route == ROUTE_PANIC_ID or (isinstance(route, tuple) and route[1] == wan)
        nif = self.netifs[wan]
        snat = (nif.ip, f[1]) if nif.nat_enable else None
        return (V_HIT if same else V_OVERRIDE), wan, f[1], self.gateways[wan], snat

    @staticmethod
    def apply_snat(op: dict, snat) -> dict:
        """The op fields the lookup writes (and no other)."""
        if snat is not None:
            op = dict(op, steps=op["steps"] | TX_NAT_SRC, src_ip=snat[0], src_port=snat[1])
        return op

    # ---- the WAN-side half for one frame (:238-247): the key it records, or None ----
    @staticmethod
    def candidate(tup, wan_verdict: int, arp_verdict: int, op_dst_ip: int, op_dst_port: int):
        """(key, wan_port) when the inbound lookup found a NatPortMappingEntry and ARP succeeded."""
        proto, src, _dst, sport, dport = tup
        if wan_verdict != NAT_V_MAPPING or arp_verdict != AM.HIT:
            return None
        return (src, sport, op_dst_ip, op_dst_port, proto), dport


def encap_via(arp: AM.Model, frame: bytes, route, via, in_netif: int, selected: bool = True):
    """arp_model.Model.encap with the override of :180-186: `via` = (verdict, wan_netif, wan_port,
    next_hop) or None. An OVERRIDE replaces the route by (next_hop, wan_netif) — whatever the route
    id was, a no-route id included — and everything after is the plain step."""
    if via is not None and via[0] == V_OVERRIDE:
        route = (via[3], via[1])
    return arp.encap(frame, route, in_netif, selected)


def snat_frame(frame: bytes, steps: int, src_ip: int, src_port: int, check_sum_enable: bool = True):
    """The fixup the chain applies to a frame (oracle/ref_tx_py.py): (frame afterwards, result byte)."""
    b = bytearray(frame)
    r = T.tx_frame(b, steps, src_ip=src_ip, src_port=src_port, check_sum_enable=check_sum_enable)
    return bytes(b), r
