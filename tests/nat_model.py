"""Not a test: the expected answers of the NAT flow-table tests.

A from-scratch model of the reference's NAT state (engine/ipv4_engine.go:423-759) over plain dicts
keyed by the normalised key tuples (remote ip, remote port, local ip, local port, proto): no
hashing, so nothing here depends on halo_amd/csrc/flow_key.h or on the device layout. One
allocator (a set of used ports) per normalised remote address, the port-mapping list in call
order, LastAliveTime and the NatTableClear rule in uint32 arithmetic. Flow ids count successful
NatAddFlow calls from 0, which is the numbering include/halo_rx.h promises (fresh, never reused).
"""
from __future__ import annotations

import numpy as np

SYMMETRIC, FULL_CONE = 0, 1
LAN, WAN = 0, 1  # HALO_FLOW_NAT_LAN / _WAN
V_NONE, V_SKIP, V_MISS, V_FLOW, V_MAPPING, V_DROP = range(6)
NO_FLOW = 0xFFFFFFFF
TX_NAT_DST, TX_NAT_SRC = 0x01, 0x04
M32 = 0xFFFFFFFF
FLOW_FIELDS = ("remote_ip", "wan_ip", "lan_ip", "last_alive", "remote_port", "wan_port", "lan_port", "proto", "id")


class NatModel:
    def __init__(self, wan_ip: int, nat_type: int):
        self.wan_ip, self.nat_type = wan_ip, nat_type
        self.lan: dict = {}    # NatFlowTable
        self.wan: dict = {}    # NatWanFlowTable
        self.alloc: dict = {}  # NatPortAlloc: remote ip -> set of used ports
        self.maps: list = []   # NatPortMappingTable: (wan_port, lan_ip, lan_port, proto)
        self.next_id = 0

    def _norm(self, rip, rport, proto):
        if self.nat_type != SYMMETRIC:
            rip, rport = 0, 0
        if proto == 1:
            rport = 0
        return rip, rport

    def add_port_mapping(self, wan_port, lan_ip, lan_port, proto):
        self.maps.append((wan_port, lan_ip, lan_port, proto))

    def add_flow(self, lan_ip, remote_ip, lan_port, remote_port, proto, now):
        if lan_port == 0 or remote_port == 0:
            return None
        rip, rport = self._norm(remote_ip, remote_port, proto)
        used = self.alloc.setdefault(rip, set())
        port = 32768
        while port in used:
            port = (port + 1) & 0xFFFF
            if port == 0:
                return None
        used.add(port)
        f = dict(remote_ip=rip, remote_port=rport, wan_ip=self.wan_ip, wan_port=port, lan_ip=lan_ip,
                 lan_port=lan_port, proto=proto, last_alive=now & M32, id=self.next_id)
        self.next_id += 1
        self.lan[(rip, rport, lan_ip, lan_port, proto)] = f  # HashMap.Set replaces an existing value
        self.wan[(rip, rport, self.wan_ip, port, proto)] = f
        return f

    def get_lan(self, remote_ip, remote_port, lan_ip, lan_port, proto):
        return self.lan.get((*self._norm(remote_ip, remote_port, proto), lan_ip, lan_port, proto))

    def get_wan(self, remote_ip, remote_port, wan_ip, wan_port, proto):
        return self.wan.get((*self._norm(remote_ip, remote_port, proto), wan_ip, wan_port, proto))

    def check_mapping(self, direction, ip, port, proto):
        if proto not in (6, 17):
            return None
        for k, (wp, lip, lp, pr) in enumerate(self.maps):
            if direction == WAN and wp == port and pr == proto:
                return k
            if direction == LAN and lip == ip and lp == port and pr == proto:
                return k
        return None

    def list(self):
        return list(self.lan.values())

    def expire(self, now):
        gone = [(k, f) for k, f in self.lan.items() if ((now - f["last_alive"]) & M32) > 60]
        for k, f in gone:
            del self.lan[k]
            self.wan.pop((f["remote_ip"], f["remote_port"], f["wan_ip"], f["wan_port"], f["proto"]), None)
            used = self.alloc.get(f["remote_ip"])
            if used is not None:
                used.discard(f["wan_port"])
                if not used:
                    del self.alloc[f["remote_ip"]]
        return len(gone)

    # ---- the forward path over records --------------------------------------------------------
    def _apply(self, direction, op, ip, port):
        if direction == WAN:
            op["steps"] |= TX_NAT_DST
            op["dst_ip"], op["dst_port"] = ip, port
        else:
            op["steps"] |= TX_NAT_SRC
            op["src_ip"], op["src_port"] = ip, port

    def _find(self, direction, r):
        """(verdict, ref, ip, port, flow) of one record whose lookup runs."""
        proto, src, dst = int(r["ip_proto"]), int(r["src_ip"]), int(r["dst_ip"])
        sport, dport = int(r["sport"]), int(r["dport"])
        if direction == WAN:
            k = self.check_mapping(WAN, None, dport, proto)
            if k is not None:
                return V_MAPPING, k, self.maps[k][1], self.maps[k][2], None
            f = self.get_wan(src, sport, dst, dport, proto)
            return (V_FLOW, f["id"], f["lan_ip"], f["lan_port"], f) if f else (V_MISS, NO_FLOW, 0, 0, None)
        k = self.check_mapping(LAN, src, sport, proto)
        if k is not None:
            return V_MAPPING, k, self.wan_ip, self.maps[k][0], None
        f = self.get_lan(dst, dport, src, sport, proto)
        return (V_FLOW, f["id"], f["wan_ip"], f["wan_port"], f) if f else (V_MISS, NO_FLOW, 0, 0, None)

    def lookup(self, direction, records, now, ops, skip=None):
        """What halo_nat_lookup_{wan,lan}_device answers from this state: (verdict u8, ref u32,
        misses); `ops` (a TX_OP structured array) is updated in place and hit flows are stamped."""
        n = len(records)
        verdict = np.zeros(n, np.uint8)
        ref = np.full(n, NO_FLOW, np.uint32)
        misses = 0
        for i in range(n):
            r = records[i]
            if int(r["ip_proto"]) == 0xFF:
                verdict[i] = V_NONE
            elif skip is not None and skip[i]:
                verdict[i] = V_SKIP
            else:
                v, rf, ip, port, f = self._find(direction, r)
                verdict[i], ref[i] = v, rf
                if v == V_MISS:
                    misses += 1
                    continue
                if f is not None:
                    f["last_alive"] = now & M32
                self._apply(direction, ops[i:i + 1], ip, port)
        return verdict, ref, misses

    def resolve(self, direction, records, verdicts, now, ops):
        """halo_nat_resolve_misses: (verdicts_out, n_added)."""
        out = verdicts.copy()
        added = 0
        for i in np.nonzero(verdicts == V_MISS)[0]:
            r = records[i]
            v, _, ip, port, f = self._find(direction, r)
            if v == V_MISS:
                if direction == WAN:
                    continue
                f = self.add_flow(int(r["src_ip"]), int(r["dst_ip"]), int(r["sport"]), int(r["dport"]),
                                  int(r["ip_proto"]), now)
                if f is None:
                    out[i] = V_DROP
                    continue
                added += 1
                v, ip, port = V_FLOW, f["wan_ip"], f["wan_port"]
            if f is not None:
                f["last_alive"] = now & M32
            self._apply(direction, ops[i:i + 1], ip, port)
            out[i] = v
        return out, added

    def quote(self, quote_records):
        """halo_nat_lookup_quote_device: (lan_ip, lan_port, found) per quote record."""
        out = []
        for r in quote_records:
            f = None
            if int(r["status"]) == 0:
                f = self.get_wan(int(r["src_ip"]), int(r["sport"]), int(r["dst_ip"]), int(r["dport"]), int(r["ip_proto"]))
            out.append((f["lan_ip"], f["lan_port"], 1) if f else (0, 0, 0))
        return out


def flow_tuple(f) -> tuple:
    """A flow (model dict or NAT_FLOW_DTYPE record) as a comparable tuple."""
    return tuple(int(f[k]) for k in FLOW_FIELDS)


def sorted_flows(flows) -> list:
    return sorted(flow_tuple(f) for f in flows)


# ---- shared fixtures -----------------------------------------------------------------------------
WAN_IP = 0xCB007101  # 203.0.113.1
# The forced-capacity table of the GPU tests: 12 flows in 16 slots. The seed was picked on the CPU
# so that the layout has probe chains of 3 or more slots and chains that wrap past the last slot
# in both indexes (tests/test_nat_table.py::test_forced_fixture_exercises_collisions_and_wrap).
FIXTURE_SEED = {SYMMETRIC: 7, FULL_CONE: 13}  # per NAT type
FIXTURE_LOG2 = 4
FIXTURE_FLOWS = 12


def random_tuples(seed: int, n: int):
    """n distinct (lan_ip, remote_ip, lan_port, remote_port, proto) tuples with non-zero ports."""
    rng = np.random.RandomState(seed)
    out, seen = [], set()
    while len(out) < n:
        t = (0xC0A80000 | int(rng.randint(2, 250)), 0x08080000 | int(rng.randint(1, 1 << 16)),
             int(rng.randint(1024, 65536)), int(rng.randint(1, 65536)), int(rng.choice([1, 6, 17])))
        if (t[0], t[2], t[4]) not in seen:
            seen.add((t[0], t[2], t[4]))
            out.append(t)
    return out


def fill(table, model, tuples, now):
    """The same NatAddFlow calls on a halo_amd.nat.NatTable and on its model."""
    for lan_ip, remote_ip, lan_port, remote_port, proto in tuples:
        got = table.AddFlow(lan_ip, remote_ip, lan_port, remote_port, proto, now)
        want = model.add_flow(lan_ip, remote_ip, lan_port, remote_port, proto, now)
        assert (got is None) == (want is None)
        if want is not None:
            assert flow_tuple(got) == flow_tuple(want)


# ---- the record and op builders of the device tests ------------------------------------------------
REMOTE = 0x08080000
TX_TTL = 0x02


def records(m: NatModel, direction, n, seed):
    """n records for `direction`: about half hit a flow of the model (ICMP ones with a remote port
    the key ignores), the rest are misses, port-mapping hits and unparsed (0xFF) records."""
    from halo_amd._lib import RESULT_DTYPE

    rng = np.random.RandomState(seed)
    flows = m.list()
    r = np.zeros(n, RESULT_DTYPE)
    r["l4_seq"] = rng.randint(0, 1 << 31, n)  # fields no lookup reads
    for i in range(n):
        kind = rng.randint(0, 10)
        if kind < 5 and flows:
            f = flows[rng.randint(0, len(flows))]
            rip = f["remote_ip"] or (REMOTE | rng.randint(1, 1 << 16))
            rport = f["remote_port"] or rng.randint(1, 65536)
            if direction == WAN:
                rec = (f["proto"], rip, rport, f["wan_ip"], f["wan_port"])
            else:
                rec = (f["proto"], f["lan_ip"], f["lan_port"], rip, rport)
        elif kind < 7:  # a miss: a random tuple
            rec = (int(rng.choice([1, 6, 17])), REMOTE | rng.randint(1, 1 << 16), rng.randint(1, 65536),
                   WAN_IP if direction == WAN else 0xC0A80000 | rng.randint(2, 250), rng.randint(1, 65536))
        elif kind < 9 and m.maps:  # a port mapping (or, for ICMP, not)
            wp, lip, lp, pr = m.maps[rng.randint(0, len(m.maps))]
            pr = pr if rng.randint(0, 4) else 1
            rec = (pr, REMOTE | 7, 999, WAN_IP, wp) if direction == WAN else (pr, lip, lp, REMOTE | 7, 999)
        else:
            rec = (0xFF, 0, 0, 0, 0)
        r["ip_proto"][i], r["src_ip"][i], r["sport"][i], r["dst_ip"][i], r["dport"][i] = rec
    return r


def ops(n, seed):
    """Ops as a caller chaining lookups leaves them: HALO_TX_TTL set, sentinels everywhere else."""
    from halo_amd._lib import TX_OP_DTYPE

    rng = np.random.RandomState(seed)
    out = np.zeros(n, TX_OP_DTYPE)
    out["steps"] = TX_TTL
    for f in ("dst_ip", "src_ip"):
        out[f] = rng.randint(0, 1 << 31, n)
    for f in ("dst_port", "src_port", "pad2"):
        out[f] = rng.randint(0, 1 << 16, n)
    out["pad"] = 0xA5
    return out
