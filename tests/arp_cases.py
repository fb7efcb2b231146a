"""Shared pieces of the ARP tests: a library table and the dict model (tests/arp_model.py) driven
side by side, and the forced 16-slot / 15-entry table whose probe chains collide and wrap."""
from __future__ import annotations

import numpy as np

from tests import arp_model as M


def mac(k: int) -> bytes:
    return bytes([0x02, 0x5A, (k >> 24) & 255, (k >> 16) & 255, (k >> 8) & 255, k & 255])


NETIFS = [M.NetIf(bytes([0x02, 0, 0, 0, 0, 1]), 0x0A000001, False),   # 10.0.0.1
          M.NetIf(bytes([0x02, 0, 0, 0, 0, 2]), 0x0A010001, True),    # 10.1.0.1, NATing
          M.NetIf(bytes([0x02, 0, 0, 0, 0, 3]), 0xC0A80001, False)]   # 192.168.0.1


def lib_netifs(netifs=NETIFS):
    from halo_amd._lib import NetIf

    out = []
    for m in netifs:
        n = NetIf()
        for i in range(6):
            n.mac[i] = m.mac[i]
        n.ip, n.nat_enable = m.ip, 1 if m.nat_enable else 0
        out.append(n)
    return out


class Pair:
    """An ArpTable and a Model that receive the same calls; `check` compares everything visible."""

    def __init__(self, capacity: int, slots_log2: int = 0, netifs=NETIFS, device: int = 0):
        from halo_amd.arp import ArpTable

        self.t = ArpTable(lib_netifs(netifs), capacity, slots_log2, device)
        self.m = M.Model(netifs, capacity)

    def set(self, netif, ip, mac_, now):
        self.t.SetArpCache(netif, ip, mac_, now)
        self.m.set(netif, ip, mac_, now)

    def handle(self, msgs, now):
        """msgs: (netif, payload28, eth_src) tuples. Returns the library's verdicts."""
        arr = msg_array(msgs)
        v, replies, changed = self.t.HandleArp(arr, now)
        want = [self.m.handle(nif, p, s, now) for nif, p, s in msgs]
        assert list(v) == [w[0] for w in want]
        assert [bytes(r) for r in replies] == [w[1] for w in want if w[1] is not None]
        assert changed == sum(w[2] for w in want)
        return v

    def expire(self, now):
        got = self.t.ArpTableClear(now)
        assert got == self.m.expire(now)
        return got

    def check(self, now=None):
        ls = self.t.ListArp()
        got = sorted((int(e["netif"]), int(e["ip"]), bytes(e["mac"]), int(e["exp_time"])) for e in ls)
        assert got == self.m.listing()
        if now is not None:
            nifs, ips = self.t.ArpTableRefresh(now)
            assert sorted(zip(map(int, nifs), map(int, ips))) == self.m.refresh(now)

    def close(self):
        self.t.close()


def msg_array(msgs, first_index: int = 0) -> np.ndarray:
    from halo_amd._lib import ARP_MSG_DTYPE

    arr = np.zeros(len(msgs), ARP_MSG_DTYPE)
    for i, (nif, payload, src) in enumerate(msgs):
        arr[i]["index"], arr[i]["netif"] = first_index + i, nif
        arr[i]["eth_src"] = np.frombuffer(src, np.uint8)
        arr[i]["arp"] = np.frombuffer(payload[:28], np.uint8)
    return arr


def forced_table(make_pair, netifs=NETIFS):
    """A 16-slot table holding 15 entries whose layout has a chain of >= 3 slots and a chain that
    wraps past the last slot — found by search over key sets, and asserted. Returns (pair, keys)."""
    for seed in range(64):
        rng = np.random.default_rng(7000 + seed)
        p = make_pair(capacity=15, slots_log2=4)
        keys = []
        while len(keys) < 15:
            nif = int(rng.integers(0, len(netifs)))
            ip = (netifs[nif].ip & 0xFFFFFF00) | int(rng.integers(2, 255))
            if (nif, ip) not in keys:
                keys.append((nif, ip))
        for k, (nif, ip) in enumerate(keys):
            p.set(nif, ip, mac(100 + k), 50)
        st = p.t.layout_stats()
        if int(st["longest_chain"]) >= 3 and int(st["wrapped"]) >= 1:
            assert int(st["slots"]) == 16 and int(st["entries"]) == 15
            return p, keys
        p.close()
    raise AssertionError("no key set with a long and a wrapped chain")


# ---- the mixed batches of the device tests (tests/test_gpu_arp.py, tests/test_gpu_scale.py) ------
NH_HIT, NH_MISS, NH_OWN, PANIC, ECMP, BAD_NETIF = 0xAC100000, 0xAC110000, 0xAC120000, 0xAC140000, 0xAC150000, 0xAC160000
LENS_POOL = [34, 60, 61, 62, 63, 64, 100, 1514]


def absent(keys, nif, k):
    """The k-th address of NetIf nif's /24 that is neither a key nor the own address."""
    base = NETIFS[nif].ip & 0xFFFFFF00
    free = [base | h for h in range(2, 255) if (nif, base | h) not in keys]
    return free[k % len(free)]


def world_route_ops(keys):
    """The route table the forced ARP table is synced with: direct routes, next-hop routes, an
    emptied list, an ECMP list and a route to a NetIf the ARP table does not have — as
    ("add" | "del", [dst, mask, next_hop, netif]) in call order."""
    ops = [("add", [m.ip & 0xFFFFFF00, 0xFFFFFF00, 0, nif]) for nif, m in enumerate(NETIFS)]
    hit_nif, hit_ip = keys[0]
    ops.append(("add", [NH_HIT, 0xFFFF0000, hit_ip, hit_nif]))
    ops.append(("add", [NH_MISS, 0xFFFF0000, absent(keys, 2, 0), 2]))
    ops.append(("add", [NH_OWN, 0xFFFF0000, NETIFS[1].ip, 1]))
    gone = [PANIC, 0xFFFF0000, keys[1][1], keys[1][0]]
    ops += [("add", gone), ("del", gone)]  # the emptied list still ends a lookup
    ops.append(("add", [ECMP, 0xFFFF0000, keys[2][1], keys[2][0]]))
    ops.append(("add", [ECMP, 0xFFFF0000, absent(keys, 0, 1), 0]))
    ops.append(("add", [BAD_NETIF, 0xFFFF0000, 0, 9]))  # a NetIf the ARP table does not have
    return ops


def world_routes(keys, device: int = 0):
    """world_route_ops(keys) in a halo_amd.route.RouteTable (not yet synced)."""
    from halo_amd.route import RouteTable

    rt = RouteTable(device)
    for what, r in world_route_ops(keys):
        (rt.AddRoute if what == "add" else rt.DeleteRoute)(RouteTable.entry(*r))
    return rt


def route_of(rt, rid):
    """A route id as arp_model.Model.encap takes it."""
    if rid in (M.ROUTE_NONE, M.ROUTE_PANIC_ID):
        return rid
    try:
        r = rt.get(rid)[0]
    except Exception:
        return None
    return int(r["next_hop"]), int(r["netif"])


def ipv4_frame(rng, length, dst_ip, ethertype=0x0800):
    """`length` bytes: a MAC header that is not ours to judge, an EtherType, random bytes, and the
    destination address at bytes 30-33 when the frame has them."""
    f = bytearray(rng.integers(0, 256, length, dtype=np.uint8).tobytes())
    if length >= 14:
        f[12:14] = bytes([ethertype >> 8, ethertype & 255])
    if length >= 34:
        f[30:34] = M.ip_bytes(dst_ip)
    return bytes(f)


def pack(rng, frames):
    """Frames at 4-byte boundaries with random extra 4-byte gaps and garbage between them."""
    offs, pos = [], 0
    for f in frames:
        pos += 4 * int(rng.integers(0, 3))
        offs.append(pos)
        pos += (len(f) + 3) & ~3
    data = rng.integers(0, 256, pos + 16, dtype=np.uint8)
    for o, f in zip(offs, frames):
        data[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return data, (np.array(offs, np.int64) // 4).astype(np.uint32), np.array([len(f) for f in frames], np.uint16)


def mixed_batch(rng, keys, n, lens_pool=LENS_POOL):
    """n frames cycling through every case of the L2 step: (frames, intended dst per frame, select,
    forced route id or None, case name)."""
    frames, dsts, select, forced, names = [], [], [], [], []
    kinds = ["hit_direct", "unselected", "short33", "len34_hit", "not_ipv4", "bad_route_id", "no_route", "panic", "own_dst",
             "own_next_hop", "miss_direct", "miss_next_hop", "hit_next_hop", "ecmp", "bad_netif", "hit_direct"]
    for i in range(n):
        kind = kinds[i % len(kinds)] if n > 1 else "hit_direct"
        nif, ip = keys[(i // len(kinds) + i) % len(keys)]
        length, et, sel, frc = lens_pool[i % len(lens_pool)], 0x0800, 1, None
        dst = ip
        if kind == "unselected":
            sel = 0
        elif kind == "short33":
            length = 33
        elif kind == "len34_hit":
            length = 34
        elif kind == "not_ipv4":
            et = [0x0806, 0x86DD, 0x0801, 0x0900][i % 4]
        elif kind == "bad_route_id":
            frc = 1000 + i
        elif kind == "no_route":
            dst = 0x08080808
        elif kind == "panic":
            dst = PANIC | 7
        elif kind == "own_dst":
            dst = NETIFS[i % 3].ip
        elif kind == "own_next_hop":
            dst = NH_OWN | (i & 0xFFFF)
        elif kind == "miss_direct":
            dst = absent(keys, i % 3, i)
        elif kind == "miss_next_hop":
            dst = NH_MISS | (i & 0xFFFF)
        elif kind == "hit_next_hop":
            dst = NH_HIT | (i & 0xFFFF)
        elif kind == "ecmp":
            dst = ECMP | ((i * 7919) & 0xFFFF)
        elif kind == "bad_netif":
            dst = BAD_NETIF | 5
        frames.append(ipv4_frame(rng, length, dst, et))
        dsts.append(dst)
        select.append(sel)
        forced.append(frc)
        names.append(kind)
    return frames, np.array(dsts, np.uint32), np.array(select, np.uint8), forced, names


def lookup_mix(rng, keys, n):
    """n (netif, ip) pairs for the bare lookup: every entry (the end of the longest chain and the
    wrapped ones among them), absent addresses, own addresses, NetIfs the table does not have and
    random addresses. Returns (netifs u8, ips u32)."""
    nifs = np.zeros(n, np.uint8)
    ips = np.zeros(n, np.uint32)
    for i in range(n):
        kind = i % 5
        nif, ip = keys[i % len(keys)]
        if kind == 1:  # absent: with one empty slot in sixteen its probe runs to the end of a chain
            nif = i % 3
            ip = absent(keys, nif, i)
        elif kind == 2 and i % 2:
            nif = i % 3
            ip = NETIFS[nif].ip
        elif kind == 3 and i % 3 == 0:
            nif = [3, 64, 255][(i // 15) % 3]  # a NetIf the table does not have
        elif kind == 4:
            ip = int(rng.integers(0, 1 << 32))
        nifs[i], ips[i] = nif, ip
    return nifs, ips
