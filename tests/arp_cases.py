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
