"""The L2 switch as the reference runs it, one frame at a time, over a dict: SwitchPort.RxEthernet /
HandleEthernet, SwitchMacAddrClear and ListSwitchMacAddr (engine/ethernet_engine.go:58-163,
protocol/ethernet.go:29-82). The expected answer of the switch tests. Like the other models here it
is a same-author restatement of the Go code (there is no Go toolchain to run the original)."""
from __future__ import annotations

import numpy as np

ETH_LEN, ETH_TYPE, SRC_MCAST, TABLE_FULL, UNICAST, FLOOD = range(6)
ETHERTYPES = (0x05DC, 0x0800, 0x0806, 0x86DD)


class SwitchModel:
    def __init__(self, vlan_ids, capacity):
        self.vlan = list(vlan_ids)
        self.capacity = capacity
        self.table = {}  # mac bytes -> [port, create_time]

    def flood_mask(self, port):
        return sum(1 << q for q in range(len(self.vlan)) if q != port and self.vlan[q] == self.vlan[port])

    def forward(self, port, frames, now):
        """frames: a list of bytes. Returns (verdict, out_port, tx_len) arrays and the six counts."""
        n = len(frames)
        verdict, out_port = np.zeros(n, np.uint8), np.full(n, 0xFF, np.uint8)
        tx_len = np.zeros(n, np.uint16)
        now &= 0xFFFFFFFF
        for i, f in enumerate(frames):
            if len(f) < 42 or len(f) > 1514:
                verdict[i] = ETH_LEN
                continue
            if (f[12] << 8 | f[13]) not in ETHERTYPES:
                verdict[i] = ETH_TYPE
                continue
            dst, src = bytes(f[0:6]), bytes(f[6:12])
            if src[0] & 1:
                verdict[i] = SRC_MCAST
                continue
            e = self.table.get(src)
            if e is None:
                if len(self.table) >= self.capacity:
                    verdict[i] = TABLE_FULL
                    continue
                e = self.table[src] = [port, now]
            e[0], e[1] = port, now
            d = self.table.get(dst)
            if d is not None:
                verdict[i], out_port[i] = UNICAST, d[0]
            else:
                verdict[i] = FLOOD
            tx_len[i] = max(len(f), 60)
        return verdict, out_port, tx_len, np.bincount(verdict, minlength=6).astype(np.uint32)

    def expire(self, now):
        now &= 0xFFFFFFFF
        dead = [m for m, e in self.table.items() if now > ((e[1] + 300) & 0xFFFFFFFF)]
        for m in dead:
            del self.table[m]
        return len(dead)

    def entries(self):
        return {(m, e[0], e[1]) for m, e in self.table.items()}


def frame(dst: bytes, src: bytes, length: int = 64, ethertype: int = 0x0800) -> bytes:
    """An Ethernet frame of `length` bytes (shorter than 14: the header is cut)."""
    f = bytes(dst) + bytes(src) + bytes([ethertype >> 8, ethertype & 0xFF])
    return (f + bytes((7 * k + length) & 0xFF for k in range(max(0, length - 14))))[:length]


def mac(k: int) -> bytes:
    """The k-th unicast test MAC (even first byte)."""
    return bytes([0x02, 0x10, (k >> 24) & 0xFF, (k >> 16) & 0xFF, (k >> 8) & 0xFF, k & 0xFF])


def pack(frames, lead_dw=None):
    """(bytes u8, offsets_dw u32, lens u16): frames laid out at dword boundaries; lead_dw[i] extra
    dwords before frame i (to move headers across 64-byte lines)."""
    offs, lens, parts, pos = [], [], [], 0
    for i, f in enumerate(frames):
        gap = 4 * (lead_dw[i] if lead_dw is not None else 0)
        parts.append(bytes(gap))
        pos += gap
        offs.append(pos // 4)
        lens.append(len(f))
        padded = f + bytes(-len(f) % 4)
        parts.append(padded)
        pos += len(padded)
    data = np.frombuffer(b"".join(parts) + bytes(16), np.uint8).copy()
    return data, np.array(offs, np.uint32), np.array(lens, np.uint16)


def listed(entries: np.ndarray):
    return {(bytes(e["mac"]), int(e["port"]), int(e["create_time"])) for e in entries}
