"""Not a test: shared by tests/test_pmflow_table.py and tests/test_gpu_pmflow.py — the three-NetIf
router of the return-flow tests, its frames, the forced 16-slot fixture, and, in the manner of
tests/respond_cases.py, where halo_pmflow_record_device changes behaviour with the batch size: the
tile and the scan pass, read out of the sources by regular expression so that a moved constant
moves the shapes."""
from __future__ import annotations

import os
import re

import numpy as np

from oracle import ref_py as R
from tests import arp_model as AM
from tests import pmflow_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo_amd", "csrc")

SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
FILL = 0xA5
# NetIf 0 = LAN (not NATing), 1 = WAN1 (NATing, the default route), 2 = WAN2 (NATing, port mapping), 3 = DMZ (not NATing)
LAN, WAN1, WAN2, DMZ = 0, 1, 2, 3
MACS = [bytes([0x02, 0, 0, 0, 0, q + 1]) for q in range(4)]
IPS = [0xC0A80101, 0xCB007101, 0xC6336401, 0x0A090801]  # 192.168.1.1, 203.0.113.1, 198.51.100.1, 10.9.8.1
NAT = [False, True, True, False]
GATEWAYS = [0, 0xCB0071FE, 0xC63364FE, 0]  # WAN1 .254, WAN2 .254; DMZ and LAN have none
SERVER = 0xC0A80114  # 192.168.1.20, the port-forwarded LAN host
GW_MAC = {WAN1: bytes([0x02, 0xAA, 0, 0, 0, 1]), WAN2: bytes([0x02, 0xAA, 0, 0, 0, 2])}
SERVER_MAC = bytes([0x02, 0xBB, 0, 0, 0, 0x14])


def model_netifs():
    return [AM.NetIf(MACS[q], IPS[q], NAT[q]) for q in range(4)]


def lib_netifs():
    from halo_amd._lib import NetIf

    out = []
    for q in range(4):
        n = NetIf()
        for k in range(6):
            n.mac[k] = MACS[q][k]
        n.ip, n.nat_enable = IPS[q], 1 if NAT[q] else 0
        out.append(n)
    return out


def _ip(u: int) -> bytes:
    return u.to_bytes(4, "big")


def l4_frame(proto: int, src: int, sport: int, dst: int, dport: int, dst_mac: bytes, ttl: int = 64,
             payload: bytes = b"0123456789") -> bytes:
    if proto == 17:
        l4 = R.build_udp(payload, sport, dport, _ip(src), _ip(dst))
    elif proto == 6:
        l4 = R.build_tcp(payload, sport, dport, _ip(src), _ip(dst), 1000, 2000, 0x18)
    else:
        l4 = R.build_icmp(payload, 8, sport.to_bytes(2, "big"), 1)
    return R.build_eth(R.build_ipv4(l4, proto, _ip(src), _ip(dst), ident=9, ttl=ttl), dst_mac, bytes([0x02, 0xCC, 0, 0, 0, 9]),
                       0x0800)


def pack(frames):
    """Frames packed at 4-byte boundaries: (data u8, offsets_dw u32, lens u16)."""
    offs, pos = [], 0
    for f in frames:
        offs.append(pos // 4)
        pos += (len(f) + 3) & ~3
    data = np.zeros(max(pos, 4), np.uint8)
    for f, o in zip(frames, offs):
        data[4 * o:4 * o + len(f)] = np.frombuffer(f, np.uint8)
    return data, np.array(offs, np.uint32), np.array([len(f) for f in frames], np.uint16)


def item_array(items, index=None):
    """Model items (remote_ip, remote_port, lan_ip, lan_port, proto, wan_port) as PMFLOW_ITEM_DTYPE."""
    from halo_amd._lib import PMFLOW_ITEM_DTYPE

    a = np.zeros(len(items), PMFLOW_ITEM_DTYPE)
    for j, it in enumerate(items):
        a[j] = (j if index is None else index[j], it[0], it[2], it[1], it[3], it[5], it[4], 0)
    return a


def listing_of(entries):
    """A PMFLOW_ENTRY_DTYPE array in the model's listing() form."""
    return sorted((int(e["id"]), int(e["remote_ip"]), int(e["remote_port"]), int(e["lan_ip"]), int(e["lan_port"]),
                   int(e["proto"]), int(e["wan_netif"]), int(e["wan_port"]), int(e["last_alive"])) for e in entries)


def fixture_items(make_table):
    """12 flows for a forced 16-slot table whose layout has a chain of >= 3 slots and a wrapped
    chain, found on the CPU with halo_pmflow_layout_stats: the first seed that gives both.
    `make_table()` returns a fresh 16-slot table. Returns (items, stats)."""
    for seed in range(64):
        rng = np.random.RandomState(1000 + seed)
        items = [(int(rng.randint(1, 1 << 31)), int(rng.randint(1, 65536)), SERVER + int(rng.randint(0, 4)),
                  int(rng.randint(1, 65536)), int(rng.choice([6, 17])), int(rng.randint(1, 65536))) for _ in range(12)]
        if len({it[:5] for it in items}) != 12:
            continue
        t = make_table()
        dropped, added = t.record(WAN2, item_array(items), 100)
        st = t.layout_stats()
        t.close()
        assert added == 12 and not dropped.any()
        if st["longest_chain"] >= 3 and st["wrapped"] >= 1:
            return items, st
    raise AssertionError("no seed gives a chain of 3 and a wrapped chain")


def _one(pat: str, text: str) -> str:
    m = re.findall(pat, text)
    assert len(m) == 1, (pat, m)
    return m[0]


def read_constants() -> dict:
    with open(os.path.join(CSRC, "pmflow_fwd.hip")) as fh:
        hip = fh.read()
    with open(os.path.join(CSRC, "pmflow_table.h")) as fh:
        hdr = fh.read()
    with open(os.path.join(CSRC, "arp_table.h")) as fh:
        arp = fh.read()
    # one workgroup per tile in both tile kernels: no grid cap, so no further edge
    assert len(re.findall(r"dim3\(n_tiles\), dim3\(kRecordTile\)", hip)) == 2
    assert "static_assert(kRecordTile == arp::kGatherTile" in hip
    from tests import scale_cases as S

    return {"kRecordTile": int(_one(r"constexpr uint32_t kRecordTile = (\d+);", hdr)),
            "kScanPass": S.scan_pass("pmflow_fwd.hip", "pmflow_scan_kernel"),
            "kGatherTile": int(_one(r"constexpr uint32_t kGatherTile = (\d+);", arp))}


def derived(c: dict) -> dict:
    """The first batch sizes past one tile and past one scan pass."""
    return {"record_tile": c["kRecordTile"] + 1, "record_scan_pass": c["kRecordTile"] * c["kScanPass"] + 1}


__all__ = ["PM", "AM"]
