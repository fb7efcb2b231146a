"""Not a test: shared by tests/test_respond_host.py and tests/test_gpu_respond.py — the crafted
frames that reach every row of the responders' table, the batches built from them, and, in the
manner of tests/egress_cases.py, where the responder kernels change behaviour with the batch size:
the tile and the scan pass, read out of the sources by regular expression so that a moved constant
moves the shapes. The count and scatter kernels launch one workgroup per tile, so no grid cap
exists; read_constants asserts that it stays so."""
from __future__ import annotations

import os
import re

import numpy as np

from oracle import ref_py as R
from tests import arp_cases as K
from tests import respond_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo_amd", "csrc")

SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
MAC = bytes([0xAA] * 6)
OWN_IP = 0xC0A86464  # 192.168.100.100, the golden fixtures' NetIf
PEER_MAC = bytes([0x02, 0x11, 0x22, 0x33, 0x44, 0x55])
SERVED = (80, 8080, 65535, 0)
NAT_V_SKIP, NAT_V_MISS, NAT_V_FLOW = 1, 2, 3
TX_TTL, TX_RECALC, R_ALIVE = 0x02, 0x08, 0x01
FILL = 0xA5


def model_netif(nat_enable=False) -> RM.NetIf:
    return RM.NetIf(MAC, OWN_IP, nat_enable)


def lib_netif(nat_enable=False):
    from halo_amd._lib import NetIf

    return NetIf.make("AA:AA:AA:AA:AA:AA", "192.168.100.100", nat_enable)


def _ip(u: int) -> bytes:
    return u.to_bytes(4, "big")


def eth_ip(l4: bytes, proto: int, src: int, dst: int, ttl=64, dst_mac=MAC) -> bytes:
    return R.build_eth(R.build_ipv4(l4, proto, _ip(src), _ip(dst), ident=7, ttl=ttl), dst_mac, PEER_MAC, 0x0800)


def echo_request(src: int, dst: int = OWN_IP, ident=0x1234, seq=7, payload=b"abcdefgh" * 2, typ=8, ttl=64, **kw) -> bytes:
    return eth_ip(R.build_icmp(payload, typ, ident.to_bytes(2, "big"), seq, **kw), 1, src, dst, ttl)


def tcp(src: int, dport: int, flags: int, seq: int, dst: int = OWN_IP, sport=40000, payload=b"") -> bytes:
    return eth_ip(R.build_tcp(payload, sport, dport, _ip(src), _ip(dst), seq, 99, flags), 6, src, dst)


def udp(src: int, dst: int, ttl=64, payload=b"0123456789", sport=5000, dport=53) -> bytes:
    return eth_ip(R.build_udp(payload, sport, dport, _ip(src), _ip(dst)), 17, src, dst, ttl)


PEER, FAR = 0xC0A86407, 0x08080808  # a LAN peer; somewhere the frame is forwarded to
ALIVE, DEAD, NO_TTL = (TX_TTL | TX_RECALC, R_ALIVE), (TX_TTL | TX_RECALC, 0), (TX_RECALC, 0)


def crafted():
    """(name, frame, nat verdict, (steps, result)) — every row of the table and its near misses.
    The nat and fix columns are what the forward path's state would say for that frame when the
    receiving NetIf forwards it; a test may drop either column (an absent input)."""
    c = []

    def add(name, frame, nat=NAT_V_FLOW, fix=ALIVE):
        c.append((name, frame, nat, fix))

    add("echo_local", echo_request(PEER))
    add("echo_local_odd_payload", echo_request(PEER, payload=b"xyz", ident=0xFFFF, seq=0xFFFF))
    add("echo_local_empty_payload", echo_request(PEER, payload=b"", ident=0, seq=0))
    add("echo_reply_no_answer", echo_request(PEER, typ=0))
    add("echo_bad_checksum", echo_request(PEER, csum=0x1234))
    add("echo_other_mac", R.build_eth(echo_request(PEER)[14:], PEER_MAC, PEER_MAC, 0x0800))
    add("echo_nat_miss", echo_request(FAR, dst=OWN_IP), nat=NAT_V_MISS)           # the NAT-miss ICMP fallback
    add("echo_forward_nat_miss", echo_request(FAR, dst=PEER), nat=NAT_V_MISS)     # FORWARD on any NetIf
    add("echo_reply_nat_miss", echo_request(FAR, dst=PEER, typ=0), nat=NAT_V_MISS)
    add("echo_nat_miss_dead_ttl", echo_request(FAR, dst=PEER, ttl=1), nat=NAT_V_MISS, fix=DEAD)  # echo wins
    add("udp_nat_miss", udp(FAR, PEER), nat=NAT_V_MISS)                           # a WAN miss that is not ICMP
    add("udp_nat_miss_dead_ttl", udp(FAR, PEER, ttl=1), nat=NAT_V_MISS, fix=DEAD)  # still nothing
    add("udp_ttl_dead", udp(PEER, FAR, ttl=1), fix=DEAD)
    add("udp_ttl_dead_min_frame", udp(PEER, FAR, ttl=0, payload=b""), fix=DEAD)
    add("udp_ttl_dead_nat_skip", udp(PEER, FAR, ttl=1), nat=NAT_V_SKIP, fix=DEAD)
    add("udp_ttl_alive", udp(PEER, FAR))
    add("udp_no_ttl_step", udp(PEER, FAR, ttl=1), fix=NO_TTL)
    add("icmp_ttl_dead", echo_request(PEER, dst=FAR, ttl=1), fix=DEAD)
    add("udp_local", udp(PEER, OWN_IP), fix=DEAD)                                 # LOCAL_UDP: the handlers' job
    add("tcp_syn_served", tcp(PEER, 80, 0x02, 1000))
    add("tcp_syn_served_65535", tcp(PEER, 65535, 0x02, 5))
    add("tcp_syn_served_port0", tcp(PEER, 0, 0x02, 5))
    add("tcp_syn_unserved", tcp(PEER, 81, 0x02, 1000))                            # an unserved TCP port
    add("tcp_synack", tcp(PEER, 8080, 0x12, 2000))                                # a SYN|ACK
    add("tcp_syn_wrap", tcp(PEER, 80, 0x02, 0xFFFFFFFF))                          # ack wraps to 0
    add("tcp_synack_wrap", tcp(PEER, 80, 0x12, 0xFFFFFFFF))
    add("tcp_ack_only", tcp(PEER, 80, 0x10, 1))
    add("tcp_syn_psh_payload", tcp(PEER, 80, 0x0A, 77, payload=b"hello"))
    add("tcp_syn_forwarded", tcp(PEER, 80, 0x02, 1, dst=FAR))
    add("tcp_syn_forwarded_dead", tcp(PEER, 80, 0x02, 1, dst=FAR), fix=DEAD)
    add("arp", R.build_eth(bytes(28), b"\xff" * 6, PEER_MAC, 0x0806))
    add("bcast_udp", udp(PEER, 0xC0A864FF), fix=DEAD)
    add("short", bytes(20))
    return c


# what the issue says the corpus must hold: name -> (nat_enable, kind or None)
MUST = {"echo_local": (False, RM.ECHO), "echo_nat_miss": (True, RM.ECHO), "udp_nat_miss": (True, None),
        "udp_ttl_dead": (False, RM.TTL), "tcp_syn_served": (False, RM.TCP_SYN), "tcp_syn_unserved": (False, None),
        "tcp_synack": (False, RM.TCP_SYNACK), "tcp_syn_wrap": (False, RM.TCP_SYN)}


def columns(cases):
    frames = [f for _, f, _, _ in cases]
    nat = np.array([v for _, _, v, _ in cases], np.uint8)
    steps = np.array([s for _, _, _, (s, _) in cases], np.uint8)
    result = np.array([r for _, _, _, (_, r) in cases], np.uint8)
    return frames, nat, steps, result


def batch(seed: int, n: int, density: str):
    """n frames for the device tests: density "none" (plain local UDP), "sparse" (replies only at
    both sides of a wave and a tile boundary and at the ends), "mixed" (the crafted frames in
    rotation from a random start) or "all" (every frame an echo request). Returns crafted-style
    tuples."""
    rng = np.random.default_rng(seed)
    pool = crafted()
    quiet = ("quiet", udp(PEER, OWN_IP), NAT_V_FLOW, ALIVE)
    if density == "none":
        return [quiet] * n
    if density == "all":
        return [("echo", echo_request(PEER, seq=i & 0xFFFF, payload=bytes(rng.integers(0, 256, 1 + i % 23, dtype=np.uint8))),
                 NAT_V_FLOW, ALIVE) for i in range(n)]
    if density == "sparse":
        at = {0: "echo_local", 63: "udp_ttl_dead", 64: "tcp_syn_served", 255: "tcp_synack", 256: "echo_local",
              n - 1: "tcp_syn_wrap"}
        by_name = {c[0]: c for c in pool}
        return [by_name[at[i]] if i in at else quiet for i in range(n)]
    assert density == "mixed"
    first = int(rng.integers(0, len(pool)))
    return [pool[(first + i) % len(pool)] for i in range(n)]


def pack(seed: int, frames):
    return K.pack(np.random.default_rng(seed), frames)


def ops_array(steps):
    from halo_amd import protocol

    ops = protocol.tx_ops(len(steps))
    ops["steps"] = steps
    ops["dst_ip"], ops["src_port"] = 0xDEADBEEF, 0xBEEF  # never read by the responder
    return ops


def check_outputs(o, want: RM.Want, what=""):
    """Every output of a responder call whole: `o` holds the raw arrays (desc [cap + slack, 40],
    src [.., 8], dst_ip, count [2], kinds [5], actions [n + slack]), prefilled with FILL (kinds with
    o["kc0"]). The first min(count, cap) entries equal the model's, everything else is still the
    prefill."""
    from halo_amd._lib import BUILD_DESC_DTYPE, RESPOND_SRC_DTYPE

    desc, src, dst_ip = want.arrays(BUILD_DESC_DTYPE, RESPOND_SRC_DTYPE)
    w = min(want.count, o["cap"])
    assert int(o["count"][0]) == want.count, (what, int(o["count"][0]), want.count)
    assert int(o["count"][1]) == 0xA5A5A5A5
    got = o["desc"].reshape(-1).view(BUILD_DESC_DTYPE)
    bad = np.flatnonzero(got[:w] != desc[:w])
    assert bad.size == 0, (what, [(int(k), got[k], desc[k]) for k in bad[:3]])
    assert np.all(o["desc"][w:] == FILL), what
    assert np.array_equal(o["src"].reshape(-1).view(RESPOND_SRC_DTYPE)[:w], src[:w]), what
    assert np.all(o["src"][w:] == FILL), what
    assert np.array_equal(o["dst_ip"][:w], dst_ip[:w]) and np.all(o["dst_ip"][w:] == 0xA5A5A5A5), what
    assert np.array_equal(o["kinds"][:4] - o["kc0"], want.kind_counts) and int(o["kinds"][4]) == o["kc0"], what
    assert np.array_equal(o["actions"][:o["n"]], want.actions), what
    assert np.all(o["actions"][o["n"]:] == FILL), what


# ---- past the edges ------------------------------------------------------------------------------
# edge -> the constants it follows from and the first n past it, as the launch code gives it today
BOUNDARIES = {
    "respond_tile": dict(kernels="respond_count_kernel, respond_scatter_kernel: second tile", constants=("kTile",),
                         first_past=257),
    "respond_scan_pass": dict(kernels="respond_scan_kernel: second pass", constants=("kTile", "kScanPass"),
                              first_past=262_145),
}


def _one(pattern: str, text: str) -> str:
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def read_constants() -> dict:
    with open(os.path.join(CSRC, "tx_respond.hip")) as fh:
        hip = fh.read()
    with open(os.path.join(CSRC, "tx_respond.h")) as fh:
        hdr = fh.read()
    # one workgroup per tile in both tile kernels: no grid cap, so no further edge
    assert len(re.findall(r"dim3\(n_tiles\), dim3\(kTile\)", hip)) == 2 and "kMax" not in hip
    from tests import scale_cases as S

    return {"kTile": int(_one(r"constexpr uint32_t kTile = (\d+);", hdr)),
            "kScanPass": S.scan_pass("tx_respond.hip", "respond_scan_kernel")}


def derived(c: dict) -> dict:
    return {"respond_tile": c["kTile"] + 1, "respond_scan_pass": c["kTile"] * c["kScanPass"] + 1}


def past(name: str, r: int) -> int:
    assert 65 <= r <= 300 and r % 64, r
    return BOUNDARIES[name]["first_past"] - 1 + r


def uniform_batch(n: int, reply_at):
    """n 64-byte frames back to back: template 0 (a plain local UDP frame) everywhere except
    template 1 (an echo request) at the indices `reply_at`. Returns (templates, tid, data,
    offsets_dw, lens)."""
    t0 = udp(PEER, OWN_IP, payload=bytes(range(22)))
    t1 = echo_request(PEER, payload=bytes(range(22)))
    assert len(t0) == len(t1) == 64
    tid = np.zeros(n, np.int64)
    tid[np.asarray(reply_at, np.int64)] = 1
    both = np.stack([np.frombuffer(t0, np.uint8), np.frombuffer(t1, np.uint8)])
    data = both[tid].reshape(-1)
    return [t0, t1], tid, data, (np.arange(n, dtype=np.int64) * 16).astype(np.uint32), np.full(n, 64, np.uint16)
