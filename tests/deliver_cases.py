"""Not a test: shared by tests/test_deliver_host.py and tests/test_gpu_deliver.py — the crafted
frames that reach every row of local delivery's decision and its near misses, the random batches at
the sizes around a wavefront and a tile, the uniform batch past the tile and the scan pass (the
constants read out of the sources by regular expression, so that a moved constant moves the
shapes), the records of a batch from the Python restatement of the rx path, and the whole-output
comparison both test files use."""
from __future__ import annotations

import os
import re

import numpy as np

from oracle import ref_py as R
from tests import arp_cases as K
from tests import deliver_model as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo_amd", "csrc")

SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
DENSITIES = ("none", "sparse", "edges", "all")
MAC = bytes([0xAA] * 6)
OWN_IP = 0xC0A86464  # 192.168.100.100, the golden fixtures' NetIf
PEER_MAC = bytes([0x02, 0x11, 0x22, 0x33, 0x44, 0x55])
PEER, FAR, BCAST = 0xC0A86407, 0x08080808, 0xC0A864FF
UDP_SERVED = (53, 4000, 65535, 0)
TCP_SERVED = (80, 8080, 65535, 0)
PAYLOAD_LENS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 1472)
JUMBO_PAYLOAD = 8972
FILL = 0xA5
MARK = 0xEE  # test_gpu_deliver's read contract: never a payload byte of the batches it marks


def model_netif(nat_enable=False) -> DM.NetIf:
    return DM.NetIf(MAC, OWN_IP, nat_enable)


def lib_netif(nat_enable=False):
    from halo_amd._lib import NetIf

    return NetIf.make("AA:AA:AA:AA:AA:AA", "192.168.100.100", nat_enable)


def _ip(u: int) -> bytes:
    return u.to_bytes(4, "big")


def eth_ip(l4: bytes, proto: int, src: int, dst: int, dst_mac=MAC) -> bytes:
    return R.build_eth(R.build_ipv4(l4, proto, _ip(src), _ip(dst), ident=7, ttl=64), dst_mac, PEER_MAC, 0x0800)


def udp(dport: int, payload: bytes = b"0123456789", src=PEER, dst=OWN_IP, sport=5000, **kw) -> bytes:
    return eth_ip(R.build_udp(payload, sport, dport, _ip(src), _ip(dst), **kw), 17, src, dst)


def tcp(dport: int, flags: int = 0x18, payload: bytes = b"", nibble: int = 5, src=PEER, dst=OWN_IP, sport=40000, seq=1000,
        ack=99) -> bytes:
    """The data-offset nibble is taken as BYTES by the reference (protocol/tcp.go:49,68): the
    handler's payload is pkt[nibble:], which starts inside the 20-byte header."""
    return eth_ip(R.build_tcp(payload, sport, dport, _ip(src), _ip(dst), seq, ack, flags, off_byte=nibble << 4), 6, src, dst)


def _bytes(n: int, salt: int = 0) -> bytes:
    return bytes((salt + 7 * k) % 251 for k in range(n))


def crafted(jumbo=False):
    """(name, frame) — every row of the decision and its near misses."""
    c = [("udp_served", udp(53)),
         ("udp_unserved", udp(54)),
         ("udp_port0", udp(0, b"to port zero")),
         ("udp_port65535", udp(65535, b"top")),
         ("udp_bad_checksum", udp(53, csum=0x1234)),
         ("udp_other_address", udp(53, dst=FAR)),
         ("bcast_67", udp(67, b"dhcp discover", src=0, dst=BCAST, sport=68)),
         ("bcast_68", udp(68, b"dhcp offer..", dst=BCAST, sport=67)),
         ("bcast_53", udp(53, b"not dhcp", dst=BCAST)),
         ("bcast_67_bad_checksum", udp(67, b"dhcp", dst=BCAST, csum=0x4321)),
         ("tcp_syn_empty", tcp(80, 0x02)),
         ("tcp_synack", tcp(8080, 0x12, seq=0xFFFFFFFF, ack=0x80000001)),
         ("tcp_unserved", tcp(81, 0x18, b"nobody listens")),
         ("tcp_port0", tcp(0, 0x10, b"zero")),
         ("tcp_bad_checksum", eth_ip(R.build_tcp(b"x", 40000, 80, _ip(PEER), _ip(OWN_IP), 1, 2, 0x18, csum=0x1111), 6, PEER, OWN_IP)),
         ("icmp_echo", eth_ip(R.build_icmp(b"abcdefgh", 8, b"\x12\x34", 7), 1, PEER, OWN_IP)),
         ("arp", R.build_eth(bytes(28), b"\xff" * 6, PEER_MAC, 0x0806)),
         ("wrong_mac", PEER_MAC + udp(53)[6:]),
         ("short", bytes(20))]
    for nib in range(16):  # payload_off = 34 + nibble: every source alignment, four times
        c.append((f"tcp_nibble_{nib}", tcp(80, 0x18, _bytes(17 + nib, nib), nibble=nib, seq=nib, ack=1000 + nib)))
    for n in PAYLOAD_LENS:
        c.append((f"udp_len_{n}", udp(4000, _bytes(n, n))))
        c.append((f"tcp_len_{n}", tcp(8080, 0x18, _bytes(n, n + 1), nibble=5 + n % 4)))
    if jumbo:
        c.append((f"udp_len_{JUMBO_PAYLOAD}", udp(4000, _bytes(JUMBO_PAYLOAD, 3))))
    return c


def as_lo_packets(cases):
    """The same set as LoChan packets: the bare IPv4 packet of every frame (what is left of a
    frame that is not IPv4 fails ParseIpv4Pkt, which is a case too)."""
    return [(name, f[14:]) for name, f in cases]


def source_alignments(frames, nif, **kw):
    """The set of (payload offset & 3) over the delivered frames: where the model's payload lies
    in the buffer, found by its length from the end of the IPv4 packet."""
    got = set()
    l3 = kw.get("l3", False)
    for f in frames:
        d = DM.delivery_of(f, nif, **kw)
        if d is None or not d["payload"]:
            continue
        pkt = f if l3 else f[14:]
        end = (0 if l3 else 14) + R.be16(pkt[2:4])
        got.add((end - len(d["payload"])) & 3)
    return got


def batch(seed: int, n: int, density: str):
    """n frames for the device tests. "none": nothing is delivered; "sparse": a delivery about
    every 37th frame; "edges": one on each side of every wave and tile boundary and at both ends;
    "all": every frame, UDP and TCP mixed with random lengths and data-offset nibbles."""
    rng = np.random.default_rng(seed)
    quiet = [udp(54), tcp(81, 0x18, b"unserved"), udp(53, dst=FAR), eth_ip(R.build_icmp(b"abcdefgh", 8, b"\0\1", 1), 1, PEER, OWN_IP)]

    def loud(i):
        pay = bytes(rng.integers(0, MARK, int(rng.integers(0, 90)), dtype=np.uint8))
        if rng.integers(0, 2):
            return udp(UDP_SERVED[i % 4], pay, sport=1024 + i % 100)
        return tcp(TCP_SERVED[i % 4], 0x18, pay, nibble=int(rng.integers(0, 16)), seq=i % 97, ack=i % 89, sport=1024 + i % 100)

    if density == "none":
        pick = lambda i: False  # noqa: E731
    elif density == "all":
        pick = lambda i: True  # noqa: E731
    elif density == "sparse":
        first = int(rng.integers(0, min(n, 37)))
        pick = lambda i: i % 37 == first  # noqa: E731
    else:
        assert density == "edges"
        pick = lambda i: i % 64 in (0, 63) or i == n - 1  # noqa: E731
    return [loud(i) if pick(i) else quiet[i % 4] for i in range(n)]


def pack(seed: int, frames):
    """Frames at 4-byte boundaries with random 4-byte gaps and garbage between them."""
    return K.pack(np.random.default_rng(seed), frames)


def records(frames, nif, *, check_sum_enable=True, jumbo=False, l3=False):
    """The records of `frames`, from the Python restatement of the rx path."""
    from halo_amd._lib import RESULT_DTYPE
    from halo_amd.protocol import STATUS_NAMES

    out = np.zeros(len(frames), RESULT_DTYPE)
    cache = {}
    for i, f in enumerate(frames):
        if f not in cache:
            cache[f] = (R.rx_lo_packet(f, nif.ip, check_sum_enable, jumbo) if l3
                        else R.rx_frame(f, nif.mac, nif.ip, check_sum_enable, jumbo))
        for k, v in cache[f].items():
            out[i][k] = STATUS_NAMES.index(v) if k == "status" else v
    return out


def new_outputs(region: int, index_cap: int):
    """0xA5-filled host outputs with a sentinel element behind each: out [region + 16], summary
    [40 + 8], index [index_cap + 1, 8]."""
    return dict(out=np.full(region + 16, FILL, np.uint8), summary=np.full(48, FILL, np.uint8),
                index=np.full((index_cap + 1, 8), FILL, np.uint8), region=region, index_cap=index_cap)


def check_outputs(o, want: DM.Want, what=""):
    """Every output of a delivery call whole: `o` holds the raw arrays as new_outputs makes them
    (downloaded, for a device call). The written prefix equals the model's stream, the summary and
    the first min(records, index_cap) index entries equal the model's, and everything else is
    still the prefill."""
    from halo_amd._lib import DELIVER_INDEX_DTYPE, DELIVER_SUMMARY_DTYPE

    stream, summary, index = want.expect(o["region"], o["index_cap"])
    s = o["summary"][:40].view(DELIVER_SUMMARY_DTYPE)[0]
    for k, v in summary.items():
        assert np.array_equal(s[k], v), (what, k, s[k], v)
    assert np.all(o["summary"][40:] == FILL), what
    got = o["out"][:len(stream)].tobytes()
    if got != stream:
        at = next(k for k in range(len(stream)) if got[k] != stream[k])
        raise AssertionError((what, "stream differs at byte", at, got[at - at % 4:at - at % 4 + 8].hex(),
                              stream[at - at % 4:at - at % 4 + 8].hex()))
    assert np.all(o["out"][len(stream):] == FILL), (what, "written past bytes_written")
    idx = o["index"].reshape(-1).view(DELIVER_INDEX_DTYPE)
    assert [(int(e["frame"]), int(e["offset"])) for e in idx[:len(index)]] == index, what
    assert np.all(o["index"][len(index):] == FILL), what


def cuts(want: DM.Want):
    """Region sizes (multiples of 16, so that the device call takes them) around the stream: 0, the
    largest below the end of a record in the middle, at or above the total, and far above it."""
    total = want.total_bytes
    mid = sum(map(len, want.recs[:max(1, len(want.recs) // 2)]))
    return sorted({0, (mid - 1) & ~15, (total + 15) & ~15, total + 4096})


# ---- past the edges ------------------------------------------------------------------------------
def _one(pattern: str, text: str) -> str:
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def read_constants() -> dict:
    with open(os.path.join(CSRC, "rx_deliver.hip")) as fh:
        hip = fh.read()
    with open(os.path.join(CSRC, "rx_deliver.h")) as fh:
        hdr = fh.read()
    with open(os.path.join(CSRC, "tile_scan.h")) as fh:
        scan = fh.read()
    with open(os.path.join(CSRC, "stream_scan.h")) as fh:
        stream = fh.read()
    # one workgroup per tile in both tile kernels: no grid cap, so no further edge; the scan kernel
    # calls the streams' fused scan (stream_scan.h), whose one loop advances by the shared kScanPass
    assert len(re.findall(r"dim3\(q\.n_tiles\), dim3\(kTile\)", hip)) == 2 and "kMax" not in hip
    assert '#include "stream_scan.h"' in hip and "t0 +=" not in hip and "kScanPass =" not in hip + stream
    _one(r"__global__ void __launch_bounds__\(256\) deliver_scan_kernel\([^)]*\) \{[^}]*?=\s*scan_stream_tiles\(", hip)
    assert len(re.findall(r"scan_stream_tiles\(", hip)) == 1 and '#include "tile_scan.h"' in stream
    assert _one(r"t0 < n_tiles; t0 \+= (\w+),", stream) == "kScanPass"
    return {"kTile": int(_one(r"constexpr uint32_t kTile = (\d+);", hdr)),
            "kScanPass": int(_one(r"constexpr uint32_t kScanPass = (\d+);", scan))}


OVERRUN = 4  # uniform_batch's template whose record is made to overrun its frame


def uniform_batch(n: int, deliver_at, tcp_at=(), dhcp_at=(), overrun_at=()):
    """n 64-byte frames back to back: template 0 (UDP to an unserved port) everywhere except
    template 1 (UDP to a served port) at the indices `deliver_at`, template 2 (TCP to a served
    port) at `tcp_at`, template 3 (a DHCP broadcast) at `dhcp_at` and template 4 (UDP to a served
    port; uniform_records makes its record overrun the frame) at `overrun_at`. Returns (templates,
    tid, data, offsets_dw, lens)."""
    templates = [udp(54, bytes(range(22))), udp(53, bytes(range(100, 122))), tcp(80, 0x18, bytes(range(50, 60)), seq=7, ack=11),
                 udp(67, bytes(range(200, 222)), src=0, dst=BCAST, sport=68), udp(4000, bytes(range(150, 172)))]
    assert {len(t) for t in templates} == {64}
    tid = np.zeros(n, np.int64)
    for k, at in enumerate((deliver_at, tcp_at, dhcp_at, overrun_at), 1):
        at = np.asarray(at, np.int64)
        assert not tid[at].any(), "an index is given twice"
        tid[at] = k
    data = np.stack([np.frombuffer(t, np.uint8) for t in templates])[tid].reshape(-1)
    return templates, tid, data, (np.arange(n, dtype=np.int64) * 16).astype(np.uint32), np.full(n, 64, np.uint16)


def uniform_records(templates, tid, nif):
    """The records of a uniform batch; those of template OVERRUN end one byte behind their frames,
    as tests/test_gpu_deliver.py's overrun test makes them."""
    recs = records(templates, nif)[tid]
    bad = tid == OVERRUN
    recs["payload_len"][bad] = 64 - recs["payload_off"][bad] + 1
    return recs


def uniform_want(templates, tid, nif, **kw) -> DM.Want:
    per = [None if k == OVERRUN else DM.delivery_of(t, nif, **kw) for k, t in enumerate(templates)]
    return DM.Want([(int(i), per[tid[i]]) for i in np.flatnonzero(np.array([p is not None for p in per])[tid])],
                   skipped=int(np.count_nonzero(tid == OVERRUN)))
