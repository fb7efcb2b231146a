"""TEST INFRASTRUCTURE ONLY: KCP ingest's crafted datagrams and the helpers its CPU and GPU tests
share — a small encoder restating segment.encode (protocol/kcp/kcp.go:134-155) and BuildEnet
(enet.go:75-97), a delivery stream made by hand from (kind, local_port, payload) items (the layout
of include/halo_rx.h's "local delivery": 24-byte header, payload, zeros to the next 4-byte
boundary), and the bit-for-bit comparison of a call's prefilled outputs with tests/kcp_model.py."""
from __future__ import annotations

import os
import re
import struct

import numpy as np

from tests import kcp_model as M

FILL = 0xA5
PORT = 22102
CONV = 0x1122334455667788
UDP, TCP, DHCP = 0, 1, 2
PUSH, ACK, WASK, WINS = 81, 82, 83, 84
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read_constants() -> dict:
    """The kernels' sizes, from the headers."""
    out = {}
    for name, pat in (("rx_kcp.h", r"constexpr uint32_t (kTile) = (\d+)"), ("tile_scan.h", r"constexpr uint32_t (kScanPass) = (\d+)"),
                      ("rx_kcp.h", r"constexpr uint32_t kCrcLanes = (\d+), (kCrcChunk) = (\d+)")):
        src = open(os.path.join(ROOT, "halo_amd", "csrc", name)).read()
        m = re.search(pat, src)
        if len(m.groups()) == 3:
            out["kCrcLanes"], out["kCrcChunk"] = int(m.group(1)), int(m.group(3))
        else:
            out[m.group(1)] = int(m.group(2))
    out["kCrcStride"] = out["kCrcLanes"] * out["kCrcChunk"]
    return out


def seg(mode, cmd=PUSH, data=b"", *, conv=CONV, frg=0, wnd=256, ts=1000, sn=0, una=0, field=None, length=None) -> bytes:
    """segment.encode + the data: the hash field is byte_check_hash(data) for a PUSH segment and 0
    for the others unless ``field`` says otherwise; ``length`` overrides the length word."""
    h = struct.pack("<QBBHIIII", conv, cmd, frg, wnd, ts, sn, una, len(data) if length is None else length)
    if mode != M.DISABLED:
        if field is None:
            field = M.byte_check_hash(mode, data) if cmd == PUSH else 0
        h += struct.pack("<I", field)
    return h + data


def enet(t, session_id=0x01020304, conv=0x0A0B0C0D, enet_type=1234567890) -> bytes:
    head, tail = M.MAGIC[t]
    return head + struct.pack(">III", session_id, conv, enet_type) + tail


def rnd(seed, n) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def crafted(mode):
    """[(name, payload)] — every payload is delivered as UDP to PORT."""
    H = M.overhead(mode)
    c = read_constants()
    K, S = c["kCrcChunk"], c["kCrcStride"]
    out = [(f"len{n}", rnd(n, n)) for n in (0, 1, 19, 21, H - 1, 2 * H - 1)]
    out += [("len20_random", rnd(20, 20)), ("len20_zeros", bytes(20))]
    out += [(f"enet{t}", enet(t, 100 + t, 200 + t, 300 + t)) for t in range(4)]
    out.append(("enet_wrong_tail", enet(1)[:16] + M.MAGIC[2][1]))
    out.append(("enet_wrong_head", M.MAGIC[3][0][:3] + b"\x28" + enet(3)[4:]))
    out.append(("one_empty_ack", seg(mode, ACK)))                                   # L == H
    out.append(("one_byte_push", seg(mode, PUSH, b"\x7f")))                         # L == H + 1
    out.append(("short_tail", seg(mode, PUSH, b"abc") + rnd(1, H - 1)))
    out.append(("length_past", seg(mode, PUSH, b"abcd", length=5)))                # -2
    out.append(("length_past_2nd", seg(mode, ACK) + seg(mode, PUSH, b"xy", length=3)))
    out.append(("length_huge", seg(mode, PUSH, b"", length=0xFFFFFFFF)))
    out += [(f"cmd{cmd}", seg(mode, ACK) + seg(mode, cmd, b"zz")) for cmd in (80, 85, 0, 255)]  # -3
    out.append(("conv_changes", seg(mode, PUSH, b"first") + seg(mode, PUSH, b"second", conv=CONV ^ 1 << 40)))  # -1, n_segs 1
    out.append(("conv_low_changes", seg(mode, ACK) + seg(mode, ACK) + seg(mode, ACK, conv=CONV ^ 1)))
    out.append(("bad_hash_1st", seg(mode, PUSH, b"payload-one", field=0xDEADBEEF) + seg(mode, PUSH, b"payload-two")))
    out.append(("bad_hash_2nd", seg(mode, PUSH, b"payload-one") + seg(mode, PUSH, b"payload-two", field=0xDEADBEEF)
                + seg(mode, PUSH, b"payload-three") + seg(mode, ACK)))
    out.append(("bad_hash_then_bad_cmd", seg(mode, PUSH, b"q" * 40, field=1) + seg(mode, 99)))
    out.append(("ack_garbage_field", seg(mode, ACK, field=0xCAFEF00D) + seg(mode, WASK, field=7) + seg(mode, WINS, field=9)))
    out.append(("empty_push", seg(mode, PUSH, b"")))
    out.append(("empty_push_bad_field", seg(mode, PUSH, b"", field=5)))
    out.append(("zero_mode_nonzero_field", seg(mode, PUSH, b"data", field=1)))
    out.append(("bytes_28_31", seg(M.DISABLED, PUSH, b"\x01\x02\x03\x04rest")))     # disabled: bytes 28..31 are data
    out.append(("mtu", seg(mode, PUSH, rnd(5, 1368), sn=7, frg=2)))
    out.append(("mixed", seg(mode, ACK, sn=3, ts=5) + seg(mode, PUSH, rnd(6, 100), sn=4) + seg(mode, WASK) + seg(mode, PUSH, rnd(7, 17), sn=5)
                + seg(mode, WINS)))
    # hash coverage: each start alignment (the data starts H + a bytes into a 4-aligned payload)
    # crossed with each end residue, for lengths of every XXH3 class and around the CRC chunk / stride
    lens = [0, 1, 3, 4, 8, 9, 16, 17, 128, 129, 240, 241, 1024, 1025, K - 1, K, K + 1, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1]
    for a in range(4):
        body = seg(mode, ACK, b"\x00" * a)  # a first segment of a data bytes shifts what follows
        for n in lens:
            body += seg(mode, PUSH, rnd(1000 * a + n, n), sn=n)
            if len(body) > 1200:
                out.append((f"hash_a{a}_upto{n}", body))
                body = seg(mode, ACK, b"\x00" * a)
        for r in range(4):
            body += seg(mode, PUSH, rnd(77 + 4 * a + r, 60 + r))
        out.append((f"hash_a{a}_tail", body))
    out.append(("one_big_segment", seg(mode, PUSH, rnd(9, 65507 - H))))
    out.append(("many_empty_segments", b"".join(seg(mode, (ACK, PUSH, WASK, WINS)[i & 3], sn=i) for i in range(2040))))
    return out


class Delivery:
    """A delivery made by hand: what halo_amd.deliver.DeliverResult shows, for the model and the
    host call. items: (kind, local_port, payload); ``unwritten`` further records lie beyond the
    region (index offset 0xFFFFFFFF); ``index_cap`` defaults to every record."""

    def __init__(self, items, *, unwritten=0, index_cap=None):
        parts, offs = [], []
        at = 0
        for i, (kind, port, payload) in enumerate(items):
            offs.append(at)
            rec = struct.pack("<IBBHIHHII", i * 3 + 1, kind, 0x18 if kind == TCP else 0, len(payload), 0x0A000001 + i, 4000 + i % 1000,
                              port, i, 2 * i) + payload
            rec += bytes(-len(rec) % 4)
            parts.append(rec)
            at += len(rec)
        self.records_total = len(items) + unwritten
        self.index_cap = self.records_total if index_cap is None else index_cap
        self.region_bytes = (at + 15) & ~15
        self.out = np.full(self.region_bytes + 16, 0xEE, np.uint8)  # bytes beyond bytes_written are not the stream's
        self.out[:at] = np.frombuffer(b"".join(parts), np.uint8)
        summary = np.zeros(1, np.dtype([("records", "<u4"), ("records_written", "<u4"), ("bytes", "<u8"), ("bytes_written", "<u8"),
                                        ("kind_counts", "<u4", (3,)), ("skipped", "<u4")]))
        summary["records"], summary["records_written"] = self.records_total, len(items)
        summary["bytes"], summary["bytes_written"] = at + 48 * unwritten, at
        self.summary_raw = summary.view(np.uint8).reshape(-1)
        index = np.zeros((max(self.index_cap, 1), 2), np.uint32)
        for k in range(min(self.index_cap, self.records_total)):
            index[k] = (3 * k + 1, offs[k] if k < len(items) else 0xFFFFFFFF)
        self.index_raw = index.view(np.uint8).reshape(-1, 8)
        self._items, self.bytes_written = items, at

    def records(self):
        from halo_amd._lib import DELIVER_HDR_DTYPE

        raw = self.out[:self.bytes_written].tobytes()
        at = 0
        while at < len(raw):
            h = np.frombuffer(raw, DELIVER_HDR_DTYPE, 1, at)[0]
            n = int(h["payload_len"])
            yield h, raw[at + 24:at + 24 + n]
            at += 24 + ((n + 3) & ~3)

    def stream(self):
        return self.out[:self.bytes_written]


def udp(payloads, port=PORT):
    return [(UDP, port, p) for p in payloads]


def check_outputs(got, want: M.Want, dgram_cap, seg_cap, what=""):
    """got: dict(dgrams=[dgram_cap + 1, 40] u8, segs=[seg_cap + 1, 32] u8, summary=[96 + 8] u8), each
    0xA5-prefilled with a sentinel element behind it."""
    s = got["summary"][:96].view(M.SUMMARY)[0]
    for f in M.SUMMARY.names:
        assert np.array_equal(s[f], want.summary[f]), (what, f, s[f], want.summary[f])
    assert (got["summary"][96:] == FILL).all(), (what, "summary sentinel")
    nd, ns = int(s["dgrams_written"]), int(s["segs_written"])
    assert nd == len(want.dgrams) <= dgram_cap and ns == len(want.segs) <= seg_cap, what
    d = got["dgrams"][:nd].reshape(-1).view(M.DGRAM)
    x = got["segs"][:ns].reshape(-1).view(M.SEG)
    for f in M.DGRAM.names:
        assert np.array_equal(d[f], want.dgrams[f]), (what, "dgram", f, np.flatnonzero(d[f] != want.dgrams[f])[:5])
    for f in M.SEG.names:
        bad = np.flatnonzero((x[f] != want.segs[f]).reshape(ns, -1).any(axis=1)) if ns else []
        assert len(bad) == 0, (what, "seg", f, bad[:5], x[f][bad[:5]], want.segs[f][bad[:5]])
    assert got["dgrams"][:nd].tobytes() == want.dgrams.tobytes() and got["segs"][:ns].tobytes() == want.segs.tobytes(), what
    assert (got["dgrams"][nd:] == FILL).all() and (got["segs"][ns:] == FILL).all(), (what, "written beyond the prefixes")


def feed_log(result):
    """KcpIngestResult.feed's calls in the model's form."""
    log = []
    result.feed(
        on_kcp=lambda d, segs, payloads: log.append(("kcp", int(d["index"]), int(d["conv0"]), int(d["ret"]), [
            (int(s["cmd"]), int(s["frg"]), int(s["wnd"]), int(s["ts"]), int(s["sn"]), int(s["una"]), bytes(p))
            for s, p in zip(segs, payloads)])),
        on_enet=lambda d: log.append(("enet", int(d["index"]), int(d["conn_type"]), int(d["session_id"]), int(d["conv"]),
                                      int(d["enet_type"]), int(d["conv0"]))))
    return log


def device_entry_answers(base: int, send_well_formed: bool = True):
    """halo_kcp_ingest_device's argument checks over 64-byte-aligned addresses from ``base`` (4 KiB
    of zeros: an empty delivery, every array whole and apart): returns (well_formed, [(what,
    answer)]) — the answer of a well-formed call (None when not sent), and of calls that each
    differ from it in one argument and must be HALO_E_INVAL. Nothing is dereferenced before the
    checks, so host addresses serve where there is no device; with device addresses the
    well-formed call runs (and finds no record)."""
    import ctypes

    from halo_amd import _lib

    L = _lib.lib
    wsb = int(L.halo_kcp_ingest_workspace(300, 8))
    assert wsb == 8 * 2 + 24 * 8
    # stream 64 B | delivery summary 40 | summary 96 | dgrams 4 x 40 | segs 8 x 32 | workspace 208 | index 300 x 8
    at = dict(stream=base, dsum=base + 64, summary=base + 128, dgrams=base + 256, segs=base + 512, ws=base + 768, index=base + 1024)
    assert at["index"] + 8 * 300 <= base + 4096

    def call(mode=1, port=PORT, dgram_cap=4, seg_cap=8, cfg_null=False, cap=300, ws_bytes=wsb, **ptr):
        a = {**at, **ptr}
        cfg = _lib.KcpConfig()
        cfg.byte_check_mode, cfg.port, cfg.dgram_cap, cfg.seg_cap = mode, port, dgram_cap, seg_cap
        return L.halo_kcp_ingest_device(None if cfg_null else ctypes.byref(cfg), a["stream"], a["dsum"], a["index"], cap, a["dgrams"],
                                        a["segs"], a["summary"], a["ws"], ws_bytes, None)

    bad = [dict(cfg_null=True), dict(summary=None), dict(dsum=None), dict(mode=-2), dict(mode=3), dict(mode=7), dict(port=65536),
           dict(stream=None), dict(index=None), dict(dgrams=None), dict(segs=None), dict(ws=None), dict(ws_bytes=wsb - 1),
           # one per documented alignment: segs 16; dgrams, index, both summaries, workspace 8; stream 4
           dict(segs=at["segs"] + 8), dict(segs=at["segs"] + 4), dict(dgrams=at["dgrams"] + 4), dict(index=at["index"] + 4),
           dict(summary=at["summary"] + 4), dict(dsum=at["dsum"] + 4), dict(ws=at["ws"] + 4), dict(stream=base + 2),
           dict(stream=base + 1)]
    return (call() if send_well_formed else None), [(kw, call(**kw)) for kw in bad]
