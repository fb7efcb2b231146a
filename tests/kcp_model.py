"""TEST INFRASTRUCTURE ONLY: a from-scratch Python model of KCP ingest (include/halo_rx.h, "KCP
ingest"), restated from the reference's lines — Listener.packetInput (protocol/kcp/session.go:
866-921), ParseEnet (enet.go:100-145), KCP.Input's loop (kcp.go:613-709) and the DefaultSnmp adds
(session.go:722-726, kcp.go:710) — with zlib.crc32 and oracle.ref_xxh3_py.xxh3_64 as the byte
checks. It takes payloads from ``DeliverResult.records()`` (never from descriptors) and shares no
code with halo_amd or the library."""
from __future__ import annotations

import struct
import zlib

import numpy as np

from oracle.ref_xxh3_py import xxh3_64

DISABLED, ZERO, CRC32, XXH3 = -1, 0, 1, 2
MODES = (DISABLED, ZERO, CRC32, XXH3)
KCP, ENET = 0, 1
NA, PASSED, FAILED = 0, 1, 2
UDP = 0
HDR = 24
MAGIC = ((bytes.fromhex("000000ff"), bytes.fromhex("ffffffff")), (bytes.fromhex("00000145"), bytes.fromhex("14514545")),
         (bytes.fromhex("00000194"), bytes.fromhex("19419494")), (bytes.fromhex("00000227"), bytes.fromhex("22722727")))

DGRAM = np.dtype([("index", "<u4"), ("kind", "u1"), ("conn_type", "u1"), ("ret", "i1"), ("reserved", "u1"), ("conv0", "<u8"),
                  ("n_segs", "<u2"), ("n_walked", "<u2"), ("first_seg", "<u4"), ("payload_len", "<u4"), ("session_id", "<u4"),
                  ("conv", "<u4"), ("enet_type", "<u4")])
SEG = np.dtype([("dgram", "<u4"), ("cmd", "u1"), ("frg", "u1"), ("wnd", "<u2"), ("ts", "<u4"), ("sn", "<u4"), ("una", "<u4"),
                ("len", "<u4"), ("data_off", "<u4"), ("check", "u1"), ("reserved", "u1", (3,))])
SUMMARY = np.dtype([("dgrams", "<u4"), ("dgrams_written", "<u4"), ("segs", "<u4"), ("segs_written", "<u4"),
                    ("ret_counts", "<u4", (5,)), ("enet_counts", "<u4", (4,)), ("ignored", "<u4"), ("bytes_hashed", "<u8"),
                    ("in_pkts", "<u8"), ("in_bytes", "<u8"), ("in_errs", "<u8"), ("in_segs", "<u8")])
assert (DGRAM.itemsize, SEG.itemsize, SUMMARY.itemsize) == (40, 32, 96)


def overhead(mode):
    return 28 if mode == DISABLED else 32


def byte_check_hash(mode, data):
    if mode == CRC32:
        return zlib.crc32(data) & 0xFFFFFFFF
    if mode == XXH3:
        return xxh3_64(data) & 0xFFFFFFFF
    return 0


def parse_enet(p):
    """(conn_type, session_id, conv, enet_type, raw_conv) or None."""
    for t, (head, tail) in enumerate(MAGIC):
        if p[:4] == head and p[16:] == tail:
            sid, conv, et = struct.unpack(">III", p[4:16])
            return t, sid, conv, et, int.from_bytes(p[4:12], "little")
    return None


def walk(p, mode):
    """Input over one datagram: (ret, n_segs, walked) — walked is one (cmd, frg, wnd, ts, sn, una,
    length, data position, check) per segment that passed the conv, length and cmd checks."""
    h = overhead(mode)
    conv0 = int.from_bytes(p[:8], "little")
    pos, walked, ret = 0, [], 0
    while len(p) - pos >= h:
        conv, cmd, frg, wnd, ts, sn, una, length = struct.unpack_from("<QBBHIIII", p, pos)
        field = struct.unpack_from("<I", p, pos + 28)[0] if h == 32 else 0
        pos += h
        if conv != conv0:
            ret = -1
            break
        if length > len(p) - pos:
            ret = -2
            break
        if cmd not in (81, 82, 83, 84):
            ret = -3
            break
        check = NA
        if mode != DISABLED and cmd == 81:
            check = PASSED if field == byte_check_hash(mode, p[pos:pos + length]) else FAILED
        walked.append((cmd, frg, wnd, ts, sn, una, length, pos, check))
        pos += length
    n_segs = len(walked)
    for i, w in enumerate(walked):
        if w[8] == FAILED:
            n_segs, ret = i, -4
            break
    return ret, n_segs, walked


class Want:
    """The expected outputs of one call."""

    def __init__(self, dgrams, segs, summary, feed):
        self.dgrams, self.segs, self.summary, self.feed = dgrams, segs, summary, feed


def want_of(delivery, *, port, mode, dgram_cap, seg_cap, index_cap=None) -> Want:
    """From a DeliverResult's written records. ``index_cap`` (default: the result's) bounds the
    considered entries as the call's does."""
    cap = delivery.index_cap if index_cap is None else index_cap
    dg, sg = [], []
    s = np.zeros(1, SUMMARY)[0]
    feed, cut = [], False
    at = 0
    for k, (h, payload) in enumerate(delivery.records()):
        off, at = at, at + HDR + ((len(payload) + 3) & ~3)
        if k >= cap or int(h["kind"]) != UDP or int(h["local_port"]) != port:
            continue
        L = len(payload)
        if L == 20:
            e = parse_enet(payload)
            if e is None:
                s["ignored"] += 1
                continue
            item = ("enet", e)
            n_walked = 0
        elif L >= overhead(mode):
            item = ("kcp", walk(payload, mode))
            n_walked = len(item[1][2])
        else:
            s["ignored"] += 1
            continue
        if not cut and int(s["dgrams"]) < dgram_cap and int(s["segs"]) + n_walked <= seg_cap:
            j, first = len(dg), len(sg)
            d = np.zeros(1, DGRAM)[0]
            d["index"], d["payload_len"], d["first_seg"] = k, L, first
            if item[0] == "enet":
                t, sid, conv, et, raw = item[1]
                d["kind"], d["conn_type"], d["session_id"], d["conv"], d["enet_type"], d["conv0"] = ENET, t, sid, conv, et, raw
                s["enet_counts"][t] += 1
                feed.append(("enet", k, t, sid, conv, et, raw))
            else:
                ret, n_segs, walked = item[1]
                d["kind"], d["ret"], d["n_segs"], d["n_walked"] = KCP, ret, n_segs, n_walked
                d["conv0"] = int.from_bytes(payload[:8], "little")
                for cmd, frg, wnd, ts, sn, una, length, pos, check in walked:
                    x = np.zeros(1, SEG)[0]
                    x["dgram"], x["cmd"], x["frg"], x["wnd"], x["ts"], x["sn"], x["una"] = j, cmd, frg, wnd, ts, sn, una
                    x["len"], x["data_off"], x["check"] = length, off + HDR + pos, check
                    sg.append(x)
                    if cmd == 81 and mode in (CRC32, XXH3):
                        s["bytes_hashed"] += length
                s["ret_counts"][-ret] += 1
                s["in_pkts"] += 1
                s["in_bytes"] += L
                if ret:
                    s["in_errs"] += 1
                else:
                    s["in_segs"] += n_segs  # Input returns before its InSegs add on an error (kcp.go:644-710)
                feed.append(("kcp", k, int(d["conv0"]), ret,
                             [(w[0], w[1], w[2], w[3], w[4], w[5], bytes(payload[w[7]:w[7] + w[6]])) for w in walked[:n_segs]]))
            dg.append(d)
            s["dgrams_written"] += 1
            s["segs_written"] += n_walked
        else:
            cut = True
        s["dgrams"] += 1
        s["segs"] += n_walked
    return Want(np.array(dg, DGRAM) if dg else np.zeros(0, DGRAM), np.array(sg, SEG) if sg else np.zeros(0, SEG), s, feed)
