"""TEST INFRASTRUCTURE ONLY: a from-scratch model of KCP emit (include/halo_rx.h, "KCP emit") —
KCP.flush's packing with reserved == 0 (protocol/kcp/kcp.go:770-950, makeSpace / flushBuffer),
segment.encode (kcp.go:134-155) and BuildEnet (enet.go:75-97), the per-entry status, the capacity
rule and the summary — over plain Python values, built on zlib.crc32 and oracle.ref_xxh3_py.xxh3_64.
Imports nothing from halo_amd: the record layouts are restated here."""
from __future__ import annotations

import struct
import zlib

import numpy as np

from oracle.ref_xxh3_py import xxh3_64
from tests.kcp_cases import enet as build_enet
from tests.kcp_cases import seg as encode_seg

DISABLED, ZERO, CRC32, XXH3 = -1, 0, 1, 2
MODES = (DISABLED, ZERO, CRC32, XXH3)
KCP, ENET = 0, 1
OK, SEG_TOO_LONG, BAD_MTU, BAD_RANGE = 0, 1, 2, 3
MAX_MTU = 1472

SESSION = np.dtype([("conv", "<u8"), ("first_seg", "<u4"), ("n_segs", "<u4"), ("dst_ip", "<u4"), ("dst_port", "<u2"), ("mtu", "<u2"),
                    ("kind", "u1"), ("conn_type", "u1"), ("reserved", "<u2"), ("session_id", "<u4"), ("enet_conv", "<u4"),
                    ("enet_type", "<u4")])
SEG = np.dtype([("dgram", "<u4"), ("cmd", "u1"), ("frg", "u1"), ("wnd", "<u2"), ("ts", "<u4"), ("sn", "<u4"), ("una", "<u4"),
                ("len", "<u4"), ("data_off", "<u4"), ("check", "u1"), ("reserved", "u1", (3,))])
DGRAM = np.dtype([("offset", "<u4"), ("len", "<u2"), ("n_segs", "<u2"), ("session", "<u4"), ("first_seg", "<u4")])
DESC = np.dtype([("payload_off", "<u8"), ("payload_len", "<u2"), ("proto", "u1"), ("aux", "u1"), ("src_port", "<u2"),
                 ("dst_port", "<u2"), ("src_ip", "<u4"), ("dst_ip", "<u4"), ("seq", "<u4"), ("ack", "<u4"), ("dst_mac", "u1", (6,)),
                 ("mode", "u1"), ("pad", "u1")])
SUMMARY = np.dtype([("sessions", "<u4"), ("sessions_written", "<u4"), ("dgrams", "<u4"), ("dgrams_written", "<u4"), ("segs", "<u4"),
                    ("segs_written", "<u4"), ("status_counts", "<u4", (4,)), ("bytes", "<u8"), ("bytes_written", "<u8"),
                    ("bytes_hashed", "<u8"), ("out_segs", "<u8"), ("out_pkts", "<u8"), ("out_bytes", "<u8")])
assert (SESSION.itemsize, SEG.itemsize, DGRAM.itemsize, DESC.itemsize, SUMMARY.itemsize) == (40, 32, 16, 40, 88)


def overhead(mode):
    return 28 if mode == DISABLED else 32


def byte_check_hash(mode, data):
    if mode == CRC32:
        return zlib.crc32(data) & 0xFFFFFFFF
    if mode == XXH3:
        return xxh3_64(data) & 0xFFFFFFFF
    return 0


def flush(mode, conv, mtu, segments):
    """flush's packing: segments is [(cmd, frg, wnd, ts, sn, una, data)]; returns [(datagram bytes,
    segment count)]. The buffer is kcp.buffer, `size` what flush keeps in ptr."""
    H = overhead(mode)
    out, buffer, count = [], b"", 0
    for cmd, frg, wnd, ts, sn, una, data in segments:
        need = H + len(data)
        if len(buffer) + need > mtu:  # makeSpace
            out.append((buffer, count))
            buffer, count = b"", 0
        field = byte_check_hash(mode, data) if cmd == 81 else 0
        buffer += encode_seg(mode, cmd, data, conv=conv, frg=frg, wnd=wnd, ts=ts, sn=sn, una=una, field=field)
        count += 1
    if buffer:  # flushBuffer
        out.append((buffer, count))
    return out


class Want:
    """status uint8 [n_sessions]; stream bytes (the written prefix); dgrams DGRAM[]; descs DESC[];
    summary one SUMMARY record."""

    def __init__(self, status, stream, dgrams, descs, summary):
        self.status, self.stream, self.dgrams, self.descs, self.summary = status, stream, dgrams, descs, summary


def want_of(sessions, segs, payload: bytes, *, mode, src_ip, src_port, dgram_cap, stream_cap) -> Want:
    H = overhead(mode)
    s = np.zeros(1, SUMMARY)[0]
    status = np.zeros(len(sessions), np.uint8)
    stream, dgrams, descs = bytearray(), [], []
    prev_end, cut = 0, False
    n_dg = n_bytes = n_segs = 0  # of the OK entries so far
    for k, e in enumerate(sessions):
        first, n, mtu = int(e["first_seg"]), int(e["n_segs"]), int(e["mtu"])
        st, made, hashed = OK, [], 0
        if first + n > len(segs) or first < prev_end:
            st = BAD_RANGE
        elif e["kind"] == ENET:
            if e["conn_type"] > 3 or n:
                st = BAD_RANGE
            else:
                made = [(build_enet(int(e["conn_type"]), int(e["session_id"]), int(e["enet_conv"]), int(e["enet_type"])), 0)]
        elif e["kind"] != KCP:
            st = BAD_RANGE
        elif mtu <= H or mtu > MAX_MTU:
            st = BAD_MTU
        else:
            items = []
            for x in segs[first:first + n]:
                off, ln = int(x["data_off"]), int(x["len"])
                if off + ln > len(payload):
                    st = BAD_RANGE
                    break
                if H + ln > mtu:
                    st = SEG_TOO_LONG
                    break
                items.append((int(x["cmd"]), int(x["frg"]), int(x["wnd"]), int(x["ts"]), int(x["sn"]), int(x["una"]), payload[off:off + ln]))
                if x["cmd"] == 81 and mode in (CRC32, XXH3):
                    hashed += ln
            if st == OK:
                made = flush(mode, int(e["conv"]), mtu, items)
        prev_end = first + n
        status[k] = st
        s["status_counts"][st] += 1
        if st != OK:
            continue
        padded = sum((len(d) + 3) & ~3 for d, _ in made)
        if not cut and n_dg + len(made) <= dgram_cap and n_bytes + padded <= stream_cap and n_segs + n <= len(segs):
            at = first
            for d, c in made:
                rec = np.zeros(1, DGRAM)[0]
                rec["offset"], rec["len"], rec["n_segs"], rec["session"], rec["first_seg"] = len(stream), len(d), c, k, at
                at += c
                dsc = np.zeros(1, DESC)[0]
                dsc["payload_off"], dsc["payload_len"], dsc["proto"] = len(stream), len(d), 17
                dsc["src_ip"], dsc["src_port"], dsc["dst_ip"], dsc["dst_port"] = src_ip, src_port, e["dst_ip"], e["dst_port"]
                dgrams.append(rec)
                descs.append(dsc)
                stream += d + bytes(-len(d) % 4)
                s["out_bytes"] += len(d)
            s["sessions_written"] += 1
            s["dgrams_written"] += len(made)
            s["segs_written"] += n
            s["bytes_written"] += padded
            s["bytes_hashed"] += hashed
        else:
            cut = True
        s["sessions"] += 1
        n_dg, n_bytes, n_segs = n_dg + len(made), n_bytes + padded, n_segs + n
    s["dgrams"], s["bytes"], s["segs"] = n_dg, n_bytes, n_segs
    s["out_segs"], s["out_pkts"] = s["segs_written"], s["dgrams_written"]
    return Want(status, bytes(stream), np.array(dgrams, DGRAM) if dgrams else np.zeros(0, DGRAM),
                np.array(descs, DESC) if descs else np.zeros(0, DESC), s)


def enet_fields(data: bytes):
    """BuildEnet's packet back into (session_id, conv, enet_type)."""
    return struct.unpack(">III", data[4:16])
