"""Not a test: the egress step restated in plain Python / numpy (include/halo_rx.h, "egress") — no
tiles, no scans. One loop over the frames appends each selected, sendable frame's ring record to
its ports' streams; `egress_uniform` is the same for batches of one length, vectorised so that the
scale cases stay fast. Both return a `Want`: per-port written streams, summaries, index lists and
the skip count; `Want.out(fill)` is the whole output buffer a call leaves behind."""
from __future__ import annotations

import numpy as np

PORT_DTYPE = np.dtype([("frames", "<u4"), ("frames_written", "<u4"), ("bytes", "<u8"), ("bytes_written", "<u8")])
ARP_HIT, SW_UNICAST, SW_FLOOD = 6, 4, 5


def tx_len(length: int) -> int:
    return max(length, 60)  # BuildEthFrm


def record_size(length: int) -> int:
    return (4 + tx_len(length) + 3) & ~3  # ringBufferRecordSize


def sendable(length: int, jumbo: bool = False) -> bool:
    return 14 <= length <= (9014 if jumbo else 1514)


def record(frame: bytes) -> bytes:
    """u32 tx_len, the frame, zeros to tx_len, zeros to the 4-byte boundary."""
    return tx_len(len(frame)).to_bytes(4, "little") + frame + bytes(record_size(len(frame)) - 4 - len(frame))


def masks_of_arp(results: np.ndarray) -> np.ndarray:
    """A HIT goes to its out NetIf; everything else nowhere."""
    out = np.zeros(len(results), np.uint64)
    for i, r in enumerate(results):
        if int(r["verdict"]) == ARP_HIT and int(r["out_netif"]) < 64:
            out[i] = 1 << int(r["out_netif"])
    return out


def masks_of_switch(results: np.ndarray, flood_mask: int) -> np.ndarray:
    out = np.zeros(len(results), np.uint64)
    for i, r in enumerate(results):
        if int(r["verdict"]) == SW_FLOOD:
            out[i] = flood_mask
        elif int(r["verdict"]) == SW_UNICAST and int(r["out_port"]) < 64:
            out[i] = 1 << int(r["out_port"])
    return out


class Want:
    def __init__(self, n_ports, region_bytes, index_cap, streams, ports, index, skipped, offsets=None):
        self.n_ports, self.region_bytes, self.index_cap = n_ports, region_bytes, index_cap
        self.streams, self.ports, self.index, self.skipped = streams, ports, index, skipped
        self.offsets = offsets  # per port: the byte offset of every written record in its stream

    def out(self, fill: int = 0xA5, size: int | None = None) -> np.ndarray:
        buf = np.full(self.n_ports * self.region_bytes if size is None else size, fill, np.uint8)
        for p, s in enumerate(self.streams):
            buf[p * self.region_bytes:p * self.region_bytes + len(s)] = np.frombuffer(s, np.uint8) if isinstance(
                s, (bytes, bytearray)) else s
        return buf

    def index_array(self, fill: int = 0xA5A5A5A5) -> np.ndarray:
        arr = np.full((self.n_ports, self.index_cap), fill, np.uint32)
        for p, ix in enumerate(self.index):
            arr[p, :len(ix)] = ix
        return arr


def egress(frames, masks, n_ports: int, region_bytes: int, index_cap: int = 0, jumbo: bool = False) -> Want:
    streams = [bytearray() for _ in range(n_ports)]
    offsets = [[] for _ in range(n_ports)]
    index = [[] for _ in range(n_ports)]
    ports = np.zeros(n_ports, PORT_DTYPE)
    closed = [False] * n_ports
    skipped = 0
    for i, f in enumerate(frames):
        m = int(masks[i]) & ((1 << n_ports) - 1)
        if not m:
            continue
        if not sendable(len(f), jumbo):
            skipped += 1
            continue
        rec = record(bytes(f))
        for p in range(n_ports):
            if not (m >> p) & 1:
                continue
            if len(index[p]) < index_cap:
                index[p].append(i)
            ports[p]["frames"] += 1
            ports[p]["bytes"] += len(rec)
            if not closed[p] and len(streams[p]) + len(rec) <= region_bytes:
                offsets[p].append(len(streams[p]))
                streams[p] += rec
            else:
                closed[p] = True  # the first record that does not fit ends the prefix
    for p in range(n_ports):
        ports[p]["frames_written"], ports[p]["bytes_written"] = len(offsets[p]), len(streams[p])
    return Want(n_ports, region_bytes, index_cap, [bytes(s) for s in streams], ports,
                [np.array(ix, np.uint32) for ix in index], skipped, offsets)


def egress_uniform(frames2d: np.ndarray, masks: np.ndarray, n_ports: int, region_bytes: int, index_cap: int = 0) -> Want:
    """The same for n frames of one sendable length, frames2d uint8 [n, length]."""
    n, length = frames2d.shape
    assert sendable(length)
    rec = record_size(length)
    masks = np.asarray(masks, np.uint64)
    streams, index = [], []
    ports = np.zeros(n_ports, PORT_DTYPE)
    for p in range(n_ports):
        sel = np.flatnonzero((masks >> np.uint64(p)) & np.uint64(1))
        written = min(len(sel), region_bytes // rec)
        s = np.zeros((written, rec), np.uint8)
        s[:, :4] = np.frombuffer(tx_len(length).to_bytes(4, "little"), np.uint8)
        s[:, 4:4 + length] = frames2d[sel[:written]]
        streams.append(s.reshape(-1))
        index.append(sel[:index_cap].astype(np.uint32))
        ports[p] = (len(sel), written, len(sel) * rec, written * rec)
    return Want(n_ports, region_bytes, index_cap, streams, ports, index, 0)
