"""Not a test: the loopback step (include/halo_rx.h, "loopback") restated from scratch in plain
Python, working from frame BYTES — no tiles, no scans, no records.

* `forward_copy` — Ipv4RouteForward's LoChan branch (engine/ipv4_engine.go:193-201) for one frame
  over tests/arp_model.py's NetIf and route state: the out NetIf and the packet it is sent, or None.
  `mark_of` is the same decision taken where the chain takes it, ahead of the NAT step, from the
  frame as it was received.
* `tx_copy` — TxIpv4's (:71-80) for one locally built frame: exactly totalLen bytes.
* `gather` — the channel order: one loop over the frames appends each copy to its NetIf's region;
  `gather_uniform` is the same for batches of one length, vectorised so that the scale cases stay
  fast. Both return a `Want`: the whole output buffer, summaries, per-packet arrays, skip count.
* `drain` — PacketHandle's drain of one NetIf's packets (engine/engine.go:353-381): parsed with the
  restated rx path (oracle/ref_py.py), answered as the restated responders answer (tests/
  respond_model.py over oracle/ref_tx_py.py's tx_build), delivered as tests/deliver_model.py says.
"""
from __future__ import annotations

import numpy as np

from oracle import ref_py as R
from tests import arp_model as AM
from tests import deliver_model as DM
from tests import respond_model as RM

PORT_DTYPE = np.dtype([("frames", "<u4"), ("frames_written", "<u4"), ("bytes", "<u8"), ("bytes_written", "<u8")])
NOT_WRITTEN = 0xFFFFFFFF
V_OVERRIDE = 3  # HALO_PMFLOW_V_OVERRIDE


def _out_netif(arp: AM.Model, route, via):
    """The out NetIf of :180-186: the via's when it overrides, else the route's; None for no route,
    the emptied list, an id the device copy does not know or a NetIf the table does not have."""
    if via is not None and via[0] == V_OVERRIDE:
        out = via[1]
    elif route is None or route in (AM.ROUTE_NONE, AM.ROUTE_PANIC_ID):
        return None
    else:
        out = route[1]
    return out if out < len(arp.netifs) else None


def forward_copy(arp: AM.Model, frame: bytes, route, in_netif: int, via=None, selected: bool = True):
    """:193-201 for a frame as it is when the L2 step sees it (TTL decremented): (out NetIf, the
    ethPayload) when the packet goes into the out NetIf's LoChan, else None."""
    if not selected or len(frame) < 34 or frame[12:14] != b"\x08\x00":
        return None
    out = _out_netif(arp, route, via)
    if out is None or arp.netifs[in_netif].nat_enable:
        return None
    if AM.ip_of(frame[30:34]) != arp.netifs[out].ip:
        return None
    return out, frame[14:]


def mark_of(arp: AM.Model, frame: bytes, nif, route, in_netif: int, via=None) -> int:
    """The same decision from the frame as it was received by NetIf `nif` (an arp_model NetIf), for
    every frame whose parse reached the IPv4 addresses (ip_proto is set)."""
    r = R.rx_frame(frame, nif.mac, nif.ip)
    if r["ip_proto"] == 0xFF:
        return 0
    out = _out_netif(arp, route, via)
    if out is None or arp.netifs[in_netif].nat_enable:
        return 0
    return 1 if r["dst_ip"] == arp.netifs[out].ip else 0


def tx_copy(arp: AM.Model, frame: bytes, route, self_netif: int, selected: bool = True):
    """:71-80 for a built frame: (out NetIf, pkt[:totalLen]) when TxIpv4 puts it into a LoChan."""
    v, out, _tx, _target, _after = RM.tx_ipv4(arp, frame, route, self_netif, selected)
    if v != AM.LOOPBACK:
        return None
    total = frame[16] << 8 | frame[17]
    return out, frame[14:14 + total]


def netifs_of_results(results, n_netifs: int):
    """Per frame the NetIf whose LoChan the gather sends it to, or None: LOOPBACK and a NetIf below n_netifs."""
    return [int(r["out_netif"]) if int(r["verdict"]) == AM.LOOPBACK and int(r["out_netif"]) < n_netifs else None
            for r in results]


def packet_of(frame: bytes, tx: bool, jumbo: bool = False):
    """The bytes a selected frame sends, or None when it is not sendable."""
    n = len(frame)
    if tx:
        if n < 18:
            return None
        total = frame[16] << 8 | frame[17]
        return frame[14:14 + total] if 20 <= total <= n - 14 else None
    return frame[14:] if 34 <= n <= (9014 if jumbo else 1514) else None


class Want:
    def __init__(self, n_netifs, region_bytes, index_cap, streams, ports, pkt_off, pkt_len, index, skipped):
        self.n_netifs, self.region_bytes, self.index_cap = n_netifs, region_bytes, index_cap
        self.streams, self.ports, self.skipped = streams, ports, skipped
        self.pkt_off, self.pkt_len, self.index = pkt_off, pkt_len, index  # per NetIf, min(frames, index_cap) entries

    def out(self, fill: int = 0xA5, size: int | None = None) -> np.ndarray:
        buf = np.full(self.n_netifs * self.region_bytes if size is None else size, fill, np.uint8)
        for p, s in enumerate(self.streams):
            buf[p * self.region_bytes:p * self.region_bytes + len(s)] = np.frombuffer(s, np.uint8) if isinstance(
                s, (bytes, bytearray)) else s
        return buf

    def _array(self, lists, dtype, fill):
        arr = np.full((self.n_netifs, max(self.index_cap, 1)), fill, dtype)
        for p, x in enumerate(lists):
            arr[p, :len(x)] = x
        return arr

    def arrays(self):
        """(pkt_off_dw u32, pkt_len u16, index u32), each [n_netifs, max(index_cap, 1)], 0xA5 where no entry is written."""
        return (self._array(self.pkt_off, np.uint32, 0xA5A5A5A5), self._array(self.pkt_len, np.uint16, 0xA5A5),
                self._array(self.index, np.uint32, 0xA5A5A5A5))


def gather(frames, netifs, n_netifs: int, region_bytes: int, index_cap: int, tx: bool = False, jumbo: bool = False) -> Want:
    """`netifs[i]`: the NetIf frame i's copy goes to, or None (netifs_of_results)."""
    streams = [bytearray() for _ in range(n_netifs)]
    pkt_off, pkt_len, index = ([[] for _ in range(n_netifs)] for _ in range(3))
    ports = np.zeros(n_netifs, PORT_DTYPE)
    closed = [False] * n_netifs
    skipped = 0
    for i, f in enumerate(frames):
        p = netifs[i]
        if p is None or p >= n_netifs:
            continue
        pkt = packet_of(bytes(f), tx, jumbo)
        if pkt is None:
            skipped += 1
            continue
        size = (len(pkt) + 3) & ~3
        fits = not closed[p] and len(streams[p]) + size <= region_bytes
        if len(index[p]) < index_cap:
            pkt_off[p].append(len(streams[p]) // 4 if fits else NOT_WRITTEN)
            pkt_len[p].append(len(pkt))
            index[p].append(i)
        ports[p]["frames"] += 1
        ports[p]["bytes"] += size
        if fits:
            streams[p] += pkt + bytes(size - len(pkt))
            ports[p]["frames_written"] += 1
        else:
            closed[p] = True  # the first packet that does not fit ends the prefix
    for p in range(n_netifs):
        ports[p]["bytes_written"] = len(streams[p])
    return Want(n_netifs, region_bytes, index_cap, [bytes(s) for s in streams], ports, pkt_off, pkt_len, index, skipped)


def gather_uniform(templates: np.ndarray, tid: np.ndarray, netifs: np.ndarray, n_netifs: int, region_bytes: int,
                   index_cap: int) -> Want:
    """Forward mode for n frames of one sendable length: frame i is templates[tid[i]] (uint8 [k,
    length]) and goes to NetIf netifs[i] (int, -1 for none)."""
    length = templates.shape[1]
    assert 34 <= length <= 1514
    plen = length - 14
    size = (plen + 3) & ~3
    streams, pkt_off, pkt_len, index = [], [], [], []
    ports = np.zeros(n_netifs, PORT_DTYPE)
    for p in range(n_netifs):
        sel = np.flatnonzero(netifs == p)
        written = min(len(sel), region_bytes // size)
        s = np.zeros((written, size), np.uint8)
        s[:, :plen] = templates[tid[sel[:written]], 14:]
        streams.append(s.reshape(-1))
        k = min(len(sel), index_cap)
        off = np.arange(k, dtype=np.uint64) * (size // 4)
        off[written:] = NOT_WRITTEN
        pkt_off.append(off.astype(np.uint32))
        pkt_len.append(np.full(k, plen, np.uint16))
        index.append(sel[:k].astype(np.uint32))
        ports[p] = (len(sel), written, len(sel) * size, written * size)
    return Want(n_netifs, region_bytes, index_cap, streams, ports, pkt_off, pkt_len, index, 0)


# ---- the drain (engine/engine.go:353-381) -----------------------------------------------------------
class Drain:
    """What the drain of one NetIf's packets does: `actions` per packet (oracle/ref_py.ACTIONS names),
    `replies` = [(packet index, reply dict)] in order, `frames` = the built reply frames after
    TxIpv4's L2 step with their (verdict, out_netif), `deliveries` = tests/deliver_model.Want."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def drain(packets, offsets_dw, data: np.ndarray, arp: AM.Model, self_netif: int, route_of, ip_id: int, *, tcp_ports=(),
          udp_ports=(), check_sum_enable: bool = True) -> Drain:
    """`packets`: the NetIf's LoChan packets in channel order, lying in `data` at offsets_dw (for the
    replies' payload offsets). `route_of(dst_ip)` is FindRoute as arp_model.Model.encap takes it."""
    me = arp.netifs[self_netif]
    nif = RM.NetIf(me.mac, me.ip, me.nat_enable)
    want = RM.respond([bytes(p) for p in packets], offsets_dw, nif, l3=True, tcp_ports=tuple(tcp_ports),
                      check_sum_enable=check_sum_enable)
    built, ip_end = RM.build_frames(want.replies, data, me.mac, ip_id, check_sum_enable)
    frames = []
    for (res, f), (_i, r) in zip(built, want.replies):
        assert res == 0
        v, out, tx, target, after = RM.tx_ipv4(arp, bytes(f), route_of(int(r["dst_ip"])), self_netif)
        frames.append((v, out, tx, target, after))
    deliveries = DM.want_of([bytes(p) for p in packets], DM.NetIf(me.mac, me.ip, me.nat_enable), l3=True,
                            udp_ports=tuple(udp_ports), tcp_ports=tuple(tcp_ports), check_sum_enable=check_sum_enable)
    return Drain(actions=[R.ACTIONS[a] for a in want.actions], replies=want.replies, frames=frames, ip_id=ip_end,
                 deliveries=deliveries)
