"""The local responders (include/halo_rx.h, "local responders"): the echo reply of ``RxIcmp``, the
time-exceeded message of ``Ipv4RouteForward`` and the handshake answers of ``RxTcp`` for a parsed
batch at once, as reply descriptors in frame order, and ``TxIpv4``'s route / ARP step for the
frames built from them.

* ``respond`` — over cuda tensors, asynchronous on the stream (three launches).
* ``respond_host`` — the sequential loop over numpy arrays, for polls at the reference's cadence.
* ``tcp_port_map`` — the served-port bitmap (``TcpServiceMap``'s keys) both take.
* ``ArpTable.encap_tx`` — ``TxIpv4``'s broadcast / FindRoute / loopback / GetArpCache decision and
  the Ethernet header, on built frames (defined here, bound to ``ArpTable``).
* ``build_replies`` — respond -> ``TxBuilder.build`` (payload = the rx batch) -> ``FindRoute`` ->
  ``encap_tx``, with fixed-stride slots; ``egress_arp`` takes its result as it stands.

Both responders return a ``RespondResult``: ``.count``, ``.desc``, ``.src``, ``.dst_ip``, ``.actions``.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import (ARP_V_COUNT, BUILD_DESC_DTYPE, HALO_RX_L3_START, RESPOND_KIND, RESPOND_KIND_COUNT,  # noqa: F401
                   RESPOND_KIND_NAMES, RESPOND_SRC_DTYPE)
from .arp import ArpTable


def tcp_port_map(ports) -> np.ndarray:
    """The 65,536-bit map of served TCP ports as uint32 [2048]: bit ``p & 31`` of word ``p >> 5``."""
    m = np.zeros(2048, np.uint32)
    for p in ports:
        p = int(p)
        assert 0 <= p <= 0xFFFF, p
        m[p >> 5] |= np.uint32(1 << (p & 31))
    return m


class RespondResult:
    """What one responder call wrote. ``desc_raw`` (uint8 [cap, 40]), ``src_raw`` (uint8 [cap, 8]),
    ``dst_ip_raw`` (int32 / uint32 [cap]), ``count_raw`` ([1]), ``kind_counts_raw`` ([4]) and
    ``actions_raw`` (uint8 [n]) are the buffers themselves; device results hold cuda tensors and the
    properties copy on access (which synchronises)."""

    def __init__(self, cap, desc_raw, src_raw, dst_ip_raw, count_raw, kind_counts_raw, actions_raw):
        self.cap = cap
        self.desc_raw, self.src_raw, self.dst_ip_raw = desc_raw, src_raw, dst_ip_raw
        self.count_raw, self.kind_counts_raw, self.actions_raw = count_raw, kind_counts_raw, actions_raw

    @staticmethod
    def _host(x) -> np.ndarray:
        return x.cpu().numpy() if hasattr(x, "cpu") else x

    @property
    def count(self) -> int:
        """The number of replies, also beyond ``cap``."""
        return int(self._host(self.count_raw).reshape(-1).view(np.uint32)[0])

    @property
    def written(self) -> int:
        return min(self.count, self.cap)

    @property
    def desc(self) -> np.ndarray:
        """The written descriptors as BUILD_DESC_DTYPE."""
        return self._host(self.desc_raw).reshape(-1).view(np.uint8).view(BUILD_DESC_DTYPE)[:self.written].copy()

    @property
    def src(self) -> np.ndarray:
        """{index, kind} of the written replies as RESPOND_SRC_DTYPE."""
        return self._host(self.src_raw).reshape(-1).view(np.uint8).view(RESPOND_SRC_DTYPE)[:self.written].copy()

    @property
    def dst_ip(self) -> np.ndarray:
        return self._host(self.dst_ip_raw).reshape(-1).view(np.uint32)[:self.written].copy()

    @property
    def kind_counts(self) -> np.ndarray:
        return self._host(self.kind_counts_raw).reshape(-1).view(np.uint32).copy()

    @property
    def actions(self) -> np.ndarray:
        return self._host(self.actions_raw).reshape(-1).view(np.uint8).copy()


def _flags(l3_start: bool) -> int:
    return HALO_RX_L3_START if l3_start else 0


def respond(offsets_dw, lens, records, *, netif, nat_verdict=None, ops=None, fixup_result=None, tcp_ports=None,
            cap: int | None = None, l3_start: bool = False, kind_counts=None, workspace=None, stream=None) -> RespondResult:
    """The reply descriptors of a parsed batch over cuda tensors: ``offsets_dw`` int32 [n], ``lens``
    int16 [n], ``records`` uint8 [n, 32]; optional ``nat_verdict`` uint8 [n], ``ops`` uint8 [n, 16]
    with ``fixup_result`` uint8 [n], ``tcp_ports`` int32 [2048] (``tcp_port_map`` uploaded).
    ``kind_counts`` (int32 [4]) is incremented; ``workspace`` (int32, at least
    ``halo_tx_respond_workspace(n)`` bytes) may be shared by calls on one stream."""
    import torch

    n = int(lens.shape[0])
    cap = n if cap is None else cap
    dev = records.device
    desc = torch.zeros((max(cap, 1), 40), dtype=torch.uint8, device=dev)
    src = torch.zeros((max(cap, 1), 8), dtype=torch.uint8, device=dev)
    dst_ip = torch.zeros(max(cap, 1), dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    actions = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
    if kind_counts is None:
        kind_counts = torch.zeros(RESPOND_KIND_COUNT, dtype=torch.int32, device=dev)
    wsb = int(_lib.lib.halo_tx_respond_workspace(n))
    if workspace is None:
        workspace = torch.empty(wsb // 4, dtype=torch.int32, device=dev)
    s = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
    _lib.check("halo_tx_respond_device", _lib.lib.halo_tx_respond_device(
        _lib.ptr(offsets_dw), _lib.ptr(lens), _lib.ptr(records), n, _flags(l3_start), netif, _lib.ptr(nat_verdict),
        _lib.ptr(ops), _lib.ptr(fixup_result), _lib.ptr(tcp_ports), _lib.ptr(desc), _lib.ptr(src), _lib.ptr(dst_ip), cap,
        _lib.ptr(count), _lib.ptr(kind_counts), _lib.ptr(actions), _lib.ptr(workspace),
        workspace.numel() * workspace.element_size(), s))
    return RespondResult(cap, desc, src, dst_ip, count, kind_counts, actions[:n])


def respond_host(offsets_dw, lens, records, *, netif, nat_verdict=None, ops=None, fixup_result=None, tcp_ports=None,
                 cap: int | None = None, l3_start: bool = False, kind_counts=None) -> RespondResult:
    """The same from the sequential loop over numpy arrays (``halo_tx_respond_host``): ``records``
    is RESULT_DTYPE [n] (or uint8 [n, 32]), ``ops`` TX_OP_DTYPE [n]."""
    lens = np.ascontiguousarray(lens).view(np.uint16)
    offsets_dw = np.ascontiguousarray(offsets_dw).view(np.uint32)
    records = np.ascontiguousarray(records)
    n = int(lens.shape[0])
    cap = n if cap is None else cap
    opt = [None if x is None else np.ascontiguousarray(x) for x in (nat_verdict, ops, fixup_result, tcp_ports)]
    desc = np.zeros((max(cap, 1), 40), np.uint8)
    src = np.zeros((max(cap, 1), 8), np.uint8)
    dst_ip = np.zeros(max(cap, 1), np.uint32)
    count = np.zeros(1, np.uint32)
    actions = np.zeros(max(n, 1), np.uint8)
    if kind_counts is None:
        kind_counts = np.zeros(RESPOND_KIND_COUNT, np.uint32)
    _lib.check("halo_tx_respond_host", _lib.lib.halo_tx_respond_host(
        _lib.ptr(offsets_dw), _lib.ptr(lens), _lib.ptr(records), n, _flags(l3_start), netif, *[_lib.ptr(x) for x in opt],
        _lib.ptr(desc), _lib.ptr(src), _lib.ptr(dst_ip), cap, _lib.ptr(count), _lib.ptr(kind_counts), _lib.ptr(actions)))
    return RespondResult(cap, desc, src, dst_ip, count, kind_counts, actions[:n])


def _encap_tx(self, data, offsets_dw, lens, route_ids, self_netif: int, select=None, counts=None, miss_count=None,
              stream=None):
    """``TxIpv4``'s L3 / L2 step for frames NetIf ``self_netif`` originated (cuda tensors as
    ``encap``): a x.x.x.255 destination is a HIT to the broadcast MAC out of ``self_netif`` without
    a route; dst == the out NetIf's address is a LOOPBACK whatever ``nat_enable`` says; the rest is
    ``encap``'s. Returns (results uint8 [n, 8], counts int32 [7], miss_count int32 [1])."""
    import torch

    n = int(lens.shape[0])
    results = torch.empty((n, 8), dtype=torch.uint8, device=data.device)
    if counts is None:
        counts = torch.zeros(ARP_V_COUNT, dtype=torch.int32, device=data.device)
    if miss_count is None:
        miss_count = torch.zeros(1, dtype=torch.int32, device=data.device)
    _lib.check("halo_arp_encap_tx_device", _lib.lib.halo_arp_encap_tx_device(
        self._t, _lib.ptr(data), _lib.ptr(offsets_dw), _lib.ptr(lens), n, _lib.ptr(route_ids), self_netif,
        _lib.ptr(select), _lib.ptr(results), _lib.ptr(counts), _lib.ptr(miss_count), self._stream(stream)))
    return results, counts, miss_count


ArpTable.encap_tx = _encap_tx


class Replies:
    """``build_replies``' result: the responder's ``RespondResult`` (``.respond``), the built slots
    (``frames`` uint8 [cap, stride], ``lens`` int16 [cap], ``build_result`` uint8 [cap]), the
    ``offsets_dw`` int32 [cap] that address them as a ragged batch, ``route_ids`` and the encap's
    ``results`` / ``counts`` / ``miss_count`` — what ``egress_arp(frames, offsets_dw, lens, results,
    ...)`` takes."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def build_replies(data, offsets_dw, lens, records, *, netif, self_netif: int, builder, routes, arp, nat_verdict=None,
                  ops=None, fixup_result=None, tcp_ports=None, cap: int | None = None, out_stride: int = 128,
                  check_sum_enable: bool = True, stream=None, l3_start: bool = False) -> Replies:
    """respond -> ``builder.build`` with the rx batch ``data`` as payload -> ``routes.FindRoute`` of
    the replies' destinations -> ``arp.encap_tx``. Slot k of ``frames`` (``out_stride`` bytes, a
    multiple of 4) holds reply k; slots at and beyond the reply count are masked out (``select``), so
    the whole chain runs without a host round trip. Every reply is built (and takes its iphId)
    before the route and ARP verdicts drop any. ``builder`` is a ``TxBuilder`` for at least ``cap``
    frames, ``routes`` a synced ``RouteTable``, ``arp`` an ``ArpTable`` synced with it. ``l3_start``: the
    batch is a NetIf's LoChan packets (``loopback.drain``), every buffer starting at its IPv4 header."""
    import torch

    assert out_stride % 4 == 0 and out_stride >= 60
    n = int(lens.shape[0])
    cap = n if cap is None else cap
    r = respond(offsets_dw, lens, records, netif=netif, nat_verdict=nat_verdict, ops=ops, fixup_result=fixup_result,
                tcp_ports=tcp_ports, cap=cap, l3_start=l3_start, stream=stream)
    dev = data.device
    slots = max(cap, 1)
    # a slot at or beyond the count keeps the zeroed descriptor: proto 0 is HALO_TX_B_PROTO, not built, length 0
    frames, out_lens, build_result = builder.build(r.desc_raw, data, netif=netif, out_stride=out_stride,
                                                   check_sum_enable=check_sum_enable, stream=stream)
    route_ids = routes.FindRoute(r.dst_ip_raw, stream=stream)
    slot_offsets = torch.arange(slots, dtype=torch.int32, device=dev) * (out_stride // 4)
    select = (torch.arange(slots, dtype=torch.int32, device=dev) < r.count_raw).to(torch.uint8)
    results, counts, miss_count = arp.encap_tx(frames.reshape(-1), slot_offsets, out_lens, route_ids, self_netif,
                                               select=select, stream=stream)
    return Replies(respond=r, frames=frames, lens=out_lens, build_result=build_result, offsets_dw=slot_offsets,
                   route_ids=route_ids, select=select, results=results, counts=counts, miss_count=miss_count)
