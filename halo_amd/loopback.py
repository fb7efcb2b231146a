"""The loopback step (include/halo_rx.h, "loopback"): the producer side of a NetIf's ``LoChan``.

``Ipv4RouteForward`` copies a packet addressed to the out NetIf's own address into that NetIf's
``LoChan`` and returns before the SNAT step (engine/ipv4_engine.go:193-201); ``TxIpv4`` does the same
for a locally built packet (:71-80); ``PacketHandle`` drains the channel through the L3 parse and the
local ``Rx{Icmp,Udp,Tcp}`` (engine/engine.go:353-381).

* ``mark`` — the encap's ``LOOPBACK`` test alone, from records, ahead of the NAT lookup: the ``skip``
  of ``NatTable.lookup_lan``, so a LoChan packet keeps its source and no flow is added for it.
  ``forward_return_flows(loopback=True)`` runs it.
* ``gather`` — over cuda tensors after the encap, asynchronous on the stream (three launches): one L3
  batch per out NetIf, in frame order. ``tx=True`` after ``ArpTable.encap_tx``.
* ``gather_host`` — the sequential loop over numpy arrays, for polls at the reference's cadence.
* ``drain`` — one NetIf's batch through L3 parse -> respond -> build -> FindRoute -> ``encap_tx``.

Both gathers return a ``LoResult``: ``.ports`` (EGRESS_PORT_DTYPE), ``.n_skipped``, ``.batch(p)``.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import EGRESS_PORT_DTYPE, HALO_LO_TX, HALO_RX_JUMBO_EXT, LO_NOT_WRITTEN  # noqa: F401
from .egress import EgressResult, _device_outputs


def packet_size(pkt_len: int) -> int:
    """A packet's bytes in its NetIf's region: the packet, then zeros to the next 4-byte boundary."""
    return (int(pkt_len) + 3) & ~3


class LoResult(EgressResult):
    """What one gather wrote: an ``EgressResult`` whose ports are the NetIfs (``out`` is uint8
    [n_netifs * region_bytes]), with ``pkt_off_dw_raw`` / ``pkt_len_raw`` beside ``index_raw``, the
    per-packet arrays ([n_netifs, index_cap])."""

    def __init__(self, n_netifs, region_bytes, index_cap, out, ports_raw, pkt_off_dw_raw, pkt_len_raw, index_raw, skipped):
        super().__init__(n_netifs, region_bytes, index_cap, out, ports_raw, index_raw, skipped)
        self.n_netifs, self.pkt_off_dw_raw, self.pkt_len_raw = n_netifs, pkt_off_dw_raw, pkt_len_raw

    def n_listed(self, p: int) -> int:
        """Entries of NetIf p in the per-packet arrays: min(frames, index_cap)."""
        return min(int(self.ports[p]["frames"]), self.index_cap)

    def n_parsable(self, p: int) -> int:
        """Packets of NetIf p that were written and are listed: min(frames_written, index_cap)."""
        return min(int(self.ports[p]["frames_written"]), self.index_cap)

    def batch(self, p: int):
        """(packets, offsets_dw, lens) of NetIf p's written packets, as ``parse_frames_batch(...,
        l3_start=True)`` takes them: views of the outputs, no copy."""
        k = self.n_parsable(p)
        lo = p * self.region_bytes
        return self.out[lo:lo + self.region_bytes], self.pkt_off_dw_raw[p, :k], self.pkt_len_raw[p, :k]

    def pkt_off_dw(self, p: int) -> np.ndarray:
        k = self.n_listed(p)
        return self._host(self.pkt_off_dw_raw[p, :k]).view(np.uint32).copy() if k else np.zeros(0, np.uint32)

    def pkt_len(self, p: int) -> np.ndarray:
        k = self.n_listed(p)
        return self._host(self.pkt_len_raw[p, :k]).view(np.uint16).copy() if k else np.zeros(0, np.uint16)


def _config(n_netifs, region_bytes, index_cap, tx, jumbo):
    cfg = _lib.LoConfig()
    cfg.n_netifs, cfg.flags = n_netifs, (HALO_LO_TX if tx else 0) | (HALO_RX_JUMBO_EXT if jumbo else 0)
    cfg.region_bytes, cfg.index_cap = region_bytes, index_cap
    return cfg


def workspace_bytes(n: int, n_netifs: int) -> int:
    return int(_lib.lib.halo_lo_gather_workspace(n, n_netifs))


def mark(arp, records, route_ids, in_netif: int, via=None, out=None, stream=None):
    """``halo_arp_loopback_mark_device`` over cuda tensors: ``records`` uint8 [n, 32], ``route_ids``
    int32 [n], optional ``via`` uint8 [n, 8] (``PortMappingFlowTable.lookup``'s). Returns uint8 [n]:
    1 where the encap of a batch NetIf ``in_netif`` received will say LOOPBACK. ``arp`` is an
    ``ArpTable`` synced with the routes."""
    import torch

    n = int(records.shape[0])
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=records.device)
    _lib.check("halo_arp_loopback_mark_device", _lib.lib.halo_arp_loopback_mark_device(
        arp._t, _lib.ptr(records), n, _lib.ptr(route_ids), in_netif, _lib.ptr(via), _lib.ptr(out), arp._stream(stream)))
    return out


def gather(data, offsets_dw, lens, results, n_netifs: int, region_bytes: int, index_cap: int, *, tx: bool = False,
           jumbo: bool = False, out=None, workspace=None, skipped=None, stream=None) -> LoResult:
    """Cuda tensors: uint8 bytes, int32 dword offsets, int16 lengths and the encap's ``results``
    (uint8 [n, 8]), after the encap on the same stream. ``out`` (uint8, n_netifs * region_bytes,
    16-byte aligned), ``workspace`` (``workspace_bytes``) and ``skipped`` (int32 [1], incremented) are
    allocated when not given."""
    import ctypes

    import torch

    n = int(lens.shape[0])
    dev = data.device
    cfg = _config(n_netifs, region_bytes, index_cap, tx, jumbo)
    out, ports, skipped, workspace, ws_bytes = _device_outputs(dev, n_netifs, region_bytes, workspace_bytes(n, n_netifs), out,
                                                               skipped, workspace)
    cap = max(index_cap, 1)
    pkt_off = torch.empty((n_netifs, cap), dtype=torch.int32, device=dev)
    pkt_len = torch.empty((n_netifs, cap), dtype=torch.int16, device=dev)
    index = torch.empty((n_netifs, cap), dtype=torch.int32, device=dev)
    st = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
    _lib.check("halo_lo_gather_device", _lib.lib.halo_lo_gather_device(
        ctypes.byref(cfg), _lib.ptr(data), _lib.ptr(offsets_dw), _lib.ptr(lens), n, _lib.ptr(results), _lib.ptr(out),
        _lib.ptr(ports), _lib.ptr(pkt_off), _lib.ptr(pkt_len), _lib.ptr(index), _lib.ptr(skipped), _lib.ptr(workspace),
        ws_bytes, st))
    return LoResult(n_netifs, region_bytes, index_cap, out, ports, pkt_off, pkt_len, index, skipped)


def gather_host(data: np.ndarray, offsets_dw: np.ndarray, lens: np.ndarray, results: np.ndarray, n_netifs: int,
                region_bytes: int, index_cap: int, *, tx: bool = False, jumbo: bool = False, out=None,
                skipped=None) -> LoResult:
    """``halo_lo_gather_host`` over numpy arrays: ``results`` is ARP_RESULT_DTYPE [n]."""
    import ctypes

    data = np.ascontiguousarray(data, np.uint8)
    offsets_dw = np.ascontiguousarray(offsets_dw, np.uint32)
    lens = np.ascontiguousarray(lens, np.uint16)
    results = np.ascontiguousarray(results)
    n = int(lens.shape[0])
    cfg = _config(n_netifs, region_bytes, index_cap, tx, jumbo)
    if out is None:
        out = np.zeros(max(n_netifs * region_bytes, 1), np.uint8)
    ports = np.zeros(n_netifs, EGRESS_PORT_DTYPE)
    cap = max(index_cap, 1)
    pkt_off = np.zeros((n_netifs, cap), np.uint32)
    pkt_len = np.zeros((n_netifs, cap), np.uint16)
    index = np.zeros((n_netifs, cap), np.uint32)
    if skipped is None:
        skipped = np.zeros(1, np.uint32)
    _lib.check("halo_lo_gather_host", _lib.lib.halo_lo_gather_host(
        ctypes.byref(cfg), _lib.ptr(data), _lib.ptr(offsets_dw), _lib.ptr(lens), n, _lib.ptr(results), _lib.ptr(out),
        _lib.ptr(ports), _lib.ptr(pkt_off), _lib.ptr(pkt_len), _lib.ptr(index), _lib.ptr(skipped)))
    return LoResult(n_netifs, region_bytes, index_cap, out, ports, pkt_off, pkt_len, index, skipped)


class Drained:
    """``drain``'s result: ``records`` (the L3 records of the NetIf's packets, uint8 [k, 32]), the
    batch they describe (``packets``, ``offsets_dw``, ``lens`` — what ``deliver(..., l3_start=True)``
    takes with ``records``) and ``replies``, what ``build_replies`` returns."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def drain(lo: LoResult, p: int, *, netif, self_netif: int, builder, routes, arp, tcp_ports=None, cap: int | None = None,
          out_stride: int = 128, check_sum_enable: bool = True, stream=None) -> Drained:
    """``PacketHandle``'s LoChan drain for NetIf ``p`` of a device ``LoResult`` (engine/engine.go:353-381):
    L3 parse -> ``respond`` with ``l3_start`` -> ``builder.build`` -> ``routes.FindRoute`` ->
    ``arp.encap_tx``. ``netif`` is NetIf p's ``_lib.NetIf``, ``self_netif`` its index for the
    replies it originates. Reads ``lo.ports`` (synchronises) to learn the packet count."""
    from . import protocol
    from .respond import build_replies

    packets, offsets_dw, lens = lo.batch(p)
    records = protocol.parse_frames_batch(packets, offsets_dw, lens, netif=netif, check_sum_enable=check_sum_enable,
                                          l3_start=True, stream=stream)
    replies = build_replies(packets, offsets_dw, lens, records, netif=netif, self_netif=self_netif, builder=builder,
                            routes=routes, arp=arp, tcp_ports=tcp_ports, cap=cap, out_stride=out_stride,
                            check_sum_enable=check_sum_enable, stream=stream, l3_start=True)
    return Drained(records=records, packets=packets, offsets_dw=offsets_dw, lens=lens, replies=replies)
