"""Local delivery (include/halo_rx.h, "local delivery"): what ``RxUdp`` / ``RxTcp`` hand to the
registered service handlers, and ``RxUdpBroadcast`` to ``RxDhcp``, for a parsed batch at once — one
stream of delivery records (24-byte header, payload, zero padding) in frame order, so that a batch
left in HBM reaches its handlers without being downloaded.

* ``deliver`` — over cuda tensors, asynchronous on the stream (three launches, no host round trip).
* ``deliver_host`` — the sequential loop over numpy arrays, for polls at the reference's cadence.
* ``port_map`` — the served-port bitmap (``UdpServiceMap``'s / ``TcpServiceMap``'s keys) both take.

Both return a ``DeliverResult``: ``.summary``, ``.index``, ``.stream()`` / ``.device_stream()``,
``.records()`` and ``.dispatch(netif)``, which calls the handlers as ``NetIf._deliver`` does.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import (DELIVER_HDR_DTYPE, DELIVER_INDEX_DTYPE, DELIVER_KIND, DELIVER_KIND_COUNT,  # noqa: F401
                   DELIVER_KIND_NAMES, DELIVER_NOT_WRITTEN, DELIVER_SUMMARY_DTYPE, HALO_DELIVER_DHCP, HALO_RX_L3_START)
from .respond import tcp_port_map

HDR_BYTES = DELIVER_HDR_DTYPE.itemsize


def port_map(ports) -> np.ndarray:
    """The 65,536-bit map of served ports as uint32 [2048]: bit ``p & 31`` of word ``p >> 5``
    (``respond.tcp_port_map``'s)."""
    return tcp_port_map(ports)


def record_size(payload_len: int) -> int:
    return HDR_BYTES + ((int(payload_len) + 3) & ~3)


class DeliverResult:
    """What one delivery call wrote. ``out`` is the whole output buffer (uint8 [region_bytes]),
    ``summary_raw`` the 40 summary bytes and ``index_raw`` the index ([index_cap, 8] bytes, or
    None); device results hold cuda tensors and copy on access (which synchronises)."""

    def __init__(self, region_bytes, index_cap, out, summary_raw, index_raw):
        self.region_bytes, self.index_cap = region_bytes, index_cap
        self.out, self.summary_raw, self.index_raw = out, summary_raw, index_raw
        self._summary = None

    @staticmethod
    def _host(x) -> np.ndarray:
        return x.cpu().numpy() if hasattr(x, "cpu") else x

    @property
    def summary(self) -> np.void:
        """The summary as one DELIVER_SUMMARY_DTYPE record (synchronises a device result)."""
        if self._summary is None:
            raw = self._host(self.summary_raw).reshape(-1).view(np.uint8)[:DELIVER_SUMMARY_DTYPE.itemsize]
            self._summary = raw.view(DELIVER_SUMMARY_DTYPE).copy()[0]
        return self._summary

    @property
    def bytes_written(self) -> int:
        return int(self.summary["bytes_written"])

    @property
    def index(self) -> np.ndarray:
        """{frame, offset} of the first min(records, index_cap) records as DELIVER_INDEX_DTYPE."""
        k = min(int(self.summary["records"]), self.index_cap)
        if k == 0 or self.index_raw is None:
            return np.zeros(0, DELIVER_INDEX_DTYPE)
        return self._host(self.index_raw[:k]).reshape(-1).view(np.uint8).view(DELIVER_INDEX_DTYPE).copy()

    def stream(self) -> np.ndarray:
        """The written records: uint8 [bytes_written], host memory."""
        return np.ascontiguousarray(self._host(self.out[:self.bytes_written])).view(np.uint8)

    def device_stream(self):
        """The same as a view of ``out`` (a cuda tensor for a device result)."""
        return self.out[:self.bytes_written]

    def records(self):
        """(header, payload) of every written record in stream order: header is one
        DELIVER_HDR_DTYPE record, payload ``bytes``."""
        s = self.stream()
        at, raw = 0, s.tobytes()
        while at < len(raw):
            h = np.frombuffer(raw, DELIVER_HDR_DTYPE, 1, at)[0]
            n = int(h["payload_len"])
            yield h, raw[at + HDR_BYTES:at + HDR_BYTES + n]
            at += record_size(n)

    def dispatch(self, netif, dhcp=None) -> int:
        """Calls the service handlers of ``netif`` (an ``engine.NetIf``) for the written records, in
        stream order and with the arguments ``NetIf._deliver`` gives them: ``UdpServiceMap[
        local_port](UdpSession(remote_ip, remote_port), payload)`` and ``TcpServiceMap[local_port](
        TcpSession(remote_ip, remote_port), payload, seq, ack, flags)``. A DHCP record goes to
        ``dhcp(payload, remote_port, local_port, remote_ip)`` (``RxDhcp``'s arguments) when given.
        Returns the number of handler calls."""
        from .engine import TcpSession, UdpSession

        calls = 0
        for h, payload in self.records():
            kind, port = int(h["kind"]), int(h["local_port"])
            if kind == DELIVER_KIND["UDP"]:
                fn = netif.UdpServiceMap.get(port)
                if fn is not None:
                    fn(UdpSession(int(h["remote_ip"]), int(h["remote_port"])), payload)
                    calls += 1
            elif kind == DELIVER_KIND["TCP"]:
                fn = netif.TcpServiceMap.get(port)
                if fn is not None:
                    fn(TcpSession(int(h["remote_ip"]), int(h["remote_port"])), payload, int(h["seq"]), int(h["ack"]),
                       int(h["tcp_flags"]))
                    calls += 1
            elif dhcp is not None:
                dhcp(payload, int(h["remote_port"]), port, int(h["remote_ip"]))
                calls += 1
        return calls


def _config(region_bytes, index_cap, l3_start, dhcp):
    cfg = _lib.DeliverConfig()
    cfg.flags = (HALO_RX_L3_START if l3_start else 0) | (HALO_DELIVER_DHCP if dhcp else 0)
    cfg.index_cap, cfg.region_bytes = index_cap, region_bytes
    return cfg


def workspace_bytes(n: int) -> int:
    return int(_lib.lib.halo_rx_deliver_workspace(n))


def deliver(data, offsets_dw, lens, records, *, netif, region_bytes: int, udp_ports=None, tcp_ports=None,
            index_cap: int = 0, l3_start: bool = False, dhcp: bool = False, out=None, summary=None, index=None,
            workspace=None, stream=None) -> DeliverResult:
    """The delivery records of a parsed batch over cuda tensors: ``data`` uint8, ``offsets_dw`` int32
    [n], ``lens`` int16 [n], ``records`` uint8 [n, 32]; optional ``udp_ports`` / ``tcp_ports`` int32
    [2048] (``port_map`` uploaded). ``netif`` is the receiving ``_lib.NetIf``. ``out`` (uint8,
    ``region_bytes``, a multiple of 16), ``summary`` (40 bytes), ``index`` ([index_cap, 8] bytes) and
    ``workspace`` (int64, at least ``workspace_bytes(n)``; may be shared by calls on one stream) are
    allocated when not given."""
    import torch

    n = int(lens.shape[0])
    dev = data.device
    cfg = _config(region_bytes, index_cap, l3_start, dhcp)
    if out is None:
        out = torch.empty(max(region_bytes, 16), dtype=torch.uint8, device=dev)
    if summary is None:
        summary = torch.empty(DELIVER_SUMMARY_DTYPE.itemsize // 8, dtype=torch.int64, device=dev)
    if index is None and index_cap:
        index = torch.empty((index_cap, 2), dtype=torch.int32, device=dev)
    if workspace is None:
        workspace = torch.empty(max(workspace_bytes(n), 8) // 8, dtype=torch.int64, device=dev)
    st = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
    _lib.check("halo_rx_deliver_device", _lib.lib.halo_rx_deliver_device(
        ctypes.byref(cfg), _lib.ptr(data), _lib.ptr(offsets_dw), _lib.ptr(lens), _lib.ptr(records), n, netif,
        _lib.ptr(udp_ports), _lib.ptr(tcp_ports), _lib.ptr(out), _lib.ptr(summary), _lib.ptr(index), _lib.ptr(workspace),
        workspace.numel() * workspace.element_size(), st))
    return DeliverResult(region_bytes, index_cap, out, summary, index)


def deliver_host(data, offsets_dw, lens, records, *, netif, region_bytes: int, udp_ports=None, tcp_ports=None,
                 index_cap: int = 0, l3_start: bool = False, dhcp: bool = False, out=None) -> DeliverResult:
    """The same from the sequential loop over numpy arrays (``halo_rx_deliver_host``): ``records`` is
    RESULT_DTYPE [n] (or uint8 [n, 32]); ``region_bytes`` may be any value."""
    data = np.ascontiguousarray(data, np.uint8)
    offsets_dw = np.ascontiguousarray(offsets_dw).view(np.uint32)
    lens = np.ascontiguousarray(lens).view(np.uint16)
    records = np.ascontiguousarray(records)
    maps = [None if m is None else np.ascontiguousarray(m).view(np.uint32) for m in (udp_ports, tcp_ports)]
    n = int(lens.shape[0])
    cfg = _config(region_bytes, index_cap, l3_start, dhcp)
    if out is None:
        out = np.zeros(max(region_bytes, 1), np.uint8)
    summary = np.zeros(DELIVER_SUMMARY_DTYPE.itemsize, np.uint8)
    index = np.zeros((index_cap, 8), np.uint8) if index_cap else None
    _lib.check("halo_rx_deliver_host", _lib.lib.halo_rx_deliver_host(
        ctypes.byref(cfg), _lib.ptr(data), _lib.ptr(offsets_dw), _lib.ptr(lens), _lib.ptr(records), n, netif,
        _lib.ptr(maps[0]), _lib.ptr(maps[1]), _lib.ptr(out), _lib.ptr(summary), _lib.ptr(index)))
    return DeliverResult(region_bytes, index_cap, out, summary, index)
