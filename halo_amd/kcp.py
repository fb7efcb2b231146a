"""KCP ingest (include/halo_rx.h, "KCP ingest"): the stateless part of the reference's KCP receive
path — ``Listener.packetInput``'s ENet / KCP split and ``KCP.Input``'s segment walk with its
length, cmd and byte checks — over the UDP payloads of one served port in a delivery stream
(``halo_amd.deliver``), so that a host runs ``Input``'s state machine from 32-byte segment
descriptors and touches payload bytes only to hand them on.

* ``ingest`` — over a device ``DeliverResult``, asynchronous on the stream, no host round trip.
* ``ingest_host`` — the sequential loop over a host ``DeliverResult`` (picked by name).

Both return a ``KcpIngestResult``: ``.summary``, ``.dgrams``, ``.segs``, ``.segments_of(j)`` and
``.feed(on_kcp, on_enet)``.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import (KCP_CHECK_MODES, KCP_DGRAM_DTYPE, KCP_DGRAM_ENET, KCP_DGRAM_KCP, KCP_ENET_NAMES,  # noqa: F401
                   KCP_SEG_CHECK_FAILED, KCP_SEG_CHECK_NA, KCP_SEG_CHECK_PASSED, KCP_SEG_DTYPE, KCP_SUMMARY_DTYPE)


def overhead(byte_check_mode: int) -> int:
    """IKCP_OVERHEAD: 28 with the byte check disabled, else 32."""
    return 28 if byte_check_mode == -1 else 32


def _mode(byte_check_mode) -> int:
    return KCP_CHECK_MODES[byte_check_mode] if isinstance(byte_check_mode, str) else int(byte_check_mode)


class KcpIngestResult:
    """What one ingest call wrote. ``dgrams_raw`` ([dgram_cap, 40] bytes), ``segs_raw`` ([seg_cap,
    32] bytes) and ``summary_raw`` (96 bytes) are cuda tensors for a device result and copied on
    access (which synchronises); ``delivery`` is the ``DeliverResult`` the call read."""

    def __init__(self, delivery, dgrams_raw, segs_raw, summary_raw, workspace=None):
        self.delivery = delivery
        self.workspace = workspace  # held while the call may still run: its memory must not be handed out again
        self.dgrams_raw, self.segs_raw, self.summary_raw = dgrams_raw, segs_raw, summary_raw
        self._summary = self._dgrams = self._segs = self._stream = None

    @staticmethod
    def _host(x) -> np.ndarray:
        return x.cpu().numpy() if hasattr(x, "cpu") else x

    @property
    def summary(self) -> np.void:
        """The summary as one KCP_SUMMARY_DTYPE record."""
        if self._summary is None:
            raw = self._host(self.summary_raw).reshape(-1).view(np.uint8)[:KCP_SUMMARY_DTYPE.itemsize]
            self._summary = raw.view(KCP_SUMMARY_DTYPE).copy()[0]
        return self._summary

    def _prefix(self, raw, count, dtype):
        if count == 0 or raw is None:
            return np.zeros(0, dtype)
        return self._host(raw[:count]).reshape(-1).view(np.uint8).view(dtype).copy()

    @property
    def dgrams(self) -> np.ndarray:
        """The written datagram records as KCP_DGRAM_DTYPE [dgrams_written]."""
        if self._dgrams is None:
            self._dgrams = self._prefix(self.dgrams_raw, int(self.summary["dgrams_written"]), KCP_DGRAM_DTYPE)
        return self._dgrams

    @property
    def segs(self) -> np.ndarray:
        """The written segment descriptors as KCP_SEG_DTYPE [segs_written]."""
        if self._segs is None:
            self._segs = self._prefix(self.segs_raw, int(self.summary["segs_written"]), KCP_SEG_DTYPE)
        return self._segs

    def segments_of(self, j: int) -> np.ndarray:
        """The processed segments' descriptors of written datagram ``j``: [first_seg, first_seg + n_segs)."""
        d = self.dgrams[j]
        return self.segs[int(d["first_seg"]):int(d["first_seg"]) + int(d["n_segs"])]

    def feed(self, on_kcp=None, on_enet=None) -> int:
        """Calls back per written datagram, in stream order: ``on_kcp(dgram, segs, payloads)`` with the
        datagram's record, its processed segments' descriptors and their data as ``bytes``;
        ``on_enet(dgram)`` for an ENet control packet. Returns the number of calls."""
        if self._stream is None:
            self._stream = self.delivery.stream().tobytes()
        calls = 0
        for j, d in enumerate(self.dgrams):
            if int(d["kind"]) == KCP_DGRAM_ENET:
                if on_enet is not None:
                    on_enet(d)
                    calls += 1
            elif on_kcp is not None:
                segs = self.segments_of(j)
                on_kcp(d, segs, [self._stream[int(s["data_off"]):int(s["data_off"]) + int(s["len"])] for s in segs])
                calls += 1
        return calls


def _config(port, byte_check_mode, dgram_cap, seg_cap):
    cfg = _lib.KcpConfig()
    cfg.byte_check_mode, cfg.port, cfg.dgram_cap, cfg.seg_cap = _mode(byte_check_mode), port, dgram_cap, seg_cap
    return cfg


def workspace_bytes(index_cap: int, seg_cap: int) -> int:
    return int(_lib.lib.halo_kcp_ingest_workspace(index_cap, seg_cap))


def ingest(deliver_result, *, port: int, byte_check_mode=-1, seg_cap: int, dgram_cap: int, dgrams=None, segs=None,
           summary=None, workspace=None, stream=None) -> KcpIngestResult:
    """KCP ingest of a device ``DeliverResult`` (made with an index). ``byte_check_mode`` is -1 / 0 /
    1 / 2 or "disabled" / "zero" / "crc32" / "xxh3". ``dgrams`` ([dgram_cap, 5] int64), ``segs``
    ([seg_cap, 4] int64 16-byte aligned), ``summary`` (12 int64) and ``workspace`` (int64, at least
    ``workspace_bytes(index_cap, seg_cap)``; may be shared by calls on one stream) are allocated
    when not given; the result holds the workspace, and with ``stream`` given every tensor is
    recorded on it. A delivery without an index is a ValueError."""
    import torch

    r = deliver_result
    if r.index_raw is None or r.index_cap == 0:
        raise ValueError("kcp.ingest needs a delivery made with an index (index_cap > 0)")
    dev = r.out.device
    cfg = _config(port, byte_check_mode, dgram_cap, seg_cap)
    if dgrams is None:
        dgrams = torch.empty((max(dgram_cap, 1), 5), dtype=torch.int64, device=dev)
    if segs is None:
        segs = torch.empty((max(seg_cap, 1), 4), dtype=torch.int64, device=dev)
    if summary is None:
        summary = torch.empty(KCP_SUMMARY_DTYPE.itemsize // 8, dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = torch.empty(max(workspace_bytes(r.index_cap, seg_cap), 8) // 8, dtype=torch.int64, device=dev)
    st = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
    _lib.check("halo_kcp_ingest_device", _lib.lib.halo_kcp_ingest_device(
        ctypes.byref(cfg), _lib.ptr(r.out), _lib.ptr(r.summary_raw), _lib.ptr(r.index_raw), r.index_cap,
        _lib.ptr(dgrams), _lib.ptr(segs), _lib.ptr(summary), _lib.ptr(workspace), workspace.numel() * workspace.element_size(), st))
    if stream is not None:  # allocated under the current stream, used on this one
        for t in (dgrams, segs, summary, workspace):
            t.record_stream(stream)
    return KcpIngestResult(r, dgrams, segs, summary, workspace)


def ingest_host(deliver_result, *, port: int, byte_check_mode=-1, seg_cap: int, dgram_cap: int) -> KcpIngestResult:
    """The same from the sequential loop (``halo_kcp_ingest_host``) over a host ``DeliverResult``
    (``deliver_host``'s, or a device result's arrays downloaded by the caller)."""
    r = deliver_result
    if r.index_raw is None or r.index_cap == 0:
        raise ValueError("kcp.ingest_host needs a delivery made with an index (index_cap > 0)")
    out = np.ascontiguousarray(KcpIngestResult._host(r.out)).view(np.uint8)
    dsum = np.ascontiguousarray(KcpIngestResult._host(r.summary_raw)).reshape(-1).view(np.uint8)
    index = np.ascontiguousarray(KcpIngestResult._host(r.index_raw)).reshape(-1).view(np.uint8)
    cfg = _config(port, byte_check_mode, dgram_cap, seg_cap)
    dgrams = np.zeros((max(dgram_cap, 1), KCP_DGRAM_DTYPE.itemsize), np.uint8)
    segs = np.zeros((max(seg_cap, 1), KCP_SEG_DTYPE.itemsize), np.uint8)
    summary = np.zeros(KCP_SUMMARY_DTYPE.itemsize, np.uint8)
    _lib.check("halo_kcp_ingest_host", _lib.lib.halo_kcp_ingest_host(
        ctypes.byref(cfg), _lib.ptr(out), _lib.ptr(dsum), _lib.ptr(index), r.index_cap,
        _lib.ptr(dgrams), _lib.ptr(segs), _lib.ptr(summary)))
    host = r if not hasattr(r.out, "cpu") else type(r)(r.region_bytes, r.index_cap, out, dsum, index.reshape(-1, 8))
    return KcpIngestResult(host, dgrams, segs, summary)
