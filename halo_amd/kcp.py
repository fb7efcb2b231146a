"""KCP ingest (include/halo_rx.h, "KCP ingest"): the stateless part of the reference's KCP receive
path — ``Listener.packetInput``'s ENet / KCP split and ``KCP.Input``'s segment walk with its
length, cmd and byte checks — over the UDP payloads of one served port in a delivery stream
(``halo_amd.deliver``), so that a host runs ``Input``'s state machine from 32-byte segment
descriptors and touches payload bytes only to hand them on.

* ``ingest`` — over a device ``DeliverResult``, asynchronous on the stream, no host round trip.
* ``ingest_host`` — the sequential loop over a host ``DeliverResult`` (picked by name).

Both return a ``KcpIngestResult``: ``.summary``, ``.dgrams``, ``.segs``, ``.segments_of(j)`` and
``.feed(on_kcp, on_enet)``.

KCP emit (include/halo_rx.h, "KCP emit") is the other direction: the stateless tail of
``KCP.flush`` — the packing of a session's send list into datagrams of at most ``mtu`` bytes,
``segment.encode`` with the byte check of every PUSH, the copy of the data — and ``BuildEnet``'s
control packets, over payload that lies in HBM, into the UDP payload stream and the descriptors
``halo_tx_build_batch_device`` takes.

* ``emit`` — device arrays in, asynchronous on the stream, no host round trip.
* ``emit_host`` — the sequential loop over host arrays (picked by name).
* ``sessions_of`` / ``relay_segments`` — the input records from plain values, and from an ingest
  result's descriptors.

Both return a ``KcpEmitResult``: ``.summary``, ``.status``, ``.dgrams()``, ``.descs()``,
``.datagrams()`` and ``.build(builder, netif=...)``.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import (BUILD_DESC_DTYPE, KCP_CHECK_MODES, KCP_DGRAM_DTYPE, KCP_DGRAM_ENET, KCP_DGRAM_KCP,  # noqa: F401
                   KCP_EMIT_STATUS, KCP_EMIT_STATUS_NAMES, KCP_EMIT_SUMMARY_DTYPE, KCP_ENET_NAMES, KCP_OUT_DGRAM_DTYPE,
                   KCP_OUT_SESSION_DTYPE, KCP_SEG_CHECK_FAILED, KCP_SEG_CHECK_NA, KCP_SEG_CHECK_PASSED, KCP_SEG_DTYPE,
                   KCP_SUMMARY_DTYPE)


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


# ---- KCP emit -----------------------------------------------------------------------------------
class KcpEmitResult:
    """What one emit call wrote. ``stream_raw`` ([stream_cap] bytes), ``dgrams_raw`` ([dgram_cap, 16]
    bytes), ``descs_raw`` ([dgram_cap, 40] bytes), ``status_raw`` ([n_sessions]) and ``summary_raw``
    (88 bytes) are cuda tensors for a device result and copied on access (which synchronises)."""

    def __init__(self, n_sessions, stream_raw, dgrams_raw, descs_raw, status_raw, summary_raw, workspace=None):
        self.n_sessions = n_sessions
        self.workspace = workspace  # held while the call may still run: its memory must not be handed out again
        self.stream_raw, self.dgrams_raw, self.descs_raw = stream_raw, dgrams_raw, descs_raw
        self.status_raw, self.summary_raw = status_raw, summary_raw
        self._summary = None

    _host = staticmethod(KcpIngestResult._host)

    @property
    def summary(self) -> np.void:
        """The summary as one KCP_EMIT_SUMMARY_DTYPE record."""
        if self._summary is None:
            raw = self._host(self.summary_raw).reshape(-1).view(np.uint8)[:KCP_EMIT_SUMMARY_DTYPE.itemsize]
            self._summary = raw.view(KCP_EMIT_SUMMARY_DTYPE).copy()[0]
        return self._summary

    @property
    def status(self) -> np.ndarray:
        """HALO_KCP_EMIT_* per entry, uint8 [n_sessions]."""
        return self._host(self.status_raw).reshape(-1).view(np.uint8)[:self.n_sessions].copy()

    @staticmethod
    def _bytes(raw, n) -> np.ndarray:
        """The first n bytes of a tensor or array of any element type, on the host."""
        if hasattr(raw, "cpu"):
            import torch

            return raw.reshape(-1).view(torch.uint8)[:n].cpu().numpy()
        return raw.reshape(-1).view(np.uint8)[:n].copy()

    def _prefix(self, raw, dtype):
        return self._bytes(raw, int(self.summary["dgrams_written"]) * dtype.itemsize).view(dtype)

    def dgrams(self) -> np.ndarray:
        """The written datagram records as KCP_OUT_DGRAM_DTYPE [dgrams_written]."""
        return self._prefix(self.dgrams_raw, KCP_OUT_DGRAM_DTYPE)

    def descs(self) -> np.ndarray:
        """The written build descriptors as BUILD_DESC_DTYPE [dgrams_written]."""
        return self._prefix(self.descs_raw, BUILD_DESC_DTYPE)

    def stream(self) -> np.ndarray:
        """The written stream bytes, uint8 [bytes_written]."""
        return self._bytes(self.stream_raw, int(self.summary["bytes_written"]))

    def datagrams(self) -> list:
        """The UDP payload of every written datagram, as ``bytes``."""
        s = self.stream().tobytes()
        return [s[int(d["offset"]):int(d["offset"]) + int(d["len"])] for d in self.dgrams()]

    def build(self, builder, *, netif, out_stride: int = 1536, n=None, **kw):
        """Hands the descriptors and the stream to ``builder.build`` (a ``protocol.TxBuilder``; a device
        result only): one frame per written datagram. ``n`` defaults to ``dgrams_written``, which is
        read from the device; give it (at most ``dgram_cap``) to stay asynchronous."""
        if not hasattr(self.descs_raw, "cpu"):
            raise ValueError("KcpEmitResult.build needs a device result")
        import torch

        n = int(self.summary["dgrams_written"]) if n is None else n
        desc = self.descs_raw.reshape(-1).view(torch.uint8)[:n * BUILD_DESC_DTYPE.itemsize]
        return builder.build(desc, self.stream_raw.reshape(-1).view(torch.uint8), netif=netif, out_stride=out_stride, **kw)


def sessions_of(entries) -> np.ndarray:
    """KCP_OUT_SESSION_DTYPE records from dicts: a KCP entry gives ``conv``, ``n_segs``, ``mtu``,
    ``dst_ip``, ``dst_port`` (``first_seg`` defaults to the running end of the entries before it); an
    ENet entry gives ``conn_type`` (0..3 or its name), ``session_id``, ``enet_conv``, ``enet_type``,
    ``dst_ip``, ``dst_port``."""
    out = np.zeros(len(entries), KCP_OUT_SESSION_DTYPE)
    end = 0
    for o, e in zip(out, entries):
        e = dict(e)
        if "conn_type" in e:
            t = e.pop("conn_type")
            o["kind"], o["conn_type"] = KCP_DGRAM_ENET, KCP_ENET_NAMES.index(t) if isinstance(t, str) else t
        o["first_seg"] = e.pop("first_seg", end)
        for k, v in e.items():
            o[k] = v
        end = int(o["first_seg"]) + int(o["n_segs"])
    return out


def relay_segments(ingest_result, datagrams=None):
    """An emit segment list from an ingest result: the processed segments' descriptors of the written
    KCP datagrams ``datagrams`` (default: all with ret == 0), concatenated. Their ``data_off`` is
    already the offset in the delivery stream, so the emit call's payload is the delivery's ``out``.
    Returns (segs KCP_SEG_DTYPE, [(datagram, first_seg, n_segs)])."""
    r = ingest_result
    if datagrams is None:
        datagrams = [j for j, d in enumerate(r.dgrams) if int(d["kind"]) == KCP_DGRAM_KCP and int(d["ret"]) == 0]
    parts, ranges, at = [], [], 0
    for j in datagrams:
        s = r.segments_of(j)
        parts.append(s)
        ranges.append((j, at, len(s)))
        at += len(s)
    segs = np.concatenate(parts) if parts else np.zeros(0, KCP_SEG_DTYPE)
    segs["dgram"], segs["check"] = 0, 0
    return segs, ranges


def _emit_config(byte_check_mode, src_ip, src_port, dgram_cap, stream_cap):
    cfg = _lib.KcpEmitConfig()
    cfg.byte_check_mode, cfg.src_ip, cfg.src_port = _mode(byte_check_mode), src_ip, src_port
    cfg.dgram_cap, cfg.stream_cap = dgram_cap, stream_cap
    return cfg


def emit_workspace_bytes(n_sessions: int, n_segs: int) -> int:
    return int(_lib.lib.halo_kcp_emit_workspace(n_sessions, n_segs))


def _nbytes(x) -> int:
    return x.numel() * x.element_size() if hasattr(x, "numel") else x.nbytes


def emit(sessions, segs, payload, *, byte_check_mode=-1, src_ip: int, src_port: int, dgram_cap: int, stream_cap: int,
         n_sessions=None, n_segs=None, payload_bytes=None, out=None, dgrams=None, descs=None, status=None, summary=None,
         workspace=None, stream=None) -> KcpEmitResult:
    """KCP emit over device arrays: ``sessions`` (KCP_OUT_SESSION_DTYPE records, 8-byte aligned),
    ``segs`` (KCP_SEG_DTYPE records, 16-byte aligned: an ingest result's ``segs_raw`` serves) and
    ``payload`` (bytes; 4-byte aligned) as cuda tensors of any element type; the counts default to what
    the tensors hold. ``out`` ([stream_cap] bytes), ``dgrams`` ([dgram_cap, 2] int64, 16-byte
    aligned), ``descs`` ([dgram_cap, 5] int64), ``status`` (uint8 [n_sessions]), ``summary`` (11
    int64) and ``workspace`` (int64, at least ``emit_workspace_bytes(n_sessions, n_segs)``; may be
    shared by calls on one stream) are allocated when not given."""
    import torch

    dev = sessions.device
    n_sessions = _nbytes(sessions) // KCP_OUT_SESSION_DTYPE.itemsize if n_sessions is None else n_sessions
    n_segs = _nbytes(segs) // KCP_SEG_DTYPE.itemsize if n_segs is None else n_segs
    payload_bytes = _nbytes(payload) if payload_bytes is None else payload_bytes
    cfg = _emit_config(byte_check_mode, src_ip, src_port, dgram_cap, stream_cap)
    if out is None:
        out = torch.empty((stream_cap + 7) // 8 or 1, dtype=torch.int64, device=dev)
    if dgrams is None:
        dgrams = torch.empty((max(dgram_cap, 1), 2), dtype=torch.int64, device=dev)
    if descs is None:
        descs = torch.empty((max(dgram_cap, 1), 5), dtype=torch.int64, device=dev)
    if status is None:
        status = torch.empty(max(n_sessions, 1), dtype=torch.uint8, device=dev)
    if summary is None:
        summary = torch.empty(KCP_EMIT_SUMMARY_DTYPE.itemsize // 8, dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = torch.empty(max(emit_workspace_bytes(n_sessions, n_segs), 8) // 8, dtype=torch.int64, device=dev)
    st = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
    _lib.check("halo_kcp_emit_device", _lib.lib.halo_kcp_emit_device(
        ctypes.byref(cfg), _lib.ptr(sessions), n_sessions, _lib.ptr(segs), n_segs, _lib.ptr(payload), payload_bytes, _lib.ptr(out),
        _lib.ptr(dgrams), _lib.ptr(descs), _lib.ptr(status), _lib.ptr(summary), _lib.ptr(workspace),
        workspace.numel() * workspace.element_size(), st))
    if stream is not None:  # allocated under the current stream, used on this one
        for t in (out, dgrams, descs, status, summary, workspace):
            t.record_stream(stream)
    return KcpEmitResult(n_sessions, out, dgrams, descs, status, summary, workspace)


def emit_host(sessions, segs, payload, *, byte_check_mode=-1, src_ip: int, src_port: int, dgram_cap: int,
              stream_cap: int) -> KcpEmitResult:
    """The same from the sequential loop (``halo_kcp_emit_host``) over numpy arrays."""
    sessions = np.ascontiguousarray(sessions).reshape(-1).view(np.uint8)
    segs = np.ascontiguousarray(segs).reshape(-1).view(np.uint8)
    payload = np.ascontiguousarray(payload).reshape(-1).view(np.uint8)
    n_sessions, n_segs = sessions.size // KCP_OUT_SESSION_DTYPE.itemsize, segs.size // KCP_SEG_DTYPE.itemsize
    cfg = _emit_config(byte_check_mode, src_ip, src_port, dgram_cap, stream_cap)
    out = np.zeros(max(stream_cap, 1), np.uint8)
    dgrams = np.zeros((max(dgram_cap, 1), KCP_OUT_DGRAM_DTYPE.itemsize), np.uint8)
    descs = np.zeros((max(dgram_cap, 1), BUILD_DESC_DTYPE.itemsize), np.uint8)
    status = np.zeros(max(n_sessions, 1), np.uint8)
    summary = np.zeros(KCP_EMIT_SUMMARY_DTYPE.itemsize, np.uint8)
    _lib.check("halo_kcp_emit_host", _lib.lib.halo_kcp_emit_host(
        ctypes.byref(cfg), _lib.ptr(sessions), n_sessions, _lib.ptr(segs), n_segs, _lib.ptr(payload), payload.size, _lib.ptr(out),
        _lib.ptr(dgrams), _lib.ptr(descs), _lib.ptr(status), _lib.ptr(summary)))
    return KcpEmitResult(n_sessions, out, dgrams, descs, status, summary)
