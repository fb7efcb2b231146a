"""The DHCP service (include/halo_rx.h, "DHCP"): ``engine/dhcp_engine.go`` for a batch at once.

* ``decode`` / ``decode_host`` — from the DHCP records of a delivery stream (``halo_amd.deliver``
  with ``dhcp=True`` and an index) to one 128-byte message record each: ``RxDhcp``'s port test,
  ``ParseDhcpPkt`` and ``ParseDhcpOption``. ``decode`` runs over a device ``DeliverResult``,
  asynchronous on the stream; ``decode_host`` is the sequential loop (picked by name). Both return
  a ``DhcpDecodeResult``: ``.summary``, ``.msgs`` and ``.feed(server, now)``.
* ``DhcpServer`` — the lease table and ``RxDhcp``'s state machine, one per NetIf: ``handle``,
  ``leases()`` (``ListDhcp``), ``clear`` (one ``DhcpLeaseClear`` tick), ``discover``
  (``DhcpDiscover``) and ``rx_dhcp(payload, sport, dport, src_ip)`` with ``RxDhcp``'s arguments, so
  that ``DeliverResult.dispatch(netif, dhcp=server.rx_dhcp)`` has a consumer.
* ``build_replies`` / ``build_replies_host`` — from reply descriptors to the UDP payloads
  ``BuildDhcpPkt`` makes (288-byte slots) and the descriptors ``halo_tx_build_batch_device`` takes.
  Both return a ``DhcpBuildResult``: ``.payloads()``, ``.descs()`` and ``.build(builder, netif=...)``.

Addresses are ints in ``IpAddrToU`` form (``a.b.c.d`` = ``a << 24 | b << 16 | c << 8 | d``).
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np

from . import _lib
from ._lib import (BUILD_DESC_DTYPE, DHCP_ACK, DHCP_DISCOVER, DHCP_EVENT_DTYPE, DHCP_H, DHCP_H_F_REPLY,  # noqa: F401
                   DHCP_H_F_REUSED, DHCP_H_MASK, DHCP_H_NAMES, DHCP_LEASE_DTYPE, DHCP_MSG_DTYPE, DHCP_NAK, DHCP_OFFER,
                   DHCP_RELEASE, DHCP_REPLY_DTYPE, DHCP_REQUEST, DHCP_SLOT_BYTES, DHCP_STATUS, DHCP_STATUS_NAMES,
                   DHCP_SUMMARY_DTYPE, DELIVER_KIND)

REPLY_LEN = {DHCP_OFFER: 286, DHCP_ACK: 286, DHCP_NAK: 250, DHCP_REQUEST: 270, DHCP_DISCOVER: 258}


def _host(x) -> np.ndarray:
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def _bytes(raw, n) -> np.ndarray:
    """The first n bytes of a tensor or array of any element type, on the host."""
    if hasattr(raw, "cpu"):
        import torch

        return raw.reshape(-1).view(torch.uint8)[:n].cpu().numpy()
    return raw.reshape(-1).view(np.uint8)[:n].copy()


def _nbytes(x) -> int:
    return x.numel() * x.element_size() if hasattr(x, "numel") else x.nbytes


# ---- the server object ----------------------------------------------------------------------------
class DhcpHandleResult:
    """What one ``DhcpServer.handle`` call gave: ``replies`` (DHCP_REPLY_DTYPE, in the order the
    reference would send them), ``verdicts`` (uint8 per message: a ``DHCP_H`` code | flag bits) and
    ``events`` (DHCP_EVENT_DTYPE, one per client ACK)."""

    def __init__(self, replies, verdicts, events):
        self.replies, self.verdicts, self.events = replies, verdicts, events

    def verdict_names(self) -> list:
        return [DHCP_H_NAMES[int(v) & DHCP_H_MASK] for v in self.verdicts]


class DhcpServer:
    """One NetIf's DHCP state: the lease table, the server and client switches and the client's
    transaction id. ``capacity`` is the most leases (the stand-in for the reference's allocator
    running out). ``time_now`` (``Router.TimeNow``) is what ``rx_dhcp`` stamps leases with."""

    def __init__(self, *, ip: int, network_mask: int, dns: int = 0, mac: bytes = bytes(6), server_enable: bool = True,
                 client_enable: bool = False, capacity: int = 1 << 16):
        cfg = _lib.DhcpConfig()
        cfg.ip, cfg.network_mask, cfg.dns, cfg.capacity = ip, network_mask, dns, capacity
        cfg.mac[:] = list(bytes(mac))
        cfg.server_enable, cfg.client_enable = int(bool(server_enable)), int(bool(client_enable))
        h = ctypes.c_void_p()
        _lib.check("halo_dhcp_server_create", _lib.lib.halo_dhcp_server_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        self.time_now = 0
        self.tx_queue: list = []  # rx_dhcp's replies (DHCP_REPLY_DTYPE records), for build_replies
        self.events: list = []    # rx_dhcp's client ACK events

    def close(self) -> None:
        if self._h:
            _lib.lib.halo_dhcp_server_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def config(self) -> _lib.DhcpConfig:
        """The current halo_dhcp_config_t (``set_dns`` changes it)."""
        cfg = _lib.DhcpConfig()
        _lib.check("halo_dhcp_server_config", _lib.lib.halo_dhcp_server_config(self._h, ctypes.byref(cfg)))
        return cfg

    def handle(self, msgs, now: int) -> DhcpHandleResult:
        """``RxDhcp`` for every message record (DHCP_MSG_DTYPE, or the raw bytes), in order."""
        msgs = np.ascontiguousarray(msgs).reshape(-1).view(np.uint8)
        n = msgs.size // DHCP_MSG_DTYPE.itemsize
        replies = np.zeros(max(2 * n, 1), DHCP_REPLY_DTYPE)
        events = np.zeros(max(n, 1), DHCP_EVENT_DTYPE)
        verdicts = np.zeros(max(n, 1), np.uint8)
        nr, ne = ctypes.c_uint32(), ctypes.c_uint32()
        _lib.check("halo_dhcp_handle_msgs", _lib.lib.halo_dhcp_handle_msgs(
            self._h, _lib.ptr(msgs), n, int(now), _lib.ptr(replies), 2 * n, _lib.ptr(verdicts), ctypes.byref(nr),
            _lib.ptr(events), n, ctypes.byref(ne)))
        return DhcpHandleResult(replies[:nr.value].copy(), verdicts[:n].copy(), events[:ne.value].copy())

    def leases(self) -> np.ndarray:
        """``ListDhcp``: the leases as DHCP_LEASE_DTYPE, in ascending address order."""
        n = int(_lib.lib.halo_dhcp_list(self._h, None, 0))
        out = np.zeros(max(n, 1), DHCP_LEASE_DTYPE)
        n = min(n, int(_lib.lib.halo_dhcp_list(self._h, _lib.ptr(out), n)))
        return out[:n]

    def clear(self, now: int) -> int:
        """One ``DhcpLeaseClear`` tick: deletes the leases with ``now > ExpTime``; returns how many."""
        return int(_lib.lib.halo_dhcp_clear(self._h, int(now)))

    def set_dns(self, dns: int) -> None:
        _lib.check("halo_dhcp_set_dns", _lib.lib.halo_dhcp_set_dns(self._h, dns))

    def set_client_xid(self, xid: bytes) -> None:
        x = np.frombuffer(bytes(xid), np.uint8).copy()
        if x.size != 4:
            raise ValueError("a transaction id is four bytes")
        _lib.check("halo_dhcp_set_client_xid", _lib.lib.halo_dhcp_set_client_xid(self._h, _lib.ptr(x)))

    def discover(self, xid: bytes) -> np.ndarray:
        """``DhcpDiscover`` with the caller's random ``xid``: sets the client's transaction id and
        returns the DISCOVER message as one DHCP_REPLY_DTYPE record."""
        x = np.frombuffer(bytes(xid), np.uint8).copy()
        if x.size != 4:
            raise ValueError("a transaction id is four bytes")
        out = np.zeros(1, DHCP_REPLY_DTYPE)
        _lib.check("halo_dhcp_discover", _lib.lib.halo_dhcp_discover(self._h, _lib.ptr(x), _lib.ptr(out)))
        return out

    def rx_dhcp(self, payload: bytes, sport: int, dport: int, src_ip: int) -> DhcpHandleResult:
        """``RxDhcp(udpPayload, udpSrcPort, udpDstPort, ipv4SrcAddr)`` for one datagram, at
        ``time_now``: decodes it with the host loop and handles it. The replies are appended to
        ``tx_queue`` and the client events to ``events``."""
        r = self.handle(decode_host(_one_record(payload, sport, dport, src_ip), msg_cap=1).msgs, self.time_now)
        self.tx_queue.extend(r.replies)
        self.events.extend(r.events)
        return r


class _OneRecord:
    """A delivery of one DHCP record, as DeliverResult shows it."""

    def __init__(self, out, summary_raw, index_raw):
        self.out, self.summary_raw, self.index_raw, self.index_cap = out, summary_raw, index_raw, 1


def _one_record(payload: bytes, sport: int, dport: int, src_ip: int) -> _OneRecord:
    payload = bytes(payload)
    rec = struct.pack("<IBBHIHHII", 0, DELIVER_KIND["DHCP"], 0, len(payload), src_ip, sport, dport, 0, 0) + payload
    rec += bytes(-len(rec) % 4)
    summary = np.zeros(1, _lib.DELIVER_SUMMARY_DTYPE)
    summary["records"], summary["records_written"] = 1, 1
    summary["bytes"], summary["bytes_written"] = len(rec), len(rec)
    summary["kind_counts"][0, DELIVER_KIND["DHCP"]] = 1
    index = np.zeros(1, _lib.DELIVER_INDEX_DTYPE)
    return _OneRecord(np.frombuffer(rec, np.uint8).copy(), summary.view(np.uint8), index.view(np.uint8))


# ---- decode ---------------------------------------------------------------------------------------
class DhcpDecodeResult:
    """What one decode call wrote. ``msgs_raw`` ([msg_cap, 128] bytes) and ``summary_raw`` (64 bytes)
    are cuda tensors for a device result and copied on access (which synchronises); ``delivery`` is
    the ``DeliverResult`` the call read."""

    def __init__(self, delivery, msgs_raw, summary_raw, workspace=None):
        self.delivery = delivery
        self.workspace = workspace  # held while the call may still run: its memory must not be handed out again
        self.msgs_raw, self.summary_raw = msgs_raw, summary_raw
        self._summary = self._msgs = None

    @property
    def summary(self) -> np.void:
        """The summary as one DHCP_SUMMARY_DTYPE record."""
        if self._summary is None:
            self._summary = _bytes(self.summary_raw, DHCP_SUMMARY_DTYPE.itemsize).view(DHCP_SUMMARY_DTYPE).copy()[0]
        return self._summary

    @property
    def msgs(self) -> np.ndarray:
        """The written message records as DHCP_MSG_DTYPE [msgs_written]: 128 bytes each are what a
        host downloads, not the stream."""
        if self._msgs is None:
            n = int(self.summary["msgs_written"])
            self._msgs = _bytes(self.msgs_raw, n * DHCP_MSG_DTYPE.itemsize).view(DHCP_MSG_DTYPE).copy()
        return self._msgs

    def feed(self, server: DhcpServer, now: int) -> DhcpHandleResult:
        """``server.handle`` over the written messages, in stream order."""
        return server.handle(self.msgs, now)


def workspace_bytes(index_cap: int) -> int:
    return int(_lib.lib.halo_dhcp_decode_workspace(index_cap))


def decode(deliver_result, *, msg_cap: int, msgs=None, summary=None, workspace=None, stream=None) -> DhcpDecodeResult:
    """DHCP decode of a device ``DeliverResult`` (made with ``dhcp=True`` and an index). ``msgs``
    ([msg_cap, 16] int64, 16-byte aligned), ``summary`` (8 int64) and ``workspace`` (int64, at least
    ``workspace_bytes(index_cap)``; may be shared by calls on one stream) are allocated when not
    given; the result holds the workspace, and with ``stream`` given every tensor is recorded on
    it. A delivery without an index is a ValueError."""
    import torch

    r = deliver_result
    if r.index_raw is None or r.index_cap == 0:
        raise ValueError("dhcp.decode needs a delivery made with an index (index_cap > 0)")
    dev = r.out.device
    if msgs is None:
        msgs = torch.empty((max(msg_cap, 1), 16), dtype=torch.int64, device=dev)
    if summary is None:
        summary = torch.empty(DHCP_SUMMARY_DTYPE.itemsize // 8, dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = torch.empty(max(workspace_bytes(r.index_cap), 8) // 8, dtype=torch.int64, device=dev)
    st = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
    _lib.check("halo_dhcp_decode_device", _lib.lib.halo_dhcp_decode_device(
        _lib.ptr(r.out), _lib.ptr(r.summary_raw), _lib.ptr(r.index_raw), r.index_cap, _lib.ptr(msgs), msg_cap,
        _lib.ptr(summary), _lib.ptr(workspace), _nbytes(workspace), st))
    if stream is not None:  # allocated under the current stream, used on this one
        for t in (msgs, summary, workspace):
            t.record_stream(stream)
    return DhcpDecodeResult(r, msgs, summary, workspace)


def decode_host(deliver_result, *, msg_cap: int) -> DhcpDecodeResult:
    """The same from the sequential loop (``halo_dhcp_decode_host``) over a host ``DeliverResult``
    (``deliver_host``'s, or a device result's arrays, which are downloaded here)."""
    r = deliver_result
    if r.index_raw is None or r.index_cap == 0:
        raise ValueError("dhcp.decode_host needs a delivery made with an index (index_cap > 0)")
    out = np.ascontiguousarray(_host(r.out)).view(np.uint8)
    dsum = np.ascontiguousarray(_host(r.summary_raw)).reshape(-1).view(np.uint8)
    index = np.ascontiguousarray(_host(r.index_raw)).reshape(-1).view(np.uint8)
    msgs = np.zeros((max(msg_cap, 1), DHCP_MSG_DTYPE.itemsize), np.uint8)
    summary = np.zeros(DHCP_SUMMARY_DTYPE.itemsize, np.uint8)
    _lib.check("halo_dhcp_decode_host", _lib.lib.halo_dhcp_decode_host(
        _lib.ptr(out), _lib.ptr(dsum), _lib.ptr(index), r.index_cap, _lib.ptr(msgs), msg_cap, _lib.ptr(summary)))
    return DhcpDecodeResult(r, msgs, summary)


# ---- reply build ----------------------------------------------------------------------------------
class DhcpBuildResult:
    """What one reply build wrote: ``payload_raw`` ([n * 288] bytes) and ``descs_raw`` ([n, 40]
    bytes); cuda tensors for a device result, copied on access (which synchronises)."""

    def __init__(self, n, payload_raw, descs_raw):
        self.n, self.payload_raw, self.descs_raw = n, payload_raw, descs_raw

    def descs(self) -> np.ndarray:
        """The build descriptors as BUILD_DESC_DTYPE [n]."""
        return _bytes(self.descs_raw, self.n * BUILD_DESC_DTYPE.itemsize).view(BUILD_DESC_DTYPE)

    def slots(self) -> np.ndarray:
        """The payload buffer as uint8 [n, 288]."""
        return _bytes(self.payload_raw, self.n * DHCP_SLOT_BYTES).reshape(self.n, DHCP_SLOT_BYTES)

    def payloads(self) -> list:
        """The UDP payload of every reply, as ``bytes``."""
        s = self.slots()
        return [s[i, :int(d["payload_len"])].tobytes() for i, d in enumerate(self.descs())]

    def build(self, builder, *, netif, out_stride: int = 1536, **kw):
        """Hands the descriptors and the payloads to ``builder.build`` (a ``protocol.TxBuilder``; a
        device result only): one broadcast frame per reply."""
        if not hasattr(self.descs_raw, "cpu"):
            raise ValueError("DhcpBuildResult.build needs a device result")
        import torch

        desc = self.descs_raw.reshape(-1).view(torch.uint8)[:self.n * BUILD_DESC_DTYPE.itemsize]
        return builder.build(desc, self.payload_raw.reshape(-1).view(torch.uint8), netif=netif, out_stride=out_stride, **kw)


def _cfg_of(config) -> _lib.DhcpConfig:
    return config.config if isinstance(config, DhcpServer) else config


def build_replies(replies, *, config, n=None, payload=None, descs=None, stream=None) -> DhcpBuildResult:
    """The reply build over a cuda tensor of DHCP_REPLY_DTYPE records (any element type, 16-byte
    aligned). ``config`` is a ``DhcpServer`` or a ``_lib.DhcpConfig`` (own ip, mask and DNS).
    ``payload`` ([n * 288] bytes) and ``descs`` ([n, 5] int64) are allocated when not given."""
    import torch

    n = _nbytes(replies) // DHCP_REPLY_DTYPE.itemsize if n is None else n
    dev = replies.device
    if payload is None:
        payload = torch.empty(max(n, 1) * DHCP_SLOT_BYTES // 8, dtype=torch.int64, device=dev)
    if descs is None:
        descs = torch.empty((max(n, 1), 5), dtype=torch.int64, device=dev)
    st = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
    _lib.check("halo_dhcp_reply_build_device", _lib.lib.halo_dhcp_reply_build_device(
        ctypes.byref(_cfg_of(config)), _lib.ptr(replies), n, _lib.ptr(payload), _lib.ptr(descs), st))
    if stream is not None:
        for t in (payload, descs):
            t.record_stream(stream)
    return DhcpBuildResult(n, payload, descs)


def build_replies_host(replies, *, config) -> DhcpBuildResult:
    """The same from the sequential loop (``halo_dhcp_reply_build_host``) over a numpy array."""
    replies = np.ascontiguousarray(replies).reshape(-1).view(np.uint8)
    n = replies.size // DHCP_REPLY_DTYPE.itemsize
    payload = np.zeros(max(n, 1) * DHCP_SLOT_BYTES, np.uint8)
    descs = np.zeros((max(n, 1), BUILD_DESC_DTYPE.itemsize), np.uint8)
    _lib.check("halo_dhcp_reply_build_host", _lib.lib.halo_dhcp_reply_build_host(
        ctypes.byref(_cfg_of(config)), _lib.ptr(replies), n, _lib.ptr(payload), _lib.ptr(descs)))
    return DhcpBuildResult(n, payload, descs)
