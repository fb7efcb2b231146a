"""Batch mirror of a Router's ARP state (include/halo_rx.h, "ARP neighbour cache").

The host table is the control plane and carries the reference's names — ``SetArpCache``,
``GetArpCache``, ``HandleArp`` over a batch of messages, ``ArpTableClear``, ``ArpTableRefresh``,
``ListArp``, ``SendArpReq``, ``SendFreeArp`` (engine/arp_engine.go). ``sync`` compiles it into HBM;
``lookup`` is the bare ``GetArpCache`` over cuda tensors, ``encap`` the forward path's L2 step
(route id -> next hop -> MAC -> Ethernet header, in place) and ``gather`` brings a parsed batch's
ARP messages to the host in frame order. Device lookups see the table as of the last ``sync``;
``dirty`` says when a re-sync is worthwhile.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import (ARP_ENTRY_DTYPE, ARP_GET_ABSENT, ARP_GET_FOUND, ARP_GET_OWN_IP, ARP_H, ARP_H_F_NOT_LEARNED,  # noqa: F401
                   ARP_H_F_REPLY, ARP_H_MASK, ARP_H_NAMES, ARP_LAYOUT_DTYPE, ARP_MSG_DTYPE, ARP_RESULT_DTYPE, ARP_V,
                   ARP_V_COUNT, ARP_VERDICT_NAMES)


def _mac_bytes(mac) -> np.ndarray:
    if isinstance(mac, str):
        mac = [int(p, 16) for p in mac.split(":")]
    if isinstance(mac, (bytes, bytearray)):
        mac = np.frombuffer(bytes(mac), np.uint8)
    m = np.ascontiguousarray(np.asarray(mac, np.uint8))
    assert m.shape == (6,)
    return m


class ArpTable:
    def __init__(self, netifs, capacity: int, slots_log2: int = 0, device: int = 0):
        """``netifs``: the Router's ``_lib.NetIf`` objects, NetIf 0 first (at most 64)."""
        self._t = None  # before anything can raise: __del__ closes
        cfg = _lib.ArpConfig()
        netifs = list(netifs)
        cfg.n_netifs = len(netifs)
        for q, nif in enumerate(netifs[:_lib.ARP_MAX_NETIFS]):
            cfg.netif[q] = nif
        cfg.capacity, cfg.slots_log2 = capacity, slots_log2
        self._ips = [int(nif.ip) for nif in netifs]
        h = ctypes.c_void_p()
        _lib.check("halo_arp_table_create", _lib.lib.halo_arp_table_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._t = h
        self.n_netifs, self.capacity, self.device = cfg.n_netifs, capacity, device

    def close(self):
        if self._t:
            _lib.lib.halo_arp_table_destroy(self._t)
            self._t = None

    def __del__(self):
        self.close()

    # ---- host control plane -------------------------------------------------------------------
    def SetArpCache(self, netif: int, ip: int, mac, now: int) -> None:  # noqa: N802
        _lib.check("halo_arp_set", _lib.lib.halo_arp_set(self._t, netif, ip, _lib.ptr(_mac_bytes(mac)), now & 0xFFFFFFFF))

    def GetArpCache(self, netif: int, ip: int):  # noqa: N802
        """(found, entry): found is ARP_GET_ABSENT (a SendArpReq is owed), ARP_GET_FOUND or
        ARP_GET_OWN_IP; entry is an ARP_ENTRY_DTYPE record when found, else None."""
        e = np.zeros(1, ARP_ENTRY_DTYPE)
        f = ctypes.c_uint32()
        _lib.check("halo_arp_get", _lib.lib.halo_arp_get(self._t, netif, ip, _lib.ptr(e), ctypes.byref(f)))
        return int(f.value), (e[0] if f.value == ARP_GET_FOUND else None)

    def HandleArp(self, msgs: np.ndarray, now: int):  # noqa: N802
        """HandleArp over ``msgs`` (ARP_MSG_DTYPE) in order: (verdicts u8 [n], reply frames u8
        [n_replies, 60], n_changed)."""
        msgs = np.ascontiguousarray(msgs, ARP_MSG_DTYPE)
        n = int(msgs.shape[0])
        verdicts = np.zeros(n, np.uint8)
        replies = np.zeros((max(n, 1), 60), np.uint8)
        nr, nc = ctypes.c_uint32(), ctypes.c_uint32()
        _lib.check("halo_arp_handle_msgs", _lib.lib.halo_arp_handle_msgs(
            self._t, _lib.ptr(msgs), n, now & 0xFFFFFFFF, _lib.ptr(verdicts), _lib.ptr(replies), ctypes.byref(nr),
            ctypes.byref(nc)))
        return verdicts, replies[:nr.value], int(nc.value)

    def SendArpReq(self, netif: int, target_ip: int) -> np.ndarray:  # noqa: N802
        """The 60-byte request frame SendArpReq(target_ip) transmits on ``netif``."""
        out = np.zeros(60, np.uint8)
        _lib.check("halo_arp_build_request", _lib.lib.halo_arp_build_request(self._t, netif, target_ip, _lib.ptr(out)))
        return out

    def SendFreeArp(self, netif: int) -> np.ndarray:  # noqa: N802
        return self.SendArpReq(netif, self._ips[netif])

    def ArpTableClear(self, now: int) -> int:  # noqa: N802
        """One clear tick: the number of entries removed. Republishes a device copy that lost entries."""
        n = ctypes.c_uint32()
        _lib.check("halo_arp_expire", _lib.lib.halo_arp_expire(self._t, now & 0xFFFFFFFF, ctypes.byref(n)))
        return int(n.value)

    def ArpTableRefresh(self, now: int):  # noqa: N802
        """One refresh tick: (netifs u8 [k], ips u32 [k]) to SendArpReq for."""
        n = ctypes.c_uint32()
        _lib.check("halo_arp_refresh_list", _lib.lib.halo_arp_refresh_list(self._t, now & 0xFFFFFFFF, None, None, 0,
                                                                          ctypes.byref(n)))
        cap = int(n.value)
        netifs, ips = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.uint32)
        _lib.check("halo_arp_refresh_list", _lib.lib.halo_arp_refresh_list(
            self._t, now & 0xFFFFFFFF, _lib.ptr(netifs), _lib.ptr(ips), cap, ctypes.byref(n)))
        k = min(cap, n.value)
        return netifs[:k], ips[:k]

    def ListArp(self, cap: int | None = None) -> np.ndarray:  # noqa: N802
        n = ctypes.c_uint32()
        _lib.check("halo_arp_list", _lib.lib.halo_arp_list(self._t, None, 0, ctypes.byref(n)))
        cap = n.value if cap is None else cap
        out = np.zeros(max(cap, 1), ARP_ENTRY_DTYPE)
        _lib.check("halo_arp_list", _lib.lib.halo_arp_list(self._t, _lib.ptr(out), cap, ctypes.byref(n)))
        return out[:min(cap, n.value)]

    def layout_stats(self) -> np.ndarray:
        out = np.zeros(1, ARP_LAYOUT_DTYPE)
        _lib.check("halo_arp_layout_stats", _lib.lib.halo_arp_layout_stats(self._t, _lib.ptr(out)))
        return out[0]

    @property
    def dirty(self) -> bool:
        return _lib.lib.halo_arp_dirty(self._t) == 1

    # ---- device side --------------------------------------------------------------------------
    def sync(self, routes=None) -> None:
        """Compile and publish the device copy; ``routes`` (a ``RouteTable``) adds the route-entry
        array ``encap`` needs."""
        _lib.check("halo_arp_sync_device", _lib.lib.halo_arp_sync_device(
            self._t, None if routes is None else routes._t, self.device))

    @staticmethod
    def _stream(stream):
        import torch

        return (stream if stream is not None else torch.cuda.current_stream()).cuda_stream

    def lookup(self, ips, netifs=None, netif: int = 0, miss_count=None, stream=None):
        """GetArpCache for cuda tensors: ``ips`` int32 [n] (the u32 bit pattern), ``netifs`` uint8
        [n] or None with a uniform ``netif``. Returns (mac8 uint8 [n, 8], verdict uint8 [n],
        miss_count int32 [1], incremented)."""
        import torch

        n = int(ips.numel())
        mac8 = torch.empty((n, 8), dtype=torch.uint8, device=ips.device)
        verdict = torch.empty(n, dtype=torch.uint8, device=ips.device)
        if miss_count is None:
            miss_count = torch.zeros(1, dtype=torch.int32, device=ips.device)
        _lib.check("halo_arp_lookup_device", _lib.lib.halo_arp_lookup_device(
            self._t, _lib.ptr(ips), _lib.ptr(netifs), netif, n, _lib.ptr(mac8), _lib.ptr(verdict), _lib.ptr(miss_count),
            self._stream(stream)))
        return mac8, verdict, miss_count

    def encap(self, data, offsets_dw, lens, route_ids, in_netif: int, select=None, counts=None, miss_count=None,
              stream=None):
        """The forward path's L2 step over cuda tensors (uint8 bytes, int32 dword offsets, int16
        lengths, int32 route ids, optional uint8 select); HIT frames are rewritten in place.
        Returns (results uint8 [n, 8] = ARP_RESULT_DTYPE, counts int32 [7], miss_count int32 [1]);
        both counters are incremented."""
        import torch

        n = int(lens.shape[0])
        results = torch.empty((n, 8), dtype=torch.uint8, device=data.device)
        if counts is None:
            counts = torch.zeros(ARP_V_COUNT, dtype=torch.int32, device=data.device)
        if miss_count is None:
            miss_count = torch.zeros(1, dtype=torch.int32, device=data.device)
        _lib.check("halo_arp_encap_device", _lib.lib.halo_arp_encap_device(
            self._t, _lib.ptr(data), _lib.ptr(offsets_dw), _lib.ptr(lens), n, _lib.ptr(route_ids), in_netif,
            _lib.ptr(select), _lib.ptr(results), _lib.ptr(counts), _lib.ptr(miss_count), self._stream(stream)))
        return results, counts, miss_count

    @classmethod
    def gather(cls, data, offsets_dw, lens, records, netif: int, cap: int | None = None, stream=None):
        """The ARP messages of a parsed batch (cuda tensors; ``records`` uint8 [n, 32]), in frame
        order: (msgs uint8 [cap, 40] = ARP_MSG_DTYPE, count int32 [1]). ``count`` is the number
        selected even when it exceeds ``cap`` (default n)."""
        import torch

        n = int(lens.shape[0])
        cap = n if cap is None else cap
        msgs = torch.zeros((max(cap, 1), 40), dtype=torch.uint8, device=data.device)
        count = torch.zeros(1, dtype=torch.int32, device=data.device)
        wsb = int(_lib.lib.halo_arp_gather_workspace(n))
        ws = torch.empty(wsb // 4, dtype=torch.int32, device=data.device)
        _lib.check("halo_arp_gather_device", _lib.lib.halo_arp_gather_device(
            _lib.ptr(data), _lib.ptr(offsets_dw), _lib.ptr(lens), _lib.ptr(records), n, netif, _lib.ptr(msgs), cap,
            _lib.ptr(count), _lib.ptr(ws), wsb, cls._stream(stream)))
        return msgs, count
