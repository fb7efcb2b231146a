"""Batch mirror of a Router's ``NatPortMappingFlowTable`` (include/halo_rx.h, "port-mapping return
flows"): what sends the replies of a port-forwarded connection back out of the WAN NetIf it came in
on (engine/ipv4_engine.go:160-186, :203-207, :238-266, :489-516).

The host table is the control plane — ``record`` (the Get / MallocType / Set of :238-266 over a
batch of items), ``get`` (:164-179), ``TableClear`` (one ``NatPortMappingFlowClear`` tick), ``List``.
``sync`` compiles it into HBM; ``lookup`` is the LAN-side half over cuda tensors, ``record_device``
lists the frames of a WAN-side batch that record a flow, and ``ArpTable.encap_via`` (defined here)
is the L2 step with the out-interface override. ``forward_return_flows`` chains route -> ``lookup`` ->
the out NetIf's ``lookup_lan`` -> fixup -> ``encap_via`` without a host round trip.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import (ARP_V_COUNT, PMFLOW_ENTRY_DTYPE, PMFLOW_ITEM_DTYPE, PMFLOW_LAYOUT_DTYPE, PMFLOW_V,  # noqa: F401
                   PMFLOW_V_COUNT, PMFLOW_VERDICT_NAMES, PMFLOW_VIA_DTYPE, TX_TTL)
from .arp import ArpTable


class PortMappingFlowTable:
    def __init__(self, netifs, gateways, capacity: int, capacity_log2: int = 0, device: int = 0):
        """``netifs``: the Router's ``_lib.NetIf`` objects, NetIf 0 first (at most 64); ``gateways``:
        ``IpAddrToU(NetIf.Gateway)`` per NetIf, 0 for nil."""
        self._t = None  # before anything can raise: __del__ closes
        cfg = _lib.PmflowConfig()
        netifs, gateways = list(netifs), list(gateways)
        assert len(netifs) == len(gateways)
        cfg.n_netifs = len(netifs)
        for q, nif in enumerate(netifs[:_lib.ARP_MAX_NETIFS]):
            cfg.netif[q] = nif
            cfg.gateway[q] = int(gateways[q]) & 0xFFFFFFFF
        cfg.capacity, cfg.capacity_log2 = capacity, capacity_log2
        h = ctypes.c_void_p()
        _lib.check("halo_pmflow_table_create", _lib.lib.halo_pmflow_table_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._t = h
        self.n_netifs, self.capacity, self.device = cfg.n_netifs, capacity, device

    def close(self):
        if self._t:
            _lib.lib.halo_pmflow_table_destroy(self._t)
            self._t = None

    def __del__(self):
        self.close()

    # ---- host control plane -------------------------------------------------------------------
    def record(self, in_netif: int, items: np.ndarray, now: int):
        """:238-266 over ``items`` (PMFLOW_ITEM_DTYPE) in order, for frames NetIf ``in_netif``
        received: (dropped uint8 [k], n_added). A dropped frame must not be sent."""
        items = np.ascontiguousarray(items, PMFLOW_ITEM_DTYPE)
        k = int(items.shape[0])
        dropped = np.zeros(max(k, 1), np.uint8)
        added = ctypes.c_uint32()
        _lib.check("halo_pmflow_record", _lib.lib.halo_pmflow_record(
            self._t, in_netif, _lib.ptr(items), k, now & 0xFFFFFFFF, _lib.ptr(dropped), ctypes.byref(added)))
        return dropped[:k], int(added.value)

    def get(self, remote_ip, remote_port, lan_ip, lan_port, proto, now: int | None = None):
        """The host lookup of :164-179: the flow (a PMFLOW_ENTRY_DTYPE record) or None. With ``now``
        a found flow is stamped, as the forward path does."""
        e = np.zeros(1, PMFLOW_ENTRY_DTYPE)
        f = ctypes.c_uint32()
        stamp = None if now is None else ctypes.byref(ctypes.c_uint32(now & 0xFFFFFFFF))
        _lib.check("halo_pmflow_get", _lib.lib.halo_pmflow_get(
            self._t, remote_ip, remote_port, lan_ip, lan_port, proto, stamp, _lib.ptr(e), ctypes.byref(f)))
        return e[0].copy() if f.value else None

    def TableClear(self, now: int) -> int:  # noqa: N802
        """One NatPortMappingFlowClear tick (halo_pmflow_expire): the number of flows removed.
        Synchronise the streams of earlier lookups first."""
        n = ctypes.c_uint32()
        _lib.check("halo_pmflow_expire", _lib.lib.halo_pmflow_expire(self._t, now & 0xFFFFFFFF, ctypes.byref(n)))
        return int(n.value)

    def List(self, cap: int | None = None) -> np.ndarray:  # noqa: N802
        n = ctypes.c_uint32()
        _lib.check("halo_pmflow_list", _lib.lib.halo_pmflow_list(self._t, None, 0, ctypes.byref(n)))
        cap = n.value if cap is None else cap
        out = np.zeros(max(cap, 1), PMFLOW_ENTRY_DTYPE)
        _lib.check("halo_pmflow_list", _lib.lib.halo_pmflow_list(self._t, _lib.ptr(out), cap, ctypes.byref(n)))
        return out[:min(cap, n.value)]

    def layout_stats(self) -> np.ndarray:
        out = np.zeros(1, PMFLOW_LAYOUT_DTYPE)
        _lib.check("halo_pmflow_layout_stats", _lib.lib.halo_pmflow_layout_stats(self._t, _lib.ptr(out)))
        return out[0]

    @property
    def dirty(self) -> bool:
        return _lib.lib.halo_pmflow_dirty(self._t) == 1

    # ---- device side --------------------------------------------------------------------------
    def sync(self, routes=None) -> None:
        """Compile and publish the device copy; ``routes`` (a ``RouteTable``) adds the NetIf of every
        route id, which ``lookup`` needs."""
        _lib.check("halo_pmflow_sync_device", _lib.lib.halo_pmflow_sync_device(
            self._t, None if routes is None else routes._t, self.device))

    @staticmethod
    def _stream(stream):
        import torch

        return (stream if stream is not None else torch.cuda.current_stream()).cuda_stream

    def lookup(self, records, now: int, route_ids, ops=None, select=None, counts=None, stream=None):
        """The LAN-side half over cuda tensors: ``records`` uint8 [n, 32], ``route_ids`` int32 [n],
        optional ``select`` uint8 [n]; ``ops`` (uint8 [n, 16], zeroed when None) is updated in place.
        Returns (ops, via uint8 [n, 8] = PMFLOW_VIA_DTYPE, hit uint8 [n], counts int32 [4],
        incremented). ``hit`` is the ``skip`` of the out NetIf's ``NatTable.lookup_lan``."""
        import torch

        n = int(records.shape[0])
        dev = records.device
        if ops is None:
            ops = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
        via = torch.empty((n, 8), dtype=torch.uint8, device=dev)
        hit = torch.empty(n, dtype=torch.uint8, device=dev)
        if counts is None:
            counts = torch.zeros(PMFLOW_V_COUNT, dtype=torch.int32, device=dev)
        _lib.check("halo_pmflow_lookup_device", _lib.lib.halo_pmflow_lookup_device(
            self._t, _lib.ptr(records), n, now & 0xFFFFFFFF, _lib.ptr(route_ids), _lib.ptr(select), _lib.ptr(ops),
            _lib.ptr(via), _lib.ptr(hit), _lib.ptr(counts), self._stream(stream)))
        return ops, via, hit, counts

    def record_device(self, in_netif: int, records, wan_verdict, ops, arp_results, now: int, cap: int | None = None,
                      workspace=None, stream=None):
        """The frames of a batch NetIf ``in_netif`` received that record a flow, after the encap in
        stream order (cuda tensors: ``records`` uint8 [n, 32], ``wan_verdict`` uint8 [n], ``ops`` uint8
        [n, 16], ``arp_results`` uint8 [n, 8]): (items uint8 [cap, 20] = PMFLOW_ITEM_DTYPE, count int32
        [1]). ``count`` is the number listed even when it exceeds ``cap`` (default n). ``workspace``
        (int32, at least ``halo_pmflow_record_workspace(n)`` bytes) may be shared by calls on one stream."""
        import torch

        n = int(records.shape[0])
        cap = n if cap is None else cap
        dev = records.device
        items = torch.zeros((max(cap, 1), 20), dtype=torch.uint8, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        if workspace is None:
            workspace = torch.empty(int(_lib.lib.halo_pmflow_record_workspace(n)) // 4, dtype=torch.int32, device=dev)
        _lib.check("halo_pmflow_record_device", _lib.lib.halo_pmflow_record_device(
            self._t, in_netif, _lib.ptr(records), _lib.ptr(wan_verdict), _lib.ptr(ops), _lib.ptr(arp_results), n,
            now & 0xFFFFFFFF, _lib.ptr(items), cap, _lib.ptr(count), _lib.ptr(workspace),
            workspace.numel() * workspace.element_size(), self._stream(stream)))
        return items, count

    @classmethod
    def drop(cls, arp_results, index, stream=None) -> None:
        """``halo_arp_drop_device``: the frames ``index`` (cuda int32 [k]) of ``arp_results`` (cuda
        uint8 [n, 8]) become NONE, so the egress leaves them out."""
        _lib.check("halo_arp_drop_device", _lib.lib.halo_arp_drop_device(
            _lib.ptr(arp_results), _lib.ptr(index), int(index.numel()), cls._stream(stream)))


def items_of(items, count) -> np.ndarray:
    """The written items of ``record_device`` as PMFLOW_ITEM_DTYPE (synchronises)."""
    k = int(count.cpu().numpy().view(np.uint32)[0])
    a = items.cpu().numpy().reshape(-1).view(PMFLOW_ITEM_DTYPE)
    return a[:min(k, a.shape[0])].copy()


def _encap_via(self, data, offsets_dw, lens, route_ids, in_netif: int, via, select=None, counts=None, miss_count=None,
               stream=None):
    """``encap`` with the return-flow override: where ``via`` (cuda uint8 [n, 8], ``lookup``'s)
    says OVERRIDE, the out NetIf and next hop come from it and the route id is not consulted.
    ``via`` None gives ``encap``'s results. Returns (results uint8 [n, 8], counts int32 [7],
    miss_count int32 [1])."""
    import torch

    n = int(lens.shape[0])
    results = torch.empty((n, 8), dtype=torch.uint8, device=data.device)
    if counts is None:
        counts = torch.zeros(ARP_V_COUNT, dtype=torch.int32, device=data.device)
    if miss_count is None:
        miss_count = torch.zeros(1, dtype=torch.int32, device=data.device)
    _lib.check("halo_arp_encap_via_device", _lib.lib.halo_arp_encap_via_device(
        self._t, _lib.ptr(data), _lib.ptr(offsets_dw), _lib.ptr(lens), n, _lib.ptr(route_ids), in_netif,
        _lib.ptr(select), _lib.ptr(via), _lib.ptr(results), _lib.ptr(counts), _lib.ptr(miss_count),
        self._stream(stream)))
    return results, counts, miss_count


ArpTable.encap_via = _encap_via


class ReturnFlows:
    """``forward_return_flows``' result: ``records``, ``route_ids``, ``ops``, ``via``, ``hit``,
    ``pm_counts``, the out NetIf's ``nat_verdict`` / ``nat_ref`` / ``nat_miss`` (None without a NAT
    table), ``fixup_result`` and the encap's ``results`` / ``counts`` / ``miss_count`` — what
    ``egress_arp(data, offsets_dw, lens, results, ...)`` takes — and ``mark`` (``loopback.mark``'s, None
    without ``loopback=True``) and ``nat_new`` (``(n_listed, n_added)``, None without ``new_flows=True``)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def forward_return_flows(data, offsets_dw, lens, *, netif, in_netif: int, now: int, pmflow, routes, arp, nat=None,
                         records=None, steps: int = TX_TTL, check_sum_enable: bool = True, stream=None,
                         loopback: bool = False, new_flows: bool = False) -> ReturnFlows:
    """The forward chain for a batch a non-NAT NetIf received (cuda tensors as ``parse_frames_batch``),
    rewritten in place: parse (unless ``records`` is given) -> ``routes.FindRouteRecords`` ->
    ``pmflow.lookup`` -> ``nat.lookup_lan`` with the return-flow hits skipped (``nat``: the NAT table
    of the NetIf the routes point at, or None) -> fixup (TTL, then the SNAT the lookups chose) ->
    ``arp.encap_via`` for the frames whose TTL survived. No host round trip. A ``nat`` MISS (a new
    flow) keeps the caller's slow path, ``NatTable.resolve_misses``, as before.

    ``new_flows=True`` (with a ``nat``) resolves those misses inside the chain instead:
    ``nat.resolve_misses_device(LAN, ...)`` runs between ``nat.lookup_lan`` and the fixup — one item
    per new key goes to the host table and comes back — so a new flow's first packets leave with their
    SNAT in this batch. Only frames whose TTL byte is above 1 are selected (the reference returns at
    :135-142, before any NatAddFlow, so a TTL-dead packet adds no flow), and the records the host
    answered DROP are not passed to the encap (:214-217: nothing is transmitted). The result then
    carries ``nat_new = (n_listed, n_added)``.

    ``loopback=True`` puts ``loopback.mark`` between ``pmflow.lookup`` and ``nat.lookup_lan``: a packet
    addressed to the out NetIf's own address is skipped by the NAT lookup as the return-flow hits are
    (the reference returns at :201, ahead of :203-225), so it reaches the encap's LOOPBACK verdict
    with its LAN source and no flow is added for it. The result then carries ``mark``; ``loopback.gather``
    takes ``results`` as it stands."""
    import torch

    from . import protocol

    if records is None:
        records = protocol.parse_frames_batch(data, offsets_dw, lens, netif=netif, check_sum_enable=check_sum_enable,
                                              stream=stream)
    n = int(lens.shape[0])
    route_ids = routes.FindRouteRecords(records, stream=stream)
    ops = torch.zeros((n, 16), dtype=torch.uint8, device=data.device)
    ops[:, 0] = steps  # the steps every frame takes (HALO_TX_TTL; callers add HALO_TX_RECALC / _DPDK_FILL)
    ops, via, hit, pm_counts = pmflow.lookup(records, now, route_ids, ops=ops, stream=stream)
    nat_verdict = nat_ref = nat_miss = None
    lo_mark, skip = None, hit
    if loopback:
        from . import loopback as lo

        lo_mark = lo.mark(arp, records, route_ids, in_netif, via=via, stream=stream)
        skip = hit | lo_mark
    if nat is not None:
        ops, nat_verdict, nat_ref, nat_miss = nat.lookup_lan(records, now, ops=ops, skip=skip, stream=stream)
    nat_new = None
    if new_flows and nat is not None:
        # the frame's TTL byte (Ethernet 14 + IPv4 8), for frames that reach it
        at = (offsets_dw.to(torch.int64) & 0xFFFFFFFF) * 4 + 22
        reach = (lens.to(torch.int32) & 0xFFFF) > 22
        ttl = data[torch.where(reach, at, torch.zeros_like(at))]
        select = (reach & (ttl > 1)).to(torch.uint8)
        nat_new = nat.resolve_misses_device(_lib.FLOW_NAT_LAN, records, ops, nat_verdict, nat_ref, now, select=select,
                                            stream=stream)
    fixup_result = torch.zeros(n, dtype=torch.uint8, device=data.device)
    protocol.tx_fixup_batch(data, offsets_dw, lens, ops.reshape(-1), check_sum_enable=check_sum_enable,
                            result=fixup_result, stream=stream)
    alive = fixup_result & protocol.TX_R_TTL_ALIVE
    if nat_new is not None:
        alive = alive * (nat_verdict != _lib.NAT_V_DROP)  # NatAddFlow returned nil: not transmitted
    results, counts, miss_count = arp.encap_via(data, offsets_dw, lens, route_ids, in_netif, via, select=alive,
                                                stream=stream)
    return ReturnFlows(records=records, route_ids=route_ids, ops=ops, via=via, hit=hit, pm_counts=pm_counts,
                       nat_verdict=nat_verdict, nat_ref=nat_ref, nat_miss=nat_miss, fixup_result=fixup_result,
                       alive=alive, results=results, counts=counts, miss_count=miss_count, mark=lo_mark,
                       nat_new=nat_new)
