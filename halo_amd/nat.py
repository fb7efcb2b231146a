"""Batch mirror of a NATing ``engine.NetIf``'s flow table (include/halo_rx.h, "NAT flow table").

``NatAddFlow / NatGetFlowByHash / NatGetFlowByWan / ListNat / NatTableClear``
(engine/ipv4_engine.go:524-759) run on the host table through the C ABI; ``sync()`` compiles it
into the device's open-addressing tables; ``lookup_wan / lookup_lan / lookup_quote`` run the
forward path's lookups over device-resident parsed records and fill the ``halo_tx_op_t`` array of
``halo_tx_fixup_batch_device``; ``resolve_misses`` is the host slow path for new flows.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import (FLOW_NAT_LAN, FLOW_NAT_WAN, NAT_FLOW_DTYPE, NAT_LAYOUT_DTYPE, NAT_NO_FLOW,  # noqa: F401
                   NAT_V_DROP, NAT_V_FLOW, NAT_V_MAPPING, NAT_V_MISS, NAT_V_NONE, NAT_V_SKIP, TX_OP_DTYPE)


class NatTable:
    def __init__(self, wan_ip: int, nat_type: int = _lib.NAT_SYMMETRIC, capacity_log2: int = 0, device: int = 0):
        h = ctypes.c_void_p()
        cfg = _lib.NatConfig(wan_ip, nat_type, capacity_log2, 0)
        _lib.check("halo_nat_table_create", _lib.lib.halo_nat_table_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._t = h
        self.wan_ip, self.nat_type, self.device = wan_ip, nat_type, device

    def close(self):
        if self._t:
            _lib.lib.halo_nat_table_destroy(self._t)
            self._t = None

    def __del__(self):
        self.close()

    # ---- control plane (host) -----------------------------------------------------------------
    def add_port_mapping(self, wan_port: int, lan_ip: int, lan_port: int, proto: int) -> None:
        _lib.check("halo_nat_port_mapping_add",
                   _lib.lib.halo_nat_port_mapping_add(self._t, wan_port, lan_ip, lan_port, proto))

    @staticmethod
    def _flow(out: np.ndarray):
        return None if int(out["id"][0]) == NAT_NO_FLOW else out[0].copy()

    def AddFlow(self, lan_ip, remote_ip, lan_port, remote_port, proto, now):  # noqa: N802
        """NatAddFlow: the new flow (a NAT_FLOW_DTYPE record) or None for nil."""
        out = np.zeros(1, NAT_FLOW_DTYPE)
        _lib.check("halo_nat_add_flow", _lib.lib.halo_nat_add_flow(
            self._t, lan_ip, remote_ip, lan_port, remote_port, proto, now & 0xFFFFFFFF, _lib.ptr(out), None))
        return self._flow(out)

    def GetFlowByHash(self, remote_ip, remote_port, lan_ip, lan_port, proto):  # noqa: N802
        out = np.zeros(1, NAT_FLOW_DTYPE)
        _lib.check("halo_nat_get_flow_lan", _lib.lib.halo_nat_get_flow_lan(
            self._t, remote_ip, remote_port, lan_ip, lan_port, proto, _lib.ptr(out), None))
        return self._flow(out)

    def GetFlowByWan(self, remote_ip, remote_port, wan_ip, wan_port, proto):  # noqa: N802
        out = np.zeros(1, NAT_FLOW_DTYPE)
        _lib.check("halo_nat_get_flow_wan", _lib.lib.halo_nat_get_flow_wan(
            self._t, remote_ip, remote_port, wan_ip, wan_port, proto, _lib.ptr(out), None))
        return self._flow(out)

    def ListNat(self, cap: int | None = None) -> np.ndarray:  # noqa: N802
        n = ctypes.c_uint32()
        _lib.check("halo_nat_list", _lib.lib.halo_nat_list(self._t, None, 0, ctypes.byref(n)))
        cap = n.value if cap is None else cap
        out = np.zeros(max(cap, 1), NAT_FLOW_DTYPE)
        _lib.check("halo_nat_list", _lib.lib.halo_nat_list(self._t, _lib.ptr(out), cap, ctypes.byref(n)))
        return out[:min(cap, n.value)]

    def TableClear(self, now: int) -> int:  # noqa: N802
        """One NatTableClear tick (halo_nat_expire): the number of flows removed. Synchronise the
        streams of earlier lookups first."""
        n = ctypes.c_uint32()
        _lib.check("halo_nat_expire", _lib.lib.halo_nat_expire(self._t, now & 0xFFFFFFFF, ctypes.byref(n)))
        return int(n.value)

    def layout_stats(self) -> np.ndarray:
        out = np.zeros(1, NAT_LAYOUT_DTYPE)
        _lib.check("halo_nat_layout_stats", _lib.lib.halo_nat_layout_stats(self._t, _lib.ptr(out)))
        return out[0]

    def resolve_misses(self, direction: int, records: np.ndarray, verdicts: np.ndarray, now: int, ops: np.ndarray):
        """halo_nat_resolve_misses over host arrays: ``ops`` is updated in place; returns
        (verdicts_out, n_added)."""
        n = len(records)
        assert records.dtype == _lib.RESULT_DTYPE and ops.dtype == TX_OP_DTYPE and verdicts.dtype == np.uint8
        assert len(verdicts) == n and len(ops) == n
        out = np.empty(n, np.uint8)
        added = ctypes.c_uint32()
        _lib.check("halo_nat_resolve_misses", _lib.lib.halo_nat_resolve_misses(
            self._t, direction, _lib.ptr(records), _lib.ptr(verdicts), n, now & 0xFFFFFFFF, _lib.ptr(ops),
            _lib.ptr(out), ctypes.byref(added)))
        return out, int(added.value)

    # ---- device ------------------------------------------------------------------------------
    def sync(self):
        _lib.check("halo_nat_sync_device", _lib.lib.halo_nat_sync_device(self._t, self.device))

    def _lookup(self, direction, records, now, ops, skip, stream):
        import torch

        compact = records.shape[1] == 16
        n = int(records.shape[0])
        dev = records.device
        if ops is None:
            ops = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
        verdict = torch.empty(n, dtype=torch.uint8, device=dev)
        ref = torch.empty(n, dtype=torch.int32, device=dev)
        miss = torch.zeros(1, dtype=torch.int32, device=dev)
        s = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
        name = f"halo_nat_lookup_{direction}{'_compact' if compact else ''}_device"
        _lib.check(name, getattr(_lib.lib, name)(self._t, _lib.ptr(records), n, now & 0xFFFFFFFF, _lib.ptr(skip),
                                                 _lib.ptr(ops), _lib.ptr(verdict), _lib.ptr(ref), _lib.ptr(miss), s))
        return ops, verdict, ref, miss

    def lookup_wan(self, records, now, ops=None, skip=None, stream=None):
        """The inbound half over cuda uint8 records [n, 32] (or compact [n, 16]). ``ops`` (cuda
        uint8 [n, 16], zeroed when None) is updated in place. Returns (ops, verdict u8 [n],
        ref i32 [n], miss_count i32 [1]) — all device tensors, asynchronous."""
        return self._lookup("wan", records, now, ops, skip, stream)

    def lookup_lan(self, records, now, ops=None, skip=None, stream=None):
        """The outbound half; arguments and results as lookup_wan."""
        return self._lookup("lan", records, now, ops, skip, stream)

    def lookup_quote(self, quote_records, out=None, stream=None):
        """IcmpTtlDeepNat's lookup over the quote records of the deep-NAT first pass (cuda uint8
        [n, 32]): a cuda uint8 [n, 8] tensor of halo_tx_deep_nat_t for the second pass."""
        import torch

        n = int(quote_records.shape[0])
        if out is None:
            out = torch.empty((n, 8), dtype=torch.uint8, device=quote_records.device)
        s = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
        _lib.check("halo_nat_lookup_quote_device",
                   _lib.lib.halo_nat_lookup_quote_device(self._t, _lib.ptr(quote_records), n, _lib.ptr(out), s))
        return out
