"""Batch mirror of a NATing ``engine.NetIf``'s flow table (include/halo_rx.h, "NAT flow table").

``NatAddFlow / NatGetFlowByHash / NatGetFlowByWan / ListNat / NatTableClear``
(engine/ipv4_engine.go:524-759) run on the host table through the C ABI; ``sync()`` compiles it
into the device's open-addressing tables; ``lookup_wan / lookup_lan / lookup_quote`` run the
forward path's lookups over device-resident parsed records and fill the ``halo_tx_op_t`` array of
``halo_tx_fixup_batch_device``. New flows take one of two slow paths: ``resolve_misses`` over host
copies of the whole batch, or ``resolve_misses_device`` (``collect_misses`` -> ``resolve_items`` ->
``apply_answers``), which leaves the batch in HBM and brings one item per new key to the host.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import (FLOW_NAT_LAN, FLOW_NAT_WAN, NAT_ANSWER_DTYPE, NAT_FLOW_DTYPE, NAT_LAYOUT_DTYPE,  # noqa: F401
                   NAT_MISS_ITEM_DTYPE, NAT_NO_FLOW, NAT_V_DROP, NAT_V_FLOW, NAT_V_MAPPING, NAT_V_MISS, NAT_V_NONE, NAT_V_SKIP, TX_OP_DTYPE)


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

    def collect_misses_host(self, direction: int, records: np.ndarray, verdict: np.ndarray, select=None, cap=None):
        """halo_nat_collect_misses_host over host arrays: (items NAT_MISS_ITEM_DTYPE [min(count, cap)],
        count, pos uint32 [n]) — the answer ``collect_misses`` must give."""
        n = len(records)
        assert records.dtype == _lib.RESULT_DTYPE and verdict.dtype == np.uint8 and len(verdict) == n
        if select is not None:
            select = np.ascontiguousarray(select, np.uint8)
            assert len(select) == n
        cap = n if cap is None else cap
        items = np.zeros(max(cap, 1), NAT_MISS_ITEM_DTYPE)
        pos = np.empty(max(n, 1), np.uint32)
        count = np.zeros(1, np.uint32)
        _lib.check("halo_nat_collect_misses_host", _lib.lib.halo_nat_collect_misses_host(
            self._t, direction, _lib.ptr(records), _lib.ptr(verdict), _lib.ptr(select), n, _lib.ptr(items), cap,
            _lib.ptr(count), _lib.ptr(pos)))
        return items[:min(cap, int(count[0]))], int(count[0]), pos[:n]

    def resolve_items(self, direction: int, items: np.ndarray, now: int):
        """halo_nat_resolve_items over ``items`` in order: (answers NAT_ANSWER_DTYPE [k], n_added)."""
        items = np.ascontiguousarray(items, NAT_MISS_ITEM_DTYPE)
        k = int(items.shape[0])
        answers = np.zeros(max(k, 1), NAT_ANSWER_DTYPE)
        added = ctypes.c_uint32()
        _lib.check("halo_nat_resolve_items", _lib.lib.halo_nat_resolve_items(
            self._t, direction, _lib.ptr(items), k, now & 0xFFFFFFFF, _lib.ptr(answers), ctypes.byref(added)))
        return answers[:k], int(added.value)

    # ---- device ------------------------------------------------------------------------------
    @staticmethod
    def _stream(stream):
        import torch

        return (stream if stream is not None else torch.cuda.current_stream()).cuda_stream

    def collect_misses(self, direction: int, records, verdict, select=None, cap=None, scratch_log2: int = 0,
                       workspace=None, stream=None):
        """The records of a looked-up batch that are still MISS (and selected: ``select`` cuda uint8
        [n], optional), once per key and in ascending index (cuda tensors: ``records`` uint8 [n, 32] or
        compact [n, 16], ``verdict`` uint8 [n]): (items uint8 [cap, 20] = NAT_MISS_ITEM_DTYPE, count
        int32 [1], pos int32 [n]). ``count`` is the number listed even when it exceeds ``cap`` (default
        n); ``pos[i]`` is the list position of record i's key, -1 where not selected. ``workspace``
        (int32, at least ``halo_nat_miss_workspace(n, scratch_log2)`` bytes) may be shared by calls on
        one stream. Asynchronous."""
        import torch

        n = int(records.shape[0])
        cap = n if cap is None else cap
        dev = records.device
        items = torch.zeros((max(cap, 1), 20), dtype=torch.uint8, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        pos = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
        if workspace is None:
            need = int(_lib.lib.halo_nat_miss_workspace(n, scratch_log2))
            workspace = torch.empty(max(need // 4, 1), dtype=torch.int32, device=dev)
        name = f"halo_nat_collect_misses{'_compact' if records.shape[1] == 16 else ''}_device"
        _lib.check(name, getattr(_lib.lib, name)(
            self._t, direction, _lib.ptr(records), _lib.ptr(verdict), _lib.ptr(select), n, scratch_log2,
            _lib.ptr(items), cap, _lib.ptr(count), _lib.ptr(pos), _lib.ptr(workspace),
            workspace.numel() * workspace.element_size(), self._stream(stream)))
        return items, count, pos

    @classmethod
    def apply_answers(cls, direction: int, pos, answers, ops, verdict, ref, counts=None, stream=None) -> None:
        """halo_nat_apply_answers_device: the answers (cuda uint8 [k, 16] = NAT_ANSWER_DTYPE) of the
        items ``collect_misses`` listed, written into ``ops`` / ``verdict`` / ``ref`` of every record
        whose ``pos`` is below k. ``counts`` (cuda int32 [6], optional) is incremented per verdict."""
        _lib.check("halo_nat_apply_answers_device", _lib.lib.halo_nat_apply_answers_device(
            direction, _lib.ptr(pos), int(pos.shape[0]), _lib.ptr(answers), int(answers.shape[0]), _lib.ptr(ops),
            _lib.ptr(verdict), _lib.ptr(ref), _lib.ptr(counts), cls._stream(stream)))

    def resolve_misses_device(self, direction: int, records, ops, verdict, ref, now: int, select=None, stream=None):
        """The miss path's round trip on device-resident arrays: collect, read ``count`` (one 4-byte
        synchronising copy; 0 ends the call), download that many items, ``resolve_items`` on the host
        table, upload the answers, apply. ``ops`` / ``verdict`` / ``ref`` end as ``resolve_misses`` over
        host copies would leave them. Returns (n_listed, n_added)."""
        import torch

        items, count, pos = self.collect_misses(direction, records, verdict, select=select, stream=stream)
        s = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(s):
            k = int(count.cpu().numpy().view(np.uint32)[0])
            if k == 0:
                return 0, 0
            host = items[:k].cpu().numpy().reshape(-1).view(NAT_MISS_ITEM_DTYPE)
            answers, added = self.resolve_items(direction, host, now)
            d_answers = torch.from_numpy(answers.view(np.uint8).reshape(k, 16)).to(records.device)
        self.apply_answers(direction, pos, d_answers, ops, verdict, ref, stream=stream)
        return k, added

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
