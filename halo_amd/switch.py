"""Batch mirror of an ``engine.Switch`` (include/halo_rx.h, "L2 switch").

``forward`` runs ``SwitchPort.RxEthernet / HandleEthernet`` (engine/ethernet_engine.go:58-114) over
one batch of frames from one ingress port — MAC learning and the unicast / flood decision, in the
reference's frame order — ``expire`` is one ``SwitchMacAddrClear`` tick and ``ListSwitchMacAddr``
lists the table. With ``device=None`` the switch is a host switch (numpy arrays, the sequential
loop in C); with a device index the table lives in HBM and ``forward`` takes cuda tensors and is
asynchronous on the current stream. Calls on one switch go on one stream.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import SW_ENTRY_DTYPE, SW_LAYOUT_DTYPE, SW_RESULT_DTYPE, SW_V, SW_V_COUNT, SW_VERDICT_NAMES  # noqa: F401


class Switch:
    def __init__(self, vlan_ids, capacity: int, max_batch: int = 1 << 16, slots_log2: int = 0,
                 device: int | None = None):
        self._s = None  # before anything can raise: __del__ closes
        cfg = _lib.SwitchConfig()
        cfg.n_ports = len(vlan_ids)
        for q, vid in enumerate(list(vlan_ids)[:_lib.SW_MAX_PORTS]):
            cfg.vlan_id[q] = vid
        cfg.capacity, cfg.slots_log2, cfg.max_batch = capacity, slots_log2, max_batch
        cfg.device = -1 if device is None else device
        h = ctypes.c_void_p()
        _lib.check("halo_switch_create", _lib.lib.halo_switch_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._s = h
        self.n_ports, self.capacity, self.max_batch, self.device = cfg.n_ports, capacity, max_batch, device

    def close(self):
        if self._s:
            _lib.lib.halo_switch_destroy(self._s)
            self._s = None

    def __del__(self):
        self.close()

    def flood_mask(self, port: int) -> int:
        m = ctypes.c_uint64()
        _lib.check("halo_switch_flood_mask", _lib.lib.halo_switch_flood_mask(self._s, port, ctypes.byref(m)))
        return int(m.value)

    def forward(self, port: int, data, offsets_dw, lens, now: int, results=None, counts=None, stream=None):
        """One batch from ingress ``port`` at ``now``. Host switch: numpy uint8 bytes, uint32 dword
        offsets, uint16 lengths; returns (results as SW_RESULT_DTYPE, counts u32 [6]). Device
        switch: cuda tensors (uint8 bytes, int32 offsets, int16 lengths); returns (results uint8
        [n, 4], counts int32 [6]) — device tensors, asynchronous. ``counts`` is incremented."""
        n = int(lens.shape[0])
        if self.device is None:
            assert data.dtype == np.uint8 and offsets_dw.dtype == np.uint32 and lens.dtype == np.uint16
            if results is None:
                results = np.zeros(n, SW_RESULT_DTYPE)
            if counts is None:
                counts = np.zeros(SW_V_COUNT, np.uint32)
            s = None
        else:
            import torch

            if results is None:
                results = torch.empty((n, 4), dtype=torch.uint8, device=data.device)
            if counts is None:
                counts = torch.zeros(SW_V_COUNT, dtype=torch.int32, device=data.device)
            s = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
        _lib.check("halo_switch_forward", _lib.lib.halo_switch_forward(
            self._s, port, _lib.ptr(data), _lib.ptr(offsets_dw), _lib.ptr(lens), n, now & 0xFFFFFFFF,
            _lib.ptr(results), _lib.ptr(counts), s))
        return results, counts

    def expire(self, now: int) -> int:
        """One SwitchMacAddrClear tick: the number of entries removed. Synchronous."""
        n = ctypes.c_uint32()
        _lib.check("halo_switch_expire", _lib.lib.halo_switch_expire(self._s, now & 0xFFFFFFFF, ctypes.byref(n)))
        return int(n.value)

    def ListSwitchMacAddr(self, cap: int | None = None) -> np.ndarray:  # noqa: N802
        n = ctypes.c_uint32()
        _lib.check("halo_switch_list", _lib.lib.halo_switch_list(self._s, None, 0, ctypes.byref(n)))
        cap = n.value if cap is None else cap
        out = np.zeros(max(cap, 1), SW_ENTRY_DTYPE)
        _lib.check("halo_switch_list", _lib.lib.halo_switch_list(self._s, _lib.ptr(out), cap, ctypes.byref(n)))
        return out[:min(cap, n.value)]

    def debug_set_epoch(self, epoch: int) -> None:
        """Testing only (halo_switch_debug_set_epoch): move a device switch next to its epoch wrap."""
        _lib.check("halo_switch_debug_set_epoch", _lib.lib.halo_switch_debug_set_epoch(self._s, epoch))

    def layout_stats(self) -> np.ndarray:
        out = np.zeros(1, SW_LAYOUT_DTYPE)
        _lib.check("halo_switch_layout_stats", _lib.lib.halo_switch_layout_stats(self._s, _lib.ptr(out)))
        return out[0]
