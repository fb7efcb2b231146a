"""The egress step (include/halo_rx.h, "egress"): the forward path's last stage.

A batch that ``ArpTable.encap`` or ``Switch.forward`` has decided on is partitioned, stably, into
one contiguous byte stream per egress port, each frame laid out as one ring record (u32 length
``max(len, 60)``, the bytes, ``BuildEthFrm``'s zero padding, zeros to the next 4-byte boundary), so
that ``RingBuffer.write_span`` publishes a port's stream into its tx ring in one call.

* ``egress_arp`` / ``egress_switch`` / ``egress_masks`` — over cuda tensors, asynchronous on the
  stream (three launches, no host round trip).
* ``egress_host`` — the sequential loop over numpy arrays, for polls at the reference's cadence.

Both return an ``EgressResult``: ``.ports`` (EGRESS_PORT_DTYPE), ``.stream(p)``, ``.index(p)``.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import (EGRESS_KIND_ARP, EGRESS_KIND_MASKS, EGRESS_KIND_SWITCH, EGRESS_MAX_PORTS,  # noqa: F401
                   EGRESS_PORT_DTYPE, HALO_RX_JUMBO_EXT)


def tx_len(length: int) -> int:
    return max(int(length), 60)


def record_size(length: int) -> int:
    """ringBufferRecordSize(tx_len)."""
    return (4 + tx_len(length) + 3) & ~3


class EgressResult:
    """What one egress call wrote. ``out`` is the whole output buffer (uint8 [n_ports *
    region_bytes]), ``ports_raw`` the summaries, ``index_raw`` the index lists ([n_ports, index_cap]
    or None) and ``skipped`` the counter; device results hold cuda tensors and copy on access."""

    def __init__(self, n_ports, region_bytes, index_cap, out, ports_raw, index_raw, skipped):
        self.n_ports, self.region_bytes, self.index_cap = n_ports, region_bytes, index_cap
        self.out, self.ports_raw, self.index_raw, self.skipped = out, ports_raw, index_raw, skipped
        self._ports = None

    @staticmethod
    def _host(x) -> np.ndarray:
        return x.cpu().numpy() if hasattr(x, "cpu") else x

    @property
    def ports(self) -> np.ndarray:
        """The n_ports summaries as EGRESS_PORT_DTYPE (synchronises a device result)."""
        if self._ports is None:
            self._ports = self._host(self.ports_raw).reshape(-1).view(np.uint8).view(EGRESS_PORT_DTYPE).copy()
        return self._ports

    @property
    def n_skipped(self) -> int:
        return int(self._host(self.skipped).reshape(-1).view(np.uint32)[0])

    def stream(self, p: int) -> np.ndarray:
        """Port p's written records: uint8 [bytes_written], host memory."""
        lo = p * self.region_bytes
        return np.ascontiguousarray(self._host(self.out[lo:lo + int(self.ports[p]["bytes_written"])]))

    def device_stream(self, p: int):
        """The same as a view of ``out`` (a cuda tensor for a device result)."""
        lo = p * self.region_bytes
        return self.out[lo:lo + int(self.ports[p]["bytes_written"])]

    def index(self, p: int) -> np.ndarray:
        """The batch indices of port p's first min(frames, index_cap) records: uint32."""
        k = min(int(self.ports[p]["frames"]), self.index_cap)
        if k == 0 or self.index_raw is None:
            return np.zeros(0, np.uint32)
        return self._host(self.index_raw[p, :k]).view(np.uint32).copy()


def _config(n_ports, region_bytes, index_cap, jumbo):
    cfg = _lib.EgressConfig()
    cfg.n_ports, cfg.flags = n_ports, HALO_RX_JUMBO_EXT if jumbo else 0
    cfg.region_bytes, cfg.index_cap = region_bytes, index_cap
    return cfg


def workspace_bytes(n: int, n_ports: int) -> int:
    return int(_lib.lib.halo_tx_egress_workspace(n, n_ports))


def _device_outputs(dev, n_ports, region_bytes, wsb, out, skipped, workspace):
    """What a per-port stream call on the device (here and in ``loopback.gather``) allocates when not
    given: (out, the 24-byte summaries, skipped, workspace, the workspace's bytes)."""
    import torch

    if out is None:
        out = torch.empty(max(n_ports * region_bytes, 16), dtype=torch.uint8, device=dev)
    ports = torch.empty((n_ports, 24), dtype=torch.uint8, device=dev)
    if skipped is None:
        skipped = torch.zeros(1, dtype=torch.int32, device=dev)
    if workspace is None:
        workspace = torch.empty(max(wsb, 8) // 8, dtype=torch.int64, device=dev)
    return out, ports, skipped, workspace, workspace.numel() * workspace.element_size()


def _device(kind, data, offsets_dw, lens, selectors, n_ports, region_bytes, index_cap, jumbo, flood_mask, out, workspace,
            skipped, stream, index=None):
    import ctypes

    import torch

    n = int(lens.shape[0])
    cfg = _config(n_ports, region_bytes, index_cap, jumbo)
    out, ports, skipped, workspace, ws_bytes = _device_outputs(data.device, n_ports, region_bytes, workspace_bytes(n, n_ports),
                                                               out, skipped, workspace)
    if index is None and index_cap:
        index = torch.empty((n_ports, index_cap), dtype=torch.int32, device=data.device)
    st = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
    args = [ctypes.byref(cfg), _lib.ptr(data), _lib.ptr(offsets_dw), _lib.ptr(lens), n, _lib.ptr(selectors)]
    if kind == EGRESS_KIND_SWITCH:
        args.append(flood_mask)
    args += [_lib.ptr(out), _lib.ptr(ports), _lib.ptr(index), _lib.ptr(skipped), _lib.ptr(workspace), ws_bytes, st]
    name = ("halo_tx_egress_masks_device", "halo_tx_egress_arp_device", "halo_tx_egress_switch_device")[kind]
    _lib.check(name, getattr(_lib.lib, name)(*args))
    return EgressResult(n_ports, region_bytes, index_cap, out, ports, index, skipped)


def egress_masks(data, offsets_dw, lens, masks, n_ports: int, region_bytes: int, index_cap: int = 0, jumbo: bool = False,
                 out=None, workspace=None, skipped=None, stream=None, index=None) -> EgressResult:
    """Cuda tensors: uint8 bytes, int32 dword offsets, int16 lengths, int64 masks (bit p: port p).
    ``out`` (uint8, n_ports * region_bytes, 16-byte aligned), ``workspace`` (``workspace_bytes``) and
    ``skipped`` (int32 [1], incremented) and ``index`` (int32 [n_ports, index_cap]) are allocated when
    not given."""
    return _device(EGRESS_KIND_MASKS, data, offsets_dw, lens, masks, n_ports, region_bytes, index_cap, jumbo, 0, out,
                   workspace, skipped, stream, index)


def egress_arp(data, offsets_dw, lens, results, n_ports: int, region_bytes: int, index_cap: int = 0,
               jumbo: bool = False, out=None, workspace=None, skipped=None, stream=None, index=None) -> EgressResult:
    """After ``ArpTable.encap`` on the same stream; ``results`` is its uint8 [n, 8] tensor. A HIT
    goes to its out NetIf, every other verdict nowhere."""
    return _device(EGRESS_KIND_ARP, data, offsets_dw, lens, results, n_ports, region_bytes, index_cap, jumbo, 0, out,
                   workspace, skipped, stream, index)


def egress_switch(data, offsets_dw, lens, results, flood_mask: int, n_ports: int, region_bytes: int, index_cap: int = 0,
                  jumbo: bool = False, out=None, workspace=None, skipped=None, stream=None, index=None) -> EgressResult:
    """After ``Switch.forward`` (a device switch) on the same stream; ``results`` is its uint8
    [n, 4] tensor and ``flood_mask`` the switch's flood mask of the batch's ingress port."""
    return _device(EGRESS_KIND_SWITCH, data, offsets_dw, lens, results, n_ports, region_bytes, index_cap, jumbo,
                   flood_mask, out, workspace, skipped, stream, index)


def egress_host(kind: int, data: np.ndarray, offsets_dw: np.ndarray, lens: np.ndarray, selectors: np.ndarray, n_ports: int,
                region_bytes: int, index_cap: int = 0, jumbo: bool = False, flood_mask: int = 0, out=None,
                skipped=None) -> EgressResult:
    """``halo_tx_egress_host`` over numpy arrays: ``selectors`` is uint64 masks, ARP_RESULT_DTYPE or
    SW_RESULT_DTYPE records according to ``kind`` (EGRESS_KIND_*)."""
    import ctypes

    data = np.ascontiguousarray(data, np.uint8)
    offsets_dw = np.ascontiguousarray(offsets_dw, np.uint32)
    lens = np.ascontiguousarray(lens, np.uint16)
    selectors = np.ascontiguousarray(selectors)
    n = int(lens.shape[0])
    cfg = _config(n_ports, region_bytes, index_cap, jumbo)
    if out is None:
        out = np.zeros(max(n_ports * region_bytes, 1), np.uint8)
    ports = np.zeros(n_ports, EGRESS_PORT_DTYPE)
    index = np.zeros((n_ports, index_cap), np.uint32) if index_cap else None
    if skipped is None:
        skipped = np.zeros(1, np.uint32)
    _lib.check("halo_tx_egress_host", _lib.lib.halo_tx_egress_host(
        ctypes.byref(cfg), kind, _lib.ptr(data), _lib.ptr(offsets_dw), _lib.ptr(lens), n, _lib.ptr(selectors), flood_mask,
        _lib.ptr(out), _lib.ptr(ports), _lib.ptr(index), _lib.ptr(skipped)))
    return EgressResult(n_ports, region_bytes, index_cap, out, ports, index, skipped)
