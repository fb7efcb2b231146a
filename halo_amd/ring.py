"""halo's SPSC packet ring as the receive source of GPU batches.

The reference moves received frames from the DPDK lcore to Go through ``mem.RingBuffer``
(mem/ring_buffer.go:18-352, the Go twin of cgo/ring_buffer.h), and ``engine.Wire``
(engine/engine.go:507-559) is the same ring used as an in-memory link. Its consumer reads one
record per ``ReadPacket`` call into a 1514-byte buffer and ``PacketHandle`` parses it.

* ``RingBuffer`` — ``RingBufferCreate`` over host memory this object owns, and a batch producer
  (``WritePacket`` per frame: ``halo_ring_write_batch``).
* ``RingConsumer`` — ``NewRingBufferConsumer`` + batched ``ReadPacket``: ``poll`` parses every
  frame between the consumer's cursor and the producer's head on the GPU
  (``halo_rx_ring_poll``: raw DMA of the span, record boundaries found on the GPU, parse in
  place, one record per frame), ``commit`` releases them (``tail`` store-release).
* ``Wire`` — ``engine.NewWire`` (an 8 MiB ring) with ``Tx`` and a GPU ``rx_batch``.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _lib
from ._lib import (RESULT_DTYPE, RING_HEADER, RING_PERSISTENT, RING_REGISTER, RING_SCAN_DTYPE, RING_STATS_DTYPE,
                   RING_STOP_NAMES, TXRING_RESULT_DTYPE, NetIf)
from .protocol import flags_word

WIRE_MAX_PACKET_SIZE = 1514  # engine/engine.go:507
MAX_PACKET_SIZE = 1514       # dpdk/dpdk.go:20 (EthQueueRxPkt's receive buffer)


class RingBuffer:
    """A RingBuffer (128-byte header + ``data_size``-byte power-of-two data area) in host memory."""

    def __init__(self, data_size: int = 8 << 20):
        self.mem = _lib.host_array(RING_HEADER + data_size)  # pages of its own: it may be registered
        _lib.check("halo_ring_create", _lib.lib.halo_ring_create(self.mem.ctypes.data, self.mem.nbytes))
        self.size = data_size

    @property
    def head(self) -> int:
        return int(self.mem[0:8].view(np.uint64)[0])

    @property
    def tail(self) -> int:
        return int(self.mem[64:72].view(np.uint64)[0])

    @property
    def data(self) -> np.ndarray:
        return self.mem[RING_HEADER:]

    def write_batch(self, data: np.ndarray, offsets: np.ndarray, lens: np.ndarray,
                    accepted: Optional[np.ndarray] = None) -> int:
        """WritePacket for every frame data[offsets[i]:offsets[i]+lens[i]]; refused frames are
        dropped (accepted[i] = 0). Returns the number written."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint16)
        written = ctypes.c_uint32()
        rc = _lib.lib.halo_ring_write_batch(self.mem.ctypes.data, _lib.ptr(data), _lib.ptr(offsets), _lib.ptr(lens),
                                            lens.shape[0], _lib.ptr(accepted), ctypes.byref(written))
        _lib.check("halo_ring_write_batch", rc)
        return int(written.value)

    def write_span(self, span: np.ndarray):
        """Publish a run of whole records (one port's egress stream, ``EgressResult.stream(p)``)
        with one release store of head: (records written, bytes written) — the longest prefix that
        fits the ring's free space. A malformed span raises and writes nothing."""
        span = np.ascontiguousarray(span, dtype=np.uint8)
        recs, taken = ctypes.c_uint32(), ctypes.c_uint64()
        rc = _lib.lib.halo_ring_write_span(self.mem.ctypes.data, _lib.ptr(span), span.nbytes, ctypes.byref(recs),
                                           ctypes.byref(taken))
        _lib.check("halo_ring_write_span", rc)
        return int(recs.value), int(taken.value)

    def write(self, frames) -> int:
        frames = [bytes(f) for f in frames]
        if not frames:
            return 0
        lens = np.fromiter((len(f) for f in frames), dtype=np.uint16, count=len(frames))
        offs = np.zeros(len(frames), dtype=np.uint64)
        np.cumsum(lens[:-1], out=offs[1:])
        return self.write_batch(np.frombuffer(b"".join(frames) + b"\0", np.uint8), offs, lens)

    def length_at(self, position: int) -> int:
        """The u32 length field of the record at stream position `position`."""
        p = position % self.size  # records are 4-byte aligned: the field never wraps
        return int(self.data[p:p + 4].view(np.uint32)[0])

    def frame_at(self, position: int, length: int) -> bytes:
        """The frame whose record sits at stream position `position` (unwrapped)."""
        start = (position + 4) % self.size
        idx = (start + np.arange(length)) % self.size
        return self.data[idx].tobytes()


class RingConsumer:
    """The GPU consumer of one ring (halo_rx_ring_attach). ``capacity`` is ReadPacket's
    ``len(data)`` (1514 in the DPDK driver and Wire). ``small_poll``: spans up to this many bytes
    take the one-launch small path (None: the library default; 0: always the pipelined path).
    ``persistent``: small polls are served by a resident consumer kernel (HALO_RING_PERSISTENT):
    no launch and no stream synchronisation per poll."""

    def __init__(self, ring: RingBuffer, device: int = 0, capacity: int = MAX_PACKET_SIZE, max_bytes: int = 0,
                 max_frames: int = 0, register: bool = True, small_poll: int | None = None, persistent: bool = False):
        self.ring = ring
        self._out_registered = False
        h = ctypes.c_void_p()
        flags = (RING_REGISTER if register else 0) | (RING_PERSISTENT if persistent else 0)
        rc = _lib.lib.halo_rx_ring_attach(device, ring.mem.ctypes.data, 0, capacity, max_bytes, max_frames, flags,
                                          ctypes.byref(h))
        _lib.check("halo_rx_ring_attach", rc)
        self._h = h
        if small_poll is not None:
            _lib.check("halo_rx_ring_set_small_poll", _lib.lib.halo_rx_ring_set_small_poll(h, small_poll))
        cap = max_bytes or min(ring.size, 256 << 20)
        self.max_frames = min(max_frames or (1 << 32) - 1, min(cap, ring.size) // 8)
        self._out = _lib.host_array(self.max_frames, RESULT_DTYPE)  # registered below: pages of its own
        # the records come back by DMA straight into this array: pin it too
        self._out_registered = register and _lib.lib.halo_rx_host_register(
            self._out.ctypes.data, _lib.host_pages(self._out.nbytes)) == 0

    def close(self):
        """Detach from the ring and unregister the record array. Raises HaloError if either
        registration could not be removed: the memory then stays mapped for the device, so the
        consumer keeps references to both arrays instead of letting them be freed."""
        if getattr(self, "_h", None):
            rc = _lib.lib.halo_rx_ring_detach(self._h)
            self._h = None
            rc2 = _lib.HALO_OK
            if self._out_registered:
                rc2 = _lib.lib.halo_rx_host_unregister(self._out.ctypes.data)
                self._out_registered = False
            if rc != _lib.HALO_OK or rc2 != _lib.HALO_OK:
                _lib._leaked.append((self.ring, self._out))  # still registered: never free them
                _lib.check("halo_rx_ring_detach" if rc != _lib.HALO_OK else "halo_rx_host_unregister",
                           rc if rc != _lib.HALO_OK else rc2)

    def __del__(self):
        self.close()

    def poll(self, netif: NetIf, check_sum_enable: bool = True, jumbo: bool = False, hist=None,
             positions: bool = False):
        """Parse the next frames. Returns (records view, info dict, positions or None); the records
        view is reused by the next poll."""
        info = np.zeros(1, dtype=RING_SCAN_DTYPE)
        pos = np.zeros(self.max_frames, dtype=np.uint64) if positions else None
        rc = _lib.lib.halo_rx_ring_poll(self._h, flags_word(check_sum_enable, jumbo), netif, self._out.ctypes.data,
                                        _lib.ptr(hist), _lib.ptr(pos), info.ctypes.data)
        _lib.check("halo_rx_ring_poll", rc)
        n = int(info["n_frames"][0])
        d = {"n_frames": n, "stop": RING_STOP_NAMES[int(info["stop"][0])], "end_bytes": int(info["end_bytes"][0]),
             "max_len": int(info["max_len"][0])}
        return self._out[:n], d, (pos[:n] if positions else None)

    def commit(self):
        _lib.check("halo_rx_ring_commit", _lib.lib.halo_rx_ring_commit(self._h))

    def set_service_timeout(self, us: int):
        """Bound on one resident request's wait (0 = the default 2 s; fault injection)."""
        _lib.check("halo_rx_ring_set_service_timeout", _lib.lib.halo_rx_ring_set_service_timeout(self._h, us))

    def stats(self) -> dict:
        """halo_rx_ring_get_stats: poll counters and where the small polls' time went."""
        st = np.zeros(1, RING_STATS_DTYPE)
        _lib.check("halo_rx_ring_get_stats", _lib.lib.halo_rx_ring_get_stats(self._h, st.ctypes.data))
        return {k: int(st[k][0]) for k in RING_STATS_DTYPE.names}


class RingProducer:
    """The GPU producer of one ring (halo_tx_ring_attach): ``halo_ring_write_span`` with the span in
    device memory. The device finds the records, reads head and tail, copies what fits into the
    mapped ring and publishes head; the host reads a 24-byte result. ``register=False`` attaches to a
    ring that is already mapped for the device (one a ``RingConsumer`` registered): close the
    producer before that registration goes away. One producer per ring; its writes go to one stream."""

    def __init__(self, ring: RingBuffer, device: int = 0, register: bool = True):
        self.ring, self.device = ring, device
        self._ws = None
        self._retired = []  # outgrown workspaces, kept until close(): earlier writes may still be queued on them
        h = ctypes.c_void_p()
        rc = _lib.lib.halo_tx_ring_attach(device, ring.mem.ctypes.data, 0, RING_REGISTER if register else 0,
                                          ctypes.byref(h))
        if rc == _lib.HALO_E_HIP and register:
            _lib._leaked.append(ring)  # its pages may still be pinned for the device: never free them
        _lib.check("halo_tx_ring_attach", rc)
        self._h = h

    def close(self):
        """Wait for the device's work on the ring and detach. Raises HaloError if the ring could not
        be unregistered: its pages then stay mapped for the device, so the ring is never freed."""
        if getattr(self, "_h", None):
            rc = _lib.lib.halo_tx_ring_detach(self._h)
            self._h = None
            self._ws, self._retired = None, []
            if rc != _lib.HALO_OK:
                _lib._leaked.append(self.ring)
                _lib.check("halo_tx_ring_detach", rc)

    def __del__(self):
        self.close()

    @staticmethod
    def workspace_bytes(span_bytes: int) -> int:
        return int(_lib.lib.halo_tx_ring_workspace(span_bytes))

    def _workspace(self, span_bytes: int, dev):
        import torch

        need = self.workspace_bytes(span_bytes)
        if need == 0:
            raise _lib.HaloError("halo_tx_ring_workspace", _lib.HALO_E_INVAL)
        if self._ws is None or self._ws.numel() < need:
            if self._ws is not None:
                self._retired.append(self._ws)
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return self._ws

    def write_span_async(self, d_span, span_bytes: int | None = None, stream=None, result=None, workspace=None):
        """Enqueue the write of ``d_span[:span_bytes]`` (a cuda uint8 tensor of whole records, 4-byte
        aligned) and return the result tensor (uint8 [24] on the device, ``TXRING_RESULT_DTYPE``
        once the stream has reached it). No synchronisation; writes on one stream chain."""
        import torch

        n = int(d_span.numel() if span_bytes is None else span_bytes)
        if result is None:
            result = torch.empty(24, dtype=torch.uint8, device=d_span.device)
        ws = workspace if workspace is not None else self._workspace(n, d_span.device)
        st = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
        rc = _lib.lib.halo_tx_ring_write_span_device(self._h, _lib.ptr(d_span), n, _lib.ptr(result), _lib.ptr(ws),
                                                     ws.numel() * ws.element_size(), st)
        _lib.check("halo_tx_ring_write_span_device", rc)
        return result

    @staticmethod
    def read_result(result) -> np.ndarray:
        """A result tensor as one TXRING_RESULT_DTYPE record (synchronises)."""
        return result.cpu().numpy().view(TXRING_RESULT_DTYPE)[0]

    def write_span(self, d_span, span_bytes: int | None = None, stream=None):
        """The synchronous convenience: enqueue, synchronise, read the result — (status, records
        taken, bytes taken). After ``TXRING_SHORT`` resubmit ``d_span[bytes:]``."""
        import torch

        res = self.write_span_async(d_span, span_bytes, stream)
        (stream if stream is not None else torch.cuda.current_stream()).synchronize()
        r = self.read_result(res)
        return int(r["status"]), int(r["records"]), int(r["bytes"])


def publish_egress(result, producers, stream=None):
    """Publish every port's stream of a device ``EgressResult`` into its tx ring: one
    ``write_span_async`` per port on ``stream``, then one synchronisation. Returns one
    TXRING_RESULT_DTYPE record per port; after ``TXRING_SHORT`` the caller resubmits
    ``result.device_stream(p)[bytes:]``. Reads the port summaries (a synchronisation of its own:
    span_bytes is a host value)."""
    import torch

    if len(producers) != result.n_ports:
        raise ValueError("one producer per egress port")
    ports = result.ports
    res = [prod.write_span_async(result.device_stream(p), int(ports[p]["bytes_written"]), stream)
           for p, prod in enumerate(producers)]
    (stream if stream is not None else torch.cuda.current_stream()).synchronize()
    return np.array([RingProducer.read_result(r) for r in res], TXRING_RESULT_DTYPE)


class Wire:
    """engine.Wire (engine/engine.go:507-559): a ring with an 8 MiB data area as a virtual link."""

    def __init__(self, device: int = 0, data_size: int = 8 << 20, persistent: bool = False):
        self.ring = RingBuffer(data_size)
        self.consumer = RingConsumer(self.ring, device=device, capacity=WIRE_MAX_PACKET_SIZE, persistent=persistent)

    def Tx(self, pkt: bytes) -> None:  # engine/engine.go:548-553
        if len(pkt) == 0 or len(pkt) > WIRE_MAX_PACKET_SIZE:
            return
        self.ring.write([pkt])

    def rx_batch(self, netif: NetIf, check_sum_enable: bool = True):
        """Every frame Wire.Rx would return until it returns nil, parsed: (records, frames)."""
        recs, info, pos = self.consumer.poll(netif, check_sum_enable, positions=True)
        frames = [self.ring.frame_at(int(p), self.ring.length_at(int(p))) for p in pos]
        out = recs.copy()
        self.consumer.commit()
        return out, frames

    def Destroy(self):
        self.consumer.close()
