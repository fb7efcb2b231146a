"""GPU: the lane kernel's staged, masked record stores under any store policy (plain, non-temporal
or write-through: store16 in rx_frame.h) — bit-exact records vs the C oracle at
the window edges, at every alignment of ``out``, across dependent launches into one ``out``, as
seen by every kind of consumer, in looping waves and through the other entry points that share
the window code. Nothing here depends on which policy the library was built with: a policy may
change when bytes reach memory, never which bytes.
"""
from __future__ import annotations

import numpy as np
import pytest

from tests.helpers import assert_records_equal, strip_ethernet

pytestmark = pytest.mark.gpu

NS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 8193)  # store masks switch at 2*nrec = 64 / nrec
GUARD = 4096
FILL = 0xA5


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


class Batch:
    """8193 synthetic 64 B frames on the device and the oracle's records for them (computed once;
    frames are independent, so the first n frames' records are the first n records)."""

    def __init__(self, dev, oracle_lib, first_index):
        from halo_amd import synth
        from halo_amd._lib import NetIf

        self.n = max(NS)
        self.lay = synth.layout(self.n, length=64, proto_mode=3, mutate_shift=3, first_index=first_index)
        self.fr = synth.frames_device(self.lay, NetIf.make(), device=dev)
        self.host = self.fr["bytes"].cpu().numpy()
        self.want, self.whist = oracle_lib.rx_batch(self.host, self.lay["lens"], oracle_lib.NetIf.make(), 1,
                                                    offsets_dw=self.lay["offsets_dw"], threads=8)
        assert self.whist[1:].sum() > 0  # some frames are rejected: the records are not all alike
        self.want.setflags(write=False)

    def args(self):
        from halo_amd import _lib

        return _lib.ptr(self.fr["bytes"]), _lib.ptr(self.fr["offsets_dw"]), _lib.ptr(self.fr["lens"])


@pytest.fixture(scope="module")
def batch(dev, oracle_lib):
    return Batch(dev, oracle_lib, 6_000_000)


@pytest.fixture(scope="module")
def batch2(dev, oracle_lib):
    return Batch(dev, oracle_lib, 9_000_000)


def _lane_parse(b, n, out_ptr, *, compact=False, hist=None, stream=None):
    """The first n frames of b through the lane kernel (variant 1) into the device address out_ptr."""
    import torch

    from halo_amd import _lib
    from halo_amd._lib import NetIf

    flags = 1 | _lib.variant_flags(1) | (_lib.HALO_RX_RECORD_COMPACT if compact else 0)
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = _lib.lib.halo_rx_parse_batch_device(*b.args(), n, flags, NetIf.make(), 64, out_ptr, _lib.ptr(hist),
                                             s.cuda_stream)
    _lib.check("halo_rx_parse_batch_device", rc)


def _want_bytes(b, n, compact):
    from halo_amd._lib import compact_of

    w = compact_of(b.want[:n]) if compact else b.want[:n]
    return np.ascontiguousarray(w).view(np.uint8).reshape(-1)


@pytest.mark.parametrize("compact", [False, True], ids=["rec32", "rec16"])
@pytest.mark.parametrize("align", [0, 16, 32, 112])
def test_window_edges_alignment_and_guards(dev, batch, compact, align):
    """Every n around the store masks' switch points, ``out`` starting `align` bytes past a 128-byte
    boundary (16-byte alignment is all the header asks for, so the 1 KB store rows straddle lines):
    records == the oracle's, and the 4 KB before and after ``out`` keep their fill."""
    import torch

    width = 16 if compact else 32
    buf = torch.empty(GUARD + 128 + max(NS) * width + GUARD, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 128 == 0
    start = GUARD + align
    for n in NS:
        buf.fill_(FILL)
        _lane_parse(batch, n, buf.data_ptr() + start, compact=compact)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        end = start + n * width
        bad = np.nonzero(got[start:end] != _want_bytes(batch, n, compact))[0]
        assert bad.size == 0, (n, compact, align, "first differing record", int(bad[0]) // width)
        assert np.all(got[:start] == FILL), (n, compact, align, "bytes before out written")
        assert np.all(got[end:] == FILL), (n, compact, align, "bytes after out written")


def test_dependent_launches_into_one_out(dev, batch, batch2):
    """Two different 129-frame batches parsed back to back on one stream into the same ``out`` (the
    benchmark's pattern): the second batch's records stand."""
    import torch

    from halo_amd import protocol

    n = 129
    assert batch.want[:n].tobytes() != batch2.want[:n].tobytes()
    out = torch.full((n, 32), FILL, dtype=torch.uint8, device=dev)
    _lane_parse(batch, n, out.data_ptr())
    _lane_parse(batch2, n, out.data_ptr())
    torch.cuda.synchronize()
    assert_records_equal(protocol.records(out), batch2.want[:n], None, "second of two dependent launches")


def test_visible_to_device_to_host_copy(dev, batch):
    """(a) a device-to-host copy queued straight behind the launch, no synchronisation between."""
    import torch

    from halo_amd import protocol

    n = batch.n
    out = torch.full((n, 32), FILL, dtype=torch.uint8, device=dev)
    host = torch.empty((n, 32), dtype=torch.uint8).pin_memory()
    _lane_parse(batch, n, out.data_ptr())
    host.copy_(out, non_blocking=True)
    torch.cuda.synchronize()
    assert_records_equal(protocol.records(host), batch.want, None, "device-to-host copy behind the launch")


def test_visible_to_flow_hash_on_same_stream(dev, oracle_lib, batch):
    """(b) halo_flow_hash_device over the records on the same stream == the oracle's hashes."""
    import torch

    from halo_amd import hashcode

    n = batch.n
    out = torch.full((n, 32), FILL, dtype=torch.uint8, device=dev)
    _lane_parse(batch, n, out.data_ptr())
    h, b = hashcode.flow_hash(out, 1, 0, 1 << 20)
    torch.cuda.synchronize()
    wh, wb = oracle_lib.flow_hash_batch(np.array(batch.want), 1, 0, 1 << 20)
    assert np.array_equal(h.cpu().numpy().view(np.uint64), wh)
    assert np.array_equal(b.cpu().numpy().view(np.uint32), wb)


def test_visible_to_reader_on_second_stream(dev, batch):
    """(c) a reader kernel on a second stream behind an event wait (its waves read on every XCD)."""
    import torch

    from halo_amd import protocol

    n = batch.n
    out = torch.full((n, 32), FILL, dtype=torch.uint8, device=dev)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    done = torch.cuda.Event()
    _lane_parse(batch, n, out.data_ptr(), stream=s1)
    done.record(s1)
    with torch.cuda.stream(s2):
        s2.wait_event(done)
        copy = out.clone()
    torch.cuda.synchronize()
    assert_records_equal(protocol.records(copy), batch.want, None, "reader on a second stream")


@pytest.mark.parametrize("compact", [False, True], ids=["rec32", "rec16"])
def test_looping_waves_with_histogram(dev, batch, compact):
    """With the status histogram the grid is halved: at n = 8193 a wave runs two windows through one
    LDS staging area. Records and histogram exact."""
    import torch

    n = batch.n
    width = 16 if compact else 32
    out = torch.full((n * width,), FILL, dtype=torch.uint8, device=dev)
    hist = torch.zeros(14, dtype=torch.int32, device=dev)
    _lane_parse(batch, n, out.data_ptr(), compact=compact, hist=hist)
    torch.cuda.synchronize()
    bad = np.nonzero(out.cpu().numpy() != _want_bytes(batch, n, compact))[0]
    assert bad.size == 0, ("first differing record", int(bad[0]) // width)
    assert np.array_equal(hist.cpu().numpy().astype(np.int64), batch.whist.astype(np.int64))


def test_multi_batch_entry(dev, batch, batch2):
    """halo_rx_parse_batches_device: three batches of 65, 1 and 129 frames in one launch."""
    import torch

    from halo_amd import protocol
    from halo_amd._lib import NetIf

    specs = [(batch, 65), (batch2, 1), (batch, 129)]
    outs = [torch.full((n, 32), FILL, dtype=torch.uint8, device=dev) for _, n in specs]
    hist = torch.zeros(14, dtype=torch.int32, device=dev)
    protocol.parse_frames_batches([(b.fr["bytes"], b.fr["offsets_dw"][:n], b.fr["lens"][:n], o)
                                   for (b, n), o in zip(specs, outs)], netif=NetIf.make(), max_len_hint=64,
                                  variant=1, hist=hist)
    torch.cuda.synchronize()
    want_hist = np.zeros(14, np.int64)
    for k, ((b, n), o) in enumerate(zip(specs, outs)):
        assert_records_equal(protocol.records(o), b.want[:n], None, f"multi-batch, batch {k}")
        want_hist += np.bincount(b.want[:n]["status"], minlength=14)
    assert np.array_equal(hist.cpu().numpy().astype(np.int64), want_hist)


def test_l3_start_entry(dev, oracle_lib, batch):
    """parse_ipv4_packets_batch (HALO_RX_L3_START) at n = 65: the frames' Ethernet payloads."""
    import torch

    from halo_amd import protocol
    from halo_amd._lib import HALO_RX_L3_START, NetIf

    n = 65
    pk, poffs, plens = strip_ethernet(batch.host, batch.lay["offsets_dw"][:n], batch.lay["lens"][:n])
    plens = plens.astype(np.uint16)
    want, _ = oracle_lib.rx_batch(pk, plens, oracle_lib.NetIf.make(), 1 | HALO_RX_L3_START,
                                  offsets_dw=poffs.astype(np.uint32))
    out = torch.full((n, 32), FILL, dtype=torch.uint8, device=dev)
    protocol.parse_ipv4_packets_batch(torch.from_numpy(pk).to(dev),
                                      torch.from_numpy(poffs.astype(np.uint32).view(np.int32)).to(dev),
                                      torch.from_numpy(plens.view(np.int16)).to(dev), netif=NetIf.make(),
                                      max_len_hint=64, variant=1, out=out)
    torch.cuda.synchronize()
    assert_records_equal(protocol.records(out), want, None, "L3-start entry")


def test_fused_flow_entry(dev, oracle_lib, batch):
    """halo_rx_parse_flow_batch_device at n = 129: records and the hashes of those records."""
    import torch

    from halo_amd import _lib, protocol
    from halo_amd._lib import NetIf

    n = 129
    out = torch.full((n, 32), FILL, dtype=torch.uint8, device=dev)
    h = torch.zeros(n, dtype=torch.int64, device=dev)
    b = torch.zeros(n, dtype=torch.int32, device=dev)
    _lib.check("fused", _lib.lib.halo_rx_parse_flow_batch_device(
        *batch.args(), n, 1 | _lib.variant_flags(1), NetIf.make(), 64, out.data_ptr(), None, 1, 0, h.data_ptr(),
        1 << 20, b.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert_records_equal(protocol.records(out), batch.want[:n], None, "fused parse + flow hash")
    wh, wb = oracle_lib.flow_hash_batch(np.array(batch.want[:n]), 1, 0, 1 << 20)
    assert np.array_equal(h.cpu().numpy().view(np.uint64), wh)
    assert np.array_equal(b.cpu().numpy().view(np.uint32), wb)
