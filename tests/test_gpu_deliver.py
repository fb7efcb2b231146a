"""GPU: local delivery on the device (halo_amd/csrc/rx_deliver.hip through halo_amd.deliver)
against tests/deliver_model.py, which works from frame bytes, and against the host loop — stream
bytes, summary and index bit for bit, every output 0xA5-prefilled with a sentinel element behind it
and the workspace's sentinel intact: the crafted frames of tests/deliver_cases.py as frames and as
LoChan packets (every data-offset nibble, so every source alignment; the jumbo payload); random
batches at the sizes around a wavefront and a tile with no delivery, sparse ones, one on each side
of every wave and tile boundary, and all; the region cut inside a tile and exactly on a tile
boundary, `index_cap` below the count and one workspace used by two calls on one stream; records
that overrun their frames; a batch past the tile and the scan pass; the read contract (gaps and tail bytes marked, the marker absent
from the output); and one chain from a ring span in HBM to the handlers."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import deliver_cases as C
from tests import deliver_model as DM

pytestmark = pytest.mark.gpu
FILL = C.FILL
A5_64 = int(np.array([0xA5A5A5A5A5A5A5A5], np.uint64).view(np.int64)[0])


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


def _t(dev, a, dtype=None):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dtype) if dtype is not None else a).to(dev)


def _maps(dev, udp, tcp):
    from halo_amd.deliver import port_map

    return (None if udp is None else _t(dev, port_map(udp), np.int32), None if tcp is None else _t(dev, port_map(tcp), np.int32))


def _device(dev, d, o, ln, recs, nat_enable, region, index_cap, *, udp=C.UDP_SERVED, tcp=C.TCP_SERVED, l3=False, dhcp=True,
            ws=None):
    """halo_rx_deliver_device into 0xA5-filled device outputs, straight through ctypes: the raw
    arrays downloaded, as tests/deliver_cases.check_outputs takes them. Everything but the region
    and the cap is a cuda tensor."""
    import torch

    from halo_amd import _lib

    n = int(ln.shape[0])
    out = torch.full((region + 16,), FILL, dtype=torch.uint8, device=dev)
    summary = torch.full((6,), A5_64, dtype=torch.int64, device=dev)
    index = torch.full((index_cap + 1,), A5_64, dtype=torch.int64, device=dev)
    wsb = int(_lib.lib.halo_rx_deliver_workspace(n))
    if ws is None:
        ws = torch.full((wsb // 8 + 1,), A5_64, dtype=torch.int64, device=dev)
    um, tm = _maps(dev, udp, tcp)
    cfg = _lib.DeliverConfig()
    cfg.flags = (_lib.HALO_RX_L3_START if l3 else 0) | (_lib.HALO_DELIVER_DHCP if dhcp else 0)
    cfg.index_cap, cfg.region_bytes = index_cap, region
    rc = _lib.lib.halo_rx_deliver_device(ctypes.byref(cfg), _lib.ptr(d), _lib.ptr(o), _lib.ptr(ln), _lib.ptr(recs), n,
                                         C.lib_netif(nat_enable), _lib.ptr(um), _lib.ptr(tm), _lib.ptr(out), _lib.ptr(summary),
                                         _lib.ptr(index) if index_cap else None, _lib.ptr(ws), wsb,
                                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert int(ws[-1].item()) == A5_64, "the workspace was overrun"  # its last element is the sentinel
    return dict(out=out.cpu().numpy(), summary=summary.cpu().numpy().view(np.uint8),
                index=index.cpu().numpy().view(np.uint8).reshape(-1, 8), region=region, index_cap=index_cap)


def _same_as_host(o, data, offs, lens, recs_h, nat_enable, **kw):
    """The host loop over the same inputs wrote the same stream, summary and index."""
    from halo_amd.deliver import deliver_host, port_map

    maps = {k: None if kw.get(k, dflt) is None else port_map(kw.get(k, dflt))
            for k, dflt in (("udp", C.UDP_SERVED), ("tcp", C.TCP_SERVED))}
    r = deliver_host(data, offs, lens, recs_h, netif=C.lib_netif(nat_enable), region_bytes=o["region"], udp_ports=maps["udp"],
                     tcp_ports=maps["tcp"], index_cap=o["index_cap"], l3_start=kw.get("l3", False), dhcp=kw.get("dhcp", True))
    assert np.array_equal(r.summary_raw, o["summary"][:40])
    w = r.bytes_written
    assert np.array_equal(r.out[:w], o["out"][:w])
    k = min(int(r.summary["records"]), o["index_cap"])
    if k:
        assert np.array_equal(r.index_raw[:k], o["index"][:k])


def _parse(dev, data, offs, lens, nat_enable, *, l3=False, jumbo=False):
    """(cuda bytes, offsets, lengths, records) of a batch: the records are the device parse's."""
    from halo_amd import protocol

    d, o, ln = _t(dev, data), _t(dev, offs, np.int32), _t(dev, lens, np.int16)
    fn = protocol.parse_ipv4_packets_batch if l3 else protocol.parse_frames_batch
    return d, o, ln, fn(d, o, ln, netif=C.lib_netif(nat_enable), jumbo=jumbo)


@pytest.mark.parametrize("l3", [False, True], ids=["frames", "lo_packets"])
@pytest.mark.parametrize("jumbo", [False, True], ids=["std", "jumbo"])
def test_crafted_set_matches_model_and_host(dev, l3, jumbo):
    cases = C.crafted(jumbo)
    frames = [f for _, f in (C.as_lo_packets(cases) if l3 else cases)]
    data, offs, lens = C.pack(21, frames)
    for nat_enable, dhcp in ((False, True), (False, False), (True, True)):
        nif = C.model_netif(nat_enable)
        want = DM.want_of(frames, nif, jumbo=jumbo, l3=l3, udp_ports=C.UDP_SERVED, tcp_ports=C.TCP_SERVED, dhcp=dhcp)
        d, o, ln, recs = _parse(dev, data, offs, lens, nat_enable, l3=l3, jumbo=jumbo)
        recs_h = C.records(frames, nif, jumbo=jumbo, l3=l3)
        assert np.array_equal(recs.cpu().numpy().reshape(-1), recs_h.view(np.uint8).reshape(-1))
        region = (want.total_bytes + 15) & ~15
        got = _device(dev, d, o, ln, recs, nat_enable, region, len(want.recs) + 2, l3=l3, dhcp=dhcp)
        C.check_outputs(got, want, (nat_enable, dhcp))
        _same_as_host(got, data, offs, lens, recs_h, nat_enable, l3=l3, dhcp=dhcp)
    assert want.kind_counts[DM.DHCP] == (0 if l3 else 2)
    # each map absent
    nif = C.model_netif()
    d, o, ln, recs = _parse(dev, data, offs, lens, False, l3=l3, jumbo=jumbo)
    for udp, tcp in ((None, C.TCP_SERVED), (C.UDP_SERVED, None), (None, None)):
        want = DM.want_of(frames, nif, jumbo=jumbo, l3=l3, udp_ports=udp or (), tcp_ports=tcp or (), dhcp=True)
        got = _device(dev, d, o, ln, recs, False, 1 << 16, 64, udp=udp, tcp=tcp, l3=l3)
        C.check_outputs(got, want, (udp, tcp))


@pytest.mark.parametrize("density", C.DENSITIES)
@pytest.mark.parametrize("n", C.SIZES)
def test_random_batches_match_model_and_host(dev, n, density):
    frames = C.batch(700 + n, n, density)
    nif = C.model_netif()
    want = DM.want_of(frames, nif, udp_ports=C.UDP_SERVED, tcp_ports=C.TCP_SERVED)
    assert {"none": len(want.recs) == 0, "all": len(want.recs) == n}.get(density, 0 < len(want.recs) <= n)
    data, offs, lens = C.pack(n, frames)
    d, o, ln, recs = _parse(dev, data, offs, lens, False)
    region = (want.total_bytes + 15) & ~15
    got = _device(dev, d, o, ln, recs, False, region, n)
    C.check_outputs(got, want, (n, density))
    _same_as_host(got, data, offs, lens, recs.cpu().numpy(), False)


def test_records_that_overrun_their_frames_are_skipped(dev):
    """Records that are not their frames' (payload_off + payload_len > lens[i]) on both sides of the
    wave and tile boundaries: counted in `skipped`, delivered nowhere, and the rest unchanged."""
    n, bad = 300, (0, 63, 64, 255, 256, 299)
    frames = C.batch(41, n, "all")
    nif = C.model_netif()
    good = DM.want_of(frames, nif, udp_ports=C.UDP_SERVED, tcp_ports=C.TCP_SERVED)
    want = DM.Want([it for it in good.items if it[0] not in bad], skipped=len(bad))
    data, offs, lens = C.pack(41, frames)
    recs_h = C.records(frames, nif)
    for i in bad:
        recs_h[i]["payload_len"] = int(lens[i]) - int(recs_h[i]["payload_off"]) + 1 + (i % 3) * 700
    d, o, ln = _t(dev, data), _t(dev, offs, np.int32), _t(dev, lens, np.int16)
    got = _device(dev, d, o, ln, _t(dev, recs_h.view(np.uint8).reshape(-1, 32)), False, (want.total_bytes + 15) & ~15, n)
    C.check_outputs(got, want)
    _same_as_host(got, data, offs, lens, recs_h, False)


def _uniform(dev, n, deliver_at, **other_at):
    templates, tid, data, offs, lens = C.uniform_batch(n, deliver_at, **other_at)
    nif = C.model_netif()
    want = C.uniform_want(templates, tid, nif, udp_ports=C.UDP_SERVED, tcp_ports=C.TCP_SERVED, dhcp=True)
    recs_h = C.uniform_records(templates, tid, nif)
    d, o, ln = _t(dev, data), _t(dev, offs, np.int32), _t(dev, lens, np.int16)
    return want, data, offs, lens, recs_h, (d, o, ln, _t(dev, recs_h.view(np.uint8).reshape(-1, 32)))


def test_region_cuts_index_cap_and_one_workspace_for_two_calls(dev):
    """600 frames, all delivered, 48-byte records: a tile is 256 records = 12,288 bytes."""
    import torch

    from halo_amd import _lib

    n = 600
    want, data, offs, lens, recs_h, batch = _uniform(dev, n, np.arange(n))
    assert {len(r) for r in want.recs} == {48} and want.total_bytes == 48 * n
    for region, what in ((48 * 100, "inside tile 0"), (48 * 256, "on the tile boundary"), (48 * 256 + 16, "just past it"),
                         (48 * 300, "inside tile 1"), (48 * 512, "on the second boundary"), (0, "nothing fits")):
        for cap in (0, 257, n + 1):
            got = _device(dev, *batch, False, region, cap)
            C.check_outputs(got, want, (what, cap))
            _same_as_host(got, data, offs, lens, recs_h, False)
    # one workspace, two calls on one stream, the second over a shorter batch with other tiles
    wsb = int(_lib.lib.halo_rx_deliver_workspace(n))
    ws = torch.full((wsb // 8 + 1,), A5_64, dtype=torch.int64, device=dev)
    first = _device(dev, *batch, False, 48 * 300, 40, ws=ws)
    frames2 = C.batch(31, 300, "edges")
    want2 = DM.want_of(frames2, C.model_netif(), udp_ports=C.UDP_SERVED, tcp_ports=C.TCP_SERVED)
    data2, offs2, lens2 = C.pack(31, frames2)
    second = _device(dev, *_parse(dev, data2, offs2, lens2, False), False, 4096, 300, ws=ws)
    again = _device(dev, *batch, False, 48 * 300, 40, ws=ws)
    C.check_outputs(first, want, "first")
    C.check_outputs(second, want2, "second")
    C.check_outputs(again, want, "again")


def test_batch_past_the_tile_and_the_scan_pass(dev):
    """kScanPass * kTile + 257 uniform frames with deliveries only at both sides of the tile and
    scan-pass boundaries and at the ends: the scan's second pass carries the bases over."""
    c = C.read_constants()
    tile, edge = c["kTile"], c["kScanPass"] * c["kTile"]
    n = edge + 257
    at = sorted({0, tile - 1, tile, 2 * tile - 1, edge - tile, edge - 1, edge, edge + 1, edge + tile - 1, edge + tile, n - 1})
    want, data, offs, lens, recs_h, batch = _uniform(dev, n, at)
    assert [i for i, _ in want.items] == at
    got = _device(dev, *batch, False, 48 * len(at), len(at) + 1)
    C.check_outputs(got, want, "whole")
    cut = _device(dev, *batch, False, 48 * 7, 8)  # the cut falls in the first tile of the second pass
    C.check_outputs(cut, want, "cut")
    assert int(cut["summary"][:8].view(np.uint32)[1]) == 7
    _same_as_host(cut, data, offs, lens, recs_h, False)


def test_every_kind_and_skips_across_two_scan_passes(dev):
    """The same size with served TCP, DHCP and overrunning records beside the UDP deliveries, one of
    each in the last tile of the scan's first pass and in the first tile of its second: every
    per-kind total and `skipped` is a sum over both passes, and the DHCP count is what is left of
    the records. Whole, and with the region cut in the first tile of the second pass."""
    c = C.read_constants()
    tile, edge = c["kTile"], c["kScanPass"] * c["kTile"]
    n = edge + 257
    udp_at = [0, edge - tile, edge - 1, edge, edge + tile - 1, n - 1]
    tcp_at = [1, 4, tile, edge - tile + 1, edge - 2, edge + 1, edge + tile - 5]
    dhcp_at = [2, 5, 6, edge - tile + 2, edge - 3, edge + 2, edge + 3, n - 3]
    overrun_at = [3, 7, 8, 9, tile + 1, edge - tile + 3, edge - 4, edge + 4, n - 4]
    want, data, offs, lens, recs_h, batch = _uniform(dev, n, udp_at, tcp_at=tcp_at, dhcp_at=dhcp_at, overrun_at=overrun_at)
    assert [i for i, _ in want.items] == sorted(udp_at + tcp_at + dhcp_at)
    assert list(want.kind_counts) == [len(udp_at), len(tcp_at), len(dhcp_at)] and want.skipped == len(overrun_at)
    assert (DM.UDP, DM.TCP, DM.DHCP) == (0, 1, 2)
    for lo, hi in ((edge - tile, edge), (edge, edge + tile)):  # the last tile of pass one, the first of pass two
        assert all(any(lo <= i < hi for i in at) for at in (udp_at, tcp_at, dhcp_at, overrun_at))
    got = _device(dev, *batch, False, (want.total_bytes + 15) & ~15, len(want.recs) + 1)
    C.check_outputs(got, want, "whole")
    _same_as_host(got, data, offs, lens, recs_h, False)
    before = sum(len(r) for (i, _), r in zip(want.items, want.recs) if i < edge + 2)
    cut = _device(dev, *batch, False, (before + 15) & ~15, len(want.recs))  # the record of frame edge + 2 does not fit
    C.check_outputs(cut, want, "cut")
    assert int(cut["summary"][:8].view(np.uint32)[1]) == sum(1 for i, _ in want.items if i < edge + 2)
    _same_as_host(cut, data, offs, lens, recs_h, False)


@pytest.mark.parametrize("n,density", [(200, "all"), (321, "edges")])
def test_read_contract_marked_bytes_never_reach_the_output(dev, n, density):
    """The gaps between frames and the bytes behind each frame in its last 4-byte word hold a
    marker byte that the expected stream does not contain; the written prefix must not either."""
    frames = C.batch(55 + n, n, density)
    want = DM.want_of(frames, C.model_netif(), udp_ports=C.UDP_SERVED, tcp_ports=C.TCP_SERVED)
    stream, _, _ = want.expect(1 << 30, 0)
    absent = sorted(set(range(1, 256)) - set(stream) - {FILL})
    assert absent, "no byte value is free for the marker"
    mark = absent[-1]
    rng = np.random.default_rng(n)
    offs, pos = [], 0
    for f in frames:
        pos += 4 * int(rng.integers(0, 3))
        offs.append(pos)
        pos += (len(f) + 3) & ~3
    data = np.full(pos + 16, mark, np.uint8)
    for at, f in zip(offs, frames):
        data[at:at + len(f)] = np.frombuffer(f, np.uint8)
    assert any(len(f) % 4 for f in frames) and any(b - a > ((len(f) + 3) & ~3) for a, b, f in zip(offs, offs[1:], frames))
    offs_dw = (np.array(offs, np.int64) // 4).astype(np.uint32)
    lens = np.array([len(f) for f in frames], np.uint16)
    region = (len(stream) + 15) & ~15
    got = _device(dev, *_parse(dev, data, offs_dw, lens, False), False, region, n)
    C.check_outputs(got, want, density)
    written = int(got["summary"][:40].view(np.uint64)[2])
    assert written == len(stream) and not (got["out"][:written] == mark).any()


def test_chain_ring_span_to_handlers(dev):
    """A ring's records in HBM -> the device walk (halo_rx_ring_scan_device, the consumer's poll
    over a device-resident span) -> parse -> deliver -> DeliverResult.dispatch: the handlers see
    what NetIf.packet_handle_batch shows them for the same frames, in the same order."""
    import torch

    from halo_amd import _lib, deliver, port_map, protocol
    from halo_amd.engine import NetIf
    from halo_amd.ring import RingBuffer

    frames = [f for _, f in C.crafted()] + C.batch(77, 300, "sparse") + C.batch(78, 100, "all")
    frames = [f for f in frames if len(f) <= 1514]  # what a 1514-byte receive buffer takes out of a ring

    def recording(log, rx):
        nif = NetIf("eth0", "AA:AA:AA:AA:AA:AA", "192.168.100.100", rx, cpu_below=1 << 30)
        for p in C.UDP_SERVED:
            nif.RecvUdp(p, lambda s, payload, p=p: log.append(("udp", p, s.RemoteIp, s.RemotePort, bytes(payload))))
        for p in C.TCP_SERVED:
            nif.RecvTcp(p, lambda s, payload, seq, ack, fl, p=p: log.append(("tcp", p, s.RemoteIp, s.RemotePort, bytes(payload),
                                                                            seq, ack, fl)))
        return nif

    want_log, got_log = [], []
    it = iter(frames)
    ref = recording(want_log, lambda: next(it, None))
    ref.packet_handle_batch(batch=len(frames) + 1)
    assert len(want_log) > 100

    ring = RingBuffer(1 << 20)
    assert ring.write(frames) == len(frames)
    used = ring.head
    span = torch.from_numpy(ring.data[:used].copy()).to(dev)
    d_off = torch.zeros(used // 8, dtype=torch.int32, device=dev)
    d_len = torch.zeros(used // 8, dtype=torch.int16, device=dev)
    info = torch.zeros(24, dtype=torch.uint8, device=dev)
    wsb = int(_lib.lib.halo_rx_ring_scan_workspace(used, 1514))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check("halo_rx_ring_scan_device", _lib.lib.halo_rx_ring_scan_device(
        span.data_ptr(), used, ring.size, 1514, 0, d_off.data_ptr(), d_len.data_ptr(), info.data_ptr(), ws.data_ptr(), wsb, st))
    torch.cuda.synchronize()
    k = int(info.cpu().numpy().view(_lib.RING_SCAN_DTYPE)[0]["n_frames"])
    assert k == len(frames)
    abi = C.lib_netif()
    recs = protocol.parse_frames_batch(span, d_off[:k], d_len[:k], netif=abi)
    got = recording(got_log, lambda: None)
    r = deliver(span, d_off[:k], d_len[:k], recs, netif=abi, region_bytes=1 << 20, udp_ports=_t(dev, port_map(got.UdpServiceMap), np.int32),
                tcp_ports=_t(dev, port_map(got.TcpServiceMap), np.int32), index_cap=16)
    calls = r.dispatch(got)
    assert got_log == want_log and calls == len(want_log)
    assert int(r.summary["records_written"]) == int(r.summary["records"]) == len(want_log)
    assert r.device_stream().is_cuda and int(r.device_stream().numel()) == r.bytes_written
    assert [int(e["frame"]) for e in r.index] == [int(h["frame"]) for h, _ in r.records()][:16]
