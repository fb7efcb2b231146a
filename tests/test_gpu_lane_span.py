"""GPU: dense windows through the lane kernel's two instances (with a histogram, and the
no-histogram instance rx_lane_lean_kernel) against the C oracle, bit-exact. The
cases were written for the span read of a dense window (HALO_RX_LANE_SPAN: 64 back-to-back frames of
61..64 bytes read as one 4096-byte span and transposed through LDS), which §15.13 measured and
rejected; they hold whatever reads a dense window to the same bytes. The shapes are the smallest at
which the split between the paths and the reuse of a wave's LDS can go wrong: windows at their
edges, spans at every alignment against the 128-byte lines and the 16-byte loads, windows that
are dense but not plain and plain but not dense, launches in sequence, and the other entry points
that share the window code. Every case runs with and without a histogram and with 32- and 16-byte
records, compares every record byte and the status counts with the oracle's, and depends on
nothing but the bytes: it passes with the knobs on and off.
"""
from __future__ import annotations

import numpy as np
import pytest

from tests.gen_golden import tcp_frame, udp_frame, with_bytes
from tests.helpers import assert_records_equal
from tests.test_gpu_lane_fastpath import check_packed, flip, plain, to_dev

pytestmark = pytest.mark.gpu

# (compact records, with a histogram)
KINDS = [(False, True), (False, False), (True, True), (True, False)]
KIND_IDS = ["rec32_hist", "rec32", "rec16_hist", "rec16"]
LANES = (0, 31, 63)
FLAGS = 1  # HALO_RX_CSUM_ENABLE
IP_HDR_CKSUM, L4_CKSUM = 7, 13


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


def place(frames, offs_dw, fill: int = 0x5A):
    """Frame i at dword offs_dw[i] of a buffer that ends with the dword holding the last byte of the
    frame that lies last in memory: nothing is allocated past what the read contract allows.
    (data, offsets_dw, lens)"""
    offs = np.asarray(offs_dw, np.uint32)
    end = max(4 * int(o) + ((len(f) + 3) & ~3) for o, f in zip(offs, frames))
    data = np.full(end, fill, np.uint8)
    for o, f in zip(offs, frames):
        data[4 * int(o):4 * int(o) + len(f)] = np.frombuffer(f, np.uint8)
    return data, offs, np.array([len(f) for f in frames], np.uint16)


def dense(frames, lead_dw: int = 0):
    """Frames of 61..64 bytes back to back, 16 dwords each, the first at dword lead_dw."""
    return place(frames, lead_dw + 16 * np.arange(len(frames)))


def run(dev, oracle_lib, packed, kind, what, shift: int = 0):
    """packed (data, offsets_dw, lens) through the lane kernel, the frame bytes starting `shift`
    bytes past a 16-byte boundary of device memory; records and counts == the oracle's."""
    import torch

    compact, with_hist = kind
    data, offs, lens = packed
    ref = oracle_lib.rx_batch(data, lens, oracle_lib.NetIf.make(), FLAGS, offsets_dw=offs)
    d, o, ln = to_dev(dev, data, offs, lens)
    if shift:
        room = torch.empty(shift + d.numel(), dtype=torch.uint8, device=dev)
        assert room.data_ptr() % 16 == 0
        room[shift:] = d
        d = room[shift:]
        assert d.data_ptr() % 16 == shift
    check_packed(dev, (d, o, ln), ref, FLAGS, compact, what, with_hist)
    return ref[0]


def mixed_lengths(n: int):
    """Plain frames whose lengths run through 61..64 lane by lane: all occupy 16 dwords."""
    return [plain(k, 61 + (k % 4)) for k in range(n)]


def not_dense_cases(n: int = 128, k0: int = 0):
    """(name, packed): plain windows (frames plain(k0) ..) that are not one span."""
    frames = [plain(k0 + k) for k in range(n)]
    cases = []
    for lane in (1, 31, 63):  # one frame starts a dword late, every later frame shifted with it
        offs = 16 * np.arange(n) + (np.arange(n) >= lane)
        cases.append((f"late dword at lane {lane}", place(frames, offs)))
    offs = 16 * np.arange(n)
    offs[[5, 40]] = offs[[40, 5]]  # two frames swapped in memory: offsets out of order
    cases.append(("two frames swapped", place(frames, offs)))
    offs = 16 * np.arange(n)
    offs[[0, 63]] = offs[[63, 0]]  # ... the window's first and last (lane 0 is the span's start)
    cases.append(("first and last swapped", place(frames, offs)))
    offs = 16 * np.arange(n)
    offs[32] = offs[31]  # two lanes read the same frame; slot 32 is not read at all
    cases.append(("two lanes on one offset", place(frames, offs)))
    return cases


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_window_edges(dev, oracle_lib, kind):
    """All plain and dense; the partial last window takes the general path. With a histogram a wave
    of these small grids takes two windows, one after the other through the same LDS."""
    for n in (63, 64, 65, 127, 128, 129, 64 * 5 + 1):
        want = run(dev, oracle_lib, dense([plain(k) for k in range(n)]), kind, f"dense n={n}")
        assert np.all(want["status"] == 0)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_span_alignment(dev, oracle_lib, kind):
    """The span starts at dword 0, 1, 2, 3, 29 or 31 of a 128-byte line (29 and 31: the 16-byte loads
    straddle lines), and the frame bytes 0, 4 or 12 bytes past a 16-byte boundary. Two windows; the
    buffer ends where the last frame ends."""
    frames = [plain(k) for k in range(128)]
    for lead in (0, 1, 2, 3, 29, 31):
        packed = dense(frames, lead)
        assert packed[0].size == 4 * lead + 64 * len(frames)
        for shift in (0, 4, 12):
            run(dev, oracle_lib, packed, kind, f"lead {lead} dwords, base + {shift}", shift)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_lengths_inside_a_dense_window(dev, oracle_lib, kind):
    """Lengths 61..64 mixed lane by lane stay one span; one frame of 60 bytes in its 16-dword slot
    fails the length test alone."""
    want = run(dev, oracle_lib, dense(mixed_lengths(128), 1), kind, "lengths 61..64")
    assert np.all(want["status"] == 0)
    for lane in LANES:
        frames = mixed_lengths(128)
        frames[lane] = plain(lane, 60)
        run(dev, oracle_lib, dense(frames, 1), kind, f"60 B at lane {lane}")


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_not_dense(dev, oracle_lib, kind):
    """Plain windows that are not one span give the oracle's records whichever path they take."""
    for name, packed in not_dense_cases():
        run(dev, oracle_lib, packed, kind, name)


def header_deviants():
    base = plain(7)
    tcp = tcp_frame(payload=b"0123456789")
    assert len(tcp) == 64 and len(base) == 64
    return [("tcp", tcp), ("fragment", with_bytes(base, 20, b"\x20\x00")), ("ihl 6", with_bytes(base, 14, b"\x46")),
            ("ethertype", with_bytes(base, 12, b"\x86\xdd"))]


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_header_deviants_in_a_dense_window(dev, oracle_lib, kind):
    """A dense window with one frame the header ballot rejects: read as a span, parsed by the general
    path. Window 1 stays plain."""
    for name, frame in header_deviants():
        for lane in LANES:
            frames = [plain(k) for k in range(128)]
            frames[lane] = frame
            want = run(dev, oracle_lib, dense(frames, 2), kind, f"{name} at lane {lane}")
            assert np.all(want["status"][64:] == 0)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_failing_checksums_in_a_dense_window(dev, oracle_lib, kind):
    """Frames failing the IPv4 header sum or the UDP sum are still plain: selects on the fast path."""
    frames = [plain(k) for k in range(64)]
    for i in (0, 5, 63):
        frames[i] = flip(frames[i], 22, 3)
    for i in (1, 40, 62):
        frames[i] = flip(frames[i], 50, 6)
    frames[41] = flip(flip(frames[41], 22, 3), 50, 6)
    want = run(dev, oracle_lib, dense(frames, 3), kind, "failing checksums")
    assert [int(want["status"][i]) for i in (0, 1, 5, 40, 41, 62, 63)] == [
        IP_HDR_CKSUM, L4_CKSUM, IP_HDR_CKSUM, L4_CKSUM, IP_HDR_CKSUM, L4_CKSUM, IP_HDR_CKSUM]
    bad = run(dev, oracle_lib, dense([flip(plain(k), 50, k % 8) for k in range(64)]), kind, "every UDP sum fails")
    assert np.all(bad["status"] == L4_CKSUM)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_three_dependent_launches(dev, oracle_lib, kind):
    """Dense, not dense, dense, back to back on one stream into one `out`: the last one's records."""
    import torch

    from halo_amd import _lib
    from halo_amd._lib import NetIf, compact_of

    compact, with_hist = kind
    n = 128
    sets = [dense([plain(k + 300) for k in range(n)]), not_dense_cases(n, 600)[0][1], dense([plain(k) for k in range(n)], 1)]
    refs = [oracle_lib.rx_batch(d, ln, oracle_lib.NetIf.make(), FLAGS, offsets_dw=o) for d, o, ln in sets]
    bufs = [to_dev(dev, *s) for s in sets]
    out = torch.full((n, 16 if compact else 32), 0xEE, dtype=torch.uint8, device=dev)
    hist = torch.zeros(14, dtype=torch.int32, device=dev)
    word = FLAGS | _lib.variant_flags(1) | (_lib.HALO_RX_RECORD_COMPACT if compact else 0)
    stream = torch.cuda.current_stream().cuda_stream
    for d, o, ln in bufs:
        _lib.check("parse", _lib.lib.halo_rx_parse_batch_device(
            d.data_ptr(), o.data_ptr(), ln.data_ptr(), n, word, NetIf.make(), 64, out.data_ptr(),
            hist.data_ptr() if with_hist else None, stream))
    torch.cuda.synchronize()
    want = refs[2][0]
    assert want.tobytes() != refs[1][0].tobytes()
    if compact:
        wb = np.ascontiguousarray(compact_of(want)).view(np.uint8).reshape(-1, 16)
        assert np.array_equal(out.cpu().numpy(), wb)
    else:
        assert_records_equal(out.cpu().numpy().reshape(-1).view(_lib.RESULT_DTYPE), want, None, "third launch")
    whist = sum(r[1].astype(np.int64) for r in refs) if with_hist else np.zeros(14, np.int64)
    assert np.array_equal(hist.cpu().numpy().astype(np.int64), whist)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_multi_batch_entry(dev, oracle_lib, kind):
    """halo_rx_parse_batches_device: K = 3 with n = 64, 65, 1, and K = 2 whose second batch is not
    dense."""
    import torch

    from halo_amd import protocol
    from halo_amd._lib import NetIf, compact_of

    compact, with_hist = kind
    calls = [[dense([plain(k) for k in range(64)]), dense([plain(k + 9) for k in range(65)], 3), dense([plain(77)], 1)],
             [dense([plain(k + 1) for k in range(128)], 2), not_dense_cases(128)[3][1]]]
    for c, sets in enumerate(calls):
        batches, wants, want_hist = [], [], np.zeros(14, np.int64)
        for data, offs, lens in sets:
            want, whist = oracle_lib.rx_batch(data, lens, oracle_lib.NetIf.make(), FLAGS, offsets_dw=offs)
            wants.append(want)
            want_hist += whist.astype(np.int64)
            batches.append(to_dev(dev, data, offs, lens) +
                           (torch.full((len(lens), 16 if compact else 32), 0xEE, dtype=torch.uint8, device=dev),))
        hist = torch.zeros(14, dtype=torch.int32, device=dev)
        protocol.parse_frames_batches(batches, netif=NetIf.make(), max_len_hint=64, variant=1, compact=compact,
                                      hist=hist if with_hist else None)
        torch.cuda.synchronize()
        for k, (bt, want) in enumerate(zip(batches, wants)):
            if compact:
                wb = np.ascontiguousarray(compact_of(want)).view(np.uint8).reshape(-1, 16)
                assert np.array_equal(bt[3].cpu().numpy(), wb), (c, k)
            else:
                assert_records_equal(protocol.records(bt[3]), want, None, f"call {c}, batch {k}")
        assert np.array_equal(hist.cpu().numpy().astype(np.int64), want_hist if with_hist else 0 * want_hist)


@pytest.mark.parametrize("with_hist", [True, False], ids=["hist", "no_hist"])
def test_fused_flow_and_route_entries(dev, oracle_lib, with_hist):
    """halo_rx_parse_flow_batch_device and halo_rx_parse_route_batch_device over the window-edge
    and the not-dense batches: records, hashes, buckets and route ids."""
    import torch

    from halo_amd import _lib, protocol
    from halo_amd._lib import NetIf
    from halo_amd.route import RouteTable

    g, ora = RouteTable(0), oracle_lib.RouteTable()
    for r in ([0, 0, 1, 0], [0xC0A86400, 0xFFFFFF00, 0, 1], [0xC0A86464, 0xFFFFFFFF, 0, 2], [0x0A000000, 0xFF000000, 5, 3]):
        assert g.AddRoute(RouteTable.entry(*r)) == ora.add(r)
    g.sync()
    stream = torch.cuda.current_stream().cuda_stream
    word = FLAGS | _lib.variant_flags(1)

    def frames_of(n):
        fr = [plain(k) for k in range(n)]
        fr[n // 2] = udp_frame(payload=bytes(22), dst_ip=bytes([10, 0, 0, 1]))
        return fr

    sets = [(f"dense n={n}", dense(frames_of(n), 1)) for n in (63, 64, 65, 129)] + not_dense_cases()
    for what, (data, offs, lens) in sets:
        n = len(lens)
        want, whist = oracle_lib.rx_batch(data, lens, oracle_lib.NetIf.make(), FLAGS, offsets_dw=offs)
        d, o, ln = to_dev(dev, data, offs, lens)
        out = torch.full((n, 32), 0xEE, dtype=torch.uint8, device=dev)
        h = torch.zeros(n, dtype=torch.int64, device=dev)
        b = torch.zeros(n, dtype=torch.int32, device=dev)
        hist = torch.zeros(14, dtype=torch.int32, device=dev)
        _lib.check("fused flow", _lib.lib.halo_rx_parse_flow_batch_device(
            d.data_ptr(), o.data_ptr(), ln.data_ptr(), n, word, NetIf.make(), 64, out.data_ptr(),
            hist.data_ptr() if with_hist else None, 1, 0, h.data_ptr(), 1 << 20, b.data_ptr(), stream))
        torch.cuda.synchronize()
        assert_records_equal(protocol.records(out), want, None, f"fused flow, {what}")
        wh, wb = oracle_lib.flow_hash_batch(np.array(want), 1, 0, 1 << 20)
        assert np.array_equal(h.cpu().numpy().view(np.uint64), wh), what
        assert np.array_equal(b.cpu().numpy().view(np.uint32), wb), what
        assert np.array_equal(hist.cpu().numpy().astype(np.int64), whist.astype(np.int64) * with_hist), what

        out = torch.full((n, 32), 0xEE, dtype=torch.uint8, device=dev)
        rid = torch.zeros(n, dtype=torch.int32, device=dev)
        hist.zero_()
        _lib.check("fused route", _lib.lib.halo_rx_parse_route_batch_device(
            d.data_ptr(), o.data_ptr(), ln.data_ptr(), n, word, NetIf.make(), 64, out.data_ptr(),
            hist.data_ptr() if with_hist else None, g._t, rid.data_ptr(), stream))
        torch.cuda.synchronize()
        assert_records_equal(protocol.records(out), want, None, f"fused route, {what}")
        assert np.array_equal(rid.cpu().numpy().view(np.uint32), ora.find_batch(want["dst_ip"])), what
        assert np.array_equal(hist.cpu().numpy().astype(np.int64), whist.astype(np.int64) * with_hist), what


@pytest.mark.parametrize("with_hist", [True, False], ids=["hist", "no_hist"])
@pytest.mark.parametrize("per_frame_lens", [True, False], ids=["lens", "one_len"])
def test_strided_entry(dev, oracle_lib, per_frame_lens, with_hist):
    """halo_rx_parse_strided_device at stride 64 over the window-edge batches: with one length, and
    with per-frame lengths of 61..64."""
    import torch

    from halo_amd import protocol
    from halo_amd._lib import NetIf

    for n in (63, 64, 65, 127, 128, 129, 64 * 5 + 1):
        frames = mixed_lengths(n) if per_frame_lens else [plain(k) for k in range(n)]
        buf = np.full(64 * n, 0x5A, np.uint8)
        for i, f in enumerate(frames):
            buf[64 * i:64 * i + len(f)] = np.frombuffer(f, np.uint8)
        lens = np.array([len(f) for f in frames], np.uint16)
        want, whist = oracle_lib.rx_batch(buf, lens, oracle_lib.NetIf.make(), FLAGS,
                                          offsets_dw=np.arange(n, dtype=np.uint32) * 16)
        hist = torch.zeros(14, dtype=torch.int32, device=dev)
        out = protocol.parse_frames_strided(torch.from_numpy(buf).to(dev), 64, n, netif=NetIf.make(),
                                            length=0 if per_frame_lens else 64,
                                            lens=torch.from_numpy(lens.view(np.int16)).to(dev) if per_frame_lens else None,
                                            hist=hist if with_hist else None)
        torch.cuda.synchronize()
        assert_records_equal(protocol.records(out), want, None, f"strided n={n}")
        assert np.array_equal(hist.cpu().numpy().astype(np.int64), whist.astype(np.int64) * with_hist)
