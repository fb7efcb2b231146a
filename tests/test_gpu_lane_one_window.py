"""GPU: the one-window form of the lane kernel's lean instance (rx_lane_lean1_kernel, DESIGN.md
§15.14): a launch without a histogram whose grid covers the batch gives every wave exactly one
window and runs no loop. Every
expected byte comes from the C oracle through the helpers of test_gpu_lane_fastpath.py; every case
compares every record byte, and the record array lies between two 4 KB sentinels that must stay
untouched. Shapes: n = 1, 63, 64, 65, 128 and 4097 frames of 61..64 B (the last window partial), all
plain, with one frame at lane 0, 31 or 63 that fails the length ballot or the header ballot, and
with failing IPv4 and UDP checksums inside an otherwise plain window; flags 0 and 1, 32- and 16-byte
records, with and without a histogram (with one the launch goes through rx_lane_kernel), the four
layouts, the fused entry points and the several-batches call. The last two tests overwrite one
record array fifty times and copy it on the device after every launch: a wave's record stores are
complete when its launch is, whether or not the wave waited for them before it ended (§15.14 part A).
"""
from __future__ import annotations

import numpy as np
import pytest

from tests.gen_golden import tcp_frame, udp_frame
from tests.helpers import assert_records_equal
from tests.test_gpu_lane_fastpath import L4_CKSUM, IP_HDR_CKSUM, dev, flip, pack, plain, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 128, 4097)
LANES = (0, 31, 63)
GUARD = 4096
FILL = 0xEE
# (flags, compact)
MODES = [(0, False), (1, False), (0, True), (1, True)]
MODE_IDS = ["f0", "f1", "f0_rec16", "f1_rec16"]
HIST = [False, True]
HIST_IDS = ["nohist", "hist"]


def frame61_64(k: int) -> bytes:
    return plain(k, 61 + k % 4)


def window_sets(n: int, frame=frame61_64):
    """(name, frames) for a batch of n frames made by `frame`: all plain; one deviant at lane 0 / 31 / 63 of window 0
    (where the batch has that lane) failing the length ballot (65 B) or the header ballot (a 64 B
    TCP frame); failing checksums in window 0 and, for a batch with one, in the partial last window."""
    base = [frame(k) for k in range(n)]
    sets = [("plain", base)]
    for lane in LANES:
        if lane >= n:
            continue
        f = list(base)
        f[lane] = plain(lane, 65)
        sets.append((f"len@{lane}", f))
        f = list(base)
        f[lane] = tcp_frame(payload=b"0123456789")
        assert len(f[lane]) == 64
        sets.append((f"hdr@{lane}", f))
    f = list(base)
    for i, how in ((5, "ip"), (40, "l4"), (41, "both"), (n - 1, "l4")):
        if i >= n or i < 0:
            continue
        if how in ("ip", "both"):
            f[i] = flip(f[i], 22, 3)
        if how in ("l4", "both"):
            f[i] = flip(f[i], 50, 6)
    sets.append(("csum", f))
    return sets


@pytest.fixture(scope="module")
def cases(oracle_lib):
    """Every (n, contents) batch packed once, with the oracle's records for flags 0 and 1."""
    out = []
    for n in SIZES:
        for name, frames in window_sets(n):
            data, offs, lens = pack(frames)
            refs = {fl: oracle_lib.rx_batch(data, lens, oracle_lib.NetIf.make(), fl, offsets_dw=offs) for fl in (0, 1)}
            out.append((f"n={n} {name}", frames, (data, offs, lens), refs))
    return out


def guarded(dev, n: int, width: int):
    """A record array of n x width bytes between two GUARD-byte sentinels: (whole buffer, the array)."""
    import torch

    buf = torch.full((2 * GUARD + n * width,), FILL, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + n * width].view(n, width)


def check_out(buf, want, compact, what):
    """The guarded buffer after a launch: sentinels untouched, records == the oracle's."""
    from halo_amd import _lib
    from halo_amd._lib import compact_of

    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == FILL), (what, "bytes before the record array written")
    assert np.all(got[len(got) - GUARD:] == FILL), (what, "bytes after the record array written")
    body = got[GUARD:len(got) - GUARD]
    if compact:
        wb = np.ascontiguousarray(compact_of(want)).view(np.uint8).reshape(-1, 16)
        bad = np.nonzero(np.any(body.reshape(-1, 16) != wb, axis=1))[0]
        assert bad.size == 0, (what, "compact records differ", bad[:8].tolist())
    else:
        assert_records_equal(body.view(_lib.RESULT_DTYPE), want, None, what)


def check_hist(hist, whist, with_hist, what):
    if with_hist:
        assert np.array_equal(hist.cpu().numpy().astype(np.int64), whist.astype(np.int64)), (what, "histogram")
    else:
        assert not hist.any(), (what, "a histogram nobody passed was written")


def word_of(flags, compact):
    from halo_amd import _lib

    return flags | _lib.variant_flags(1) | (_lib.HALO_RX_RECORD_COMPACT if compact else 0)


def stream_of():
    import torch

    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("with_hist", HIST, ids=HIST_IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_ragged(dev, cases, mode, with_hist):
    """Layout 0 (halo_rx_parse_batch_device): every shape and every window content."""
    import torch

    from halo_amd import _lib
    from halo_amd._lib import NetIf

    flags, compact = mode
    for what, _, packed, refs in cases:
        d, o, ln = to_dev(dev, *packed)
        want, whist = refs[flags]
        n = len(want)
        buf, out = guarded(dev, n, 16 if compact else 32)
        hist = torch.zeros(14, dtype=torch.int32, device=dev)
        _lib.check("parse", _lib.lib.halo_rx_parse_batch_device(
            d.data_ptr(), o.data_ptr(), ln.data_ptr(), n, word_of(flags, compact), NetIf.make(), 65, out.data_ptr(),
            hist.data_ptr() if with_hist else None, stream_of()))
        torch.cuda.synchronize()
        check_out(buf, want, compact, what)
        check_hist(hist, whist, with_hist, what)
        if "csum" in what and flags & 1 and n >= 64:
            assert [int(want["status"][i]) for i in (5, 40, 41)] == [IP_HDR_CKSUM, L4_CKSUM, IP_HDR_CKSUM]


STRIDE = 80


@pytest.fixture(scope="module")
def strided_cases(oracle_lib):
    """{per_frame_lens: [(what, host bytes, lens, {flags: oracle's (records, histogram)})]} at stride
    80. Layout 1 carries the frames' own lengths, so every content runs; layout 2 has one length, 64:
    64 B frames, all plain, with the header deviant (a 64 B TCP frame) and with failing checksums."""
    out = {True: [], False: []}
    for per_frame_lens in (True, False):
        for n in SIZES:
            for name, frames in window_sets(n, frame61_64 if per_frame_lens else plain):
                if not per_frame_lens and name.startswith("len@"):
                    continue
                host = np.full(STRIDE * n + 64, 0x5A, np.uint8)
                for i, f in enumerate(frames):
                    host[i * STRIDE:i * STRIDE + len(f)] = np.frombuffer(f, np.uint8)
                lens = np.array([len(f) for f in frames], np.uint16)
                assert per_frame_lens or np.all(lens == 64)
                refs = {fl: oracle_lib.rx_batch(host, lens, oracle_lib.NetIf.make(), fl,
                                                offsets_dw=np.arange(n, dtype=np.uint32) * (STRIDE // 4)) for fl in (0, 1)}
                out[per_frame_lens].append((f"n={n} {name}", host, lens, refs))
    return out


@pytest.mark.parametrize("with_hist", HIST, ids=HIST_IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("per_frame_lens", [True, False], ids=["layout1", "layout2"])
def test_strided(dev, strided_cases, per_frame_lens, mode, with_hist):
    """Layouts 1 and 2 (halo_rx_parse_strided_device): every shape, every content the layout can hold."""
    import torch

    from halo_amd import _lib
    from halo_amd._lib import NetIf

    flags, compact = mode
    for what, host, lens, refs in strided_cases[per_frame_lens]:
        want, whist = refs[flags]
        n = len(want)
        d = torch.from_numpy(host).to(dev)
        ln = torch.from_numpy(lens.view(np.int16)).to(dev)
        buf, out = guarded(dev, n, 16 if compact else 32)
        hist = torch.zeros(14, dtype=torch.int32, device=dev)
        _lib.check("strided", _lib.lib.halo_rx_parse_strided_device(
            d.data_ptr(), STRIDE, ln.data_ptr() if per_frame_lens else None, 0 if per_frame_lens else 64, n,
            word_of(flags, compact), NetIf.make(), out.data_ptr(), hist.data_ptr() if with_hist else None, stream_of()))
        torch.cuda.synchronize()
        check_out(buf, want, compact, f"stride 80, {what}")
        check_hist(hist, whist, with_hist, what)


@pytest.mark.parametrize("with_hist", HIST, ids=HIST_IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_l3_start(dev, oracle_lib, cases, mode, with_hist):
    """Layout 3 (HALO_RX_L3_START): the frames' IPv4 packets. Never fast, but a launch without a
    histogram takes the one-window instance of this layout."""
    import torch

    from halo_amd import _lib
    from halo_amd._lib import HALO_RX_L3_START, NetIf

    flags, compact = mode
    for what, frames, _, _ in cases:
        data, offs, lens = pack([f[14:] for f in frames])
        want, whist = oracle_lib.rx_batch(data, lens, oracle_lib.NetIf.make(), flags | HALO_RX_L3_START, offsets_dw=offs)
        d, o, ln = to_dev(dev, data, offs, lens)
        n = len(want)
        buf, out = guarded(dev, n, 16 if compact else 32)
        hist = torch.zeros(14, dtype=torch.int32, device=dev)
        _lib.check("l3", _lib.lib.halo_rx_parse_batch_device(
            d.data_ptr(), o.data_ptr(), ln.data_ptr(), n, word_of(flags, compact) | HALO_RX_L3_START, NetIf.make(), 64,
            out.data_ptr(), hist.data_ptr() if with_hist else None, stream_of()))
        torch.cuda.synchronize()
        check_out(buf, want, compact, f"L3 start, {what}")
        check_hist(hist, whist, with_hist, what)


@pytest.mark.parametrize("with_hist", HIST, ids=HIST_IDS)
@pytest.mark.parametrize("flags", [0, 1], ids=["f0", "f1"])
def test_fused_flow_and_route(dev, oracle_lib, cases, flags, with_hist):
    """halo_rx_parse_flow_batch_device and halo_rx_parse_route_batch_device: the plain parse's
    records between the sentinels, and the hashes / route ids of those records."""
    import torch

    from halo_amd import _lib
    from halo_amd._lib import NetIf
    from halo_amd.route import RouteTable

    g, ora = RouteTable(0), oracle_lib.RouteTable()
    for r in ([0, 0, 1, 0], [0xC0A86400, 0xFFFFFF00, 0, 1], [0xC0A86464, 0xFFFFFFFF, 0, 2], [0x0A000000, 0xFF000000, 5, 3]):
        assert g.AddRoute(RouteTable.entry(*r)) == ora.add(r)
    g.sync()
    for what, frames, _, _ in cases:
        frames = list(frames)
        if len(frames) > 70:
            frames[70] = udp_frame(payload=bytes(22), dst_ip=bytes([10, 0, 0, 1]))
        data, offs, lens = pack(frames)
        want, whist = oracle_lib.rx_batch(data, lens, oracle_lib.NetIf.make(), flags, offsets_dw=offs)
        d, o, ln = to_dev(dev, data, offs, lens)
        n = len(want)
        word = word_of(flags, False)

        buf, out = guarded(dev, n, 32)
        hist = torch.zeros(14, dtype=torch.int32, device=dev)
        h = torch.zeros(n, dtype=torch.int64, device=dev)
        b = torch.zeros(n, dtype=torch.int32, device=dev)
        _lib.check("fused flow", _lib.lib.halo_rx_parse_flow_batch_device(
            d.data_ptr(), o.data_ptr(), ln.data_ptr(), n, word, NetIf.make(), 65, out.data_ptr(),
            hist.data_ptr() if with_hist else None, 1, 0, h.data_ptr(), 1 << 20, b.data_ptr(), stream_of()))
        torch.cuda.synchronize()
        check_out(buf, want, False, f"fused flow, {what}")
        check_hist(hist, whist, with_hist, what)
        wh, wb = oracle_lib.flow_hash_batch(np.array(want), 1, 0, 1 << 20)
        assert np.array_equal(h.cpu().numpy().view(np.uint64), wh), (what, "flow hashes")
        assert np.array_equal(b.cpu().numpy().view(np.uint32), wb), (what, "flow buckets")

        buf, out = guarded(dev, n, 32)
        hist.zero_()
        rid = torch.zeros(n, dtype=torch.int32, device=dev)
        _lib.check("fused route", _lib.lib.halo_rx_parse_route_batch_device(
            d.data_ptr(), o.data_ptr(), ln.data_ptr(), n, word, NetIf.make(), 65, out.data_ptr(),
            hist.data_ptr() if with_hist else None, g._t, rid.data_ptr(), stream_of()))
        torch.cuda.synchronize()
        check_out(buf, want, False, f"fused route, {what}")
        check_hist(hist, whist, with_hist, what)
        assert np.array_equal(rid.cpu().numpy().view(np.uint32), ora.find_batch(want["dst_ip"])), (what, "route ids")


@pytest.mark.parametrize("with_hist", HIST, ids=HIST_IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("k", [2, 3])
def test_batches_entry(dev, cases, k, mode, with_hist):
    """halo_rx_parse_batches_device with 2 and 3 batches: batch j is the j-th of the contents with a
    header deviant at lane 31, the failing checksums and the all-plain frames, sizes 65, 4097 and 64."""
    import torch

    from halo_amd import protocol
    from halo_amd._lib import NetIf

    flags, compact = mode
    by_name = {what: (packed, refs) for what, _, packed, refs in cases}
    picks = [by_name[w] for w in ("n=65 hdr@31", "n=4097 csum", "n=64 plain")][:k]
    bufs, batches, want_hist = [], [], np.zeros(14, np.int64)
    for packed, refs in picks:
        want, whist = refs[flags]
        buf, out = guarded(dev, len(want), 16 if compact else 32)
        bufs.append(buf)
        batches.append(to_dev(dev, *packed) + (out,))
        want_hist += whist.astype(np.int64)
    hist = torch.zeros(14, dtype=torch.int32, device=dev)
    protocol.parse_frames_batches(batches, netif=NetIf.make(), check_sum_enable=bool(flags & 1), max_len_hint=65,
                                  variant=1, compact=compact, hist=hist if with_hist else None)
    torch.cuda.synchronize()
    for j, (buf, (_, refs)) in enumerate(zip(bufs, picks)):
        check_out(buf, refs[flags][0], compact, f"{k} batches, batch {j}")
    check_hist(hist, want_hist, with_hist, f"{k} batches")


def _two_batches(dev, cases):
    by_name = {what: (packed, refs) for what, _, packed, refs in cases}
    picks = [by_name[w] for w in ("n=4097 plain", "n=4097 csum")]
    wants = [refs[1][0] for _, refs in picks]
    assert wants[0].tobytes() != wants[1].tobytes()
    return [to_dev(dev, *packed) for packed, _ in picks], wants


def test_stores_complete_same_stream(dev, cases):
    """Two different batches of 4097 frames alternate into one `out`, 50 launches back to back on one
    stream, each followed by a device-side copy of `out` on that stream: copy i holds batch i's
    records, all of them."""
    import torch

    from halo_amd import _lib, protocol
    from halo_amd._lib import NetIf

    devb, wants = _two_batches(dev, cases)
    buf, out = guarded(dev, 4097, 32)
    copies = torch.zeros((50,) + tuple(buf.shape), dtype=torch.uint8, device=dev)
    for i in range(50):
        d, o, ln = devb[i & 1]
        _lib.check("parse", _lib.lib.halo_rx_parse_batch_device(
            d.data_ptr(), o.data_ptr(), ln.data_ptr(), 4097, word_of(1, False), NetIf.make(), 64, out.data_ptr(), None,
            stream_of()))
        copies[i].copy_(buf)
    torch.cuda.synchronize()
    for i in range(50):
        check_out(copies[i], wants[i & 1], False, f"launch {i}, copy on the launch's stream")
    assert protocol.records(out).tobytes() == wants[1].tobytes()


def test_stores_complete_second_stream(dev, cases):
    """The same with every copy taken on a second stream behind an event recorded after the launch
    (the next launch waits for the copy, which reads the array it overwrites)."""
    import torch

    from halo_amd import _lib
    from halo_amd._lib import NetIf

    devb, wants = _two_batches(dev, cases)
    buf, out = guarded(dev, 4097, 32)
    copies = torch.zeros((50,) + tuple(buf.shape), dtype=torch.uint8, device=dev)
    main, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(main)  # the fills above
    for i in range(50):
        d, o, ln = devb[i & 1]
        _lib.check("parse", _lib.lib.halo_rx_parse_batch_device(
            d.data_ptr(), o.data_ptr(), ln.data_ptr(), 4097, word_of(1, False), NetIf.make(), 64, out.data_ptr(), None,
            main.cuda_stream))
        parsed = torch.cuda.Event()
        parsed.record(main)
        side.wait_event(parsed)
        with torch.cuda.stream(side):
            copies[i].copy_(buf)
        copied = torch.cuda.Event()
        copied.record(side)
        main.wait_event(copied)
    torch.cuda.synchronize()
    for i in range(50):
        check_out(copies[i], wants[i & 1], False, f"launch {i}, copy on a second stream")
