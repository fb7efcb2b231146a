"""GPU: the lane kernel's fast path for windows of plain frames (lane_window_fast, DESIGN.md
§15.12) against the C oracle, bit-exact, at the smallest shapes where the split between the fast
path and the general one can go wrong: whole and partial windows, one deviating frame at lane 0, 31
or 63 of an otherwise plain window, failing checksums inside a fast window, every frame and segment
length the predicate admits, and the other entry points that share the window code. Every case
compares every record byte and the status histogram; nothing depends on which path a window took.
The deviating-frame and failing-checksum cases run a second time without a histogram, which changes
how many windows a wave of a small grid takes. test_gpu_lane_fastpath_sweep.py and
test_gpu_resident_fastpath.py build on the helpers here.
"""
from __future__ import annotations

import numpy as np
import pytest

from tests.gen_golden import icmp_frame, tcp_frame, udp_frame, with_bytes
from tests.helpers import assert_records_equal

pytestmark = pytest.mark.gpu

# (flags, compact): the checksum and jumbo bits as the parity tests run them, and 16 B records
MODES = [(0, False), (1, False), (2, False), (3, False), (1, True)]
MODE_IDS = ["f0", "f1", "f2", "f3", "f1_rec16"]
IP_HDR_CKSUM, L4_CKSUM = 7, 13


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


def plain(k: int = 0, length: int = 64) -> bytes:
    """A plain UDP frame of 61..64 bytes to the NetIf; k varies ports and payload."""
    pay = bytes((7 * k + j) & 0xFF for j in range(length - 42))
    return udp_frame(payload=pay, sport=1024 + k, dport=2048 + 3 * k)


def padded(frame: bytes, length: int, fill: int = 0xD7) -> bytes:
    """frame followed by padding up to `length` bytes (its totalLen stays)."""
    return frame + bytes((fill + j) & 0xFF for j in range(length - len(frame)))


def flip(frame: bytes, byte: int, bit: int = 0) -> bytes:
    return with_bytes(frame, byte, bytes([frame[byte] ^ (1 << bit)]))


def pack(frames, lead_dw: int = 1, gaps: bool = True):
    """Ragged layout: frames at 4-byte-aligned starts, `lead_dw` dwords into the buffer and with a
    gap of 0..2 dwords between neighbours, so the starts are not all 16-byte aligned; the gaps hold
    garbage. (data, offsets_dw, lens)"""
    offs, pos = [], 4 * lead_dw
    for i, f in enumerate(frames):
        offs.append(pos // 4)
        pos += ((len(f) + 3) & ~3) + (4 * (i % 3) if gaps else 0)
    data = np.full(pos + 64, 0x5A, np.uint8)
    for o, f in zip(offs, frames):
        data[4 * o:4 * o + len(f)] = np.frombuffer(f, np.uint8)
    return data, np.array(offs, np.uint32), np.array([len(f) for f in frames], np.uint16)


def to_dev(dev, data, offs, lens):
    import torch

    return (torch.from_numpy(data).to(dev), torch.from_numpy(offs.view(np.int32)).to(dev),
            torch.from_numpy(lens.view(np.int16)).to(dev))


def pack_rows(rows: np.ndarray, lens: np.ndarray, lead_dw: int = 1, gaps: bool = True):
    """pack() for frames held as the rows of a uint8 array (row i: lens[i] bytes, the rest of the row
    ignored), without a Python loop per frame: the sweeps lay out 256k frames."""
    n = len(lens)
    size = ((lens.astype(np.int64) + 3) & ~3) + (4 * (np.arange(n) % 3) if gaps else 0)
    start = 4 * lead_dw + np.concatenate([[0], np.cumsum(size)[:-1]])
    data = np.full(4 * lead_dw + int(size.sum()) + 64, 0x5A, np.uint8)
    col = np.arange(rows.shape[1])
    inside = col[None, :] < lens[:, None]
    data[(start[:, None] + col[None, :])[inside]] = rows[inside]
    return data, (start // 4).astype(np.uint32), lens.astype(np.uint16)


def check_packed(dev, devbufs, oracle_ref, flags, compact, what, with_hist=True):
    """A packed batch already on the device (devbufs: to_dev's three tensors) through the lane kernel
    (variant 1), with a histogram or without one (hist = NULL: launch_variant then gives each wave of
    a small grid one window, not two); records (32 B, or 16 B with `compact`) and counts == the
    oracle's (oracle_ref: what rx_batch returned for these frames and flags)."""
    import torch

    from halo_amd import _lib
    from halo_amd._lib import NetIf, compact_of

    d, o, ln = devbufs
    want, whist = oracle_ref
    n = len(want)
    width = 16 if compact else 32
    out = torch.full((n, width), 0xEE, dtype=torch.uint8, device=dev)
    hist = torch.zeros(14, dtype=torch.int32, device=dev)
    word = flags | _lib.variant_flags(1) | (_lib.HALO_RX_RECORD_COMPACT if compact else 0)
    _lib.check("parse", _lib.lib.halo_rx_parse_batch_device(
        d.data_ptr(), o.data_ptr(), ln.data_ptr(), n, word, NetIf.make(), int(ln.max()), out.data_ptr(),
        hist.data_ptr() if with_hist else None, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    if compact:
        wb = np.ascontiguousarray(compact_of(want)).view(np.uint8).reshape(-1, 16)
        bad = np.nonzero(np.any(got != wb, axis=1))[0]
        assert bad.size == 0, (what, "compact records differ", bad[:8].tolist())
    else:
        assert_records_equal(got.reshape(-1).view(_lib.RESULT_DTYPE), want, None, what)
    if with_hist:
        assert np.array_equal(hist.cpu().numpy().astype(np.int64), whist.astype(np.int64)), (what, "histogram")
    else:
        assert not hist.any(), (what, "a histogram nobody passed was written")


def check(dev, oracle_lib, frames, flags, compact, what, with_hist=True):
    """The frames through the lane kernel (variant 1), with a histogram unless `with_hist` is False;
    records (32 B, or 16 B with `compact`) and counts == the oracle's. Returns the oracle's records."""
    data, offs, lens = pack(frames)
    ref = oracle_lib.rx_batch(data, lens, oracle_lib.NetIf.make(), flags, offsets_dw=offs)
    check_packed(dev, to_dev(dev, data, offs, lens), ref, flags, compact, what, with_hist)
    return ref[0]


def golden_frame(golden, name: str) -> bytes:
    meta, blob = golden
    e = next(e for e in meta["frames"] if e["name"] == name)
    return bytes(blob[e["offset"]:e["offset"] + e["len"]])


def deviants(golden):
    """(name, frame): every way one frame can fall outside the predicate, or sit at its edge."""
    g = lambda name: (name, golden_frame(golden, name))  # noqa: E731
    peer, own = bytes([192, 168, 100, 1]), bytes([192, 168, 100, 100])
    from oracle import ref_py as R

    gre = R.build_eth(R.build_ipv4(bytes(30), 47, peer, own), bytes.fromhex("aaaaaaaaaaaa"),
                      bytes.fromhex("020000000001"), 0x0800)
    return [
        g("arp_request_bcast"), g("eth_type_ipv6"), g("eth_type_unknown"),
        g("ip_ver_options"), ("ip_ver_0x55", udp_frame(ip_ver_ihl=0x55)),
        g("ip_frag_mf"), g("ip_frag_offset"), ("ip_frag_mf_offset", udp_frame(ip_frag=b"\x20\x10")),
        g("icmp_echo_request"), g("tcp_ok"), g("tcp_offset_quirk_options"), ("tcp_64B", tcp_frame(payload=b"0123456789")),
        ("ip_proto_47", gre),
        ("L42", udp_frame(payload=b"")[:42]), ("L59", udp_frame(payload=b"abc")[:59]), ("L60", plain(1, 60)),
        ("L61", plain(2, 61)), ("L63", plain(3, 63)), ("L65", plain(4, 65)),
        g("ip_padding_trimmed_60B"), ("padding_64B", padded(udp_frame(payload=b"\x01\x02\x03"), 64)),
        g("ip_totlen_underflow_19"), g("ip_totlen_overrun"), ("ip_totlen_overrun_L61", udp_frame(ip_total_len=48)[:61]),
        g("udp_len_7"), g("ip_totlen_20_udp"), g("udp_len_field_small"), g("udp_len_field_large"),
        g("udp_csum_zero_not_special"),
    ]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_all_plain_windows(dev, oracle_lib, mode):
    """n = 64 (the fast path alone), 65 and 127 (the partial window takes the general path), 1."""
    flags, compact = mode
    for n in (64, 65, 127, 1):
        want = check(dev, oracle_lib, [plain(k) for k in range(n)], flags, compact, f"all plain n={n}")
        assert np.all(want["status"] == 0) and np.all(want["payload_len"] == 22)


def _one_deviating_frame(dev, oracle_lib, golden, mode, with_hist):
    flags, compact = mode
    base = [plain(k) for k in range(128)]
    clean = check(dev, oracle_lib, base, flags, compact, "128 plain", with_hist)
    for name, frame in deviants(golden):
        for lane in (0, 31, 63):
            frames = list(base)
            frames[lane] = frame
            want = check(dev, oracle_lib, frames, flags, compact, f"{name} at lane {lane}", with_hist)
            assert want[64:].tobytes() == clean[64:].tobytes(), (name, lane, "window 1 changed")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_one_deviating_frame(dev, oracle_lib, golden, mode):
    """n = 128: window 0 plain but for one frame at lane 0, 31 or 63; window 1 all plain."""
    _one_deviating_frame(dev, oracle_lib, golden, mode, True)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_one_deviating_frame_without_histogram(dev, oracle_lib, golden, mode):
    """The same with hist = NULL, the benchmark's launch: the grid is not halved, so the two windows
    go to two waves."""
    _one_deviating_frame(dev, oracle_lib, golden, mode, False)


def _failing_checksums(dev, oracle_lib, mode, with_hist):
    flags, compact = mode
    frames = [plain(k) for k in range(64)]
    clean = check(dev, oracle_lib, frames, flags, compact, "64 plain", with_hist)
    frames[5] = flip(frames[5], 22, 3)
    frames[40] = flip(frames[40], 50, 6)
    frames[41] = flip(flip(frames[41], 22, 3), 50, 6)
    want = check(dev, oracle_lib, frames, flags, compact, "failing checksums", with_hist)
    if flags & 1:
        assert [int(want["status"][i]) for i in (5, 40, 41)] == [IP_HDR_CKSUM, L4_CKSUM, IP_HDR_CKSUM]
    keep = np.ones(64, bool)
    keep[[5, 40, 41]] = False
    assert want[keep].tobytes() == clean[keep].tobytes()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_failing_checksums_inside_a_fast_window(dev, oracle_lib, mode):
    """One bit flipped in the IPv4 header of frame 5 (TTL), one in the UDP payload of frame 40, both
    in frame 41: every frame still plain by the predicate; the first failing check wins."""
    _failing_checksums(dev, oracle_lib, mode, True)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_failing_checksums_inside_a_fast_window_without_histogram(dev, oracle_lib, mode):
    _failing_checksums(dev, oracle_lib, mode, False)


def test_mac_and_address_flags(dev, oracle_lib):
    """In a plain window: destination MAC ours / broadcast / neither, destination IP ours / .255 /
    neither. flags: HALO_RX_F_MAC_MATCH 1, _IP_BCAST 2, _DST_IS_OWN 4."""
    frames = [plain(k) for k in range(64)]
    pay = bytes(range(22))
    frames[3] = udp_frame(payload=pay, dst_mac=b"\xff" * 6)
    frames[9] = udp_frame(payload=pay, dst_mac=bytes.fromhex("aaaaaaaaaaab"))
    frames[17] = udp_frame(payload=pay, dst_ip=bytes([192, 168, 100, 255]))
    frames[33] = udp_frame(payload=pay, dst_ip=bytes([10, 0, 0, 1]))
    frames[63] = udp_frame(payload=pay, dst_ip=b"\xff" * 4, dst_mac=b"\xff" * 6)
    for flags, compact in MODES:
        want = check(dev, oracle_lib, frames, flags, compact, "MAC and address flags")
        assert [int(want["flags"][i]) for i in (0, 3, 9, 17, 33, 63)] == [5, 5, 4, 3, 1, 3]


def test_lengths_inside_the_predicate(dev, oracle_lib):
    """Every frame length the predicate admits (61..64) with every segment end it admits (totalLen
    28..L - 14, the rest of the frame padding) in two windows; offsets not all 16-byte aligned."""
    frames = []
    for length in (61, 62, 63, 64):
        for pay in range(0, length - 42 + 1):
            frames.append(padded(udp_frame(payload=bytes((91 * pay + j) & 0xFF for j in range(pay)), sport=pay + 1), length,
                                 fill=0x80 + pay))
    assert len(frames) == 20 + 21 + 22 + 23
    frames += [plain(k) for k in range(128 - len(frames))]
    _, offs, _ = pack(frames)
    assert np.any(offs % 4 != 0)
    for flags, compact in MODES:
        want = check(dev, oracle_lib, frames, flags, compact, "lengths inside the predicate")
        assert np.all(want["status"] == 0)


def _one_deviant(golden, n=128, lane=31, name="icmp_echo_request"):
    frames = [plain(k) for k in range(n)]
    frames[lane] = golden_frame(golden, name)
    return frames


@pytest.mark.parametrize("per_frame_lens", [True, False], ids=["lens", "one_len"])
def test_strided_entry(dev, oracle_lib, golden, per_frame_lens):
    """halo_rx_parse_strided_device, n = 128, stride 80: with per-frame lengths (a 74 B ICMP frame
    among 64 B ones) and with one length (an IPv6 frame of 64 B among them)."""
    import torch

    from halo_amd import protocol
    from halo_amd._lib import NetIf

    frames = _one_deviant(golden, name="icmp_echo_request" if per_frame_lens else "eth_type_ipv6")
    stride, n = 80, len(frames)
    buf = np.full(stride * n, 0x5A, np.uint8)
    for i, f in enumerate(frames):
        buf[i * stride:i * stride + len(f)] = np.frombuffer(f, np.uint8)
    lens = np.array([len(f) for f in frames], np.uint16)
    want, whist = oracle_lib.rx_batch(buf, lens, oracle_lib.NetIf.make(), 1,
                                      offsets_dw=np.arange(n, dtype=np.uint32) * (stride // 4))
    hist = torch.zeros(14, dtype=torch.int32, device=dev)
    out = protocol.parse_frames_strided(torch.from_numpy(buf).to(dev), stride, n, netif=NetIf.make(),
                                        length=0 if per_frame_lens else 64,
                                        lens=torch.from_numpy(lens.view(np.int16)).to(dev) if per_frame_lens else None,
                                        hist=hist)
    torch.cuda.synchronize()
    assert_records_equal(protocol.records(out), want, None, "strided")
    assert np.array_equal(hist.cpu().numpy().astype(np.int64), whist.astype(np.int64))


def test_fused_flow_and_route_entries(dev, oracle_lib, golden):
    """halo_rx_parse_flow_batch_device and halo_rx_parse_route_batch_device at n = 128 with one
    deviating frame: the plain parse's records, and hashes / route ids of those records."""
    import torch

    from halo_amd import _lib, protocol
    from halo_amd._lib import NetIf
    from halo_amd.route import RouteTable

    frames = _one_deviant(golden, name="tcp_ok")
    frames[70] = udp_frame(payload=bytes(22), dst_ip=bytes([10, 0, 0, 1]))
    data, offs, lens = pack(frames)
    n = len(frames)
    want, _ = oracle_lib.rx_batch(data, lens, oracle_lib.NetIf.make(), 1, offsets_dw=offs)
    d, o, ln = to_dev(dev, data, offs, lens)
    stream = torch.cuda.current_stream().cuda_stream
    word = 1 | _lib.variant_flags(1)

    out = torch.full((n, 32), 0xEE, dtype=torch.uint8, device=dev)
    h = torch.zeros(n, dtype=torch.int64, device=dev)
    b = torch.zeros(n, dtype=torch.int32, device=dev)
    _lib.check("fused flow", _lib.lib.halo_rx_parse_flow_batch_device(
        d.data_ptr(), o.data_ptr(), ln.data_ptr(), n, word, NetIf.make(), 74, out.data_ptr(), None, 1, 0,
        h.data_ptr(), 1 << 20, b.data_ptr(), stream))
    torch.cuda.synchronize()
    assert_records_equal(protocol.records(out), want, None, "fused parse + flow hash")
    wh, wb = oracle_lib.flow_hash_batch(np.array(want), 1, 0, 1 << 20)
    assert np.array_equal(h.cpu().numpy().view(np.uint64), wh)
    assert np.array_equal(b.cpu().numpy().view(np.uint32), wb)

    g, ora = RouteTable(0), oracle_lib.RouteTable()
    for r in ([0, 0, 1, 0], [0xC0A86400, 0xFFFFFF00, 0, 1], [0xC0A86464, 0xFFFFFFFF, 0, 2], [0x0A000000, 0xFF000000, 5, 3]):
        assert g.AddRoute(RouteTable.entry(*r)) == ora.add(r)
    g.sync()
    out = torch.full((n, 32), 0xEE, dtype=torch.uint8, device=dev)
    rid = torch.zeros(n, dtype=torch.int32, device=dev)
    _lib.check("fused route", _lib.lib.halo_rx_parse_route_batch_device(
        d.data_ptr(), o.data_ptr(), ln.data_ptr(), n, word, NetIf.make(), 74, out.data_ptr(), None, g._t,
        rid.data_ptr(), stream))
    torch.cuda.synchronize()
    assert_records_equal(protocol.records(out), want, None, "fused parse + route")
    assert np.array_equal(rid.cpu().numpy().view(np.uint32), ora.find_batch(want["dst_ip"]))


def test_multi_batch_entry(dev, oracle_lib, golden):
    """halo_rx_parse_batches_device: batches of 64 (all plain) and 65 frames (one deviating, and a
    partial window) in one launch, with a histogram."""
    import torch

    from halo_amd import protocol
    from halo_amd._lib import NetIf

    sets = [[plain(k) for k in range(64)], _one_deviant(golden, n=65, lane=63, name="ip_frag_mf")]
    batches, wants, want_hist = [], [], np.zeros(14, np.int64)
    for frames in sets:
        data, offs, lens = pack(frames)
        want, whist = oracle_lib.rx_batch(data, lens, oracle_lib.NetIf.make(), 1, offsets_dw=offs)
        wants.append(want)
        want_hist += whist.astype(np.int64)
        batches.append(to_dev(dev, data, offs, lens) + (torch.full((len(frames), 32), 0xEE, dtype=torch.uint8, device=dev),))
    hist = torch.zeros(14, dtype=torch.int32, device=dev)
    protocol.parse_frames_batches(batches, netif=NetIf.make(), max_len_hint=64, variant=1, hist=hist)
    torch.cuda.synchronize()
    for k, (bt, want) in enumerate(zip(batches, wants)):
        assert_records_equal(protocol.records(bt[3]), want, None, f"multi-batch, batch {k}")
    assert np.array_equal(hist.cpu().numpy().astype(np.int64), want_hist)


def test_dependent_launches_into_one_out(dev, oracle_lib, golden):
    """Two different 128-frame batches parsed back to back on one stream into the same `out`: the
    second launch's records are the only ones visible."""
    import torch

    from halo_amd import protocol
    from halo_amd._lib import NetIf

    first = [plain(k + 100) for k in range(128)]
    second = _one_deviant(golden, name="arp_request_bcast", lane=0)
    out = torch.full((128, 32), 0xEE, dtype=torch.uint8, device=dev)
    args = []
    for frames in (first, second):
        data, offs, lens = pack(frames)
        args.append((to_dev(dev, data, offs, lens), oracle_lib.rx_batch(data, lens, oracle_lib.NetIf.make(), 1,
                                                                        offsets_dw=offs)[0]))
    assert args[0][1].tobytes() != args[1][1].tobytes()
    for (d, o, ln), _ in args:
        protocol.parse_frames_batch(d, o, ln, netif=NetIf.make(), max_len_hint=64, variant=1, out=out)
    torch.cuda.synchronize()
    assert_records_equal(protocol.records(out), args[1][1], None, "second of two dependent launches")
