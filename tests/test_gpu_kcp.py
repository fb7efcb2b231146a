"""GPU: KCP ingest on the device (halo_amd/csrc/rx_kcp.hip through halo_kcp_ingest_device) against
tests/kcp_model.py, which works from the delivered payload bytes, and against the host loop —
datagram records, segment descriptors and summary bit for bit, every output 0xA5-prefilled with a
sentinel element behind it and the workspace's sentinel intact: the crafted datagrams of
tests/kcp_cases.py in all four byte-check modes (payload lengths around 20 and H, every ENet type
and near miss, every structural failure, segment data at each start alignment and end residue for
the XXH3 class edges and the lengths around the CRC chunk and stride, an MTU segment, one 65,507-
byte datagram, 2,040 empty segments); datagram counts around a wavefront and a tile at three
selection densities, and past one scan pass; other kinds, other ports, unwritten records and an
index_cap below the records; capacity cuts inside a datagram and on its boundary and one workspace
for two calls; one chain from frames in HBM to ``feed``; and the XXH3 entry on its canonical
fixture, unchanged."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from tests import kcp_cases as C
from tests import kcp_model as M

pytestmark = pytest.mark.gpu
A5_64 = int(np.array([0xA5A5A5A5A5A5A5A5], np.uint64).view(np.int64)[0])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


def _t(dev, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _upload(dev, d):
    """(stream, delivery summary, index) of a tests/kcp_cases.Delivery as cuda tensors."""
    return _t(dev, d.out), _t(dev, d.summary_raw.view(np.int64)), _t(dev, d.index_raw.reshape(-1).view(np.int64))


def _device(dev, up, index_cap, mode, dgram_cap, seg_cap, *, port=C.PORT, ws=None):
    """halo_kcp_ingest_device into 0xA5-filled device outputs, straight through ctypes: the raw
    arrays downloaded, as tests/kcp_cases.check_outputs takes them."""
    import torch

    from halo_amd import _lib

    out, dsum, index = up
    dg = torch.full(((dgram_cap + 1) * 5,), A5_64, dtype=torch.int64, device=dev)
    sg = torch.full(((seg_cap + 1) * 4,), A5_64, dtype=torch.int64, device=dev)
    sm = torch.full((13,), A5_64, dtype=torch.int64, device=dev)
    wsb = int(_lib.lib.halo_kcp_ingest_workspace(index_cap, seg_cap))
    if ws is None:
        ws = torch.full((wsb // 8 + 1,), A5_64, dtype=torch.int64, device=dev)
    cfg = _lib.KcpConfig()
    cfg.byte_check_mode, cfg.port, cfg.dgram_cap, cfg.seg_cap = mode, port, dgram_cap, seg_cap
    rc = _lib.lib.halo_kcp_ingest_device(ctypes.byref(cfg), _lib.ptr(out), _lib.ptr(dsum), _lib.ptr(index), index_cap, _lib.ptr(dg),
                                         _lib.ptr(sg), _lib.ptr(sm), _lib.ptr(ws), wsb, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert int(ws[-1].item()) == A5_64, "the workspace was overrun"  # its last element is the sentinel
    return dict(dgrams=dg.cpu().numpy().view(np.uint8).reshape(-1, 40), segs=sg.cpu().numpy().view(np.uint8).reshape(-1, 32),
                summary=sm.cpu().numpy().view(np.uint8))


def _host(d, index_cap, mode, dgram_cap, seg_cap, port=C.PORT):
    from halo_amd import _lib

    cfg = _lib.KcpConfig()
    cfg.byte_check_mode, cfg.port, cfg.dgram_cap, cfg.seg_cap = mode, port, dgram_cap, seg_cap
    dg = np.full((dgram_cap + 1, 40), C.FILL, np.uint8)
    sg = np.full((seg_cap + 1, 32), C.FILL, np.uint8)
    sm = np.full(96 + 8, C.FILL, np.uint8)
    assert _lib.lib.halo_kcp_ingest_host(ctypes.byref(cfg), _lib.ptr(d.out), _lib.ptr(d.summary_raw), _lib.ptr(d.index_raw), index_cap,
                                         _lib.ptr(dg), _lib.ptr(sg), _lib.ptr(sm)) == 0
    return dict(dgrams=dg, segs=sg, summary=sm)


def _check(dev, d, mode, dgram_cap, seg_cap, what="", *, port=C.PORT, index_cap=None, up=None, ws=None):
    """device == model == host for one call; returns the model's Want."""
    cap = d.index_cap if index_cap is None else index_cap
    want = M.want_of(d, port=port, mode=mode, dgram_cap=dgram_cap, seg_cap=seg_cap, index_cap=cap)
    got = _device(dev, up or _upload(dev, d), cap, mode, dgram_cap, seg_cap, port=port, ws=ws)
    C.check_outputs(got, want, dgram_cap, seg_cap, (what, mode))
    host = _host(d, cap, mode, dgram_cap, seg_cap, port)
    for k in ("dgrams", "segs", "summary"):
        assert np.array_equal(got[k], host[k]), (what, mode, k)
    return want


@pytest.mark.parametrize("mode", M.MODES)
def test_crafted_set_matches_model_and_host(dev, mode):
    cases = C.crafted(mode)
    d = C.Delivery(C.udp([p for _, p in cases]))
    want = _check(dev, d, mode, len(cases), 8192, "crafted")
    s = want.summary
    assert int(s["dgrams_written"]) == int(s["dgrams"]) > 40 and int(s["segs"]) > 2100 and int(s["ignored"]) >= 8
    assert list(s["enet_counts"]) == [1, 1, 1, 1] and all(int(c) > 0 for c in s["ret_counts"][:4])
    assert (int(s["ret_counts"][4]) > 0) == (mode != M.DISABLED)
    assert {int(x) for x in want.segs["check"]} == {M.DISABLED: {0}}.get(mode, {0, 1, 2})
    # the same datagrams one 4-byte step further into the stream and with capacities that just fit
    d2 = C.Delivery(C.udp([b"\x00" * 5] + [p for _, p in cases]))
    _check(dev, d2, mode, int(s["dgrams"]), int(s["segs"]), "shifted, exact capacities")


@pytest.mark.parametrize("density", ("none", "sparse", "all"))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257, 600))
def test_counts_around_a_wave_and_a_tile(dev, n, density):
    mode = (M.CRC32, M.XXH3, M.ZERO, M.DISABLED)[n % 4]
    rng = np.random.default_rng(n)
    pool = [p for _, p in C.crafted(mode) if len(p) < 700]
    items = []
    for i in range(n):
        p = pool[int(rng.integers(len(pool)))]
        ours = {"none": False, "all": True}.get(density, rng.random() < 0.15 or i in (0, 63, 64, 255, 256, n - 1))
        items.append((C.UDP, C.PORT, p) if ours else ((C.TCP, C.PORT, p), (C.UDP, C.PORT ^ 1, p), (C.DHCP, 68, p))[i % 3])
    want = _check(dev, C.Delivery(items), mode, n, 16 * n + 64, (n, density))
    assert (int(want.summary["dgrams"]) + int(want.summary["ignored"]) == 0) == (density == "none")


@pytest.mark.parametrize("mode", (M.DISABLED, M.XXH3))
def test_unwritten_records_index_cap_and_other_ports(dev, mode):
    ps = [p for _, p in C.crafted(mode) if len(p) < 1500]
    items = [(C.UDP, C.PORT, p) if i % 3 else ((C.UDP, 53, p), (C.TCP, C.PORT, p))[i % 2] for i, p in enumerate(ps * 6)]
    d = C.Delivery(items, unwritten=300)  # the region cut left 300 records unwritten
    up = _upload(dev, d)
    assert d.index_cap == len(items) + 300 and d.index_cap > 256
    _check(dev, d, mode, len(items), 4096, "unwritten tail", up=up)
    _check(dev, d, mode, len(items), 4096, "port 53", port=53, up=up)
    for cap in (1, 64, 255, 256, 257, len(items) - 1):
        _check(dev, d, mode, len(items), 4096, ("index_cap below records", cap), index_cap=cap, up=up)


def _uniform(n, mode):
    """n datagrams of one empty ACK segment each (sn = the datagram's number), built with numpy;
    every 1777th has cmd 85 (ret -3, no descriptor). Returns (Delivery-like, expected arrays)."""
    H = M.overhead(mode)
    rec = np.dtype([("frame", "<u4"), ("kind", "u1"), ("fl", "u1"), ("plen", "<u2"), ("rip", "<u4"), ("rport", "<u2"), ("lport", "<u2"),
                    ("seq", "<u4"), ("ack", "<u4"), ("conv", "<u8"), ("cmd", "u1"), ("frg", "u1"), ("wnd", "<u2"), ("ts", "<u4"),
                    ("sn", "<u4"), ("una", "<u4"), ("len", "<u4")] + ([("hash", "<u4")] if H == 32 else []))
    assert rec.itemsize == 24 + H
    r = np.zeros(n, rec)
    k = np.arange(n, dtype=np.uint32)
    r["frame"], r["kind"], r["plen"], r["lport"], r["conv"], r["cmd"], r["wnd"], r["sn"] = k, C.UDP, H, C.PORT, C.CONV, C.ACK, 32, k
    bad = (k % 1777) == 5
    r["cmd"][bad] = 85
    d = C.Delivery([])
    d.out = np.concatenate([r.view(np.uint8).reshape(-1), np.full(16, 0xEE, np.uint8)])
    d.bytes_written = n * rec.itemsize
    sm = d.summary_raw.view(np.dtype([("records", "<u4"), ("records_written", "<u4"), ("bytes", "<u8"), ("bytes_written", "<u8"),
                                      ("kind_counts", "<u4", (3,)), ("skipped", "<u4")]))
    sm["records"] = sm["records_written"] = n
    sm["bytes"] = sm["bytes_written"] = d.bytes_written
    idx = np.zeros((n, 2), np.uint32)
    idx[:, 0], idx[:, 1] = k, k * rec.itemsize
    d.index_raw, d.index_cap = idx.view(np.uint8).reshape(-1, 8), n
    dg = np.zeros(n, M.DGRAM)
    dg["index"], dg["conv0"], dg["payload_len"] = k, C.CONV, H
    dg["ret"][bad] = -3
    walked = (~bad).astype(np.uint32)
    dg["n_segs"] = dg["n_walked"] = walked
    dg["first_seg"] = np.cumsum(walked) - walked
    ok = np.flatnonzero(~bad)
    sg = np.zeros(len(ok), M.SEG)
    sg["dgram"], sg["cmd"], sg["wnd"], sg["sn"], sg["data_off"] = ok, C.ACK, 32, ok, ok * rec.itemsize + 24 + H
    s = np.zeros(1, M.SUMMARY)[0]
    s["dgrams"] = s["dgrams_written"] = s["in_pkts"] = n
    s["segs"] = s["segs_written"] = s["in_segs"] = len(ok)
    s["ret_counts"][0], s["ret_counts"][3], s["in_errs"], s["in_bytes"] = len(ok), n - len(ok), n - len(ok), n * H
    return d, M.Want(dg, sg, s, None)


@pytest.mark.parametrize("mode", (M.DISABLED, M.XXH3))
def test_past_one_scan_pass(dev, mode):
    """kScanPass * kTile + 1 minimal datagrams: the scan's second pass carries both bases over."""
    c = C.read_constants()
    n = c["kScanPass"] * c["kTile"] + 1
    d, want = _uniform(n, mode)
    # the vectorised expectation is the model's on a prefix
    small, want_small = _uniform(4000, mode)
    m = M.want_of(small, port=C.PORT, mode=mode, dgram_cap=4000, seg_cap=4000)
    assert m.dgrams.tobytes() == want_small.dgrams.tobytes() and m.segs.tobytes() == want_small.segs.tobytes()
    assert m.summary.tobytes() == want_small.summary.tobytes()
    got = _device(dev, _upload(dev, d), n, mode, n, n)
    C.check_outputs(got, want, n, n, "past the scan pass")
    host = _host(d, n, mode, n, n)
    assert all(np.array_equal(got[k], host[k]) for k in got)


@pytest.mark.parametrize("mode", (M.ZERO, M.CRC32, M.XXH3))
def test_capacity_cuts_and_one_workspace_for_two_calls(dev, mode):
    import torch

    from halo_amd import _lib

    six = [C.seg(mode, C.ACK) * 3, C.enet(0), C.seg(mode, C.PUSH, b"x" * 9) * 5, C.seg(mode, C.PUSH, b"bad", field=3) + C.seg(mode, C.ACK),
           C.enet(2), C.seg(mode, C.ACK) * 2]
    d = C.Delivery(C.udp(six * 60))  # 360 datagrams, 12 walked segments per six: tiles end inside a group
    up = _upload(dev, d)
    for dgram_cap, seg_cap in ((360, 720), (360, 719), (360, 718), (360, 8), (360, 7), (360, 3), (360, 2), (360, 0), (0, 720), (1, 720),
                               (255, 720), (256, 720), (257, 720), (360, 12 * 42 + 3 + 5), (360, 12 * 42 + 3 + 4), (359, 9999)):
        want = _check(dev, d, mode, dgram_cap, seg_cap, (dgram_cap, seg_cap), up=up)
        assert int(want.summary["dgrams"]) == 360 and int(want.summary["segs"]) == 720
    # one workspace, two calls on one stream, the second over another delivery with other capacities
    ws = torch.full((int(_lib.lib.halo_kcp_ingest_workspace(d.index_cap, 720)) // 8 + 1,), A5_64, dtype=torch.int64, device=dev)
    first = _check(dev, d, mode, 360, 720, "first", up=up, ws=ws)
    d2 = C.Delivery(C.udp([p for _, p in C.crafted(mode)][:30]))
    _check(dev, d2, mode, 30, 400, "second", ws=ws)
    again = _check(dev, d, mode, 360, 720, "again", up=up, ws=ws)
    assert first.dgrams.tobytes() == again.dgrams.tobytes()


def test_empty_delivery_and_zero_index_cap(dev):
    d = C.Delivery([])
    want = _check(dev, d, M.CRC32, 4, 4, "empty delivery", index_cap=1)
    assert want.summary.tobytes() == bytes(96)
    got = _device(dev, _upload(dev, C.Delivery(C.udp([C.enet(1)]))), 0, M.CRC32, 4, 4)
    assert got["summary"][:96].tobytes() == bytes(96) and (got["dgrams"] == C.FILL).all() and (got["segs"] == C.FILL).all()


def test_device_entry_argument_checks_over_device_memory(dev):
    """tests/test_kcp_host.py's argument list over device memory: the well-formed call runs (an
    empty delivery: a zero summary), every other one is HALO_E_INVAL and writes nothing."""
    import torch

    from halo_amd import _lib

    buf = torch.zeros(4096 + 64, dtype=torch.uint8, device=dev)
    base = buf.data_ptr() + (-buf.data_ptr()) % 64
    buf[base - buf.data_ptr() + 128:base - buf.data_ptr() + 256] = C.FILL  # the summary and the gap behind it
    torch.cuda.synchronize()
    ok, answers = C.device_entry_answers(base)
    torch.cuda.synchronize()
    assert ok == 0 and len(answers) >= 22
    for what, rc in answers:
        assert rc == _lib.HALO_E_INVAL, (what, rc)
    h = buf.cpu().numpy()[base - buf.data_ptr():]
    assert not h[128:224].any() and (h[224:256] == C.FILL).all() and not h[256:4096].any() and not h[:128].any()


def test_chain_frames_to_feed(dev):
    """Frames in HBM -> parse -> deliver -> ingest -> feed: the callbacks see what the model makes
    of the frames' own UDP payloads."""
    import torch

    from halo_amd import deliver, kcp, port_map, protocol
    from tests import deliver_cases as DC

    mode = M.CRC32
    payloads = [p for _, p in C.crafted(mode) if len(p) <= 1400]
    frames, expect_items = [], []
    for i, p in enumerate(payloads):
        frames.append(DC.udp(C.PORT, p, sport=6000 + i))
        expect_items.append((C.UDP, C.PORT, p))
        if i % 4 == 0:
            frames.append(DC.tcp(80, payload=b"tcp" * i))
            expect_items.append((C.TCP, 80, b""))
        if i % 5 == 0:
            frames.append(DC.udp(53, p))
            expect_items.append((C.UDP, 53, p))
    data, offs, lens = DC.pack(3, frames)
    d, o, ln = _t(dev, data), _t(dev, offs.view(np.int32)), _t(dev, lens.view(np.int16))
    nif = DC.lib_netif()
    recs = protocol.parse_frames_batch(d, o, ln, netif=nif)
    r = deliver(d, o, ln, recs, netif=nif, region_bytes=1 << 20, udp_ports=_t(dev, port_map((C.PORT, 53)).view(np.int32)),
                tcp_ports=_t(dev, port_map((80,)).view(np.int32)), index_cap=len(frames))
    got = kcp.ingest(r, port=C.PORT, byte_check_mode="crc32", seg_cap=4096, dgram_cap=len(frames))
    torch.cuda.synchronize()
    assert int(r.summary["records"]) == len(frames)
    # the model, from the frames' payload bytes (a Delivery made by hand from them)
    want = M.want_of(C.Delivery([(k, port, p) for k, port, p in expect_items]), port=C.PORT, mode=mode, dgram_cap=len(frames), seg_cap=4096)
    log = C.feed_log(got)
    assert log == want.feed and len(log) > 20
    for f in ("dgrams", "segs", "ret_counts", "enet_counts", "ignored", "bytes_hashed", "in_pkts", "in_bytes", "in_errs", "in_segs"):
        assert np.array_equal(got.summary[f], want.summary[f]), f
    assert got.dgrams_raw.is_cuda and [int(s["cmd"]) for s in got.segments_of(0)] == [int(s[0]) for s in want.feed[0][4]]
    # on a stream that is not the current one: the same outputs, the workspace held by the result
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    other = kcp.ingest(r, port=C.PORT, byte_check_mode="crc32", seg_cap=4096, dgram_cap=len(frames), stream=side)
    side.synchronize()
    assert other.workspace is not None and other.dgrams.tobytes() == got.dgrams.tobytes() and other.segs.tobytes() == got.segs.tobytes()
    no_index = deliver(d, o, ln, recs, netif=nif, region_bytes=1 << 20, udp_ports=_t(dev, port_map((C.PORT, 53)).view(np.int32)))
    with pytest.raises(ValueError):
        kcp.ingest(no_index, port=C.PORT, seg_cap=8, dgram_cap=8)
    host = kcp.ingest_host(r, port=C.PORT, byte_check_mode=mode, seg_cap=4096, dgram_cap=len(frames))
    assert host.dgrams.tobytes() == got.dgrams.tobytes() and host.segs.tobytes() == got.segs.tobytes() and host.summary == got.summary


def test_xxh3_entry_unchanged_on_the_canonical_fixture(dev):
    """halo_xxh3_64_batch_device still equals the canonical xxHash values (tests/golden/
    xxh3_canonical.npz) — the ingest's XXH3 mode launches that kernel, and must not have changed it."""
    import torch

    from halo_amd import hashcode

    z = np.load(os.path.join(ROOT, "tests", "golden", "xxh3_canonical.npz"))
    stream = np.fromfile(os.path.join(ROOT, "tests", "golden", "hash_stream.bin"), dtype=np.uint8)
    h = hashcode.GetHashCodeXXH3(_t(dev, stream), _t(dev, z["str_off"].astype(np.uint64).view(np.int64)),
                                 _t(dev, z["str_len"].astype(np.uint32).view(np.int32)))
    torch.cuda.synchronize()
    got = h.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, z["str_hash"])
