"""GPU: the DHCP decode and reply build on the device (halo_amd/csrc/rx_dhcp.hip and tx_dhcp.hip
through halo_dhcp_decode_device / halo_dhcp_reply_build_device) against tests/dhcp_model.py and the
host loops — bit for bit, every output 0xA5-prefilled with a sentinel element behind it and the
workspace's sentinel intact: the crafted payloads of tests/dhcp_cases.py; selected-record counts
around a wavefront and a tile at three densities among UDP and TCP records; one case past one scan
pass; unwritten records and an index_cap below the record count; msg_cap cutting on and inside the
selected set; one workspace for two calls; the reply build for counts around a wavefront and a
tile; and one chain entirely in HBM, from client frames to the server's replies as frames, parsed
and decoded again."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import dhcp_cases as C
from tests import dhcp_model as M

pytestmark = pytest.mark.gpu
A5_64 = int(np.array([0xA5A5A5A5A5A5A5A5], np.uint64).view(np.int64)[0])
CASES = C.crafted()


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
    """(stream, delivery summary, index) of a Delivery as cuda tensors; the stream's buffer is padded
    to whole int64 so that it uploads 8-byte aligned."""
    out = np.concatenate([d.out, np.full(-len(d.out) % 8, 0xEE, np.uint8)])
    return _t(dev, out.view(np.int64)), _t(dev, d.summary_raw.view(np.int64)), _t(dev, d.index_raw.reshape(-1).view(np.int64))


def _device(dev, up, index_cap, msg_cap, *, ws=None):
    """halo_dhcp_decode_device into 0xA5-filled device outputs, straight through ctypes."""
    import torch

    from halo_amd import _lib

    out, dsum, index = up
    mg = torch.full(((msg_cap + 1) * 16,), A5_64, dtype=torch.int64, device=dev)
    sm = torch.full((9,), A5_64, dtype=torch.int64, device=dev)
    wsb = int(_lib.lib.halo_dhcp_decode_workspace(index_cap))
    if ws is None:
        ws = torch.full((wsb // 8 + 1,), A5_64, dtype=torch.int64, device=dev)
    rc = _lib.lib.halo_dhcp_decode_device(_lib.ptr(out), _lib.ptr(dsum), _lib.ptr(index), index_cap, _lib.ptr(mg), msg_cap, _lib.ptr(sm),
                                          _lib.ptr(ws), wsb, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert int(ws[-1].item()) == A5_64, "the workspace was overrun"  # its last element is the sentinel
    return dict(msgs=mg.cpu().numpy().view(np.uint8).reshape(-1, 128), summary=sm.cpu().numpy().view(np.uint8))


def _host(d, index_cap, msg_cap):
    from halo_amd import _lib

    got = dict(msgs=np.full((msg_cap + 1, 128), C.FILL, np.uint8), summary=np.full(64 + 8, C.FILL, np.uint8))
    assert _lib.lib.halo_dhcp_decode_host(_lib.ptr(d.out), _lib.ptr(d.summary_raw), _lib.ptr(d.index_raw), index_cap,
                                          _lib.ptr(got["msgs"]), msg_cap, _lib.ptr(got["summary"])) == 0
    return got


def _check(dev, d, msg_cap, what="", *, index_cap=None, up=None, ws=None, want=None):
    """device == model == host for one call; returns the model's Want."""
    cap = d.index_cap if index_cap is None else index_cap
    if want is None:
        want = M.decode(d.out, d.records_total, d.index, cap, msg_cap)
    got = _device(dev, up or _upload(dev, d), cap, msg_cap, ws=ws)
    C.check_outputs(got, want, msg_cap, what)
    host = _host(d, cap, msg_cap)
    for k in ("msgs", "summary"):
        assert np.array_equal(got[k], host[k]), (what, k)
    return want


def test_crafted_set_matches_model_and_host(dev):
    d = C.Delivery(C.dhcp_items(CASES))
    want = _check(dev, d, len(CASES), "crafted")
    assert (want.summary["status_counts"] > 0).all() and (want.summary["type_counts"] > 0).all()
    # the same payloads one 4-byte step further into the stream, with a capacity that just fits
    d2 = C.Delivery([(C.UDP, 5000, 53, b"\0" * 5)] + C.dhcp_items(CASES))
    _check(dev, d2, len(CASES), "shifted, exact capacity")


def _mixed(n_dhcp, density, seed):
    """n_dhcp DHCP records (crafted payloads below 700 bytes) among UDP and TCP records of other
    ports: every record, one in three, or one in fifty."""
    rng = np.random.default_rng(seed)
    pool = [(p, ports) for _, p, ports in CASES if len(p) < 700]
    step = {"all": 1, "third": 3, "fiftieth": 50}[density]
    items = []
    for i in range(n_dhcp):
        for g in range(step - 1):
            filler = C.rnd(i + g, int(rng.integers(0, 9)))
            items.append(((C.UDP, 5000, 53, filler), (C.TCP, 40000, 67, filler), (C.UDP, 68, 67, filler))[(i + g) % 3])
        p, ports = pool[int(rng.integers(len(pool)))]
        items.append((C.DHCP, ports[0], ports[1], p))
    return items


@pytest.mark.parametrize("density", ("all", "third", "fiftieth"))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257))
def test_counts_around_a_wave_and_a_tile(dev, n, density):
    d = C.Delivery(_mixed(n, density, n))
    want = _check(dev, d, n, (n, density))
    assert int(want.summary["msgs"]) == n == int(want.summary["msgs_written"])


def test_past_one_scan_pass(dev):
    """kScanPass * kTile + 300 index entries of minimal records with a few hundred DHCP ones among
    them: the scan's second pass carries the base over."""
    from tests.kcp_cases import read_constants

    c = read_constants()
    n = c["kScanPass"] * c["kTile"] + 300
    assert n == 262144 + 300
    at = sorted({0, 255, 256, n - 301, n - 300, n - 299, n - 1, *range(7, n, 911)})
    payload = C.discover(b"pc-in-the-second-pass")
    d = C.minimal_record_stream(n, at, payload)
    one = M.decode_one(0, 0, 68, 67, payload)
    msgs = np.repeat(np.array([one], M.MSG), len(at))
    msgs["index"], msgs["remote_ip"] = at, 0x0A000001 + np.array(at)
    s = np.zeros(1, M.SUMMARY)[0]
    s["msgs"] = s["msgs_written"] = len(at)
    s["status_counts"][M.OK] = s["type_counts"][M.DISCOVER] = len(at)
    want = M.Want(msgs, s)
    # the vectorised expectation is the model's on a small stream of the same make
    small_at = [0, 5, 255, 256, 999]
    small = C.minimal_record_stream(1000, small_at, payload)
    m = small.want(10)
    assert m.msgs["index"].tolist() == small_at and m.msgs[1].tobytes()[4:28] == one.tobytes()[4:28] and len(at) > 250
    _check(dev, d, len(at), "past the scan pass", want=want)
    _check(dev, d, 100, "past the scan pass, cut", want=M.Want(msgs[:100], np.array([(len(at), 100, [100, 0, 0, 0, 0], [0, 100] + [0] * 7)], M.SUMMARY)[0]))


def test_unwritten_records_index_cap_and_capacity_cuts(dev):
    import torch

    from halo_amd import _lib

    items = _mixed(300, "third", 5)
    d = C.Delivery(items, unwritten=300)  # the region cut left 300 records unwritten
    up = _upload(dev, d)
    assert d.index_cap == 1200
    _check(dev, d, 300, "unwritten tail", up=up)
    for cap in (1, 2, 3, 64, 255, 256, 257, 899):
        _check(dev, d, 300, ("index_cap below records", cap), index_cap=cap, up=up)
    for msg_cap in (0, 1, 63, 64, 65, 255, 256, 257, 299, 300, 301):
        want = _check(dev, d, msg_cap, ("msg_cap", msg_cap), up=up)
        assert int(want.summary["msgs"]) == 300 and int(want.summary["msgs_written"]) == min(msg_cap, 300)
    # one workspace, two calls on one stream, the second over another delivery
    ws = torch.full((int(_lib.lib.halo_dhcp_decode_workspace(d.index_cap)) // 8 + 1,), A5_64, dtype=torch.int64, device=dev)
    first = _check(dev, d, 300, "first", up=up, ws=ws)
    _check(dev, C.Delivery(C.dhcp_items(CASES[:30])), 30, "second", ws=ws)
    again = _check(dev, d, 300, "again", up=up, ws=ws)
    assert first.msgs.tobytes() == again.msgs.tobytes()


def test_empty_delivery_and_zero_index_cap(dev):
    d = C.Delivery([])
    want = _check(dev, d, 4, "empty delivery", index_cap=1)
    assert want.summary.tobytes() == bytes(64)
    got = _device(dev, _upload(dev, C.Delivery(C.dhcp_items(CASES[:3]))), 0, 4)
    assert got["summary"][:64].tobytes() == bytes(64) and (got["msgs"] == C.FILL).all()


def test_device_entry_argument_checks_over_device_memory(dev):
    """tests/test_dhcp_host.py's argument lists over device memory: the well-formed calls run (an
    empty delivery: a zero summary; two zero replies: zero slots), every other one is HALO_E_INVAL
    and writes nothing."""
    import torch

    from halo_amd import _lib

    buf = torch.zeros(4096 + 64, dtype=torch.uint8, device=dev)
    base = buf.data_ptr() + (-buf.data_ptr()) % 64
    buf[base - buf.data_ptr() + 128:base - buf.data_ptr() + 256] = C.FILL  # the summary, the workspace and the gap behind them
    torch.cuda.synchronize()
    ok, answers = C.decode_entry_answers(base)
    torch.cuda.synchronize()
    assert ok == 0 and len(answers) >= 16
    for what, rc in answers:
        assert rc == _lib.HALO_E_INVAL, (what, rc)
    h = buf.cpu().numpy()[base - buf.data_ptr():]
    assert not h[128:192].any() and (h[200:256] == C.FILL).all() and not h[256:4096].any() and not h[:128].any()
    buf.zero_()
    buf[base - buf.data_ptr() + 64:base - buf.data_ptr() + 1024] = C.FILL
    torch.cuda.synchronize()
    ok, answers = C.build_entry_answers(base)
    torch.cuda.synchronize()
    assert ok == 0 and len(answers) >= 9
    for what, rc in answers:
        assert rc == _lib.HALO_E_INVAL, (what, rc)
    h = buf.cpu().numpy()[base - buf.data_ptr():]
    assert not h[64:144].any() and (h[144:256] == C.FILL).all() and not h[256:832].any() and (h[832:1024] == C.FILL).all()


def _random_replies(n, seed):
    rng = np.random.default_rng(seed)
    r = np.zeros(n, M.REPLY)
    r["kind"] = rng.choice([M.OFFER, M.ACK, M.NAK, M.REQUEST, M.DISCOVER, 4, 0, 255], n, p=[.2, .2, .2, .15, .15, .04, .03, .03])
    r["xid"] = rng.integers(0, 256, (n, 4))
    r["chaddr"] = rng.integers(0, 256, (n, 6))
    for f in ("yiaddr", "req_ip", "server_id"):
        r[f] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    return r


@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
def test_reply_build_matches_model_and_host(dev, n):
    import torch

    from halo_amd import _lib
    from halo_amd.dhcp import build_replies_host

    cfg = _lib.DhcpConfig()
    cfg.ip, cfg.network_mask, cfg.dns = 0xC0A86464, 0xFFFFFF00, 0x08080404
    r = _random_replies(n, n)
    payload = torch.full(((n + 1) * 36,), A5_64, dtype=torch.int64, device=dev)  # 288 bytes = 36 int64
    descs = torch.full(((n + 1) * 5,), A5_64, dtype=torch.int64, device=dev)
    rc = _lib.lib.halo_dhcp_reply_build_device(ctypes.byref(cfg), _lib.ptr(_t(dev, r.view(np.int64))), n, _lib.ptr(payload), _lib.ptr(descs),
                                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    p, d = payload.cpu().numpy().view(np.uint8).reshape(-1, 288), descs.cpu().numpy().view(np.uint8).reshape(-1, 40)
    slots, want = M.build(r, cfg.ip, cfg.network_mask, cfg.dns)
    assert p[:n].tobytes() == slots.tobytes() and d[:n].tobytes() == want.tobytes()
    assert (p[n:] == C.FILL).all() and (d[n:] == C.FILL).all()
    host = build_replies_host(r, config=cfg)
    assert host.slots().tobytes() == p[:n].tobytes() and host.descs().tobytes() == d[:n].tobytes()


def test_chain_in_hbm(dev):
    """Client frames in HBM -> parse -> deliver(dhcp=True) -> decode; the descriptors downloaded and
    fed to a DhcpServer; the replies uploaded, built, taken through halo_tx_build_batch_device;
    those frames parsed, delivered and decoded again: the decoded OFFER / ACK / NAK fields and the
    lease table equal the model's."""
    import torch

    from halo_amd import deliver, dhcp, protocol
    from halo_amd.protocol import TxBuilder
    from tests import deliver_cases as DC

    cfg = dict(ip=DC.OWN_IP, network_mask=0xFFFFFF00, dns=0x08080808, mac=DC.MAC, capacity=40)
    net = DC.OWN_IP & 0xFFFFFF00
    rng = np.random.default_rng(11)
    frames, payloads = [], []
    for i in range(200):
        mac = bytes([2, 0, 0, 0, 0, int(rng.integers(0, 30))])
        kind = (M.DISCOVER, M.REQUEST, M.REQUEST, M.RELEASE)[int(rng.integers(0, 4))]
        ip = net + int(rng.integers(1, 60))
        name = (b"", b"pc%d" % i, C.rnd(i, 70))[int(rng.integers(0, 3))]
        if kind == M.DISCOVER:
            p = C.discover(name, req_ip=ip if i % 2 else None, chaddr=mac, xid=C.rnd(i, 4))
        elif kind == M.REQUEST:
            p = C.request(ip if i % 7 else net + 300, name, chaddr=mac, xid=C.rnd(i, 4))
        else:
            p = C.release(chaddr=mac, xid=C.rnd(i, 4))
        frames.append(DC.udp(67, p, src=ip if kind == M.RELEASE else 0, dst=DC.BCAST, sport=68))
        payloads.append((p, ip if kind == M.RELEASE else 0))
        if i % 3 == 0:
            frames.append(DC.udp(53, b"not dhcp"))
    data, offs, lens = DC.pack(3, frames)
    d, o, ln = _t(dev, data), _t(dev, offs.view(np.int32)), _t(dev, lens.view(np.int16))
    nif = DC.lib_netif()
    recs = protocol.parse_frames_batch(d, o, ln, netif=nif)
    dl = deliver(d, o, ln, recs, netif=nif, region_bytes=1 << 20, index_cap=len(frames), dhcp=True)
    dec = dhcp.decode(dl, msg_cap=len(frames))
    assert dec.msgs_raw.is_cuda and int(dec.summary["msgs_written"]) == 200 == int(dec.summary["status_counts"][M.OK])
    want_msgs = np.array([M.decode_one(0, rip, 68, 67, p) for p, rip in payloads], M.MSG)
    got_msgs = dec.msgs.copy()
    got_msgs["index"] = 0
    assert got_msgs.tobytes() == want_msgs.tobytes()
    assert dhcp.decode_host(dl, msg_cap=len(frames)).msgs.tobytes() == dec.msgs.tobytes()
    server, model = dhcp.DhcpServer(**cfg), M.Server(**cfg)
    r = dec.feed(server, 1000)
    replies, verdicts, _ = model.handle(dec.msgs, 1000)
    assert r.replies.tobytes() == replies.tobytes() and r.verdicts.tolist() == verdicts.tolist()
    assert server.leases().tobytes() == model.leases().tobytes() and 5 < len(server.leases()) <= 40
    assert {M.OFFER, M.ACK, M.NAK} == set(replies["kind"].tolist()) and len(replies) > 100
    # the way back: upload, build the payloads and descriptors, build the frames
    n = len(replies)
    b = dhcp.build_replies(_t(dev, r.replies.view(np.uint8)), config=server)
    stride = 1536
    out_frames, out_lens, res = b.build(TxBuilder(n, device=dev, ip_id=5), netif=nif, out_stride=stride, max_payload_hint=288)
    o2 = torch.arange(n, dtype=torch.int32, device=dev) * (stride // 4)
    flat = out_frames.reshape(-1)
    recs2 = protocol.parse_frames_batch(flat, o2, out_lens, netif=nif)
    dl2 = deliver(flat, o2, out_lens, recs2, netif=nif, region_bytes=1 << 20, index_cap=n, dhcp=True)
    dec2 = dhcp.decode(dl2, msg_cap=n)
    torch.cuda.synchronize()
    assert not res.cpu().numpy().any()
    slots, _ = M.build(replies, cfg["ip"], cfg["network_mask"], cfg["dns"])
    assert b.slots().tobytes() == slots.tobytes()
    m = dec2.msgs
    assert len(m) == n and (m["status"] == M.OK).all() and (m["dir"] == M.TO_CLIENT).all() and (m["remote_ip"] == cfg["ip"]).all()
    want2 = np.array([M.decode_one(k, cfg["ip"], 67, 68, M.build_one(q, cfg["ip"], cfg["network_mask"], cfg["dns"])) for k, q in enumerate(replies)],
                     M.MSG)
    assert m.tobytes() == want2.tobytes()
    assert m["msg_type"].tolist() == replies["kind"].tolist() and m["yiaddr"].tolist() == replies["yiaddr"].tolist()
    assert m["xid"].tobytes() == replies["xid"].tobytes() and m["chaddr"].tobytes() == replies["chaddr"].tobytes()
    # on a stream that is not the current one: the same outputs, the workspace held by the result
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    other = dhcp.decode(dl, msg_cap=len(frames), stream=side)
    side.synchronize()
    assert other.workspace is not None and other.msgs.tobytes() == dec.msgs.tobytes()
    no_index = deliver(d, o, ln, recs, netif=nif, region_bytes=1 << 20, dhcp=True)
    with pytest.raises(ValueError):
        dhcp.decode(no_index, msg_cap=8)
