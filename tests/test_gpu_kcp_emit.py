"""GPU: KCP emit on the device (halo_amd/csrc/tx_kcp.hip through halo_kcp_emit_device) against
tests/kcp_emit_model.py and against the host loop — status, stream, datagram records, build
descriptors and summary bit for bit, every output 0xA5-prefilled with a sentinel behind it and the
workspace's sentinel intact: the crafted batches of tests/kcp_emit_cases.py in all four byte-check
modes; entry counts around a wavefront and a tile at three densities of non-OK entries; more tiles
than one scan pass; a session with more segments than an encode workgroup has groups; both
capacity cuts; one workspace for two calls; payload taken from a delivery stream, with a device
ingest result's descriptors emitted again without a download; and one chain emit -> transmit build
-> parse -> deliver -> ingest in crc32 and xxh3 modes."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from tests import kcp_cases as KC
from tests import kcp_emit_cases as C
from tests import kcp_emit_model as M

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
    """a numpy array of any dtype as a cuda int64 tensor (8-byte elements: torch aligns them, and more, itself)"""
    import torch

    raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    raw = np.concatenate([raw, np.zeros(-raw.size % 8 or (8 if raw.size == 0 else 0), np.uint8)])
    return torch.from_numpy(raw.view(np.int64)).to(dev)


def _upload(dev, arrays):
    sessions, segs, pay, nbytes = arrays
    return _t(dev, sessions), _t(dev, segs), _t(dev, pay), len(sessions), len(segs), nbytes


def _device(dev, up, mode, dgram_cap, stream_cap, *, ws=None, src_ip=C.SRC_IP, src_port=C.SRC_PORT):
    """halo_kcp_emit_device into 0xA5-filled device outputs, straight through ctypes: the raw arrays
    downloaded, as tests/kcp_emit_cases.check_outputs takes them."""
    import torch

    from halo_amd import _lib

    sessions, segs, pay, n_sessions, n_segs, nbytes = up
    assert stream_cap % 8 == 0
    out = torch.full((stream_cap // 8 + 1,), A5_64, dtype=torch.int64, device=dev)
    dg = torch.full(((dgram_cap + 1) * 2,), A5_64, dtype=torch.int64, device=dev)
    ds = torch.full(((dgram_cap + 1) * 5,), A5_64, dtype=torch.int64, device=dev)
    status = torch.full((n_sessions + 8,), 0xA5, dtype=torch.uint8, device=dev)
    sm = torch.full((12,), A5_64, dtype=torch.int64, device=dev)
    wsb = int(_lib.lib.halo_kcp_emit_workspace(n_sessions, n_segs))
    if ws is None:
        ws = torch.full((wsb // 8 + 1,), A5_64, dtype=torch.int64, device=dev)
    cfg = _lib.KcpEmitConfig()
    cfg.byte_check_mode, cfg.src_ip, cfg.src_port, cfg.dgram_cap, cfg.stream_cap = mode, src_ip, src_port, dgram_cap, stream_cap
    rc = _lib.lib.halo_kcp_emit_device(ctypes.byref(cfg), _lib.ptr(sessions), n_sessions, _lib.ptr(segs), n_segs, _lib.ptr(pay), nbytes,
                                       _lib.ptr(out), _lib.ptr(dg), _lib.ptr(ds), _lib.ptr(status), _lib.ptr(sm), _lib.ptr(ws), wsb,
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert int(ws[-1].item()) == A5_64, "the workspace was overrun"  # its last element is the sentinel
    return dict(stream=out.cpu().numpy().view(np.uint8), dgrams=dg.cpu().numpy().view(np.uint8).reshape(-1, 16),
                descs=ds.cpu().numpy().view(np.uint8).reshape(-1, 40), status=status.cpu().numpy(), summary=sm.cpu().numpy().view(np.uint8))


def _check(dev, arrays, mode, dgram_cap, stream_cap, what="", *, up=None, ws=None):
    """device == model == host for one call; returns the model's Want."""
    if isinstance(arrays, C.Batch):
        arrays = arrays.arrays()
    want = C.want(arrays, mode, dgram_cap, stream_cap)
    got = _device(dev, up or _upload(dev, arrays), mode, dgram_cap, stream_cap, ws=ws)
    C.check_outputs(got, want, len(arrays[0]), dgram_cap, stream_cap, (what, mode))
    host = C.host_call(arrays, mode, dgram_cap, stream_cap)
    for k in host:
        assert np.array_equal(got[k], host[k]), (what, mode, k)
    return want


@pytest.mark.parametrize("mode", M.MODES)
def test_crafted_set_matches_model_and_host(dev, mode):
    cases = C.crafted(mode)
    want = _check(dev, C.batch_of(cases), mode, 4096, 1 << 20, "crafted")
    s = want.summary
    assert all(int(c) > 3 for c in s["status_counts"]) and int(s["dgrams_written"]) == int(s["dgrams"]) > 60
    # the same batch with every segment's data one byte further on, and capacities that just fit
    shifted = C.Batch()
    shifted.payload += b"\x00"
    for _, fn in cases:
        fn(shifted)
    _check(dev, shifted, mode, int(s["dgrams"]), (int(s["bytes"]) + 7) & ~7, "shifted, capacities that just fit")


@pytest.mark.parametrize("bad", (0.0, 0.1, 0.6))
@pytest.mark.parametrize("n", (63, 64, 65, 255, 256, 257))
def test_counts_around_a_wave_and_a_tile(dev, n, bad):
    mode = (M.CRC32, M.XXH3, M.ZERO, M.DISABLED)[n % 4]
    want = _check(dev, C.random_batch(n, n, bad), mode, 4 * n, 1 << 18, (n, bad))
    assert (int(want.summary["status_counts"][1:].sum()) == 0) == (bad == 0.0)


def _constants():
    out = {}
    for name, pat in (("tx_kcp.h", r"constexpr uint32_t (kTile) = (\d+)"), ("tile_scan.h", r"constexpr uint32_t (kScanPass) = (\d+)"),
                      ("tx_kcp.h", r"constexpr uint32_t (kEncodeLanes) = (\d+)"), ("tx_kcp.h", r"constexpr uint32_t (kEncodeBlock) = (\d+)")):
        m = re.search(pat, open(os.path.join(ROOT, "halo_amd", "csrc", name)).read())
        out[m.group(1)] = int(m.group(2))
    return out


def _uniform(n, mode):
    """n entries of one empty ACK each (sn = the entry's number), built with numpy; every 1777th has
    mtu 20 (BAD_MTU, no datagram). Returns (arrays, Want)."""
    H = M.overhead(mode)
    k = np.arange(n, dtype=np.uint32)
    bad = (k % 1777) == 5
    ss = np.zeros(n, M.SESSION)
    ss["conv"], ss["first_seg"], ss["n_segs"], ss["mtu"], ss["dst_ip"], ss["dst_port"] = KC.CONV, k, 1, 1400, 0x0A000000 + k, k & 0xFFFF
    ss["mtu"][bad] = 20
    sg = np.zeros(n, M.SEG)
    sg["cmd"], sg["wnd"], sg["sn"], sg["ts"] = KC.ACK, 32, k, 7
    arrays = (ss, sg, np.zeros(4, np.uint8), 4)
    ok = np.flatnonzero(~bad).astype(np.uint32)
    hdr = np.dtype([("conv", "<u8"), ("cmd", "u1"), ("frg", "u1"), ("wnd", "<u2"), ("ts", "<u4"), ("sn", "<u4"), ("una", "<u4"),
                    ("len", "<u4")] + ([("hash", "<u4")] if H == 32 else []))
    h = np.zeros(len(ok), hdr)
    h["conv"], h["cmd"], h["wnd"], h["ts"], h["sn"] = KC.CONV, KC.ACK, 32, 7, ok
    rank = np.arange(len(ok), dtype=np.uint32)
    dg = np.zeros(len(ok), M.DGRAM)
    dg["offset"], dg["len"], dg["n_segs"], dg["session"], dg["first_seg"] = rank * H, H, 1, ok, ok
    ds = np.zeros(len(ok), M.DESC)
    ds["payload_off"], ds["payload_len"], ds["proto"], ds["src_port"], ds["src_ip"] = rank.astype(np.uint64) * H, H, 17, C.SRC_PORT, C.SRC_IP
    ds["dst_ip"], ds["dst_port"] = ss["dst_ip"][ok], ss["dst_port"][ok]
    s = np.zeros(1, M.SUMMARY)[0]
    s["sessions"] = s["sessions_written"] = s["dgrams"] = s["dgrams_written"] = s["segs"] = s["segs_written"] = len(ok)
    s["out_segs"] = s["out_pkts"] = len(ok)
    s["status_counts"][M.OK], s["status_counts"][M.BAD_MTU] = len(ok), n - len(ok)
    s["bytes"] = s["bytes_written"] = s["out_bytes"] = len(ok) * H
    return arrays, M.Want(bad.astype(np.uint8) * M.BAD_MTU, h.tobytes(), dg, ds, s)


@pytest.mark.parametrize("mode", (M.DISABLED, M.XXH3))
def test_past_one_scan_pass(dev, mode):
    """kScanPass * kTile + 1 minimal entries: the scan's second pass carries all three bases over."""
    c = _constants()
    n = c["kScanPass"] * c["kTile"] + 1
    arrays, want = _uniform(n, mode)
    # the vectorised expectation is the model's on a prefix
    small, want_small = _uniform(4000, mode)
    m = C.want(small, mode, 4000, 1 << 20)
    assert m.dgrams.tobytes() == want_small.dgrams.tobytes() and m.descs.tobytes() == want_small.descs.tobytes()
    assert m.stream == want_small.stream and m.summary.tobytes() == want_small.summary.tobytes() and np.array_equal(m.status, want_small.status)
    cap = (n * M.overhead(mode) + 7) & ~7
    got = _device(dev, _upload(dev, arrays), mode, n, cap)
    C.check_outputs(got, want, n, n, cap, "past the scan pass")
    host = C.host_call(arrays, mode, n, cap)
    assert all(np.array_equal(got[k], host[k]) for k in got)


@pytest.mark.parametrize("mode", (M.ZERO, M.CRC32, M.XXH3))
def test_a_session_longer_than_an_encode_workgroup(dev, mode):
    c = _constants()
    groups = c["kEncodeBlock"] // c["kEncodeLanes"]
    b = C.Batch()
    b.kcp([(KC.ACK,)])
    b.kcp([((KC.PUSH, KC.ACK, KC.PUSH)[i % 3], KC.rnd(i, (i * 37) % 300), i % 4) for i in range(5 * groups + 3)], mtu=1000)
    b.kcp([(KC.PUSH, KC.rnd(7, 1400 - 32))] * (groups + 1))
    want = _check(dev, b, mode, 4096, 1 << 18, "long session")
    assert int(want.summary["segs_written"]) == 1 + 5 * groups + 3 + groups + 1


@pytest.mark.parametrize("mode", (M.DISABLED, M.CRC32, M.XXH3))
def test_capacity_cuts_and_one_workspace_for_two_calls(dev, mode):
    import torch

    from halo_amd import _lib

    b = C.Batch()
    for k in range(300):  # more than a tile of entries: the cut falls in either tile
        b.kcp([(KC.PUSH, KC.rnd(k, 60 + k % 3), k % 4)] * 3, mtu=200)  # two datagrams per entry
        if k % 5 == 0:
            b.kcp([(KC.ACK,)], mtu=20)  # non-OK: does not end the prefix
        if k % 7 == 0:
            b.enet(k % 4)
    arrays = b.arrays()
    up = _upload(dev, arrays)
    full = C.want(arrays, mode, 1000, 1 << 20)
    nd, nb = int(full.summary["dgrams"]), int(full.summary["bytes"])
    ends = np.cumsum([(int(d["len"]) + 3) & ~3 for d in full.dgrams])
    assert nd == 600 + 43 and nb == int(ends[-1])
    for dgram_cap in (0, 1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, nd - 1, nd, nd + 1):  # inside an entry and on its boundary
        w = _check(dev, arrays, mode, dgram_cap, 1 << 20, ("dgram_cap", dgram_cap), up=up)
        assert int(w.summary["dgrams"]) == nd and int(w.summary["dgrams_written"]) <= dgram_cap
    for e in (0, 1, 2, 3, 500, 501, 502, nd - 2, nd - 1):  # the stream ends on, before and behind a datagram's end
        for stream_cap in {int(ends[e]) & ~7, (int(ends[e]) + 7) & ~7, (int(ends[e]) + 8) & ~7}:
            w = _check(dev, arrays, mode, 1000, stream_cap, ("stream_cap", stream_cap), up=up)
            assert int(w.summary["bytes"]) == nb and int(w.summary["bytes_written"]) <= stream_cap
    _check(dev, arrays, mode, 1000, 0, "no stream", up=up)
    # one workspace, two calls on one stream, the second over another batch with other capacities
    ws = torch.full((int(_lib.lib.halo_kcp_emit_workspace(len(arrays[0]), len(arrays[1]))) // 8 + 1,), A5_64, dtype=torch.int64, device=dev)
    first = _check(dev, arrays, mode, 1000, 1 << 20, "first", up=up, ws=ws)
    _check(dev, C.batch_of(C.crafted(mode)[:20]), mode, 64, 1 << 16, "second", ws=ws)
    again = _check(dev, arrays, mode, 1000, 1 << 20, "again", up=up, ws=ws)
    assert first.stream == again.stream


def test_no_sessions_zeroes_the_summary(dev):
    got = _device(dev, _upload(dev, C.Batch().arrays()), M.CRC32, 4, 64)
    assert got["summary"][:88].tobytes() == bytes(88) and (got["summary"][88:] == C.FILL).all()
    assert (got["stream"] == C.FILL).all() and (got["dgrams"] == C.FILL).all() and (got["descs"] == C.FILL).all()


def test_device_entry_argument_checks_over_device_memory(dev):
    """tests/test_kcp_emit_host.py's argument list over device memory: every call is HALO_E_INVAL and
    writes nothing."""
    import torch

    from halo_amd import _lib
    from tests.test_kcp_emit_host import entry_answers

    buf = torch.zeros(4096 + 64, dtype=torch.uint8, device=dev)
    base = buf.data_ptr() + (-buf.data_ptr()) % 64
    answers = entry_answers("halo_kcp_emit_device", base, True)
    torch.cuda.synchronize()
    assert len(answers) >= 24
    for what, rc in answers:
        assert rc == _lib.HALO_E_INVAL, (what, rc)
    assert not buf.cpu().numpy().any()


def _frames_chain(dev, mode, payloads):
    """Frames carrying `payloads` to KC.PORT -> parse -> deliver -> device ingest."""
    from halo_amd import deliver, kcp, port_map, protocol
    from tests import deliver_cases as DC

    import torch

    frames = [DC.udp(KC.PORT, p, sport=6000 + i) for i, p in enumerate(payloads)]
    data, offs, lens = DC.pack(5, frames)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d, o, ln = to(data), to(offs.view(np.int32)), to(lens.view(np.int16))
    nif = DC.lib_netif()
    recs = protocol.parse_frames_batch(d, o, ln, netif=nif)
    dl = deliver(d, o, ln, recs, netif=nif, region_bytes=1 << 20, udp_ports=to(port_map((KC.PORT,)).view(np.int32)), index_cap=len(frames))
    return dl, kcp.ingest(dl, port=KC.PORT, byte_check_mode=mode, seg_cap=4096, dgram_cap=len(frames))


@pytest.mark.parametrize("mode", (M.DISABLED, M.CRC32, M.XXH3))
def test_relay_from_a_delivery_stream_without_a_download(dev, mode):
    """Datagrams received into a delivery stream and ingested on the device; ingest's descriptor
    array, still in HBM, is emit's segment list and the delivery stream its payload. Only the
    datagram records come to the host (the state machine's part), to make the entries."""
    import torch

    from halo_amd import kcp

    b = C.batch_of([c for c in C.crafted(mode) if c[0] in ("push_lengths", "alignments", "non_push_with_data", "many_datagrams", "fifty_acks")])
    arrays = b.arrays()
    sent = C.want(arrays, mode, 4096, 1 << 20)
    payloads = [sent.stream[int(d["offset"]):int(d["offset"]) + int(d["len"])] for d in sent.dgrams]
    dl, ing = _frames_chain(dev, mode, payloads)
    torch.cuda.synchronize()
    assert int(ing.summary["dgrams_written"]) == len(payloads) and int(ing.summary["ret_counts"][0]) == len(payloads)
    # one entry per received datagram, over its range of ingest's own descriptor array
    ents = kcp.sessions_of([dict(conv=int(g["conv0"]), first_seg=int(g["first_seg"]), n_segs=int(g["n_segs"]), mtu=1472, dst_ip=9, dst_port=10)
                            for g in ing.dgrams])
    n_segs = int(ing.summary["segs_written"])
    r = kcp.emit(_t(dev, ents), ing.segs_raw, dl.out, n_sessions=len(ents), n_segs=n_segs, byte_check_mode=mode, src_ip=1, src_port=2,
                 dgram_cap=len(ents), stream_cap=1 << 20)
    torch.cuda.synchronize()
    assert ing.segs_raw.is_cuda and dl.out.is_cuda and not r.status.any()
    assert r.datagrams() == payloads
    host = kcp.emit_host(ents, ing.segs, dl.out.cpu().numpy(), byte_check_mode=mode, src_ip=1, src_port=2, dgram_cap=len(ents),
                         stream_cap=1 << 20)
    assert host.summary == r.summary and host.dgrams().tobytes() == r.dgrams().tobytes() and host.descs().tobytes() == r.descs().tobytes()


@pytest.mark.parametrize("mode", (M.CRC32, M.XXH3))
def test_chain_emit_build_parse_deliver_ingest(dev, mode):
    """emit -> halo_tx_build_batch_device -> halo_rx_parse_batch_device -> deliver ->
    halo_kcp_ingest_device over a few hundred frames: every datagram returns 0, every PUSH check is
    PASSED, and the descriptors and the data equal the input."""
    import torch

    from halo_amd import deliver, kcp, port_map, protocol
    from halo_amd.protocol import TxBuilder
    from tests import deliver_cases as DC

    rng = np.random.default_rng(mode)
    b = C.Batch()
    for k in range(150):
        if k % 11 == 0:
            b.enet(k % 4, k, 2 * k, 3 * k, dst_ip=DC.OWN_IP, dst_port=KC.PORT)
        segs = [((KC.PUSH, KC.PUSH, KC.ACK, KC.WINS)[int(rng.integers(4))], KC.rnd(100 * k + i, int(rng.integers(0, 400))), int(rng.integers(4)))
                for i in range(int(rng.integers(1, 9)))]
        b.kcp(segs, mtu=int(rng.choice([500, 1400, 1472])), dst_ip=DC.OWN_IP, dst_port=KC.PORT)
    sessions, segs, pay, nbytes = arrays = b.arrays()
    want = C.want(arrays, mode, 4096, 1 << 20)
    nd = int(want.summary["dgrams"])
    assert 200 < nd < 1000
    up = _upload(dev, arrays)
    r = kcp.emit(up[0], up[1], up[2], n_sessions=len(sessions), n_segs=len(segs), payload_bytes=nbytes, byte_check_mode=mode,
                 src_ip=DC.PEER, src_port=KC.PORT, dgram_cap=nd, stream_cap=1 << 20)
    # what halo_arp_encap_tx_device would fill: the next hop's MAC, here the receiving NetIf's own
    r.descs_raw.view(torch.uint8).reshape(-1, 40)[:, 32:38] = torch.tensor(list(DC.MAC), dtype=torch.uint8, device=dev)
    nif = DC.lib_netif()
    stride = 1536
    frames, lens, res = r.build(TxBuilder(nd, device=dev, ip_id=77), netif=nif, out_stride=stride, n=nd, max_payload_hint=1472)
    offs = torch.arange(nd, dtype=torch.int32, device=dev) * (stride // 4)
    flat = frames.reshape(-1)
    recs = protocol.parse_frames_batch(flat, offs, lens, netif=nif)
    dl = deliver(flat, offs, lens, recs, netif=nif, region_bytes=1 << 20,
                 udp_ports=torch.from_numpy(port_map((KC.PORT,)).view(np.int32)).to(dev), index_cap=nd)
    ing = kcp.ingest(dl, port=KC.PORT, byte_check_mode=mode, seg_cap=len(segs), dgram_cap=nd)
    torch.cuda.synchronize()
    assert not res.cpu().numpy().any() and int(r.summary["dgrams_written"]) == nd and r.datagrams() == \
        [want.stream[int(d["offset"]):int(d["offset"]) + int(d["len"])] for d in want.dgrams]
    s = ing.summary
    n_enet = int((sessions["kind"] == M.ENET).sum())
    assert int(s["dgrams_written"]) == nd and int(s["ret_counts"][0]) == nd - n_enet and int(s["enet_counts"].sum()) == n_enet
    assert int(s["in_errs"]) == 0 and int(s["ignored"]) == 0 and int(s["segs_written"]) == len(segs) == int(s["in_segs"])
    got = ing.segs
    for f in ("cmd", "frg", "wnd", "ts", "sn", "una", "len"):
        assert np.array_equal(got[f], segs[f]), f
    assert np.array_equal(got["check"], np.where(segs["cmd"] == KC.PUSH, 1, 0))
    back, src = dl.stream().tobytes(), pay.tobytes()
    for a, x in zip(segs, got):
        assert back[int(x["data_off"]):int(x["data_off"]) + int(x["len"])] == src[int(a["data_off"]):int(a["data_off"]) + int(a["len"])]
    sent = want.dgrams
    for j, g in enumerate(ing.dgrams):
        e = sessions[int(sent[j]["session"])]
        if e["kind"] == M.ENET:
            assert (int(g["kind"]), int(g["conn_type"]), int(g["session_id"]), int(g["conv"]), int(g["enet_type"])) == \
                (1, int(e["conn_type"]), int(e["session_id"]), int(e["enet_conv"]), int(e["enet_type"]))
        else:
            assert int(g["ret"]) == 0 and int(g["conv0"]) == int(e["conv"]) and int(g["n_segs"]) == int(sent[j]["n_segs"])
