"""GPU: the loopback gather (halo_amd/csrc/lo_gather.hip through halo_amd.loopback.gather) against
tests/lo_model.py and against the host loop, bit for bit: every device output — the whole output
buffer with its 0xA5 sentinel beyond each NetIf's written bytes, the summaries, the three per-packet
arrays with their sentinel beyond the written entries, the skip count — and the input left as it
was. Both modes over the corpus's length / verdict / NetIf mix at the sizes around a wavefront and a
tile; all frames selected and none; the region cut inside a tile and at a tile's first packet; one
workspace for two calls; batches past one lane's tiles, one wave's and one pass of the scan; and one
past one grid of the count and scatter kernels."""
from __future__ import annotations

import numpy as np
import pytest

from tests import arp_model as AM
from tests import lo_cases as C
from tests import lo_model as LM

pytestmark = pytest.mark.gpu

FILL = C.FILL


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


def _up(dev, data, offs, lens, results):
    import torch

    return (torch.from_numpy(data).to(dev), torch.from_numpy(offs.view(np.int32)).to(dev),
            torch.from_numpy(lens.view(np.int16)).to(dev),
            torch.from_numpy(np.ascontiguousarray(results).view(np.uint8).reshape(-1, 8)).to(dev))


def _gather(dev, d, o, ln, res, n_netifs, region, index_cap, tx=False, jumbo=False, workspace=None, skipped0=7):
    """A call whose outputs were all filled with 0xA5 first: the wrapper's own arrays are replaced."""
    import ctypes

    import torch

    from halo_amd import _lib
    from halo_amd import loopback as L

    n = int(ln.shape[0])
    cap = max(index_cap, 1)
    out = torch.full((n_netifs * region + 64,), FILL, dtype=torch.uint8, device=dev)
    ports = torch.full((n_netifs, 24), FILL, dtype=torch.uint8, device=dev)
    pkt_off = torch.full((n_netifs, cap), -0x5A5A5A5B, dtype=torch.int32, device=dev)  # 0xA5A5A5A5
    pkt_len = torch.full((n_netifs, cap), -0x5A5B, dtype=torch.int16, device=dev)      # 0xA5A5
    index = torch.full((n_netifs, cap), -0x5A5A5A5B, dtype=torch.int32, device=dev)
    skipped = torch.full((1,), skipped0, dtype=torch.int32, device=dev)  # incremented, not set
    if workspace is None:
        workspace = torch.empty(max(L.workspace_bytes(n, n_netifs), 8) // 8, dtype=torch.int64, device=dev)
    cfg = L._config(n_netifs, region, index_cap, tx, jumbo)
    _lib.check("halo_lo_gather_device", _lib.lib.halo_lo_gather_device(
        ctypes.byref(cfg), _lib.ptr(d), _lib.ptr(o), _lib.ptr(ln), n, _lib.ptr(res), _lib.ptr(out), _lib.ptr(ports),
        _lib.ptr(pkt_off), _lib.ptr(pkt_len), _lib.ptr(index), _lib.ptr(skipped), _lib.ptr(workspace),
        workspace.numel() * 8, torch.cuda.current_stream().cuda_stream))
    return L.LoResult(n_netifs, region, index_cap, out, ports, pkt_off, pkt_len, index, skipped)


def _check(r, want: LM.Want, skipped0=7):
    import torch

    torch.cuda.synchronize()
    assert np.array_equal(r.ports, want.ports), (r.ports, want.ports)
    got = r.out.cpu().numpy()
    exp = want.out(FILL, size=len(got))
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"{bad.size} output bytes differ, first at {bad[:6]}"
    w_off, w_len, w_idx = want.arrays()
    if want.index_cap:
        for name, got_a, want_a in (("pkt_off_dw", r.pkt_off_dw_raw.cpu().numpy().view(np.uint32), w_off),
                                    ("pkt_len", r.pkt_len_raw.cpu().numpy().view(np.uint16), w_len),
                                    ("index", r.index_raw.cpu().numpy().view(np.uint32), w_idx)):
            assert np.array_equal(got_a, want_a), (name, np.argwhere(got_a != want_a)[:6])
    assert r.n_skipped - skipped0 == want.skipped


def _case(dev, frames, data, offs, lens, results, n_netifs, region, index_cap, tx=False, jumbo=False):
    want = LM.gather(frames, LM.netifs_of_results(results, n_netifs), n_netifs, region, index_cap, tx, jumbo)
    d, o, ln, res = _up(dev, data, offs, lens, results)
    r = _gather(dev, d, o, ln, res, n_netifs, region, index_cap, tx, jumbo)
    _check(r, want)
    assert np.array_equal(d.cpu().numpy(), data), "the input batch was written"
    _check_host(r, data, offs, lens, results, n_netifs, region, index_cap, tx, jumbo)
    return r, want


def _check_host(r, data, offs, lens, results, n_netifs, region, index_cap, tx=False, jumbo=False):
    """device == host, on every output byte"""
    from halo_amd import loopback as L

    h = L.gather_host(data, offs, lens, results, n_netifs, region, index_cap, tx=tx, jumbo=jumbo,
                      out=np.full(n_netifs * region + 64, FILL, np.uint8), skipped=np.full(1, 7, np.uint32))
    assert np.array_equal(r.out.cpu().numpy(), h.out) and np.array_equal(r.ports, h.ports) and r.n_skipped == h.n_skipped
    for p in range(n_netifs):
        assert np.array_equal(r.pkt_off_dw(p), h.pkt_off_dw(p)) and np.array_equal(r.pkt_len(p), h.pkt_len(p))
        assert np.array_equal(r.index(p), h.index(p))
    return h


@pytest.mark.parametrize("tx", [False, True], ids=["forward", "tx"])
@pytest.mark.parametrize("n_netifs", [1, 4, 64])
@pytest.mark.parametrize("n", C.SIZES)
def test_matches_model_and_host(dev, n, n_netifs, tx):
    jumbo = n == 257  # one size carries the jumbo lengths as well
    frames, data, offs, lens, results = C.mixed(2000 * n_netifs + n + (7 if tx else 0), n, n_netifs, tx, jumbo)
    if n >= 64:
        assert set((offs * 4) % 16) == {0, 4, 8, 12}
    free = LM.gather(frames, LM.netifs_of_results(results, n_netifs), n_netifs, 1 << 34, 0, tx, jumbo)
    region = C.region_for(int(free.ports["bytes"].max()))
    index_cap = int(free.ports["frames"].max()) + 3
    r, want = _case(dev, frames, data, offs, lens, results, n_netifs, region, index_cap, tx, jumbo)
    if n >= 255:
        assert want.skipped > 0 and int(want.ports["frames"][0]) > 0
    if n == 0:
        assert not r.ports.view(np.uint8).any()
    # a short list: only the first two entries per NetIf, `frames` still the total
    _case(dev, frames, data, offs, lens, results, n_netifs, region, 2, tx, jumbo)


@pytest.mark.parametrize("tx", [False, True], ids=["forward", "tx"])
@pytest.mark.parametrize("which", ["all", "none"])
def test_all_selected_and_none(dev, which, tx):
    frames, data, offs, lens, results = C.mixed(31, 700, 3, tx, loopback_share=3 if which == "all" else 0)
    if which == "all":
        results["out_netif"] = np.arange(700) % 3
    else:
        results["verdict"][results["verdict"] == AM.LOOPBACK] = AM.HIT
    r, want = _case(dev, frames, data, offs, lens, results, 3, 1 << 18, 700, tx)
    total = int(want.ports["frames"].sum()) + want.skipped
    assert total == (700 if which == "all" else 0)
    # one NetIf takes every frame: the count's one-pair-per-wave path
    results["out_netif"] = 2
    _case(dev, frames, data, offs, lens, results, 3, 1 << 19, 700, tx)


@pytest.mark.parametrize("cut", ["inside_tile", "tile_first_packet", "second_tile_boundary", "nothing_fits", "mixed_lengths"])
def test_region_cut(dev, cut):
    """600 frames of 64 bytes (52-byte packets): NetIf 0 takes all of them but every third, which
    NetIf 1 takes; NetIf 2 none. The cut inside tile 1, exactly at the first packet of tile 1 (of
    NetIf 0) and of tile 2, a region of nothing, and the mixed-length batch cut in half."""
    from tests import arp_cases as K

    n = 600
    if cut == "mixed_lengths":
        frames, data, offs, lens, results = C.mixed(77, n, 3)
        free = LM.gather(frames, LM.netifs_of_results(results, 3), 3, 1 << 34, 0)
        region = (int(free.ports["bytes"].max()) // 2) & ~15
    else:
        rng = np.random.default_rng(12)
        frames = [rng.integers(0, 256, 64, dtype=np.uint8).tobytes() for _ in range(n)]
        data, offs, lens = K.pack(rng, frames)
        results = np.zeros(n, C.ARP_RESULT_DTYPE)
        results["verdict"] = AM.LOOPBACK
        results["out_netif"] = [1 if i % 3 == 0 else 0 for i in range(n)]
        # NetIf 0's k-th packet is frame k + k // 2 + 1: its 171st is frame 256, tile 1's first; its 342nd frame 512
        region = {"inside_tile": 52 * 300, "tile_first_packet": 52 * 170 + 8, "second_tile_boundary": 52 * 341 + 12,
                  "nothing_fits": 48}[cut]
        assert region % 16 == 0
    r, want = _case(dev, frames, data, offs, lens, results, 3, region, n)
    if cut == "inside_tile":
        assert [int(x) for x in want.ports["frames_written"]] == [300, 200, 0]
    elif cut == "tile_first_packet":
        assert [int(x) for x in want.ports["frames_written"]] == [170, 170, 0] and int(want.index[0][170]) == 256
    elif cut == "second_tile_boundary":
        assert int(want.ports[0]["frames_written"]) == 341 and int(want.index[0][341]) == 512
    elif cut == "mixed_lengths":
        assert sum(int(p["frames_written"]) < int(p["frames"]) for p in want.ports) >= 2
    else:
        assert not want.ports["frames_written"].any()


def test_workspace_reuse(dev):
    """Two calls with different inputs and modes back to back on one stream with one workspace: each
    gives its own model's answer."""
    import torch

    from halo_amd import loopback as L

    cases = []
    for seed, n, n_netifs, tx in ((1, 900, 3, False), (2, 333, 7, True)):
        frames, data, offs, lens, results = C.mixed(seed, n, n_netifs, tx)
        want = LM.gather(frames, LM.netifs_of_results(results, n_netifs), n_netifs, 1 << 17, 128, tx)
        cases.append((want, n_netifs, tx, _up(dev, data, offs, lens, results)))
    ws = torch.empty(max(L.workspace_bytes(900, 3), L.workspace_bytes(333, 7)) // 8, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    got = [_gather(dev, d, o, ln, res, n_netifs, 1 << 17, 128, tx, workspace=ws) for _, n_netifs, tx, (d, o, ln, res) in cases]
    for r, (want, _, _, _) in zip(got, cases):
        _check(r, want)


def test_edges_follow_the_sources():
    """Not a device test of its own: the shapes below move with the constants they come from."""
    c = C.read_constants()
    assert C.derived(c) == {k: v["first_past"] for k, v in C.BOUNDARIES.items()}


@pytest.mark.parametrize("edge,r", [("lo_scan_lane", 5), ("lo_scan_wave", 131), ("lo_scan_pass", 299)])
def test_past_the_scan_edges(dev, edge, r):
    """past(edge) + r frames of 64 bytes repeating 1,000 templates, to three NetIfs of four by an
    irregular pattern with a few frames to none, every NetIf's region cut in one of its last tiles;
    expectations from the model's vectorised path, the comparison on the device."""
    import torch

    n = C.past(edge, r)
    assert n % 4 and n * 64 < 20 << 20
    templates, tid, data, offs, lens = C.periodic_batch(n, n)
    i = np.arange(n, dtype=np.uint64)
    netifs = ((i * np.uint64(2654435761) >> np.uint64(13)) % np.uint64(3)).astype(np.int64)
    netifs[5::29] = -1
    results = np.zeros(n, C.ARP_RESULT_DTYPE)
    results["verdict"] = np.where(netifs >= 0, AM.LOOPBACK, AM.HIT)
    results["out_netif"] = np.where(netifs >= 0, netifs, 0)
    fewest = min(int((netifs == p).sum()) for p in range(3))
    region = ((fewest - 50) * 52) & ~15  # the three NetIfs overflow, and the cut lies in one of the last tiles
    index_cap = 1000
    want = LM.gather_uniform(templates, tid, netifs, 4, region, index_cap)
    assert all(0 < int(p["frames_written"]) < int(p["frames"]) for p in want.ports[:3]) and int(want.ports[3]["frames"]) == 0
    d, o, ln, res = _up(dev, data, offs, lens, results)
    r_ = _gather(dev, d, o, ln, res, 4, region, index_cap, skipped0=0)
    torch.cuda.synchronize()
    assert np.array_equal(r_.ports, want.ports), (r_.ports, want.ports)
    exp = torch.from_numpy(want.out(FILL, size=int(r_.out.numel()))).to(dev)
    assert torch.equal(r_.out, exp), int((r_.out != exp).nonzero()[0])
    w_off, w_len, w_idx = want.arrays()
    assert np.array_equal(r_.pkt_off_dw_raw.cpu().numpy().view(np.uint32), w_off)
    assert np.array_equal(r_.pkt_len_raw.cpu().numpy().view(np.uint16), w_len)
    assert np.array_equal(r_.index_raw.cpu().numpy().view(np.uint32), w_idx)
    assert r_.n_skipped == 0
    assert torch.equal(d, torch.from_numpy(data).to(dev)), "the input batch was written"


@pytest.mark.parametrize("tx", [False, True], ids=["forward", "tx"])
def test_past_one_grid(dev, tx):
    """The first n past one grid of the count and scatter kernels, plus 299: the workgroups of the
    first tiles take a second tile. Frames of 64 bytes repeating 1,000 templates (in tx mode
    totalLen 20..51, so that lengths vary and one template in 32 is skipped), one frame in 64
    selected by an irregular pattern, to two NetIfs; among them the batch's last frames, so that
    both NetIfs have packets in a second-trip tile, and the region cuts both there or shortly
    before. Every output byte against the host loop (tests/test_lo_host.py holds it to the model)."""
    from halo_amd import loopback as L

    n = C.past("lo_grid", 299)
    first_trip = C.BOUNDARIES["lo_grid"]["first_past"] - 1
    rng = np.random.default_rng(41)
    templates = rng.integers(0, 256, (1000, 64), dtype=np.uint8)
    templates[:, 16], templates[:, 17] = 0, 20 + np.arange(1000) % 32
    data = np.ascontiguousarray(np.tile(templates.reshape(-1), n // 1000 + 1)[:n * 64])
    offs, lens = (np.arange(n, dtype=np.int64) * 16).astype(np.uint32), np.full(n, 64, np.uint16)
    i = np.arange(n, dtype=np.uint64)
    h = i * np.uint64(2654435761) >> np.uint64(13)
    chosen = h % np.uint64(64) == 0
    chosen[first_trip::7] = chosen[n - 1] = True  # the second trip's tiles, their last frame included
    assert chosen[n - 1] and 60 < n / int(chosen.sum()) < 68
    results = np.zeros(n, C.ARP_RESULT_DTYPE)
    results["verdict"] = np.where(chosen, AM.LOOPBACK, AM.HIT)
    results["out_netif"] = (h >> np.uint64(7)) % np.uint64(2)
    results["out_netif"][first_trip:] = np.arange(n - first_trip) % 2
    free = L.gather_host(data, offs, lens, results, 2, 1 << 20, 0, tx=tx)
    assert np.array_equal(free.ports["frames_written"], free.ports["frames"])
    late = results["out_netif"][first_trip:][chosen[first_trip:]]
    assert set(late.tolist()) == {0, 1} and (free.n_skipped > 0) == tx
    region = (int(free.ports["bytes"].min()) - 16) & ~15
    index_cap = int(free.ports["frames"].max()) + 3
    d, o, ln, res = _up(dev, data, offs, lens, results)
    r = _gather(dev, d, o, ln, res, 2, region, index_cap, tx)
    host = _check_host(r, data, offs, lens, results, 2, region, index_cap, tx)
    assert all(0 < int(p["frames_written"]) < int(p["frames"]) for p in host.ports)
    assert np.array_equal(d.cpu().numpy(), data), "the input batch was written"


def test_gathered_batch_parses_as_l3_packets(dev):
    """LoResult.batch(p) is what the HALO_RX_L3_START parse takes, as it lies: UDP frames addressed to
    NetIf 1, gathered, parsed as LoChan packets — OK, for me, with the frames' ports."""
    from halo_amd import protocol
    from halo_amd._lib import NetIf
    from oracle import ref_py as R
    from tests import arp_cases as K

    rng = np.random.default_rng(5)
    own = NetIf.make()
    src, dst = bytes([10, 1, 2, 3]), int(own.ip).to_bytes(4, "big")
    frames = [R.build_eth(R.build_ipv4(R.build_udp(rng.integers(0, 256, int(rng.integers(0, 90)), dtype=np.uint8).tobytes(),
                                                   4000 + k, 53, src, dst), 17, src, dst), bytes(6), K.mac(k), 0x0800)
              for k in range(300)]
    data, offs, lens = K.pack(rng, frames)
    results = np.zeros(300, C.ARP_RESULT_DTYPE)
    results["verdict"], results["out_netif"] = AM.LOOPBACK, 1
    d, o, ln, res = _up(dev, data, offs, lens, results)
    r = _gather(dev, d, o, ln, res, 2, 1 << 16, 300)
    packets, p_off, p_len = r.batch(1)
    assert int(p_off.shape[0]) == 300 and packets.data_ptr() == r.out.data_ptr() + (1 << 16)  # views, no copy
    recs = protocol.records(protocol.parse_frames_batch(packets, p_off, p_len, netif=own, l3_start=True))
    assert (recs["status"] == 0).all() and (recs["dst_ip"] == int(own.ip)).all()
    assert recs["sport"].tolist() == [4000 + k for k in range(300)] and (recs["dport"] == 53).all()
    assert int(r.batch(0)[1].shape[0]) == 0
