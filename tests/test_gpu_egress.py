"""GPU: the egress step (halo_amd/csrc/tx_egress.hip through halo_amd.egress) against
tests/egress_model.py, bit for bit: every device output — the whole output buffer with its 0xA5
sentinel beyond each port's written bytes, the summaries, the index lists, the skip count — and the
input left as it was. The masks kind over the length / mask / offset mix at the sizes around a
wavefront and a tile; the region cut inside a tile and at a tile's first record; the ARP kind
behind the encap and the switch kind behind a device switch, on one stream; host == device; one
workspace for two calls; and shapes past the tile, the scan pass and the grid cap."""
from __future__ import annotations

import numpy as np
import pytest

from tests import arp_cases as K
from tests import arp_model as AM
from tests import egress_cases as C
from tests import egress_model as EM
from tests import switch_model as SM

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


def _up(dev, data, offs, lens):
    import torch

    return (torch.from_numpy(data).to(dev), torch.from_numpy(offs.view(np.int32)).to(dev),
            torch.from_numpy(lens.view(np.int16)).to(dev))


def _buffers(dev, n_ports, region, index_cap, skipped0=7):
    import torch

    out = torch.full((n_ports * region + 64,), FILL, dtype=torch.uint8, device=dev)
    index = torch.full((n_ports, max(index_cap, 1)), -0x5A5A5A5B, dtype=torch.int32, device=dev)  # 0xA5A5A5A5
    skipped = torch.full((1,), skipped0, dtype=torch.int32, device=dev)  # incremented, not set
    return out, index, skipped


def _check(r, want: EM.Want, index, skipped0=7):
    import torch

    torch.cuda.synchronize()
    assert np.array_equal(r.ports, want.ports), (r.ports, want.ports)
    got = r.out.cpu().numpy()
    exp = want.out(FILL, size=len(got))
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"{bad.size} output bytes differ, first at {bad[:6]}"
    if want.index_cap:
        got_ix = index.cpu().numpy().view(np.uint32)
        assert np.array_equal(got_ix, want.index_array()), np.argwhere(got_ix != want.index_array())[:6]
    assert r.n_skipped - skipped0 == want.skipped


def _masks_case(dev, frames, data, offs, lens, masks, n_ports, region, index_cap, jumbo=False):
    import torch

    from halo_amd import egress as E

    want = EM.egress(frames, masks, n_ports, region, index_cap, jumbo)
    d, o, ln = _up(dev, data, offs, lens)
    d_masks = torch.from_numpy(masks.view(np.int64)).to(dev)
    out, index, skipped = _buffers(dev, n_ports, region, index_cap)
    r = E.egress_masks(d, o, ln, d_masks, n_ports, region, index_cap, jumbo, out=out, skipped=skipped,
                       index=index if index_cap else None)
    _check(r, want, index)
    assert np.array_equal(d.cpu().numpy(), data), "the input batch was written"
    return r, want


@pytest.mark.parametrize("n_ports", [1, 3, 64])
@pytest.mark.parametrize("n", C.SIZES)
def test_masks_kind_matches_model(dev, n, n_ports):
    jumbo = n == 257  # one size carries the jumbo lengths as well
    frames, data, offs, lens, masks = C.mixed(100 * n_ports + n, n, n_ports, jumbo)
    if n >= 64:
        assert set((offs * 4) % 16) == {0, 4, 8, 12}
    free = EM.egress(frames, masks, n_ports, 1 << 40, 0, jumbo)
    region = C.region_for(int(free.ports["bytes"].max()))
    index_cap = int(free.ports["frames"].max()) + 3
    r, want = _masks_case(dev, frames, data, offs, lens, masks, n_ports, region, index_cap, jumbo)
    if n >= 255:
        assert want.skipped > 0 and int(want.ports["frames"].min()) > 0
    # a short index list: only the first two entries per port, `frames` still the total
    _masks_case(dev, frames, data, offs, lens, masks, n_ports, region, 2, jumbo)


@pytest.mark.parametrize("cut", ["inside_tile", "tile_first_record", "second_tile_boundary", "nothing_fits", "mixed_lengths"])
def test_region_cut(dev, cut):
    """600 frames of 60 bytes (64-byte records): port 0 takes all of them, port 1 every third, port
    2 none. The cut inside tile 1, exactly at the first record of tile 1 (port 0) and of tile 2, a
    region of nothing, and the mixed-length batch cut in half."""
    n = 600
    if cut == "mixed_lengths":
        frames, data, offs, lens, masks = C.mixed(77, n, 3)
        free = EM.egress(frames, masks, 3, 1 << 40)
        region = (int(free.ports["bytes"].max()) // 2) & ~15
    else:
        rng = np.random.default_rng(12)
        frames = [rng.integers(0, 256, 60, dtype=np.uint8).tobytes() for _ in range(n)]
        data, offs, lens = K.pack(rng, frames)
        masks = np.array([1 | (2 if i % 3 == 0 else 0) for i in range(n)], np.uint64)
        region = {"inside_tile": 64 * 300, "tile_first_record": 64 * 256, "second_tile_boundary": 64 * 512,
                  "nothing_fits": 48}[cut]
    r, want = _masks_case(dev, frames, data, offs, lens, masks, 3, region, n)
    if cut == "inside_tile":
        assert [int(x) for x in want.ports["frames_written"]] == [300, 200, 0]
    elif cut == "tile_first_record":
        assert [int(x) for x in want.ports["frames_written"]] == [256, 200, 0]  # frame 256 is tile 1's first
    elif cut == "mixed_lengths":
        assert all(int(p["frames_written"]) < int(p["frames"]) for p in want.ports)


@pytest.fixture(scope="module")
def world(dev):
    pair, keys = K.forced_table(lambda **kw: K.Pair(**kw))
    rt = K.world_routes(keys)
    rt.sync()
    pair.t.sync(rt)
    yield pair, keys, rt
    pair.close()
    rt.close()


def test_arp_kind_behind_encap(dev, world):
    """encap, then egress, on one stream with nothing in between. HIT frames reach their out NetIf's
    stream with the rewritten MACs; the ring walk over a stream finds frames_written records at the
    model's offsets, and parsed as the next hop receives them they are addressed to it."""
    import torch

    from halo_amd import _lib, protocol
    from halo_amd import egress as E
    from halo_amd._lib import ARP_RESULT_DTYPE, NetIf
    from oracle import ref_py as R

    pair, keys, rt = world
    rng = np.random.default_rng(41)
    dsts = [ip for _, ip in keys] + [K.NH_HIT | 9, K.NH_MISS | 9, K.absent(keys, 1, 3), 0x08080808]
    src = AM.ip_bytes(0x0A0000C8)
    frames = []
    for k in range(300):
        dst = AM.ip_bytes(dsts[k % len(dsts)])
        pl = rng.integers(0, 256, int(rng.integers(1, 120)), dtype=np.uint8).tobytes()
        frames.append(R.build_eth(R.build_ipv4(R.build_udp(pl, 1000 + k, 2000, src, dst), 17, src, dst), K.NETIFS[0].mac,
                                  K.mac(800), 0x0800))
    data, offs, lens = K.pack(rng, frames)
    dst_arr = np.array([dsts[k % len(dsts)] for k in range(len(frames))], np.uint32)
    rids = rt.FindRoute(torch.from_numpy(dst_arr.view(np.int32)).to(dev))
    want_res = np.zeros(len(frames), ARP_RESULT_DTYPE)
    after = []
    rids_h = rids.cpu().numpy().view(np.uint32)
    for i, f in enumerate(frames):
        v, outp, tx, target, g = pair.m.encap(f, K.route_of(rt, int(rids_h[i])), 0, True)
        want_res[i] = (v, outp, tx, target)
        after.append(g)
    masks = EM.masks_of_arp(want_res)
    hits = np.flatnonzero(want_res["verdict"] == AM.HIT)
    assert hits.size >= 100 and (want_res["verdict"] == AM.MISS).any() and (want_res["verdict"] == AM.NO_ROUTE).any()
    assert np.array_equal(masks != 0, want_res["verdict"] == AM.HIT)
    region, index_cap = 1 << 16, 256
    want = EM.egress(after, masks, 3, region, index_cap)
    assert all(int(x) > 0 for x in want.ports["frames"])
    d, o, ln = _up(dev, data, offs, lens)
    out, index, skipped = _buffers(dev, 3, region, index_cap)
    torch.cuda.synchronize()
    res, _, _ = pair.t.encap(d, o, ln, rids, 0)
    r = E.egress_arp(d, o, ln, res, 3, region, index_cap, out=out, skipped=skipped, index=index)
    _check(r, want, index)
    assert np.array_equal(res.cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE), want_res)
    st = torch.cuda.current_stream().cuda_stream
    for p in range(3):
        span = r.device_stream(p)
        used, k = int(span.numel()), int(want.ports[p]["frames_written"])
        d_off = torch.zeros(used // 8, dtype=torch.int32, device=dev)
        d_len = torch.zeros(used // 8, dtype=torch.int16, device=dev)
        info = torch.zeros(24, dtype=torch.uint8, device=dev)
        wsb = int(_lib.lib.halo_rx_ring_scan_workspace(used, 1514))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        _lib.check("halo_rx_ring_scan_device", _lib.lib.halo_rx_ring_scan_device(
            span.data_ptr(), used, 1 << 30, 1514, 0, d_off.data_ptr(), d_len.data_ptr(), info.data_ptr(), ws.data_ptr(),
            wsb, st))
        torch.cuda.synchronize()
        inf = info.cpu().numpy().view(_lib.RING_SCAN_DTYPE)[0]
        assert int(inf["n_frames"]) == k == int(r.ports[p]["frames_written"]) and int(inf["end_bytes"]) == used
        assert [4 * int(x) - 4 for x in d_off[:k].cpu().numpy().view(np.uint32)] == want.offsets[p]
        batch_ix = want.index[p][:k]
        assert np.array_equal(d_len[:k].cpu().numpy().view(np.uint16), np.maximum(lens[batch_ix], 60))
        for outp, target in sorted({(int(want_res[i]["out_netif"]), int(want_res[i]["target_ip"])) for i in batch_ix}):
            assert outp == p
            hop = NetIf()
            for b, x in enumerate(pair.m.cache[(outp, target)][0]):
                hop.mac[b] = x
            hop.ip = target
            recs = protocol.records(protocol.parse_frames_batch(span, d_off[:k], d_len[:k], netif=hop))
            torch.cuda.synchronize()
            mine = [j for j, i in enumerate(batch_ix) if int(want_res[i]["target_ip"]) == target]
            assert mine and all(int(recs[j]["flags"]) & 1 for j in mine), (outp, target)  # MAC_MATCH


def test_switch_kind_behind_device_switch(dev):
    import torch

    from halo_amd import egress as E
    from halo_amd._lib import SW_RESULT_DTYPE
    from halo_amd.switch import Switch

    warm, frames = C.switch_batch()
    sw = Switch([10, 10, 10, 20], 4, device=0)
    for port, fr, now in warm:
        sw.forward(port, *_up(dev, *SM.pack(fr)), now)
    rng = np.random.default_rng(8)
    data, offs, lens = K.pack(rng, frames)
    d, o, ln = _up(dev, data, offs, lens)
    flood = sw.flood_mask(0)
    assert flood == 0b0110
    out, index, skipped = _buffers(dev, 4, 4096, 16)
    torch.cuda.synchronize()
    res, _ = sw.forward(0, d, o, ln, 2)
    r = E.egress_switch(d, o, ln, res, flood, 4, 4096, 16, out=out, skipped=skipped, index=index)
    torch.cuda.synchronize()
    res_h = res.cpu().numpy().reshape(-1).view(SW_RESULT_DTYPE)
    assert sorted(set(res_h["verdict"].tolist())) == list(range(6))
    assert int(res_h["out_port"][0]) == 0 and int(res_h["verdict"][0]) == SM.UNICAST  # back to the ingress port
    want = EM.egress(frames, EM.masks_of_switch(res_h, flood), 4, 4096, 16)
    assert [int(x) for x in want.ports["frames"]] == [1, 3, 4, 0]
    _check(r, want, index)
    sw.close()


def test_host_equals_device(dev):
    import torch

    from halo_amd import egress as E

    frames, data, offs, lens, masks = C.mixed(5, 700, 5)
    free = EM.egress(frames, masks, 5, 1 << 40)
    region = (int(free.ports["bytes"].max()) * 3 // 4) & ~15  # some ports cut, some not
    h = E.egress_host(0, data, offs, lens, masks, 5, region, 64, out=np.full(5 * region + 64, FILL, np.uint8))
    d, o, ln = _up(dev, data, offs, lens)
    out, index, skipped = _buffers(dev, 5, region, 64, skipped0=0)
    r = E.egress_masks(d, o, ln, torch.from_numpy(masks.view(np.int64)).to(dev), 5, region, 64, out=out, skipped=skipped,
                       index=index)
    torch.cuda.synchronize()
    assert np.array_equal(r.ports, h.ports) and r.n_skipped == h.n_skipped
    assert np.array_equal(r.out.cpu().numpy(), h.out)
    assert all(np.array_equal(r.index(p), h.index(p)) for p in range(5))
    assert any(int(p["frames_written"]) < int(p["frames"]) for p in h.ports)


def test_workspace_reuse(dev):
    """Two calls with different inputs back to back on one stream with one workspace: each gives
    its own model's answer."""
    import torch

    from halo_amd import egress as E

    cases = []
    for seed, n, n_ports in ((1, 900, 3), (2, 333, 7)):
        frames, data, offs, lens, masks = C.mixed(seed, n, n_ports)
        want = EM.egress(frames, masks, n_ports, 1 << 17, 128)
        cases.append((want, n_ports, _up(dev, data, offs, lens), torch.from_numpy(masks.view(np.int64)).to(dev),
                      _buffers(dev, n_ports, 1 << 17, 128)))
    ws = torch.empty(max(E.workspace_bytes(900, 3), E.workspace_bytes(333, 7)) // 8, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    got = [E.egress_masks(d, o, ln, m, n_ports, 1 << 17, 128, out=out, workspace=ws, skipped=skipped, index=index)
           for _, n_ports, (d, o, ln), m, (out, index, skipped) in cases]
    for r, (want, _, _, _, (_, index, _)) in zip(got, cases):
        _check(r, want, index)


@pytest.mark.parametrize("shape", ["two_ports", "flood_three"])
@pytest.mark.parametrize("edge,r", [("egress_tile", 65), ("egress_scan_pass", 131), ("egress_grid", 299)])
def test_past_the_edges(dev, edge, r, shape):
    """past(edge) + r frames of 64 bytes, to two ports by an irregular pattern (masks kind) and as a
    flood to three ports of four (switch kind); expectations from the model's vectorised path, the
    comparison on the device."""
    import torch

    from halo_amd import egress as E
    from halo_amd._lib import SW_RESULT_DTYPE

    n = C.past(edge, r)
    frames2d, data, offs, lens = C.uniform_batch(n, n)
    d, o, ln = _up(dev, data, offs, lens)
    if shape == "two_ports":
        n_ports = 2
        i = np.arange(n, dtype=np.uint64)
        masks = (np.uint64(1) << ((i * np.uint64(2654435761) >> np.uint64(13)) & np.uint64(1))).astype(np.uint64)
        masks[::17] = 3
        masks[5::29] = 0
        fewest = min(int(((masks >> np.uint64(p)) & np.uint64(1)).sum()) for p in range(2))
        region = ((fewest - 50) * 68) & ~15  # both ports overflow, and the cut lies in one of the last tiles
    else:
        n_ports, flood = 4, 0b1110
        res = np.zeros(n, SW_RESULT_DTYPE)
        res["verdict"], res["out_port"], res["tx_len"] = SM.FLOOD, 0xFF, 64
        masks = np.full(n, flood, np.uint64)
        region = (n * 68 + 64 + 15) & ~15
    index_cap = 1000
    want = EM.egress_uniform(frames2d, masks, n_ports, region, index_cap)
    out, index, skipped = _buffers(dev, n_ports, region, index_cap, skipped0=0)
    if shape == "two_ports":
        r_ = E.egress_masks(d, o, ln, torch.from_numpy(masks.view(np.int64)).to(dev), n_ports, region, index_cap, out=out,
                            skipped=skipped, index=index)
        assert all(0 < int(p["frames_written"]) < int(p["frames"]) for p in want.ports)
    else:
        r_ = E.egress_switch(d, o, ln, torch.from_numpy(res.view(np.uint8).reshape(-1, 4)).to(dev), flood, n_ports, region,
                             index_cap, out=out, skipped=skipped, index=index)
        assert [int(x) for x in want.ports["frames_written"]] == [0, n, n, n]
    torch.cuda.synchronize()
    assert np.array_equal(r_.ports, want.ports), (r_.ports, want.ports)
    exp = torch.from_numpy(want.out(FILL, size=int(out.numel()))).to(dev)
    assert torch.equal(out, exp), int((out != exp).nonzero()[0])
    assert np.array_equal(index.cpu().numpy().view(np.uint32), want.index_array())
    assert r_.n_skipped == 0
    assert torch.equal(d, torch.from_numpy(data).to(dev)), "the input batch was written"


def test_ports_that_differ_in_the_second_scan_pass(dev):
    """One call over the smallest batch with a second scan pass, three ports and one region of
    1000 records and 16 bytes: port 0 (sparse before the pass boundary, dense behind it) is cut in
    the first tile of the second pass, port 1 (every frame) is cut in the first pass, port 2 (few
    frames, some of them in the second pass) is not cut. Each port's workgroup of the scan carries
    its own bases and finds its own cut."""
    import torch

    from halo_amd import egress as E

    c = C.read_constants()
    tile, edge = c["kTile"], c["kScanPass"] * c["kTile"]
    n, n_ports, records, index_cap = edge + 257, 3, 1000, 1200
    i = np.arange(n)
    masks = np.full(n, 2, np.uint64)                                   # port 1: every frame
    masks[(i % 300 == 0) | (i >= edge + 10)] |= np.uint64(1)           # port 0: 874 records before the boundary, 247 behind it
    masks[(i % 1000 == 7) | (i >= edge + 200)] |= np.uint64(4)         # port 2: 320 records
    sel = [np.flatnonzero((masks >> np.uint64(p)) & np.uint64(1)) for p in range(n_ports)]
    assert edge <= sel[0][records] < edge + tile and sel[1][records] < edge   # the first record that does not fit
    assert len(sel[2]) < records and sel[2][-1] >= edge
    region = 68 * records + 16
    frames2d, data, offs, lens = C.uniform_batch(n, n)
    want = EM.egress_uniform(frames2d, masks, n_ports, region, index_cap)
    assert [int(x) for x in want.ports["frames"]] == [len(s) for s in sel]
    assert [int(x) for x in want.ports["frames_written"]] == [records, records, len(sel[2])]
    d, o, ln = _up(dev, data, offs, lens)
    out, index, skipped = _buffers(dev, n_ports, region, index_cap, skipped0=0)
    r = E.egress_masks(d, o, ln, torch.from_numpy(masks.view(np.int64)).to(dev), n_ports, region, index_cap, out=out,
                       skipped=skipped, index=index)
    torch.cuda.synchronize()
    assert np.array_equal(r.ports, want.ports), (r.ports, want.ports)
    exp = torch.from_numpy(want.out(FILL, size=int(out.numel()))).to(dev)
    assert torch.equal(out, exp), int((out != exp).nonzero()[0])
    assert np.array_equal(index.cpu().numpy().view(np.uint32), want.index_array())
    assert r.n_skipped == 0
