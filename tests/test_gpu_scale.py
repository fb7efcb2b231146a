"""GPU: the forwarding kernels past one grid and one scan pass. Every kernel behind the C ABI with a
capped grid and a grid-stride loop, or a one-workgroup scan that carries a sum from one pass to the
next, runs once at the smallest shape past that edge (tests/scale_cases.BOUNDARIES, pinned to the
sources by tests/test_scale_shapes.py), with the assertions of its small-shape test: every result
field, every counter, and the whole byte buffer of the in-place kernels.

Expected values: the C oracle at full size where there is one; the sequential switch model at full
size (the switch is order-dependent); for the ARP and NAT dict models one period of 1000 items whose
answer is repeated like the input (tests/scale_cases.py)."""
from __future__ import annotations

import numpy as np
import pytest

from tests import arp_cases as K
from tests import arp_model as AM
from tests import nat_model as NM
from tests import scale_cases as S
from tests import switch_cases as SWK

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _drop_tensors():
    """Each test's tensors go before the next test's arrive."""
    yield
    import gc

    import torch

    gc.collect()
    torch.cuda.empty_cache()


def _rows(a: np.ndarray) -> np.ndarray:
    """A 1-D (possibly structured) array as uint8 rows."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), -1)


def _dev_tiled(dev, a: np.ndarray, n: int):
    """scale_cases.tiled(a, n), built on the device from one upload of the period."""
    import torch

    t = torch.from_numpy(_rows(a).copy()).to(dev)
    idx = torch.arange(n, device=dev) % len(a)
    return t[idx].contiguous()


def _assert_rows(got, want, what):
    import torch

    got, want = got.reshape(want.shape[0], -1), want.reshape(want.shape[0], -1)
    if not torch.equal(got, want):
        bad = (got != want).any(1).nonzero().flatten()
        i = int(bad[0])
        raise AssertionError((what, int(bad.numel()), bad[:8].tolist(), got[i].tolist(), want[i].tolist()))


# ---- ARP gather ----------------------------------------------------------------------------------
def _gather_batch(rng, n, nif):
    """n 64-byte frames addressed to NetIf nif: IPv4 frames, and ARP messages for it at positions
    chosen per 256-frame tile so that the tiles' counts are 0, 1, 255, 256 and irregular; a few ARP
    frames for another MAC and a few of 41 bytes among them. Returns (bytes, offsets_dw, lens, the
    constructed list of message indices, per-tile counts)."""
    own = np.frombuffer(K.NETIFS[nif].mac, np.uint8)
    arr = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    arr[:, 0:6] = own
    arr[:, 12], arr[:, 13] = 0x08, 0x00
    lens = np.full(n, 64, np.uint16)
    n_tiles = -(-n // 256)
    counts = np.zeros(n_tiles, np.int64)
    picked = []
    for t in range(n_tiles):
        size = min(256, n - 256 * t)
        c = [0, 1, 255, 256, int(rng.integers(2, 255)), int(rng.integers(2, 255)), 0][t % 7]
        if t >= n_tiles - 2:
            c = 40  # the last tiles, the partial one included, hold messages
        c = min(c, size)
        counts[t] = c
        picked.append(256 * t + np.sort(rng.choice(size, c, replace=False)))
    at = np.concatenate(picked).astype(np.int64)
    arr[at, 12:14] = (0x08, 0x06)
    arr[at[::2], 0:6] = 0xFF  # every other one is a broadcast
    arr[at, 14:20] = (0x00, 0x01, 0x08, 0x00, 0x06, 0x04)
    arr[at, 20], arr[at, 21] = 0, 1 + (at % 2)
    lens[at] = np.array([42, 60, 61, 64], np.uint16)[at % 4]
    rest = np.setdiff1d(np.arange(n), at)
    other, short = rest[5::max(1, len(rest) // 7)][:7], rest[9::max(1, len(rest) // 5)][:5]
    arr[other, 12:14] = (0x08, 0x06)
    arr[other, 0:6] = np.frombuffer(K.mac(4242), np.uint8)  # an ARP frame for another MAC
    arr[short, 12:14] = (0x08, 0x06)
    lens[short] = 41  # ParseEthFrm fails
    data = np.concatenate([arr.ravel(), np.zeros(16, np.uint8)])
    return data, np.arange(n, dtype=np.uint32) * 16, lens, at, counts


def _gather(dev, d, o, ln, recs, nif, data, want, cap=None):
    import torch

    from halo_amd._lib import ARP_MSG_DTYPE
    from halo_amd.arp import ArpTable

    msgs, count = ArpTable.gather(d, o, ln, recs, nif, cap=cap)
    torch.cuda.synchronize()
    assert int(count.cpu()[0]) == len(want)
    k = len(want) if cap is None else min(cap, len(want))
    raw = msgs.cpu().numpy()
    got = raw.reshape(-1).view(ARP_MSG_DTYPE)
    assert np.array_equal(got["index"][:k], want[:k]), np.flatnonzero(got["index"][:k] != want[:k])[:8]
    assert np.all(got["netif"][:k] == nif) and not got["pad"][:k].any()
    frames = data[:-16].reshape(-1, 64)[want[:k]]
    assert np.array_equal(got["eth_src"][:k], frames[:, 6:12]) and np.array_equal(got["arp"][:k], frames[:, 14:42])
    assert not raw[k:].any()  # nothing beyond the first `cap` messages is written


@pytest.mark.parametrize("shape", ["300 tiles", "second wave", "second pass"])
def test_arp_gather(dev, oracle_lib, shape):
    """The gather's one-workgroup scan with two waves' lanes holding counts, with wave sums, and
    with a non-zero carry into a second pass that is not empty."""
    import torch

    from halo_amd import protocol

    tile = S.read_constants()["kGatherTile"]
    n = {"300 tiles": 299 * tile + 179, "second wave": S.past("arp_scan_wave", 139),
         "second pass": S.past("arp_scan_pass", 139)}[shape]
    assert n >= S.BOUNDARIES["arp_scan_lane"]["first_past"]
    nif = 1
    rng = np.random.default_rng(len(shape))
    data, offs, lens, at, counts = _gather_batch(rng, n, nif)
    assert {0, 1, 255, 256} <= set(counts.tolist()) and len(set(counts.tolist())) > 20
    m = K.NETIFS[nif]
    f = data[:-16].reshape(-1, 64)
    for_us = (f[:, :6] == np.frombuffer(m.mac, np.uint8)).all(1) | (f[:, :6] == 0xFF).all(1)
    want = np.flatnonzero((lens >= 42) & (f[:, 12] == 0x08) & (f[:, 13] == 0x06) & for_us)
    assert np.array_equal(want, at)  # arp_model.is_arp_for, vectorised, finds the constructed list
    d, o, ln = (torch.from_numpy(data).to(dev), torch.from_numpy(offs.view(np.int32)).to(dev),
                torch.from_numpy(lens.view(np.int16)).to(dev))
    recs = protocol.parse_frames_batch(d, o, ln, netif=K.lib_netifs()[nif])
    torch.cuda.synchronize()
    mac = ":".join("%02X" % b for b in m.mac)
    ip = ".".join(str(b) for b in AM.ip_bytes(m.ip))
    w_recs, _ = oracle_lib.rx_batch(data, lens, oracle_lib.NetIf.make(mac=mac, ip=ip), 1, offsets_dw=offs, threads=16)
    assert protocol.records(recs).tobytes() == w_recs.tobytes()  # the records the gather reads
    _gather(dev, d, o, ln, recs, nif, data, want)
    if shape == "second pass":
        before = int(counts[:S.read_constants()["arp_pass"]].sum())
        assert 0 < before < len(want) - 17
        _gather(dev, d, o, ln, recs, nif, data, want, cap=before + 17)  # cuts inside the second pass


# ---- ARP lookup and encap ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(dev):
    """The forced 16-slot / 15-entry table and the route table of tests/test_gpu_arp.py."""
    pair, keys = K.forced_table(lambda **kw: K.Pair(**kw))
    rt = K.world_routes(keys)
    rt.sync()
    pair.t.sync(rt)
    yield pair, keys, rt
    pair.close()
    rt.close()


def _arp_lookup(dev, pair, d_ips, d_nifs, uniform, want_v, want_m, what):
    import torch

    miss = torch.full((1,), 9, dtype=torch.int32, device=dev)
    if uniform is None:
        mac8, verdict, miss = pair.t.lookup(d_ips, d_nifs, miss_count=miss)
    else:
        mac8, verdict, miss = pair.t.lookup(d_ips, None, netif=uniform, miss_count=miss)
    torch.cuda.synchronize()
    _assert_rows(verdict, want_v, (what, "verdict"))
    _assert_rows(mac8, want_m, (what, "mac8"))
    assert int(miss.cpu()[0]) - 9 == int((want_v == AM.MISS).sum()), what


def test_arp_lookup_second_trip(dev, world):
    import torch

    pair, keys, _ = world
    n = S.past("arp_trip", 141)
    nifs, ips = K.lookup_mix(np.random.default_rng(5), keys, S.P)
    d_ips = _dev_tiled(dev, ips, n).view(torch.int32).reshape(-1)
    d_nifs = _dev_tiled(dev, nifs, n).reshape(-1)
    seen = set()
    for uniform in (None, 0, 2, 3):
        use = nifs if uniform is None else np.full(S.P, uniform, np.uint8)
        verdict, mac8 = S.arp_lookup_model(pair.m, use, ips)
        seen |= set(verdict.tolist())
        _arp_lookup(dev, pair, d_ips, d_nifs, uniform, _dev_tiled(dev, verdict, n), _dev_tiled(dev, mac8, n), uniform)
    assert seen == {AM.NONE, AM.OWN_IP, AM.MISS, AM.HIT}


def test_arp_lookup_automatic_table(dev, world):
    """About 20,000 entries in a table whose slot count the library chose: mask > 15, long chains.
    Every key, and as many absent addresses, own addresses and unknown NetIfs, against the model."""
    import torch

    _, _, rt = world
    pair, keys, nifs, ips = S.arp_auto_table(lambda **kw: K.Pair(**kw))
    try:
        pair.t.sync(rt)
        st = pair.t.layout_stats()
        assert int(st["slots"]) > 16 and int(st["longest_chain"]) >= 3
        verdict, mac8 = S.arp_lookup_model(pair.m, nifs, ips)
        assert int((verdict == AM.HIT).sum()) == len(keys)
        d_ips = torch.from_numpy(ips.view(np.int32)).to(dev)
        d_nifs = torch.from_numpy(nifs).to(dev)
        _arp_lookup(dev, pair, d_ips, d_nifs, None, torch.from_numpy(verdict).to(dev), torch.from_numpy(mac8).to(dev), "auto")
    finally:
        pair.close()


def test_arp_encap_second_trip(dev, world):
    import torch

    from halo_amd._lib import ARP_RESULT_DTYPE

    pair, keys, rt = world
    n = S.past("arp_trip", 141)

    def find_route(dsts):
        return rt.FindRoute(torch.from_numpy(dsts.view(np.int32)).to(dev)).cpu().numpy().view(np.uint32).copy()

    per = S.arp_encap_period(keys, find_route)
    big, offs, lens = S.tile_frames(per["data"], per["offs"], per["lens"], n)
    assert len(big) < 150e6 and int(lens.max()) == 1514
    idx = S.tile_index(n)
    d_o = torch.from_numpy(offs.view(np.int32)).to(dev)
    d_ln = torch.from_numpy(lens.view(np.int16)).to(dev)
    d_rids = _dev_tiled(dev, per["rids"], n).view(torch.int32).reshape(-1)
    d_sel = _dev_tiled(dev, per["select"], n).reshape(-1)
    for in_netif in (0, 1):  # NetIf 0 does not NAT (LOOPBACK), NetIf 1 does (no LOOPBACK)
        res_p, want_p = S.arp_encap_model(pair.m, rt, per["frames"], per["rids"], per["select"], in_netif, per["data"],
                                          per["offs"])
        want_res = res_p[idx]
        want = S.tile_frames_expected(per["data"], want_p, per["offs"], n)
        d = torch.from_numpy(big).to(dev)
        counts = torch.full((7,), 3, dtype=torch.int32, device=dev)  # incremented, not set
        miss = torch.full((1,), 5, dtype=torch.int32, device=dev)
        res, counts, miss = pair.t.encap(d, d_o, d_ln, d_rids, in_netif, select=d_sel, counts=counts, miss_count=miss)
        torch.cuda.synchronize()
        got_res = res.cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE)
        bad = np.nonzero(got_res != want_res)[0]
        assert bad.size == 0, [(int(i), per["names"][i % S.P], got_res[i], want_res[i]) for i in bad[:5]]
        got = d.cpu().numpy()
        diff = np.nonzero(got != want)[0]
        assert diff.size == 0, f"{diff.size} bytes differ (first {diff[:8]})"
        # the whole buffer equals the input except bytes 0-11 of HIT frames
        allowed = np.zeros(len(big), bool)
        hit = want_res["verdict"] == AM.HIT
        allowed[(4 * offs[hit].astype(np.int64))[:, None] + np.arange(12)] = True
        assert not ((got != big) & ~allowed).any()
        assert list(counts.cpu().numpy() - 3) == [int((want_res["verdict"] == v).sum()) for v in range(7)]
        assert int(miss.cpu()[0]) - 5 == int((want_res["verdict"] == AM.MISS).sum())
        assert np.all(want_res["tx_len"][hit] == np.maximum(lens, 60)[hit])
        assert set(want_res["verdict"][-141:].tolist()) >= {AM.HIT, AM.MISS, AM.NONE}  # the second trip's tail is mixed


# ---- switch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SWK.SCALE_CASES))
def test_switch_scale(dev, name):
    """The cases tests/test_switch_host.py proves in host mode, on the device: the admission scan's
    second pass, the resolve kernel's second trip with its counters, the rebuild's second trip."""
    SWK.SCALE_CASES[name](lambda **kw: SWK.Pair(device=dev, **kw))


# ---- NAT -----------------------------------------------------------------------------------------
def _nat_pair(nat_type, tuples, log2=0, mappings=(), now=100):
    from halo_amd.nat import NatTable

    t, m = NatTable(NM.WAN_IP, nat_type, capacity_log2=log2), NM.NatModel(NM.WAN_IP, nat_type)
    for e in mappings:
        t.add_port_mapping(*e)
        m.add_port_mapping(*e)
    NM.fill(t, m, tuples, now)
    t.sync()
    return t, m


@pytest.mark.parametrize("name", ["forced_sym", "5000"])
def test_nat_lookup_second_trip(dev, name):
    """lookup_wan and lookup_lan over full and compact records with skips, then the stamps: the
    flows hit from the second trip's tail alone would be enough to keep a flow alive."""
    import torch

    from halo_amd._lib import compact_of

    nat_type, tuples, log2, maps = S.nat_tables()[name]
    t, m = _nat_pair(nat_type, tuples, log2, maps)
    n = S.past("nat_trip", 203)
    seen, now = set(), 130
    for direction in (NM.WAN, NM.LAN):
        for compact in (False, True):
            now += 1
            per = S.nat_period(m, direction, now, seed=40 + direction)
            seen |= set(per["verdict"].tolist())
            d_recs = _dev_tiled(dev, compact_of(per["recs"]) if compact else per["recs"], n)
            d_ops = _dev_tiled(dev, per["ops"], n)
            d_skip = _dev_tiled(dev, per["skip"], n).reshape(-1)
            fn = t.lookup_wan if direction == NM.WAN else t.lookup_lan
            ops, verdict, ref, miss = fn(d_recs, now, ops=d_ops, skip=d_skip)
            torch.cuda.synchronize()
            what = (name, direction, compact)
            _assert_rows(verdict, _dev_tiled(dev, per["verdict"], n), (what, "verdict"))
            _assert_rows(ref.view(torch.uint8), _dev_tiled(dev, per["ref"], n), (what, "ref"))
            _assert_rows(ops, _dev_tiled(dev, per["want_ops"], n), (what, "ops"))
            assert int(miss.cpu()[0]) == int((S.tiled(per["verdict"], n) == NM.V_MISS).sum()), what
            del d_recs, d_ops, d_skip, ops, verdict, ref
    assert seen == {NM.V_NONE, NM.V_SKIP, NM.V_MISS, NM.V_FLOW, NM.V_MAPPING}
    # the stamps the device left come back in the tick: flows added at 100 and never hit leave at
    # 161, the others stay with the LastAliveTime of their last lookup
    assert t.TableClear(161) == m.expire(161)
    assert NM.sorted_flows(t.ListNat()) == NM.sorted_flows(m.list())
    assert {int(f["last_alive"]) for f in t.ListNat()} <= {131, 132, 133, 134} and len(m.list()) > 0
    t.close()


def test_nat_quote_second_trip(dev):
    import torch

    from halo_amd._lib import DEEP_NAT_DTYPE

    nat_type, tuples, log2, maps = S.nat_tables()["5000"]
    t, m = _nat_pair(nat_type, tuples, log2, maps)
    n = S.past("nat_trip", 203)
    recs = NM.records(m, NM.WAN, S.P, seed=61)
    recs["status"][::7] = 3  # a quote that did not parse is not looked up
    want = np.zeros(S.P, DEEP_NAT_DTYPE)
    for i, (ip, port, found) in enumerate(m.quote(recs)):
        want[i] = (ip, port, found, 0)
    assert 100 < int(want["found"].sum()) < S.P - 100
    out = t.lookup_quote(_dev_tiled(dev, recs, n))
    torch.cuda.synchronize()
    _assert_rows(out, _dev_tiled(dev, want, n), "quote")
    t.close()


def test_nat_large_table(dev):
    """100,000 flows with the capacity the library chooses: each looked up once from each side,
    plus as many misses, against the model."""
    import torch

    from halo_amd._lib import RESULT_DTYPE

    k = 100_000
    t, m = _nat_pair(NM.SYMMETRIC, NM.random_tuples(77, k))
    flows = m.list()
    assert len(flows) == k
    fl = {f: np.array([x[f] for x in flows], np.uint32) for f in ("proto", "remote_ip", "remote_port", "wan_ip", "wan_port",
                                                                   "lan_ip", "lan_port")}
    rport = np.where(fl["remote_port"] == 0, 4444, fl["remote_port"])  # ICMP: the key ignores it
    for direction in (NM.WAN, NM.LAN):
        recs = np.zeros(2 * k, RESULT_DTYPE)
        recs["ip_proto"][:k] = recs["ip_proto"][k:] = fl["proto"]
        if direction == NM.WAN:
            cols = (fl["remote_ip"], rport, fl["wan_ip"], fl["wan_port"])
        else:
            cols = (fl["lan_ip"], fl["lan_port"], fl["remote_ip"], rport)
        for f, c in zip(("src_ip", "sport", "dst_ip", "dport"), cols):
            recs[f][:k] = recs[f][k:] = c
        # the second half misses: the local port of a flow nobody opened
        recs["dport" if direction == NM.WAN else "sport"][k:] ^= 0x4000
        order = np.random.default_rng(direction).permutation(2 * k)
        recs = recs[order]
        ops = NM.ops(2 * k, 3)
        want_ops = ops.copy()
        w_verdict, w_ref, w_miss = m.lookup(direction, recs, 140, want_ops)
        assert w_miss == k and int((w_verdict == NM.V_FLOW).sum()) == k
        fn = t.lookup_wan if direction == NM.WAN else t.lookup_lan
        d_ops, verdict, ref, miss = fn(torch.from_numpy(_rows(recs).copy()).to(dev), 140,
                                       ops=torch.from_numpy(_rows(ops).copy()).to(dev))
        torch.cuda.synchronize()
        assert np.array_equal(verdict.cpu().numpy(), w_verdict) and np.array_equal(ref.cpu().numpy().view(np.uint32), w_ref)
        assert d_ops.cpu().numpy().tobytes() == want_ops.tobytes() and int(miss.cpu()[0]) == w_miss
    t.close()


# ---- route and flow hash against the C oracle ------------------------------------------------------
ROUTE_OPS = [("add", [0, 0, 1, 0]), ("add", [0xC0A86400, 0xFFFFFF00, 0, 1]), ("add", [0xC0A86464, 0xFFFFFFFF, 0, 2]),
             ("add", [0x0A000000, 0xFF000000, 5, 3]), ("add", [0x0A000000, 0xFF000000, 6, 3]),
             ("add", [0xC0A86480, 0xFFFFFF80, 7, 2])]  # a /25 under the /24: the second table level


@pytest.fixture(scope="module")
def routes(dev, oracle_lib):
    from halo_amd.route import RouteTable

    g, o = RouteTable(0), oracle_lib.RouteTable()
    for _, r in ROUTE_OPS:
        assert g.AddRoute(RouteTable.entry(*r)) == o.add(r)
    g.sync()
    yield g, o
    g.close()


def _route_ips(rng, n):
    """Random addresses, a third of them inside the table's prefixes (both levels, the ECMP list)."""
    ips = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    k = np.arange(n)
    ips[k % 6 == 1] = 0xC0A86400 | (ips[k % 6 == 1] & 0xFF)
    ips[k % 6 == 3] = 0x0A000000 | (ips[k % 6 == 3] & 0xFFFFFF)
    return ips


def test_route_second_trip(dev, routes):
    import torch

    g, o = routes
    n = S.past("lpm_trip", 201)
    assert n % 4  # the tail loop behind the four-per-lane body runs
    ips = _route_ips(np.random.default_rng(8), n)
    got = g.FindRoute(torch.from_numpy(ips.view(np.int32)).to(dev))
    torch.cuda.synchronize()
    want = o.find_batch(ips)
    assert len(np.unique(want)) >= 6  # the default, the /24, the /25, the /32 and both ECMP members
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)


def test_route_records_second_trip(dev, routes):
    import torch

    from halo_amd._lib import RESULT_DTYPE

    g, o = routes
    n = S.past("lpm_records_trip", 201)
    recs = np.zeros(n, RESULT_DTYPE)
    recs["dst_ip"] = _route_ips(np.random.default_rng(9), n)
    got = g.FindRouteRecords(torch.from_numpy(_rows(recs)).to(dev))
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), o.find_batch(recs["dst_ip"]))


def test_flow_hash_second_trip(dev, oracle_lib):
    """Full and compact records of a parsed 64-byte protocol mix, both kinds, with buckets."""
    import torch

    from halo_amd import hashcode, protocol, synth
    from halo_amd._lib import HALO_RX_RECORD_COMPACT, NetIf

    n = S.past("flow_hash_trip", 203)
    lay = synth.layout(n, length=64, proto_mode=synth.PROTO_MIX, mutate_shift=5, first_index=4242)
    fr = synth.frames_device(lay, NetIf.make(), device=dev)
    full = protocol.parse_frames_batch(fr["bytes"], fr["offsets_dw"], fr["lens"], netif=NetIf.make(), max_len_hint=64)
    comp = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    rc = protocol._lib.lib.halo_rx_parse_batch_device(
        fr["bytes"].data_ptr(), fr["offsets_dw"].data_ptr(), fr["lens"].data_ptr(), n, 1 | HALO_RX_RECORD_COMPACT,
        NetIf.make(), 64, comp.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    del fr
    recs = protocol.records(full)
    assert len(np.unique(recs["ip_proto"][recs["status"] == 0])) >= 3
    for kind in (0, 1):
        wh, wb = oracle_lib.flow_hash_batch(recs, kind, 0, 1000003)
        for name, r in (("full", full), ("compact", comp)):
            h, b = hashcode.flow_hash(r, kind, 0, 1000003)
            torch.cuda.synchronize()
            assert np.array_equal(h.cpu().numpy().view(np.uint64), wh), (kind, name)
            assert np.array_equal(b.cpu().numpy().view(np.uint32), wb), (kind, name)


# ---- tx_fixup --------------------------------------------------------------------------------------
# hint -> lanes per frame: 0 -> 16, 4000 -> 8, 1000 -> 4, 64 -> 1
@pytest.mark.parametrize("hint,boundary", [(0, "tx_g16_trip"), (4000, "tx_g8_trip"), (1000, "tx_g4_trip"), (64, "tx_g1_trip")])
def test_tx_fixup_second_trip(dev, oracle_lib, hint, boundary):
    """Synthetic 64-byte UDP frames with random step sets, each lanes-per-frame width past its own
    grid cap: whole buffer and results against the oracle, both flag values."""
    import torch

    from halo_amd import protocol, synth
    from halo_amd._lib import NetIf
    from tests.helpers import random_tx_ops

    n = S.past(boundary, 203)
    lay = synth.layout(n, length=64, mutate_shift=4, first_index=777_000)
    fr = synth.frames_device(lay, NetIf.make(), device=dev, fill=0x5A)
    before = fr["bytes"].cpu().numpy()
    ops = random_tx_ops(n, 5)
    d_ops = torch.from_numpy(ops.view(np.uint8)).to(dev)
    for flag in (0, 1):
        d = fr["bytes"].clone()
        res = torch.empty(n, dtype=torch.uint8, device=dev)
        protocol.tx_fixup_batch(d, fr["offsets_dw"], fr["lens"], d_ops, check_sum_enable=bool(flag), max_len_hint=hint,
                                result=res)
        torch.cuda.synchronize()
        want, wres = oracle_lib.tx_batch(before, lay["offsets_dw"], lay["lens"], ops, flags=flag, threads=16)
        got = d.cpu().numpy()
        del d
        bad = np.nonzero(got != want)[0] if not np.array_equal(got, want) else np.zeros(0, np.int64)
        assert bad.size == 0, f"flag={flag}: {bad.size} bytes differ (first {bad[:8]})"
        assert np.array_equal(res.cpu().numpy(), wres)


# ---- tx_build --------------------------------------------------------------------------------------
TXB_ROWS = {"G1": "txb_g1_trip", "G4": "txb_g4_trip", "G8": "txb_g8_trip", "G16": "txb_g16_trip", "pair": "txb_pair_grid"}


def _txb_trip_n():
    n = S.past("txb_g1_trip", 203)
    assert all(S.BOUNDARIES[row]["first_past"] in (n - 202, None) for row in TXB_ROWS.values())
    return n


@pytest.fixture(scope="module")
def txb_trip_want(oracle_lib):
    """The C oracle's answer for the second-trip batch at full size (once for the five variants), and
    the slots it implies in a prefilled buffer. Full size: 0.1 s for 262,347 descriptors."""
    from tests import build_cases as B

    desc, payload = B.second_trip_batch(_txb_trip_n())
    want = oracle_lib.tx_build_batch(desc, payload, B.MAC, 1, B.TRIP_STRIDE, 0xFFF0)
    return want, B.expected_slots(*want[:3])


@pytest.mark.parametrize("variant", sorted(TXB_ROWS, key=lambda v: (len(v), v)))
def test_tx_build_second_trip(dev, txb_trip_want, variant):
    """Each build kernel past the build launch's grid cap (the pair kernel, which has none, at the
    same n): 262,347 descriptors, so the second trip is three full tiles and one of 11 descriptors.
    The hint selects the kernel, not the payloads: 0..100 bytes, protocols and modes mixed, 156-byte
    slots (a multiple of 4, not of 16) prefilled with 0xEE, every 97th descriptor an unknown
    protocol, one SLOT refusal in the last tile, checksums on, iphId from 0xFFF0. The whole buffer,
    lengths, results and the final iphId against the oracle: the second trip's tile index and its
    rejections' ranks, the waves' LDS regions written again behind the closing barrier (G4, G8, G16),
    the lane kernel's prefetched second-trip descriptors, and the finish kernel renumbering the second
    trip's frames over five scan passes."""
    import torch

    from halo_amd._lib import TX_B_OK, TX_B_PROTO, TX_B_SLOT, NetIf
    from halo_amd.protocol import TxBuilder
    from tests import build_cases as B

    hint = B.HINTS[variant]
    assert B.variant_of(hint) == variant
    n = _txb_trip_n()
    desc, payload = B.second_trip_batch(n)
    want, slots = txb_trip_want
    wr = want[2]
    first_trip = S.BOUNDARIES["txb_g1_trip"]["first_past"] - 1
    assert set(wr[first_trip:].tolist()) == {TX_B_OK, TX_B_PROTO, TX_B_SLOT} and TX_B_SLOT in wr[(n - 1) // 64 * 64:]
    assert int((wr[:first_trip] != TX_B_OK).sum()) > 2000  # the second trip's frames are renumbered
    assert -(-n // 64) > 4 * S.read_constants()["txb_finish_pass"]  # in the finish kernel's fifth pass
    assert int(want[1].max()) == 155 and int(B.frame_len(desc)[wr == TX_B_SLOT].min()) == 157
    b = TxBuilder(n, device=dev, ip_id=0xFFF0)
    frames = torch.full((n, B.TRIP_STRIDE), B.FILL, dtype=torch.uint8, device=dev)
    frames, lens, res = b.build(torch.from_numpy(np.array(desc).view(np.uint8)).to(dev), torch.from_numpy(np.array(payload)).to(dev),
                                netif=NetIf.make(mac="02:00:00:00:00:01", ip="192.168.100.1"), out_stride=B.TRIP_STRIDE,
                                frames=frames, check_sum_enable=True, max_payload_hint=hint)
    torch.cuda.synchronize()
    got = (frames.cpu().numpy(), lens.cpu().numpy().view(np.uint16), res.cpu().numpy(), b.iph_id)
    B.assert_slots(got, slots, want, f"{variant} (hint {hint}) n={n}", desc)
