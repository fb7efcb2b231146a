"""GPU: the device side of the ARP neighbour cache (halo_amd/csrc/arp_fwd.hip through
halo_amd.arp.ArpTable) against the dict model (tests/arp_model.py), bit for bit: the bare lookup and
the forward path's L2 step over the forced 16-slot / 15-entry table, at the batch sizes around a
wavefront and a 256-frame workgroup and one of several workgroups that is no multiple of one; the
post-DNAT destination; the two generations; the gather of a batch's ARP messages; and one chain
parse -> route -> fixup -> encap -> parse."""
from __future__ import annotations

import numpy as np
import pytest

from tests import arp_cases as K
from tests import arp_model as M

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
NH_HIT, NH_MISS, NH_OWN, PANIC, ECMP, BAD_NETIF = K.NH_HIT, K.NH_MISS, K.NH_OWN, K.PANIC, K.ECMP, K.BAD_NETIF
# the batch builders are shared with tests/test_gpu_scale.py
_absent, _ipv4_frame, _pack, _mixed_batch, _route_of = K.absent, K.ipv4_frame, K.pack, K.mixed_batch, K.route_of


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def world(dev):
    """The forced table, synced with a real route table that has direct routes, next-hop routes, an
    emptied list and an ECMP list."""
    pair, keys = K.forced_table(lambda **kw: K.Pair(**kw))
    rt = K.world_routes(keys)
    rt.sync()
    pair.t.sync(rt)
    assert not pair.t.dirty
    yield pair, keys, rt
    pair.close()
    rt.close()


def _up(dev, data, offs, lens):
    import torch

    return (torch.from_numpy(data).to(dev), torch.from_numpy(offs.view(np.int32)).to(dev),
            torch.from_numpy(lens.view(np.int16)).to(dev))


@pytest.mark.parametrize("n", SIZES)
def test_encap_matches_model(dev, world, n):
    import torch

    from halo_amd._lib import ARP_RESULT_DTYPE

    pair, keys, rt = world
    rng = np.random.default_rng(500 + n)
    frames, dsts, select, forced, names = _mixed_batch(rng, keys, n)
    data, offs, lens = _pack(rng, frames)
    if n >= 64:
        assert set((offs * 4) % 16) == {0, 4, 8, 12}
    rids = rt.FindRoute(torch.from_numpy(dsts.view(np.int32)).to(dev)).cpu().numpy().view(np.uint32).copy()
    for i, frc in enumerate(forced):
        if frc is not None:
            rids[i] = frc
    d_rids = torch.from_numpy(rids.view(np.int32)).to(dev)
    d_sel = torch.from_numpy(select).to(dev)
    seen = set()
    for in_netif in (0, 1):  # NetIf 0 does not NAT (LOOPBACK), NetIf 1 does (no LOOPBACK)
        want = data.copy()
        want_res = np.zeros(n, ARP_RESULT_DTYPE)
        for i, f in enumerate(frames):
            v, out, tx, target, after = pair.m.encap(f, _route_of(rt, int(rids[i])), in_netif, bool(select[i]))
            want_res[i] = (v, out, tx, target)
            want[4 * int(offs[i]):4 * int(offs[i]) + len(f)] = np.frombuffer(after, np.uint8)
            seen.add((names[i], v))
        d, o, ln = _up(dev, data, offs, lens)
        counts = torch.full((7,), 3, dtype=torch.int32, device=dev)  # incremented, not set
        miss = torch.full((1,), 5, dtype=torch.int32, device=dev)
        res, counts, miss = pair.t.encap(d, o, ln, d_rids, in_netif, select=d_sel, counts=counts, miss_count=miss)
        torch.cuda.synchronize()
        got_res = res.cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE)
        bad = np.nonzero(got_res != want_res)[0]
        assert bad.size == 0, [(int(i), names[i], got_res[i], want_res[i]) for i in bad[:5]]
        got = d.cpu().numpy()
        diff = np.nonzero(got != want)[0]
        assert diff.size == 0, f"{diff.size} bytes differ (first {diff[:8]})"
        # the whole buffer equals the input except bytes 0-11 of HIT frames
        changed = np.nonzero(got != data)[0]
        hit_bytes = set()
        for i in np.nonzero(want_res["verdict"] == M.HIT)[0]:
            hit_bytes.update(range(4 * int(offs[i]), 4 * int(offs[i]) + 12))
        assert set(changed.tolist()) <= hit_bytes
        assert list(counts.cpu().numpy() - 3) == [int((want_res["verdict"] == v).sum()) for v in range(7)]
        assert int(miss.cpu()[0]) - 5 == int((want_res["verdict"] == M.MISS).sum())
        assert np.all(want_res["tx_len"][want_res["verdict"] == M.HIT] == np.maximum(lens, 60)[want_res["verdict"] == M.HIT])
    if n >= 255:  # the batch mixes every verdict, each reached the way its case says
        for case, v in (("unselected", M.NONE), ("short33", M.NONE), ("not_ipv4", M.NONE), ("bad_route_id", M.NONE),
                        ("bad_netif", M.NONE), ("no_route", M.NO_ROUTE), ("panic", M.ROUTE_PANIC), ("own_dst", M.LOOPBACK),
                        ("own_dst", M.OWN_IP), ("own_next_hop", M.OWN_IP), ("miss_direct", M.MISS),
                        ("miss_next_hop", M.MISS), ("hit_next_hop", M.HIT), ("hit_direct", M.HIT), ("len34_hit", M.HIT)):
            assert (case, v) in seen, (case, v)
        assert {v for c, v in seen if c == "ecmp"} == {M.HIT, M.MISS}  # both members of the ECMP list were picked


@pytest.mark.parametrize("n", SIZES)
def test_lookup_matches_model(dev, world, n):
    import torch

    pair, keys, _ = world
    rng = np.random.default_rng(900 + n)
    nifs, ips = K.lookup_mix(rng, keys, n)
    d_ips = torch.from_numpy(ips.view(np.int32)).to(dev)
    d_nifs = torch.from_numpy(nifs).to(dev)
    for uniform in (None, 0, 2, 3):
        miss = torch.full((1,), 9, dtype=torch.int32, device=dev)
        if uniform is None:
            mac8, verdict, miss = pair.t.lookup(d_ips, d_nifs, miss_count=miss)
            use = nifs
        else:
            mac8, verdict, miss = pair.t.lookup(d_ips, None, netif=uniform, miss_count=miss)
            use = np.full(n, uniform, np.uint8)
        torch.cuda.synchronize()
        want = [pair.m.lookup(int(a), int(b)) for a, b in zip(use, ips)]
        assert list(verdict.cpu().numpy()) == [w[0] for w in want]
        got = mac8.cpu().numpy()
        for i, (v, m) in enumerate(want):
            assert bytes(got[i]) == (m + b"\0\0" if v == M.HIT else bytes(8)), i
        assert int(miss.cpu()[0]) - 9 == sum(1 for w in want if w[0] == M.MISS)
    if n >= 255:
        assert {w[0] for w in want} == {M.NONE}  # uniform NetIf 3 does not exist
        mixed = {pair.m.lookup(int(a), int(b))[0] for a, b in zip(nifs, ips)}
        assert mixed == {M.NONE, M.OWN_IP, M.MISS, M.HIT}


def test_post_dnat_destination(dev, world):
    """The L2 step reads bytes 30-33 as halo_tx_fixup_batch_device left them on the same stream."""
    import torch

    from halo_amd import protocol
    from halo_amd._lib import ARP_RESULT_DTYPE, TX_NAT_DST, TX_RECALC
    from oracle import ref_py as R

    pair, keys, rt = world
    nif, new_dst = next(k for k in keys if k[0] == 0)
    wan = K.NETIFS[1].ip
    src = M.ip_bytes(0x08080404)
    frames = [R.build_eth(R.build_ipv4(R.build_udp(b"payload-%d" % k, 4000 + k, 53, src, M.ip_bytes(wan)), 17, src,
                                       M.ip_bytes(wan)), K.NETIFS[1].mac, K.mac(900), 0x0800) for k in range(3)]
    rng = np.random.default_rng(4)
    data, offs, lens = _pack(rng, frames)
    d, o, ln = _up(dev, data, offs, lens)
    ops = protocol.tx_ops(3, TX_NAT_DST | TX_RECALC, dst_ip=new_dst, dst_port=5353)
    ops["steps"][2] = 0  # the third frame keeps the router's own address
    d_ops = torch.from_numpy(ops.view(np.uint8).reshape(3, 16)).to(dev)
    rids = rt.FindRoute(torch.from_numpy(np.array([new_dst, new_dst, wan], np.uint32).view(np.int32)).to(dev))
    protocol.tx_fixup_batch(d, o, ln, d_ops)
    res, counts, miss = pair.t.encap(d, o, ln, rids, 1)  # received on the NATing NetIf: no LOOPBACK
    torch.cuda.synchronize()
    got = res.cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE)
    assert list(got["verdict"]) == [M.HIT, M.HIT, M.OWN_IP]
    assert list(got["target_ip"]) == [new_dst, new_dst, wan] and list(got["out_netif"]) == [0, 0, 1]
    out = d.cpu().numpy()
    want_mac = pair.m.cache[(0, new_dst)][0]
    for k in range(2):
        f = out[4 * int(offs[k]):4 * int(offs[k]) + 34].tobytes()
        assert f[:6] == want_mac and f[6:12] == K.NETIFS[0].mac and f[30:34] == M.ip_bytes(new_dst)


def test_generations(dev):
    import torch

    p = K.Pair(capacity=8)
    try:
        a, b, c = 0x0A000010, 0x0A000011, 0x0A000012
        ips = torch.from_numpy(np.array([a, b, c], np.uint32).view(np.int32)).to(dev)
        from halo_amd import _lib

        with pytest.raises(_lib.HaloError):  # before the first sync
            p.t.lookup(ips)
        p.set(0, a, K.mac(1), 100)
        p.set(0, b, K.mac(2), 1000)
        p.t.sync()
        assert not p.t.dirty
        _, v_old, _ = p.t.lookup(ips)  # queued; nothing waits for it before the sync
        p.set(0, c, K.mac(3), 1000)
        p.set(0, a, K.mac(4), 100)  # a changed MAC
        assert p.t.dirty
        p.t.sync()
        mac_new, v_new, _ = p.t.lookup(ips)
        torch.cuda.synchronize()
        assert list(v_old.cpu().numpy()) == [M.HIT, M.HIT, M.MISS]
        assert list(v_new.cpu().numpy()) == [M.HIT, M.HIT, M.HIT]
        assert bytes(mac_new.cpu().numpy()[0][:6]) == K.mac(4)
        # a refresh of ExpTime alone leaves the copy clean
        p.set(0, b, K.mac(2), 1001)
        assert not p.t.dirty
        # a clear tick that removes an entry republishes: the next lookup misses without a sync
        assert p.expire(401) == 1
        assert not p.t.dirty
        _, v, miss = p.t.lookup(ips)
        torch.cuda.synchronize()
        assert list(v.cpu().numpy()) == [M.MISS, M.HIT, M.HIT] and int(miss.cpu()[0]) == 1
        # learned but not synced: the host finds it, the device misses
        d = 0x0A000013
        p.handle([(0, M.arp_pkt(2, K.mac(5), d, K.NETIFS[0].mac, K.NETIFS[0].ip), K.mac(5))], 1002)
        assert p.t.GetArpCache(0, d)[0] == M.GET_FOUND and p.t.dirty
        ip_d = torch.from_numpy(np.array([d], np.uint32).view(np.int32)).to(dev)
        _, v, _ = p.t.lookup(ip_d)
        torch.cuda.synchronize()
        assert list(v.cpu().numpy()) == [M.MISS]
        # synced without a route table: the L2 step has nothing to resolve route ids with
        z = torch.zeros(16, dtype=torch.uint8, device=dev)
        with pytest.raises(_lib.HaloError):
            p.t.encap(z, z.view(torch.int32)[:1], z.view(torch.int16)[:1], z.view(torch.int32)[:1], 0)
    finally:
        p.close()


def test_route_array_grows_under_a_queued_encap(dev):
    """The route array of a generation starts at 256 entries. A sync with 300 routes follows an encap
    that nothing waited for, and a second sync then reallocates the array of the generation written
    first, while the other one is published. Both encaps, 65 frames each (a wave and a lane), give
    the model's results; the second has route ids on both sides of 256."""
    import torch

    from halo_amd._lib import ARP_RESULT_DTYPE
    from halo_amd.route import RouteTable

    n, in_netif = 65, 1
    p, rt = K.Pair(capacity=8), RouteTable(0)
    try:
        hosts = [0x0A000010 + k for k in range(4)]  # neighbours of NetIf 0
        for k, ip in enumerate(hosts):
            p.set(0, ip, K.mac(20 + k), 1000)
        rt.AddRoute(RouteTable.entry(0x0A000000, 0xFFFFFF00, 0, 0))       # id 0: direct
        rt.AddRoute(RouteTable.entry(NH_HIT, 0xFFFF0000, hosts[1], 0))    # id 1: through a neighbour
        p.t.sync(rt)
        rng = np.random.default_rng(65)

        def encap(rids):
            """Queues the L2 step; returns the tensors (kept allocated) and the model's answer."""
            frames = [_ipv4_frame(rng, 60 + i % 6, hosts[i % 4] if i % 3 else _absent([(0, h) for h in hosts], 0, i)) for i in range(n)]
            data, offs, lens = _pack(rng, frames)
            want, want_res = data.copy(), np.zeros(n, ARP_RESULT_DTYPE)
            for i, f in enumerate(frames):
                v, out, tx, target, after = p.m.encap(f, _route_of(rt, int(rids[i])), in_netif, True)
                want_res[i] = (v, out, tx, target)
                want[4 * int(offs[i]):4 * int(offs[i]) + len(f)] = np.frombuffer(after, np.uint8)
            d, o, ln = _up(dev, data, offs, lens)
            d_rids = torch.from_numpy(rids.view(np.int32)).to(dev)
            res, counts, miss = p.t.encap(d, o, ln, d_rids, in_netif)
            return (d, o, ln, d_rids, res, counts, miss), want, want_res

        first = encap(np.array([i % 2 for i in range(n)], np.uint32))  # queued; nothing waits for it before the sync
        for k in range(2, 300):  # next hops that are neighbours of NetIf 0, on NetIf 0 and on one that does not hold them
            assert rt.AddRoute(RouteTable.entry(0x0B000000 + (k << 8), 0xFFFFFF00, hosts[k % 4] if k % 2 else 0, 0 if k % 5 else 2)) == k
        p.t.sync(rt)
        p.t.sync(rt)
        second = encap(np.array([(0, 1, 255, 256, 257, 299, 258, 2)[i % 8] for i in range(n)], np.uint32))
        torch.cuda.synchronize()
        for (t, want, want_res), verdicts in ((first, {M.HIT, M.MISS}), (second, {M.HIT, M.MISS})):
            got_res = t[4].cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE)
            bad = np.nonzero(got_res != want_res)[0]
            assert bad.size == 0, [(int(i), got_res[i], want_res[i]) for i in bad[:5]]
            assert np.array_equal(t[0].cpu().numpy(), want)
            assert list(t[5].cpu().numpy()) == [int((want_res["verdict"] == v).sum()) for v in range(7)]
            assert verdicts <= set(want_res["verdict"].tolist())
        hit_ids = {int(r) for r, v in zip(second[0][3].cpu().numpy(), second[2]["verdict"]) if v == M.HIT}
        assert {0, 1, 257, 299} <= hit_ids and 255 not in hit_ids  # resolved through the old and the new part of the array
    finally:
        p.close()
        rt.close()


def _arp_frame(rng, dst, src, nif, length=60, op=None):
    m = K.NETIFS[nif]
    op = int(rng.choice([1, 1, 2, 3])) if op is None else op
    sha = src if rng.integers(0, 5) else K.mac(999)
    spa = (m.ip & 0xFFFFFF00) | int(rng.integers(1, 9))
    tpa = (m.ip & 0xFFFFFF00) | int(rng.integers(1, 3))
    f = M.eth_frame(dst, src, 0x0806, M.arp_pkt(op, sha, spa, K.mac(0), tpa, head=rng.integers(0, 256, 6, dtype=np.uint8).tobytes()))
    return f[:length] if length <= 60 else f + rng.integers(0, 256, length - 60, dtype=np.uint8).tobytes()


def _gather_case(dev, rng, frames, nif, cap=None):
    """Parse, gather, compare the messages with the frames' bytes and handle_msgs with the model."""
    import torch

    from halo_amd import protocol
    from halo_amd._lib import ARP_MSG_DTYPE
    from halo_amd.arp import ArpTable

    netif = K.lib_netifs()[nif]
    data, offs, lens = _pack(rng, frames)
    d, o, ln = _up(dev, data, offs, lens)
    if frames:
        recs = protocol.parse_frames_batch(d, o, ln, netif=netif)
    else:
        recs = torch.zeros((1, 32), dtype=torch.uint8, device=dev)[:0]
    msgs, count = ArpTable.gather(d, o, ln, recs, nif, cap=cap)
    torch.cuda.synchronize()
    want = [i for i, f in enumerate(frames) if M.is_arp_for(f, K.NETIFS[nif].mac)]
    assert int(count.cpu()[0]) == len(want)
    k = len(want) if cap is None else min(cap, len(want))
    raw = msgs.cpu().numpy()
    got = raw.reshape(-1).view(ARP_MSG_DTYPE)
    assert list(got["index"][:k]) == want[:k]
    for j in range(k):
        f = frames[want[j]]
        assert int(got[j]["netif"]) == nif and int(got[j]["pad"]) == 0
        assert bytes(got[j]["eth_src"]) == f[6:12] and bytes(got[j]["arp"]) == f[14:42]
    assert not raw[k:].any()  # nothing beyond the first `cap` messages is written
    return got[:k].copy(), want


def test_gather_indexes_and_handle(dev):
    rng = np.random.default_rng(21)
    n, nif = 1000, 0
    own = K.NETIFS[nif].mac
    at = {0, 63, 64, 255, 256, 257, n - 1}
    not_ours = {10, 300}   # an ARP frame for another MAC
    too_short = {11, 511}  # 41 bytes: ParseEthFrm fails
    frames = []
    for i in range(n):
        src = K.mac(int(rng.integers(0, 6)))
        if i in at:
            frames.append(_arp_frame(rng, own if i % 2 else M.BCAST, src, nif, length=[42, 60, 77][i % 3]))
        elif i in not_ours:
            frames.append(_arp_frame(rng, K.mac(4242), src, nif))
        elif i in too_short:
            frames.append(_arp_frame(rng, own, src, nif, length=41))
        else:
            frames.append(own + _ipv4_frame(rng, int(rng.choice([60, 61, 64, 90])), 0x0A000005)[6:])
    msgs, want = _gather_case(dev, rng, frames, nif)
    assert want == sorted(at)
    # handle_msgs on the downloaded messages equals the model run on the same frames in frame order
    p = K.Pair(capacity=3)
    try:
        v, replies, changed = p.t.HandleArp(msgs, 50)
        res = [p.m.handle(nif, frames[i][14:42], frames[i][6:12], 50) for i in want]
        assert list(v) == [r[0] for r in res] and changed == sum(r[2] for r in res)
        assert [bytes(r) for r in replies] == [r[1] for r in res if r[1] is not None]
        p.check()
    finally:
        p.close()


def test_gather_all_none_and_cap(dev):
    rng = np.random.default_rng(22)
    nif = 2
    own = K.NETIFS[nif].mac
    every = [_arp_frame(rng, own if i % 3 else M.BCAST, K.mac(i % 7), nif, length=[42, 60, 61, 64][i % 4]) for i in range(600)]
    msgs, want = _gather_case(dev, rng, every, nif)
    assert want == list(range(600))
    p = K.Pair(capacity=5)
    try:
        v, replies, changed = p.t.HandleArp(msgs, 7)
        res = [p.m.handle(nif, f[14:42], f[6:12], 7) for f in every]
        assert list(v) == [r[0] for r in res] and changed == sum(r[2] for r in res)
        assert [bytes(r) for r in replies] == [r[1] for r in res if r[1] is not None]
        assert {r[0] & 0x0F for r in res} == {M.BAD_OP, M.SRC_MISMATCH, M.CONFLICT, M.ACCEPTED}
        p.check()
    finally:
        p.close()
    # cap below the count: the count is exact, exactly the first `cap` messages are written, in order
    for cap in (0, 1, 255, 256, 599):
        _gather_case(dev, rng, every, nif, cap=cap)
    none = [own + _ipv4_frame(rng, 64, 0x0A000005)[6:] for _ in range(300)]
    _, want = _gather_case(dev, rng, none, nif)
    assert want == []
    _, want = _gather_case(dev, rng, [], nif)
    assert want == []


def test_chain_parse_route_fixup_encap_parse(dev, world):
    """Frames NetIf 0 received: parse -> route lookup on the records -> fixup (TTL) -> encap of the
    frames whose TTL survived; the rewritten HIT frames, parsed as the next hop receives them, are
    addressed to it and still valid."""
    import torch

    from halo_amd import protocol
    from halo_amd._lib import ARP_RESULT_DTYPE, NetIf, TX_R_TTL_ALIVE, TX_RECALC, TX_TTL
    from oracle import ref_py as R

    pair, keys, rt = world
    rng = np.random.default_rng(33)
    in_nif = K.lib_netifs()[0]
    dsts = [ip for _, ip in keys[:6]] + [NH_HIT | 9, NH_MISS | 9, _absent(keys, 1, 3), 0x08080808]
    frames, ttls = [], []
    src = M.ip_bytes(0x0A0000C8)
    for k in range(120):
        dst = M.ip_bytes(dsts[k % len(dsts)])
        ttl = 1 if k % 7 == 3 else 64
        pl = rng.integers(0, 256, int(rng.integers(1, 80)), dtype=np.uint8).tobytes()
        pkt = R.build_ipv4(R.build_udp(pl, 1000 + k, 2000, src, dst), 17, src, dst, ttl=ttl)
        frames.append(R.build_eth(pkt, K.NETIFS[0].mac, K.mac(800), 0x0800))
        ttls.append(ttl)
    data, offs, lens = _pack(rng, frames)
    d, o, ln = _up(dev, data, offs, lens)
    recs = protocol.parse_frames_batch(d, o, ln, netif=in_nif)
    rids = rt.FindRouteRecords(recs)
    d_ops = torch.from_numpy(protocol.tx_ops(len(frames), TX_TTL | TX_RECALC).view(np.uint8).reshape(-1, 16)).to(dev)
    d_res = torch.empty(len(frames), dtype=torch.uint8, device=dev)
    protocol.tx_fixup_batch(d, o, ln, d_ops, result=d_res)
    alive = d_res & TX_R_TTL_ALIVE
    res, counts, miss = pair.t.encap(d, o, ln, rids, 0, select=alive)
    torch.cuda.synchronize()
    got = res.cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE)
    assert np.all(protocol.records(recs)["status"] == 0)
    alive_h = alive.cpu().numpy()
    assert 0 < int((alive_h == 0).sum()) < len(frames) and np.all(got["verdict"][alive_h == 0] == M.NONE)
    hits = np.nonzero(got["verdict"] == M.HIT)[0]
    assert hits.size >= 40 and (got["verdict"] == M.MISS).any() and (got["verdict"] == M.NO_ROUTE).any()
    for out, target in sorted({(int(got[i]["out_netif"]), int(got[i]["target_ip"])) for i in hits}):
        hop = NetIf()
        for b, x in enumerate(pair.m.cache[(out, target)][0]):
            hop.mac[b] = x
        hop.ip = target
        again = protocol.records(protocol.parse_frames_batch(d, o, ln, netif=hop))
        torch.cuda.synchronize()
        mine = [i for i in hits if (int(got[i]["out_netif"]), int(got[i]["target_ip"])) == (out, target)]
        assert all(int(again[i]["status"]) == 0 and int(again[i]["flags"]) & 1 for i in mine), (out, target)
