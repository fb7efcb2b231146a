"""GPU: the loopback step in its chain. `mark` (halo_arp_loopback_mark_device) against
tests/lo_model.py and against the encap's verdicts on the same batch; a lan0 batch that pings, sends
UDP to a served port and opens TCP connections to NAT-enabled wan0's address, among ordinary
forwarded traffic, through forward_return_flows(loopback=True) -> gather -> drain -> egress and
deliver; the same batch with loopback=False, which reproduces the chain without the step; and
TxIpv4's copies: built frames addressed to the router's own addresses through gather(tx=True) and
the drain, twice."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import ref_py as R
from oracle import ref_tx_py as T
from tests import arp_cases as K
from tests import arp_model as AM
from tests import deliver_model as DM
from tests import lo_model as LM
from tests import pmflow_cases as PC
from tests import respond_model as RM

pytestmark = pytest.mark.gpu

LAN, WAN1, WAN2 = PC.LAN, PC.WAN1, PC.WAN2
HOST, HOST_MAC = 0xC0A80132, bytes([0x02, 0xBB, 0, 0, 0, 0x32])  # 192.168.1.50
V_OVERRIDE = 3


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


def _t(dev, a, dtype=None):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dtype) if dtype is not None else a).to(dev)


# ---- mark ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(dev):
    pair, keys = K.forced_table(lambda **kw: K.Pair(**kw))
    rt = K.world_routes(keys)
    rt.sync()
    pair.t.sync(rt)
    yield pair, keys, rt
    pair.close()
    rt.close()


def _mark_batch(rng, keys, n, in_netif):
    """Valid frames NetIf in_netif receives, to every kind of destination, the three own addresses
    among them; a few that are not IPv4, too short, or fail the IPv4 parse (ip_proto stays 0xFF)."""
    me = K.NETIFS[in_netif]
    dsts = [ip for _, ip in keys[:4]] + [m.ip for m in K.NETIFS] + [K.NH_HIT | 9, K.NH_MISS | 9, K.NH_OWN | 3, 0x08080808,
                                                                    K.PANIC | 7, K.BAD_NETIF | 5, K.NETIFS[1].ip, K.NETIFS[2].ip]
    frames, dst_arr, kinds = [], [], []
    for k in range(n):
        dst_u = dsts[k % len(dsts)]
        src, dst = AM.ip_bytes(0x0A0000C8 + k % 5), AM.ip_bytes(dst_u)
        kind = ["udp", "icmp", "tcp", "udp", "arp", "udp", "bad_version", "udp", "short"][k % 9]
        pl = rng.integers(0, 256, int(rng.integers(0, 80)), dtype=np.uint8).tobytes()
        if kind == "icmp":
            pkt = R.build_ipv4(R.build_icmp(pl, 8, bytes([k & 255, 1]), k), 1, src, dst)
        elif kind == "tcp":
            pkt = R.build_ipv4(R.build_tcp(pl, 4000 + k, 80, src, dst, k, 0, 0x02), 6, src, dst)
        else:
            pkt = R.build_ipv4(R.build_udp(pl, 1000 + k, 2000, src, dst), 17, src, dst)
        f = bytearray(R.build_eth(pkt, me.mac, K.mac(800 + k % 3), 0x0806 if kind == "arp" else 0x0800))
        if kind == "bad_version":
            f[14] = 0x46
        if kind == "short":
            f = f[:33]
        frames.append(bytes(f))
        dst_arr.append(dst_u)
        kinds.append(kind)
    return frames, np.array(dst_arr, np.uint32), kinds


@pytest.mark.parametrize("in_netif", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_mark_matches_model_and_the_encap(dev, world, n, in_netif):
    import torch

    from halo_amd import loopback as L
    from halo_amd import protocol
    from halo_amd._lib import ARP_RESULT_DTYPE, PMFLOW_VIA_DTYPE

    pair, keys, rt = world
    rng = np.random.default_rng(300 + 3 * n + in_netif)
    frames, dsts, kinds = _mark_batch(rng, keys, n, in_netif)
    data, offs, lens = K.pack(rng, frames)
    d, o, ln = _t(dev, data), _t(dev, offs, np.int32), _t(dev, lens, np.int16)
    recs = protocol.parse_frames_batch(d, o, ln, netif=K.lib_netifs()[in_netif])
    rids = rt.FindRoute(_t(dev, dsts, np.int32))
    rids_h = rids.cpu().numpy().view(np.uint32).copy()
    rids_h[3::17] = 5000 + np.arange(len(rids_h[3::17]))  # ids the device copy does not know
    rids = _t(dev, rids_h, np.int32)
    # a via array: OVERRIDE to NetIf 1 / 2 / a NetIf the table does not have on some frames, HIT and MISS words on others
    via = np.zeros(n, PMFLOW_VIA_DTYPE)
    for i in range(n):
        sel = i % 7
        via[i] = [(1, 0xFF, 0, 0), (V_OVERRIDE, 1, 80, 0), (2, 2, 81, 0), (V_OVERRIDE, 2, 82, K.NH_HIT | 1), (0, 0xFF, 0, 0),
                  (V_OVERRIDE, 9, 83, 0), (1, 0xFF, 0, 0)][sel]
    recs_h = protocol.records(recs)
    for use_via in (False, True):
        d_via = _t(dev, via.view(np.uint8).reshape(-1, 8)) if use_via else None
        got = L.mark(pair.t, recs, rids, in_netif, via=d_via)
        res, _, _ = pair.t.encap_via(d.clone(), o, ln, rids, in_netif, d_via)
        torch.cuda.synchronize()
        got_h = got.cpu().numpy()
        res_h = res.cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE)
        want = np.array([LM.mark_of(pair.m, f, K.NETIFS[in_netif], K.route_of(rt, int(rids_h[i])), in_netif,
                                    tuple(via[i]) if use_via else None) for i, f in enumerate(frames)], np.uint8)
        assert np.array_equal(got_h, want), np.flatnonzero(got_h != want)[:8]
        # the mark equals the encap's later verdict for every frame whose parse reached the addresses
        parsed = recs_h["ip_proto"] != 0xFF
        assert np.array_equal(got_h[parsed] == 1, res_h["verdict"][parsed] == AM.LOOPBACK)
        assert not got_h[~parsed].any()
        if n >= 255:
            if in_netif == 1:
                assert not got_h.any() and not (res_h["verdict"] == AM.LOOPBACK).any()  # a NATing in NetIf: :193 fails
            else:
                assert got_h.sum() >= 20 and {int(x) for x in res_h["out_netif"][got_h == 1]} == {0, 1, 2}
                assert (got_h[parsed] == 0).sum() >= 50


def test_mark_argument_errors(dev, world):
    import torch

    from halo_amd import _lib
    from halo_amd.arp import ArpTable

    pair, keys, rt = world
    L = _lib.lib
    recs = torch.zeros((4, 32), dtype=torch.uint8, device=dev)
    rids = torch.zeros(4, dtype=torch.int32, device=dev)
    out = torch.zeros(4, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda t, r=recs, q=rids, nif=0, v=None, m=out, n=4: L.halo_arp_loopback_mark_device(  # noqa: E731
        t, _lib.ptr(r), n, _lib.ptr(q), nif, _lib.ptr(v), _lib.ptr(m), st)
    assert call(pair.t._t) == 0 and call(pair.t._t, n=0, r=None, q=None, m=None) == 0
    assert call(None) == _lib.HALO_E_INVAL and call(pair.t._t, nif=3) == _lib.HALO_E_RANGE
    assert call(pair.t._t, r=None) == _lib.HALO_E_INVAL and call(pair.t._t, q=None) == _lib.HALO_E_INVAL
    assert call(pair.t._t, m=None) == _lib.HALO_E_INVAL
    assert call(pair.t._t, r=recs.reshape(-1)[8:]) == _lib.HALO_E_INVAL  # records 16-byte aligned
    fresh = ArpTable(K.lib_netifs(), 4)
    assert call(fresh._t) == _lib.HALO_E_INVAL  # before the first sync
    fresh.sync(None)
    assert call(fresh._t) == _lib.HALO_E_INVAL  # synced without a route table
    fresh.close()
    torch.cuda.synchronize()


# ---- the chain -------------------------------------------------------------------------------------
class _Router:
    """lan0 (not NATing), wan0 = WAN1 (NATing, the default route), WAN2; one LAN host in lan0's cache."""

    def __init__(self, dev):
        from halo_amd import ArpTable, NatTable, PortMappingFlowTable
        from halo_amd.route import RouteTable

        self.netifs = PC.lib_netifs()[:3]
        self.rt = RouteTable(0)
        for q in range(3):
            self.rt.AddRoute(RouteTable.entry(PC.IPS[q] & 0xFFFFFF00, 0xFFFFFF00, 0, q))
        self.rt.AddRoute(RouteTable.entry(0, 0, PC.GATEWAYS[WAN1], WAN1))
        self.rt.sync()
        self.arp = ArpTable(self.netifs, 16)
        self.arp_m = AM.Model(PC.model_netifs()[:3], 16)
        for nif, ip, mac in ((LAN, HOST, HOST_MAC), (WAN1, PC.GATEWAYS[WAN1], PC.GW_MAC[WAN1])):
            self.arp.SetArpCache(nif, ip, mac, 10)
            self.arp_m.set(nif, ip, mac, 10)
        self.arp.sync(self.rt)
        self.nat = NatTable(PC.IPS[WAN1])
        self.pm = PortMappingFlowTable(self.netifs, PC.GATEWAYS[:3], 16)
        self.pm.sync(self.rt)

    def close(self):
        for x in (self.pm, self.arp, self.rt, self.nat):
            x.close()

    def route_of(self, dst):
        for q in range(3):
            if dst & 0xFFFFFF00 == PC.IPS[q] & 0xFFFFFF00:
                return (0, q)
        return (PC.GATEWAYS[WAN1], WAN1)


KINDS = ["echo", "udp_served", "syn_served", "known_flow", "new_flow", "syn_unserved"]


def _lan_batch(r, rng, n):
    frames = []
    host, wan = AM.ip_bytes(HOST), AM.ip_bytes(PC.IPS[WAN1])
    for k in range(n):
        kind = KINDS[k % len(KINDS)]
        pl = rng.integers(0, 256, int(rng.integers(0, 70)), dtype=np.uint8).tobytes()
        if kind == "echo":
            pkt = R.build_ipv4(R.build_icmp(pl, 8, bytes([k & 255, 2]), k), 1, host, wan, ident=k, ttl=64)
        elif kind == "udp_served":
            pkt = R.build_ipv4(R.build_udp(b"query-%d-" % k + pl, 5000 + k, 53, host, wan), 17, host, wan, ident=k, ttl=64)
        elif kind in ("syn_served", "syn_unserved"):
            pkt = R.build_ipv4(R.build_tcp(b"", 40000 + k, 80 if kind == "syn_served" else 81, host, wan, 0xFFFFFFF0 + k % 16, 0,
                                           0x02), 6, host, wan, ident=k, ttl=64)
        else:
            far = AM.ip_bytes(0x08080808 if kind == "known_flow" else 0x08080404)
            pkt = R.build_ipv4(R.build_udp(pl, 7000 + k, 33434, host, far), 17, host, far, ident=k, ttl=64)
        frames.append(R.build_eth(pkt, PC.MACS[LAN], HOST_MAC, 0x0800))
    return frames


def _hand_chain(r, d, o, ln, now, steps):
    """forward_return_flows as it stands without the loopback step, call by call."""
    import torch

    from halo_amd import protocol

    n = int(ln.shape[0])
    recs = protocol.parse_frames_batch(d, o, ln, netif=r.netifs[LAN])
    rids = r.rt.FindRouteRecords(recs)
    ops = torch.zeros((n, 16), dtype=torch.uint8, device=d.device)
    ops[:, 0] = steps
    ops, via, hit, _ = r.pm.lookup(recs, now, rids, ops=ops)
    ops, nv, ref, miss = r.nat.lookup_lan(recs, now, ops=ops, skip=hit)
    res = torch.zeros(n, dtype=torch.uint8, device=d.device)
    protocol.tx_fixup_batch(d, o, ln, ops.reshape(-1), result=res)
    results, counts, _ = r.arp.encap_via(d, o, ln, rids, LAN, via, select=res & protocol.TX_R_TTL_ALIVE)
    return dict(records=recs, route_ids=rids, ops=ops, nat_verdict=nv, fixup_result=res, results=results, counts=counts)


def test_lan_host_reaches_the_far_side_address(dev):
    import torch

    from halo_amd import deliver, egress_arp, forward_return_flows, port_map, protocol
    from halo_amd import loopback as L
    from halo_amd._lib import (ARP_RESULT_DTYPE, FLOW_NAT_LAN, NAT_V_FLOW, NAT_V_MISS, NAT_V_SKIP, TX_OP_DTYPE, TX_RECALC,
                               TX_TTL)
    from halo_amd.respond import tcp_port_map

    r = _Router(dev)
    try:
        rng = np.random.default_rng(2024)
        n, now, steps = 150, 400, TX_TTL | TX_RECALC
        frames = _lan_batch(r, rng, n)
        kinds = [KINDS[k % len(KINDS)] for k in range(n)]
        lo_kind = np.array([k in ("echo", "udp_served", "syn_served", "syn_unserved") for k in kinds])
        for k in range(n):  # the flows that exist already
            if kinds[k] == "known_flow":
                assert r.nat.AddFlow(HOST, 0x08080808, 7000 + k, 33434, 17, now - 5) is not None
        r.nat.sync()
        flows_before = len(r.nat.ListNat())
        data, offs, lens = K.pack(rng, frames)
        up = lambda: (_t(dev, data), _t(dev, offs, np.int32), _t(dev, lens, np.int16))  # noqa: E731

        # ---- loopback=False: the chain as it stands, bit for bit ----
        d0, o0, ln0 = up()
        off_ = forward_return_flows(d0, o0, ln0, netif=r.netifs[LAN], in_netif=LAN, now=now, pmflow=r.pm, routes=r.rt,
                                    arp=r.arp, nat=r.nat, steps=steps)
        d1, o1, ln1 = up()
        hand = _hand_chain(r, d1, o1, ln1, now, steps)
        torch.cuda.synchronize()
        assert off_.mark is None
        for name in ("records", "route_ids", "ops", "nat_verdict", "fixup_result", "results", "counts"):
            assert torch.equal(getattr(off_, name), hand[name]), name
        assert torch.equal(d0, d1)
        nv_off = off_.nat_verdict.cpu().numpy()
        res_off = off_.results.cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE)
        # today: the frames for wan0's own address are NAT misses, and the slow path adds a flow for each
        assert (nv_off[lo_kind] == NAT_V_MISS).all() and (res_off["verdict"][lo_kind] == AM.LOOPBACK).all()
        probe = type(r.nat)(PC.IPS[WAN1])  # a table of the same state, so that r.nat stays as it is
        for k in range(n):
            if kinds[k] == "known_flow":
                probe.AddFlow(HOST, 0x08080808, 7000 + k, 33434, 17, now - 5)
        _, added_off = probe.resolve_misses(FLOW_NAT_LAN, protocol.records(off_.records), nv_off, now,
                                            off_.ops.cpu().numpy().reshape(-1).view(TX_OP_DTYPE).copy())
        probe.close()
        assert added_off == int(lo_kind.sum()) + kinds.count("new_flow")

        # ---- loopback=True ----
        d, o, ln = up()
        out = forward_return_flows(d, o, ln, netif=r.netifs[LAN], in_netif=LAN, now=now, pmflow=r.pm, routes=r.rt, arp=r.arp,
                                   nat=r.nat, steps=steps, loopback=True)
        lo = L.gather(d, o, ln, out.results, 3, 1 << 16, n)
        torch.cuda.synchronize()
        mark, nv = out.mark.cpu().numpy(), out.nat_verdict.cpu().numpy()
        res = out.results.cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE)
        want_mark = np.array([LM.mark_of(r.arp_m, f, r.arp_m.netifs[LAN], r.route_of(AM.ip_of(f[30:34])), LAN) for f in frames])
        assert np.array_equal(mark, want_mark) and np.array_equal(mark == 1, lo_kind)
        assert np.array_equal(mark == 1, res["verdict"] == AM.LOOPBACK)
        assert (nv[lo_kind] == NAT_V_SKIP).all()
        assert [int(nv[k]) for k in range(n) if kinds[k] == "known_flow"] == [NAT_V_FLOW] * kinds.count("known_flow")
        assert [int(nv[k]) for k in range(n) if kinds[k] == "new_flow"] == [NAT_V_MISS] * kinds.count("new_flow")
        # the frames that are not LoChan packets come out as without the step
        assert np.array_equal(res[~lo_kind], res_off[~lo_kind])
        ops_h = out.ops.cpu().numpy().reshape(-1).view(TX_OP_DTYPE).copy()
        _, added = r.nat.resolve_misses(FLOW_NAT_LAN, protocol.records(out.records), nv, now, ops_h)
        assert added == kinds.count("new_flow") and len(r.nat.ListNat()) == flows_before + added  # none for the LoChan packets
        # the model's frames at the L2 step: TTL decremented, nothing else (no SNAT: :201 returns before :203)
        after = []
        for f, is_lo in zip(frames, lo_kind):
            g = bytearray(f)
            pkt = bytearray(g[14:])
            T.tx_frame(g, steps)
            after.append(bytes(g))
            if is_lo:
                assert g[26:30] == AM.ip_bytes(HOST) and g[22] == pkt[8] - 1
        got_after = d.cpu().numpy()
        for i in np.flatnonzero(lo_kind):
            assert bytes(got_after[4 * int(offs[i]):4 * int(offs[i]) + len(frames[i])]) == after[i], i
        netifs = []
        for i, f in enumerate(after):
            c = LM.forward_copy(r.arp_m, f, r.route_of(AM.ip_of(f[30:34])), LAN) if lo_kind[i] else None
            netifs.append(None if c is None else c[0])
        assert [x for x in netifs if x is not None] == [WAN1] * int(lo_kind.sum())
        want = LM.gather(after, netifs, 3, 1 << 16, n)
        assert np.array_equal(lo.ports, want.ports) and lo.n_skipped == 0
        assert lo.stream(WAN1).tobytes() == want.streams[WAN1] and lo.index(WAN1).tolist() == want.index[WAN1]
        assert lo.pkt_len(WAN1).tolist() == want.pkt_len[WAN1] and lo.pkt_off_dw(WAN1).tolist() == want.pkt_off[WAN1]
        packets = [after[i][14:] for i in want.index[WAN1]]
        assert all(p[12:16] == AM.ip_bytes(HOST) for p in packets)  # the LAN source, not wan0's

        # ---- the drain of wan0's LoChan ----
        builder = protocol.TxBuilder(n, ip_id=0x7000)
        d_tcp = _t(dev, tcp_port_map([80]), np.int32)
        dr = L.drain(lo, WAN1, netif=r.netifs[WAN1], self_netif=WAN1, builder=builder, routes=r.rt, arp=r.arp, tcp_ports=d_tcp)
        torch.cuda.synchronize()
        region = lo.out.cpu().numpy()[WAN1 << 16:(WAN1 + 1) << 16]
        m = LM.drain(packets, want.pkt_off[WAN1], region, r.arp_m, WAN1, r.route_of, 0x7000, tcp_ports=(80,), udp_ports=(53,))
        rep = dr.replies
        assert rep.respond.count == len(m.replies) == kinds.count("echo") + kinds.count("syn_served")
        assert [R.ACTIONS[a] for a in rep.respond.actions] == m.actions
        assert set(m.actions) == {"LOCAL_ICMP", "LOCAL_UDP", "LOCAL_TCP"} and builder.iph_id == m.ip_id
        got_frames, got_lens = rep.frames.cpu().numpy(), rep.lens.cpu().numpy().view(np.uint16)
        got_res = rep.results.cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE)
        seen = set()
        for k, (v, outp, tx, target, f2) in enumerate(m.frames):
            assert int(got_lens[k]) == len(f2) and bytes(got_frames[k, :len(f2)]) == f2, k
            assert tuple(got_res[k]) == (v, outp, tx, target) == (AM.HIT, LAN, max(len(f2), 60), HOST), k
            assert f2[0:6] == HOST_MAC and f2[6:12] == PC.MACS[LAN]  # out of lan0, to the ARP'd MAC
            rec = R.rx_frame(f2, HOST_MAC, HOST)
            assert rec["status"] == "OK" and rec["flags"] & 4 and rec["src_ip"] == PC.IPS[WAN1], rec
            seen.add((rec["ip_proto"], rec["l4_aux"]))
        assert seen == {(1, 0), (6, 0x12)}  # echo replies and SYN|ACKs
        eg = egress_arp(rep.frames.reshape(-1), rep.offsets_dw, rep.lens, rep.results, n_ports=3, region_bytes=1 << 16,
                        index_cap=n)
        torch.cuda.synchronize()
        assert eg.ports["frames"].tolist() == [len(m.frames), 0, 0]
        stream, pos = eg.stream(LAN), 0
        for (_v, _o, tx, _t2, f2) in m.frames:
            assert int(stream[pos:pos + 4].view(np.uint32)[0]) == tx and bytes(stream[pos + 4:pos + 4 + len(f2)]) == f2
            pos += (4 + tx + 3) & ~3
        assert pos == len(stream)
        # local delivery on the L3 records hands the UDP payloads (and the SYNs) to the handlers
        dl = deliver(dr.packets, dr.offsets_dw, dr.lens, dr.records, netif=r.netifs[WAN1], region_bytes=1 << 16,
                     udp_ports=_t(dev, port_map([53]), np.int32), tcp_ports=d_tcp, index_cap=n, l3_start=True)
        torch.cuda.synchronize()
        got_d = [(int(h["kind"]), int(h["remote_ip"]), int(h["remote_port"]), int(h["local_port"]), p) for h, p in dl.records()]
        want_d = [(x["kind"], x["remote_ip"], x["remote_port"], x["local_port"], bytes(x["payload"])) for _, x in m.deliveries.items]
        assert got_d == want_d
        udp = [x for x in got_d if x[0] == DM.UDP]
        assert len(udp) == kinds.count("udp_served") and all(x[1] == HOST and x[3] == 53 and x[4].startswith(b"query-") for x in udp)
    finally:
        r.close()


def test_tx_copies_drain_twice(dev):
    """The router pings wan0's address from lan0's: TxIpv4 on lan0 finds the destination to be wan0's
    own address and copies exactly totalLen bytes into wan0's LoChan (the frame is padded to 60
    bytes, the packet is not); wan0's drain answers to lan0's address, which is a LoChan copy again;
    lan0's drain takes the echo replies and answers nothing."""
    import torch

    from halo_amd import loopback as L
    from halo_amd import protocol
    from halo_amd._lib import ARP_RESULT_DTYPE, BUILD_DESC_DTYPE

    r = _Router(dev)
    try:
        rng = np.random.default_rng(99)
        n = 70
        plen = rng.integers(0, 64, n).astype(np.uint16)
        plen[:4] = [0, 1, 17, 18]  # 20 + 8 + 18 = 46: the first that needs no padding
        poff = np.zeros(n, np.uint64)
        poff[1:] = np.cumsum(plen[:-1].astype(np.uint64))
        payload = rng.integers(0, 256, int(plen.sum()) + 4, dtype=np.uint8)
        desc = np.zeros(n, BUILD_DESC_DTYPE)
        desc["payload_off"], desc["payload_len"], desc["proto"], desc["aux"] = poff, plen, 1, 8
        desc["src_port"], desc["dst_port"] = 0x4242, np.arange(n)  # echo id, seq
        desc["src_ip"], desc["dst_ip"] = PC.IPS[LAN], PC.IPS[WAN1]
        desc[5]["dst_ip"] = PC.GATEWAYS[WAN1]  # one that leaves: HIT, not a copy
        b_lan = protocol.TxBuilder(n, ip_id=0x100)
        frames, flens, bres = b_lan.build(_t(dev, desc.view(np.uint8)), _t(dev, payload), netif=r.netifs[LAN], out_stride=128)
        rids = r.rt.FindRoute(_t(dev, desc["dst_ip"].astype(np.uint32), np.int32))
        slot_off = torch.arange(n, dtype=torch.int32, device=dev) * 32
        res, _, _ = r.arp.encap_tx(frames.reshape(-1), slot_off, flens, rids, LAN)
        lo1 = L.gather(frames.reshape(-1), slot_off, flens, res, 3, 1 << 14, n, tx=True)
        torch.cuda.synchronize()
        assert (bres.cpu().numpy() == 0).all()
        # the model: built frames, TxIpv4's step, the copies
        replies = [(i, {f: int(desc[i][f]) for f in RM.DESC_FIELDS}) for i in range(n)]
        built, _ = RM.build_frames(replies, payload, PC.MACS[LAN], 0x100)
        sent = [RM.tx_ipv4(r.arp_m, bytes(f), r.route_of(int(desc[i]["dst_ip"])), LAN) for i, (_res, f) in enumerate(built)]
        got = frames.cpu().numpy()
        res_h = res.cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE)
        for i, (v, outp, tx, target, f2) in enumerate(sent):
            assert bytes(got[i, :len(f2)]) == f2 and tuple(res_h[i]) == (v, outp, tx, target), i
        assert [s[0] for s in sent].count(AM.LOOPBACK) == n - 1 and sent[5][0] == AM.HIT
        copies = [LM.tx_copy(r.arp_m, bytes(f), r.route_of(int(desc[i]["dst_ip"])), LAN) for i, (_res, f) in enumerate(built)]
        netifs = [None if c is None else c[0] for c in copies]
        want1 = LM.gather([s[4] for s in sent], netifs, 3, 1 << 14, n, tx=True)
        assert np.array_equal(lo1.ports, want1.ports) and lo1.ports["frames"].tolist() == [0, n - 1, 0]
        assert lo1.stream(WAN1).tobytes() == want1.streams[WAN1] and lo1.pkt_len(WAN1).tolist() == want1.pkt_len[WAN1]
        assert want1.pkt_len[WAN1][:4] == [28, 29, 45, 46] and len(sent[0][4]) == 60  # totalLen bytes, not the padded frame's
        assert lo1.index(WAN1).tolist() == want1.index[WAN1] == [i for i in range(n) if i != 5]
        # ---- wan0's drain: echo replies to lan0's address, LoChan copies again ----
        b_wan = protocol.TxBuilder(n, ip_id=0x200)
        dr1 = L.drain(lo1, WAN1, netif=r.netifs[WAN1], self_netif=WAN1, builder=b_wan, routes=r.rt, arp=r.arp)
        rep = dr1.replies
        lo2 = L.gather(rep.frames.reshape(-1), rep.offsets_dw, rep.lens, rep.results, 3, 1 << 14, n, tx=True)
        torch.cuda.synchronize()
        packets1 = [c[1] for c in copies if c is not None]
        region1 = lo1.out.cpu().numpy()[WAN1 << 14:(WAN1 + 1) << 14]
        m1 = LM.drain(packets1, want1.pkt_off[WAN1], region1, r.arp_m, WAN1, r.route_of, 0x200)
        assert rep.respond.count == len(m1.replies) == n - 1 and m1.actions == ["LOCAL_ICMP"] * (n - 1)
        got2 = rep.frames.cpu().numpy()
        res2 = rep.results.cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE)
        for k, (v, outp, tx, target, f2) in enumerate(m1.frames):
            assert bytes(got2[k, :len(f2)]) == f2 and tuple(res2[k]) == (v, outp, tx, target) == (AM.LOOPBACK, LAN, 0, 0), k
        want2 = LM.gather([f[4] for f in m1.frames], [LAN] * (n - 1), 3, 1 << 14, n, tx=True)
        assert np.array_equal(lo2.ports, want2.ports) and lo2.ports["frames"].tolist() == [n - 1, 0, 0]
        assert lo2.stream(LAN).tobytes() == want2.streams[LAN]
        # ---- lan0's drain: echo replies are taken, nothing is answered ----
        dr2 = L.drain(lo2, LAN, netif=r.netifs[LAN], self_netif=LAN, builder=b_lan, routes=r.rt, arp=r.arp)
        torch.cuda.synchronize()
        recs2 = protocol.records(dr2.records)
        assert dr2.replies.respond.count == 0 and (recs2["status"] == 0).all() and (recs2["l4_aux"] == 0).all()
        assert (recs2["src_ip"] == PC.IPS[WAN1]).all() and (recs2["dst_ip"] == PC.IPS[LAN]).all()
        assert [int(x) & 0xFFFF for x in recs2["l4_seq"]] == [i for i in range(n) if i != 5]
        assert [R.ACTIONS[a] for a in dr2.replies.respond.actions] == ["LOCAL_ICMP"] * (n - 1)
    finally:
        r.close()
