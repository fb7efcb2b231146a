"""GPU: the device side of the port-mapping return-flow table (halo_amd/csrc/pmflow_fwd.hip and the
via variant of arp_fwd.hip's encap, through halo_amd.pmflow) against the dict model
(tests/pmflow_model.py), bit for bit behind a 0xA5 prefill: the LAN-side lookup over the forced
16-slot table at the batch sizes around a wavefront and a 256-frame workgroup; the WAN-side listing
around its tile and scan-pass edges; the L2 step with the out-interface override; the result edit
for dropped frames followed by the egress; and the chain of a three-NetIf dual-WAN router, with the
device lookup, with the host lookup before the sync, and with the table full."""
from __future__ import annotations

import numpy as np
import pytest

from tests import arp_cases as K
from tests import arp_model as AM
from tests import pmflow_cases as C
from tests import pmflow_model as PM

pytestmark = pytest.mark.gpu

SIZES = C.SIZES
FILL = C.FILL
TX_TTL, TX_NAT_DST, TX_NAT_SRC, TX_RECALC = 0x02, 0x01, 0x04, 0x08
NAT_V_MISS, NAT_V_FLOW, NAT_V_MAPPING = 2, 3, 4
T0 = 1000
_clock = [T0]  # TimeNow of the module: never goes backwards, whatever order the tests run in


def _tick() -> int:
    _clock[0] += 1
    assert _clock[0] - T0 <= 60, "a flow of the shared table that no test touches would expire"
    return _clock[0]


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


def _routes():
    """LAN, WAN1, WAN2, DMZ direct; the default route and 9.9/16 through WAN1's gateway; 7.7/16
    through WAN2's; 6.6/16 an emptied list. Returns (table, {name: route id})."""
    from halo_amd.route import RouteTable

    rt = RouteTable(0)
    ids = {}
    for q, name in enumerate(("lan", "wan1", "wan2", "dmz")):
        ids[name] = rt.AddRoute(RouteTable.entry(C.IPS[q] & 0xFFFFFF00, 0xFFFFFF00, 0, q))
    ids["default"] = rt.AddRoute(RouteTable.entry(0, 0, C.GATEWAYS[C.WAN1], C.WAN1))
    ids["via_wan2"] = rt.AddRoute(RouteTable.entry(0x07070000, 0xFFFF0000, C.GATEWAYS[C.WAN2], C.WAN2))
    gone = RouteTable.entry(0x06060000, 0xFFFF0000, C.GATEWAYS[C.WAN1], C.WAN1)
    rt.AddRoute(gone)
    rt.DeleteRoute(gone)
    return rt, ids


@pytest.fixture(scope="module")
def world(dev):
    """The forced 16-slot table (nine flows recorded from WAN2, three from the DMZ NetIf, which does
    not NAT) with its model, synced with the route table."""
    from halo_amd import PortMappingFlowTable

    make = lambda: PortMappingFlowTable(C.lib_netifs(), C.GATEWAYS, 15, 4)  # noqa: E731
    items, st = C.fixture_items(make)
    t, m = make(), PM.Model(C.model_netifs(), C.GATEWAYS, 15)
    for nif, part in ((C.WAN2, items[:9]), (C.DMZ, items[9:])):
        t.record(nif, C.item_array(part), T0)
        m.record(nif, part, T0)
    assert t.layout_stats()["longest_chain"] == st["longest_chain"] >= 3 and t.layout_stats()["wrapped"] >= 1
    rt, ids = _routes()
    rt.sync()
    assert t.dirty
    t.sync(rt)
    assert not t.dirty
    yield t, m, items, rt, ids
    t.close()
    rt.close()


def _up(dev, data, offs, lens):
    import torch

    return (torch.from_numpy(data).to(dev), torch.from_numpy(offs.view(np.int32)).to(dev),
            torch.from_numpy(lens.view(np.int16)).to(dev))


def _t(dev, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _route_arg(rt, rid):
    return K.route_of(rt, int(rid))


def _ops_prefill(n, extra=0):
    from halo_amd._lib import TX_OP_DTYPE

    ops = np.frombuffer(bytes([FILL]) * (16 * (n + extra)), TX_OP_DTYPE).copy()
    ops["steps"][:n] = TX_TTL
    return ops


def _reply_frame(it, ttl=64):
    """The LAN server's packet of flow `it` (a model item): LAN host -> remote."""
    rip, rport, lip, lport, proto, _wan_port = it
    return C.l4_frame(proto, lip, lport, rip, rport, C.MACS[C.LAN], ttl)


def _lookup_batch(items, n, mode, ids):
    """n frames the LAN NetIf received and a route id for each. mode: 'none' (no flow in the
    batch), 'all' (a hit per record), 'mixed' (every case, hits on both sides of the wave and
    workgroup boundaries)."""
    rid_cycle = [ids["via_wan2"], ids["default"], AM.ROUTE_NONE, AM.ROUTE_PANIC_ID, ids["lan"], ids["dmz"], 1000, ids["wan2"]]
    edges = {62, 63, 64, 65, 254, 255, 256, 257}
    frames, select, rids, names = [], [], [], []
    for i in range(n):
        it = items[(i * 7 + i // 12) % len(items)]
        kind = {"none": "absent", "all": "hit"}.get(mode) or (
            "hit" if i in edges else ["hit", "absent", "icmp", "not_ipv4", "unselected", "hit", "near_miss", "hit"][i % 8])
        sel = 1
        if kind == "hit":
            f = _reply_frame(it)
        elif kind == "unselected":
            f, sel = _reply_frame(it), 0
        elif kind == "near_miss":  # one key field off: the whole key is compared
            rip, rport, lip, lport, proto, wp = it
            f = _reply_frame([(rip ^ 1, rport, lip, lport, proto, wp), (rip, rport ^ 1, lip, lport, proto, wp),
                              (rip, rport, lip, lport ^ 1, proto, wp), (rip, rport, lip, lport, 23 - proto, wp)][(i // 8) % 4])
        elif kind == "icmp":
            f = C.l4_frame(1, it[2], it[3], it[0], it[1], C.MACS[C.LAN])
        elif kind == "not_ipv4":  # ParseIpv4Pkt never ran: ip_proto 0xFF
            f = bytearray(_reply_frame(it))
            f[12:14] = b"\x08\x06"
            f = bytes(f)
        else:
            f = C.l4_frame([6, 17][i % 2], C.SERVER + 9, 1000 + i, 0x08080808, 53, C.MACS[C.LAN])
        frames.append(f)
        select.append(sel)
        rids.append(rid_cycle[(i + i // 8) % len(rid_cycle)])
        names.append(kind)
    return frames, np.array(select, np.uint8), np.array(rids, np.uint32), names


def _device_lookup(dev, t, d_recs, n, now, d_rids, d_sel, ops):
    """halo_pmflow_lookup_device over prefilled buffers with eight spare entries behind each."""
    import torch

    from halo_amd import _lib

    d_ops = _t(dev, ops.view(np.uint8).reshape(-1, 16))
    d_via = torch.full((n + 8, 8), FILL, dtype=torch.uint8, device=dev)
    d_hit = torch.full((n + 8,), FILL, dtype=torch.uint8, device=dev)
    d_counts = torch.full((4,), 3, dtype=torch.int32, device=dev)  # incremented, not set
    _lib.check("halo_pmflow_lookup_device", _lib.lib.halo_pmflow_lookup_device(
        t._t, _lib.ptr(d_recs), n, now, _lib.ptr(d_rids), _lib.ptr(d_sel), _lib.ptr(d_ops), _lib.ptr(d_via), _lib.ptr(d_hit),
        _lib.ptr(d_counts), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return (d_ops.cpu().numpy().reshape(-1).view(ops.dtype), d_via.cpu().numpy().reshape(-1).view(_lib.PMFLOW_VIA_DTYPE),
            d_hit.cpu().numpy(), d_counts.cpu().numpy() - 3)


@pytest.mark.parametrize("mode", ["none", "mixed", "all"])
@pytest.mark.parametrize("n", SIZES)
def test_lookup_matches_model(dev, world, n, mode):
    from halo_amd import _lib, protocol

    t, m, items, rt, ids = world
    frames, select, rids, names = _lookup_batch(items, n, mode, ids)
    data, offs, lens = C.pack(frames)
    d, o, ln = _up(dev, data, offs, lens)
    d_recs = protocol.parse_frames_batch(d, o, ln, netif=C.lib_netifs()[C.LAN])
    now = _tick()
    ops = _ops_prefill(n, 8)
    want_ops = ops.copy()
    want_via = np.frombuffer(bytes([FILL]) * (8 * (n + 8)), _lib.PMFLOW_VIA_DTYPE).copy()
    want_hit = np.full(n + 8, FILL, np.uint8)
    seen = set()
    for i, f in enumerate(frames):
        tup = PM.five_tuple(f, C.MACS[C.LAN], C.IPS[C.LAN])
        v, wan, port, hop, snat = m.lookup(tup, _route_arg(rt, rids[i]), now, bool(select[i]))
        want_via[i] = (v, wan, port, hop)
        want_hit[i] = 1 if v in (PM.V_HIT, PM.V_OVERRIDE) else 0
        if snat is not None:
            want_ops[i]["steps"] |= TX_NAT_SRC
            want_ops[i]["src_ip"], want_ops[i]["src_port"] = snat
        seen.add((names[i], v, snat is not None))
    got_ops, got_via, got_hit, got_counts = _device_lookup(dev, t, d_recs, n, now, _t(dev, rids.view(np.int32)),
                                                           _t(dev, select), ops)
    bad = np.nonzero(got_via != want_via)[0]
    assert bad.size == 0, [(int(i), names[i] if i < n else "tail", got_via[i], want_via[i]) for i in bad[:5]]
    assert np.array_equal(got_hit, want_hit)
    assert got_ops.tobytes() == want_ops.tobytes()  # whole ops: no other field written, nothing past n
    assert list(got_counts) == [int((want_via["verdict"][:n] == v).sum()) for v in range(4)]
    # the stamps, read back through expire / List
    assert t.TableClear(now) == 0 == m.expire(now)
    assert C.listing_of(t.List()) == m.listing()
    if mode == "none":
        assert set(want_via["verdict"][:n]) == {PM.V_MISS}
    if mode == "all":
        assert set(want_via["verdict"][:n]) <= {PM.V_HIT, PM.V_OVERRIDE} and want_hit[:n].all()
    if mode == "mixed" and n >= 255:
        vs = {(k, v) for k, v, _ in seen}
        for case in (("hit", PM.V_HIT), ("hit", PM.V_OVERRIDE), ("absent", PM.V_MISS), ("near_miss", PM.V_MISS),
                     ("icmp", PM.V_MISS), ("not_ipv4", PM.V_NONE), ("unselected", PM.V_NONE)):
            assert case in vs, case
        assert ("hit", PM.V_HIT, False) in seen and ("hit", PM.V_OVERRIDE, False) in seen  # the DMZ flows: no NAT_SRC
        assert ("hit", PM.V_HIT, True) in seen and ("hit", PM.V_OVERRIDE, True) in seen
        for i in (63, 64, 255, 256):
            if i < n:
                assert want_hit[i] == 1
        # every verdict a route id can give a hit: WAN2 route, another NetIf, no route, the panic id, an unknown id
        by_rid = {(int(rids[i]), int(want_via["verdict"][i])) for i in range(n) if names[i] == "hit"}
        assert (ids["via_wan2"], PM.V_HIT) in by_rid or (ids["wan2"], PM.V_HIT) in by_rid
        assert (ids["default"], PM.V_OVERRIDE) in by_rid and (AM.ROUTE_NONE, PM.V_OVERRIDE) in by_rid
        assert (AM.ROUTE_PANIC_ID, PM.V_HIT) in by_rid and (1000, PM.V_OVERRIDE) in by_rid


def _records(n):
    from halo_amd._lib import RESULT_DTYPE

    r = np.zeros(n, RESULT_DTYPE)
    r["ethertype"], r["ip_proto"] = 0x0800, 17
    return r


def test_generations_grow_under_queued_lookups(dev):
    """Three writes of the device copy around lookups nothing waits for: a sync of 3 flows; a lookup;
    197 more flows and a sync, whose slot array no longer fits the first allocation (256 slots); a
    lookup that hits three flows in four; an expiry tick, which folds the device's stamps, removes
    the flows never hit and publishes into the generation written first, reallocating it while the
    other one is published; a lookup without a sync. One synchronise at the end: every lookup is the
    model's at its own table state, and the survivors carry the stamps the device wrote."""
    import torch

    from halo_amd import PortMappingFlowTable
    from halo_amd._lib import PMFLOW_VIA_DTYPE, TX_OP_DTYPE

    n_flows, T = 200, 5000
    rng = np.random.RandomState(77)
    items = []
    while len(items) < n_flows:
        it = (int(rng.randint(1, 1 << 31)), int(rng.randint(1, 65536)), C.SERVER + int(rng.randint(0, 4)),
              int(rng.randint(1, 65536)), int(rng.choice([6, 17])), int(rng.randint(1, 65536)))
        if it[:5] not in {x[:5] for x in items}:
            items.append(it)
    recs = _records(n_flows + 8)  # every flow's reply from the LAN host, then eight records of no flow
    recs["src_ip"], recs["sport"], recs["dst_ip"], recs["dport"] = C.SERVER + 9, 1000, 0x08080808, 53
    for i, it in enumerate(items):
        recs[i]["dst_ip"], recs[i]["dport"], recs[i]["src_ip"], recs[i]["sport"], recs[i]["ip_proto"] = it[:5]
    rt, ids = _routes()
    cycle = [ids["via_wan2"], ids["default"], AM.ROUTE_NONE, ids["lan"], 1000, ids["wan2"], AM.ROUTE_PANIC_ID]
    rids = np.array([cycle[i % len(cycle)] for i in range(len(recs))], np.uint32)
    t, m = PortMappingFlowTable(C.lib_netifs(), C.GATEWAYS, 400), PM.Model(C.model_netifs(), C.GATEWAYS, 400)

    def record(nif, part, now):
        dropped, added = t.record(nif, C.item_array(part), now)
        assert added == len(part) == m.record(nif, part, now)[1] and not dropped.any()

    def lookup(which, now):
        """Queues a lookup of the records `which`: its tensors and the model's answer at this state."""
        r, rd = recs[which], rids[which]
        want_via, want_ops = np.zeros(len(r), PMFLOW_VIA_DTYPE), np.zeros(len(r), TX_OP_DTYPE)
        for i in range(len(r)):
            tup = tuple(int(r[i][k]) for k in ("ip_proto", "src_ip", "dst_ip", "sport", "dport"))
            v, wan, port, hop, snat = m.lookup(tup, _route_arg(rt, rd[i]), now)
            want_via[i] = (v, wan, port, hop)
            if snat is not None:
                want_ops[i]["steps"], want_ops[i]["src_ip"], want_ops[i]["src_port"] = TX_NAT_SRC, snat[0], snat[1]
        d_recs, d_rids = _t(dev, r.view(np.uint8).reshape(-1, 32)), _t(dev, rd.view(np.int32))
        return (d_recs, d_rids) + t.lookup(d_recs, now, d_rids), want_via, want_ops

    try:
        record(C.WAN2, items[:3], T)
        t.sync(rt)
        every = np.arange(len(recs))
        calls = [lookup(every, T + 1)]  # queued; nothing waits for it before the sync
        record(C.WAN2, items[3:100], T)
        record(C.DMZ, items[100:], T)
        assert int(t.layout_stats()["slots"]) > 256
        t.sync(rt)
        calls.append(lookup(every[every % 4 != 3], T + 50))
        removed = t.TableClear(T + 70)
        assert removed == m.expire(T + 70) and 0 < removed < n_flows - 3
        assert int(t.layout_stats()["slots"]) > 256  # the generation written first has to grow as well
        calls.append(lookup(every, T + 71))
        torch.cuda.synchronize()
        for k, ((_, _, ops, via, hit, counts), want_via, want_ops) in enumerate(calls):
            got_via = via.cpu().numpy().reshape(-1).view(PMFLOW_VIA_DTYPE)
            bad = np.nonzero(got_via != want_via)[0]
            assert bad.size == 0, (k, [(int(i), got_via[i], want_via[i]) for i in bad[:5]])
            assert np.array_equal(hit.cpu().numpy(), (want_via["verdict"] >= PM.V_HIT).astype(np.uint8)), k
            assert ops.cpu().numpy().tobytes() == want_ops.tobytes(), k
            assert list(counts.cpu().numpy()) == [int((want_via["verdict"] == v).sum()) for v in range(4)], k
        hits = [int((w["verdict"] >= PM.V_HIT).sum()) for _, w, _ in calls]
        assert hits[0] == 3 and hits[1] == 150 and hits[2] == n_flows - removed == 150
        assert t.TableClear(T + 71) == 0 == m.expire(T + 71)  # folds the third lookup's stamps
        assert C.listing_of(t.List()) == m.listing()
        assert {e[8] for e in m.listing()} == {T + 71}
    finally:
        t.close()
        rt.close()


def _record_inputs(items, n, cand_at):
    """Synthetic inputs of halo_pmflow_record_device for frames WAN2 received: records, inbound
    verdicts, ops and ARP results, with the candidates at `cand_at` cycling through known-identical,
    known-different (another WAN port; recorded from another NetIf), and absent, and near-candidates
    (a FLOW verdict, an ARP MISS) in between."""
    from halo_amd._lib import ARP_RESULT_DTYPE, TX_OP_DTYPE

    recs, ops = _records(n), np.zeros(n, TX_OP_DTYPE)
    wv = np.full(n, NAT_V_MISS, np.uint8)
    arp = np.zeros(n, ARP_RESULT_DTYPE)
    arp["verdict"], arp["out_netif"] = AM.MISS, C.LAN
    recs["src_ip"], recs["sport"] = 0x08080000 + (np.arange(n) & 0xFFFF), 1024 + (np.arange(n) % 60000)
    recs["dst_ip"], recs["dport"] = C.IPS[C.WAN2], 8080
    ops["steps"], ops["dst_ip"], ops["dst_port"] = TX_TTL | TX_NAT_DST, C.SERVER, 80
    for j, i in enumerate(sorted(cand_at)):
        kind = j % 6
        it = items[j % 9] if kind in (0, 1) else items[9 + j % 3] if kind == 2 else None
        if it is not None:  # a flow the device copy holds: items[:9] from WAN2, items[9:] from the DMZ NetIf
            recs[i]["src_ip"], recs[i]["sport"], recs[i]["ip_proto"] = it[0], it[1], it[4]
            ops[i]["dst_ip"], ops[i]["dst_port"] = it[2], it[3]
            recs[i]["dport"] = it[5] if kind in (0, 2) else it[5] ^ 1  # kind 1: another WAN port
        wv[i] = NAT_V_FLOW if kind == 4 else NAT_V_MAPPING
        arp[i]["verdict"] = AM.MISS if kind == 5 else AM.HIT
    return recs, wv, ops, arp


def _record_expect(m, recs, wv, ops, arp, in_netif, now):
    """The model's listing of a batch: items in frame order; stamps the known-identical ones."""
    want = []
    for i in np.nonzero((wv == NAT_V_MAPPING) & (arp["verdict"] == AM.HIT))[0]:
        tup = (int(recs[i]["ip_proto"]), int(recs[i]["src_ip"]), int(recs[i]["dst_ip"]), int(recs[i]["sport"]),
               int(recs[i]["dport"]))
        key, wan_port = PM.Model.candidate(tup, int(wv[i]), int(arp[i]["verdict"]), int(ops[i]["dst_ip"]), int(ops[i]["dst_port"]))
        f = m.flows.get(key)
        if f is not None and f[0] == in_netif and f[1] == wan_port:
            f[2] = now  # :264, nothing else changes
        else:
            want.append((int(i),) + key + (wan_port,))
    return want


def _run_record(dev, t, recs, wv, ops, arp, now, cap, ws=None):
    import torch

    from halo_amd import _lib

    n = len(recs)
    d_items = torch.full((cap + 4, 20), FILL, dtype=torch.uint8, device=dev)
    d_count = torch.full((1,), 77, dtype=torch.int32, device=dev)  # SET, not incremented
    wsb = int(_lib.lib.halo_pmflow_record_workspace(n))
    if ws is None:
        ws = torch.full((wsb // 4 + 2,), -1, dtype=torch.int32, device=dev)
    # named, so that the inputs stay allocated through the call
    d_recs, d_wv = _t(dev, recs.view(np.uint8).reshape(-1, 32)), _t(dev, wv)
    d_ops, d_arp = _t(dev, ops.view(np.uint8).reshape(-1, 16)), _t(dev, arp.view(np.uint8).reshape(-1, 8))
    _lib.check("halo_pmflow_record_device", _lib.lib.halo_pmflow_record_device(
        t._t, C.WAN2, _lib.ptr(d_recs), _lib.ptr(d_wv), _lib.ptr(d_ops), _lib.ptr(d_arp), n, now,
        _lib.ptr(d_items), cap, _lib.ptr(d_count), _lib.ptr(ws), wsb, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = d_items.cpu().numpy().reshape(-1).view(_lib.PMFLOW_ITEM_DTYPE)
    return got, int(d_count.cpu()[0]), ws


def _item_rows(want):
    from halo_amd._lib import PMFLOW_ITEM_DTYPE

    a = np.zeros(len(want), PMFLOW_ITEM_DTYPE)
    for j, (i, rip, rport, lip, lport, proto, wp) in enumerate(want):
        a[j] = (i, rip, lip, rport, lport, wp, proto, 0)
    return a


@pytest.mark.parametrize("n", SIZES)
def test_record_device_matches_model(dev, world, n):
    t, m, items, rt, ids = world
    c = C.derived(C.read_constants())
    tile = c["record_tile"] - 1
    cand = {i for i in range(n) if i % 5 == 0 or i in (62, 63, 64, 65, tile - 2, tile - 1, tile, tile + 1)}
    recs, wv, ops, arp = _record_inputs(items, n, cand)
    ws = None
    total = None
    for cap_kind in ("above", "at", "below", "zero"):  # one workspace serves all four calls
        now = _tick()
        want = _record_expect(m, recs, wv, ops, arp, C.WAN2, now)
        total = len(want)
        cap = {"above": total + 3, "at": total, "below": total // 2, "zero": 0}[cap_kind]
        got, count, ws = _run_record(dev, t, recs, wv, ops, arp, now, cap, ws)
        assert count == total
        k = min(cap, total)
        assert got[:k].tobytes() == _item_rows(want[:k]).tobytes(), cap_kind
        assert got[k:].tobytes() == bytes([FILL]) * (20 * (cap + 4 - k)), cap_kind  # nothing at or beyond min(count, cap)
        assert t.TableClear(now) == 0 == m.expire(now)
        assert C.listing_of(t.List()) == m.listing()  # the known-identical candidates were stamped, the others not
    if n >= 255:
        kinds = {j % 6 for j in range(len(cand))}
        assert kinds == set(range(6)) and 0 < total < len(cand)
    if n > tile:
        idx = {w[0] for w in want}  # candidates on both sides of the tile edge, items from both tiles
        assert {tile - 1, tile} <= cand and min(idx) < tile <= max(idx)


def test_record_device_past_one_scan_pass(dev, world):
    """Candidates on both sides of the scan's pass edge: the first batch size whose tiles need a
    second pass of the one-workgroup scan, plus most of another tile."""
    t, m, items, rt, ids = world
    c = C.read_constants()
    edge = c["kRecordTile"] * c["kScanPass"]  # the first frame of the second pass
    n = edge + 200
    assert n == C.derived(c)["record_scan_pass"] + 199
    cand = {0, 255, 256, 100000, edge - 257, edge - 256, edge - 2, edge - 1, edge, edge + 1, edge + 64, n - 1}
    cand |= {edge - 3 * k for k in range(3, 40)} | {edge + 2 * k for k in range(3, 40)}
    recs, wv, ops, arp = _record_inputs(items, n, cand)
    now = _tick()
    want = _record_expect(m, recs, wv, ops, arp, C.WAN2, now)
    got, count, _ = _run_record(dev, t, recs, wv, ops, arp, now, len(want))
    assert count == len(want) and got[:count].tobytes() == _item_rows(want).tobytes()
    idx = [w[0] for w in want]
    assert any(edge - 120 <= i < edge for i in idx) and any(i >= edge for i in idx) and idx == sorted(idx)
    assert t.TableClear(now) == 0 == m.expire(now)
    assert C.listing_of(t.List()) == m.listing()


# ---- the L2 step with the override -----------------------------------------------------------------
@pytest.fixture(scope="module")
def arp_world(dev):
    pair, keys = K.forced_table(lambda **kw: K.Pair(**kw))
    rt = K.world_routes(keys)
    rt.sync()
    pair.t.sync(rt)
    yield pair, keys, rt
    pair.close()
    rt.close()


def _via_for(rng, keys, i, kind, dst):
    """(verdict, wan_netif, wan_port, next_hop) for frame i of a mixed batch."""
    nif, ip = keys[(i * 5) % len(keys)]
    k = i % 12
    if k in (0, 7):
        return (PM.V_NONE, 0xFF, 0, 0)
    if k == 1:
        return (PM.V_MISS, 0xFF, 0, 0)
    if k == 2:  # a HIT leaves the route alone, whatever it carries
        return (PM.V_HIT, nif, 8080, ip)
    if kind == "own_dst":  # forced out of the NetIf whose address dst is: LOOPBACK unless the in NetIf NATs
        q = [nf.ip for nf in K.NETIFS].index(dst)
        return (PM.V_OVERRIDE, q, 8085, K.absent(keys, q, i) if i % 2 else 0)
    if k == 3:  # gateway set and known
        return (PM.V_OVERRIDE, nif, 8080, ip)
    if k == 4:  # gateway 0: direct ARP of dst
        return (PM.V_OVERRIDE, nif, 8081, 0)
    if k == 5:  # gateway set and absent
        return (PM.V_OVERRIDE, nif, 8082, K.absent(keys, nif, i))
    if k == 6:  # a NetIf the table does not have
        return (PM.V_OVERRIDE, [3, 64, 255][(i // 12) % 3], 8083, ip)
    if k == 8:  # the gateway is the out NetIf's own address
        return (PM.V_OVERRIDE, nif, 8084, K.NETIFS[nif].ip)
    return (PM.V_OVERRIDE, nif, 8086 + k, ip if k == 10 else 0)


@pytest.mark.parametrize("n", SIZES)
def test_encap_via_matches_restatement(dev, arp_world, n):
    import torch

    from halo_amd._lib import ARP_RESULT_DTYPE, PMFLOW_VIA_DTYPE

    pair, keys, rt = arp_world
    rng = np.random.default_rng(1500 + n)
    frames, dsts, select, forced, names = K.mixed_batch(rng, keys, n)
    data, offs, lens = K.pack(rng, frames)
    rids = rt.FindRoute(torch.from_numpy(dsts.view(np.int32)).to(dev)).cpu().numpy().view(np.uint32).copy()
    for i, frc in enumerate(forced):
        if frc is not None:
            rids[i] = frc
    via = np.zeros(n, PMFLOW_VIA_DTYPE)
    for i in range(n):
        via[i] = _via_for(rng, keys, i, names[i], int(dsts[i]))
    d_rids, d_sel, d_via = _t(dev, rids.view(np.int32)), _t(dev, select), _t(dev, via.view(np.uint8).reshape(-1, 8))
    seen = set()
    for in_netif in (0, 1):  # NetIf 0 does not NAT (LOOPBACK), NetIf 1 does
        want, want_res = data.copy(), np.zeros(n, ARP_RESULT_DTYPE)
        for i, f in enumerate(frames):
            v, out, tx, target, after = PM.encap_via(pair.m, f, K.route_of(rt, int(rids[i])), tuple(int(x) for x in via[i]),
                                                     in_netif, bool(select[i]))
            want_res[i] = (v, out, tx, target)
            want[4 * int(offs[i]):4 * int(offs[i]) + len(f)] = np.frombuffer(after, np.uint8)
            if via[i]["verdict"] == PM.V_OVERRIDE:
                seen.add((names[i], i % 12, v))
        d, o, ln = _up(dev, data, offs, lens)
        counts = torch.full((7,), 3, dtype=torch.int32, device=dev)
        miss = torch.full((1,), 5, dtype=torch.int32, device=dev)
        res, counts, miss = pair.t.encap_via(d, o, ln, d_rids, in_netif, d_via, select=d_sel, counts=counts, miss_count=miss)
        torch.cuda.synchronize()
        got_res = res.cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE)
        bad = np.nonzero(got_res != want_res)[0]
        assert bad.size == 0, [(int(i), names[i], via[i], got_res[i], want_res[i]) for i in bad[:5]]
        got = d.cpu().numpy()
        assert np.array_equal(got, want)
        # the whole buffer equals the input except bytes 0-11 of HIT frames
        hit_bytes = set()
        for i in np.nonzero(want_res["verdict"] == AM.HIT)[0]:
            hit_bytes.update(range(4 * int(offs[i]), 4 * int(offs[i]) + 12))
        assert set(np.nonzero(got != data)[0].tolist()) <= hit_bytes
        assert list(counts.cpu().numpy() - 3) == [int((want_res["verdict"] == v).sum()) for v in range(7)]
        assert int(miss.cpu()[0]) - 5 == int((want_res["verdict"] == AM.MISS).sum())
    if n >= 255:
        got_v = {(k, v) for _, k, v in seen}
        for case in ((3, AM.HIT), (4, AM.HIT), (4, AM.MISS), (5, AM.MISS), (6, AM.NONE), (8, AM.OWN_IP)):
            assert case in got_v, case
        assert {v for nm, _, v in seen if nm == "own_dst"} >= {AM.LOOPBACK, AM.OWN_IP}  # after the override
        # an OVERRIDE on a no-route, a panicking and an unknown route id still resolves
        for name in ("no_route", "panic", "bad_route_id", "bad_netif"):
            assert any(nm == name and v in (AM.HIT, AM.MISS, AM.OWN_IP) for nm, _, v in seen), name


@pytest.mark.parametrize("n", [257, 1000])
def test_encap_via_without_via_equals_encap(dev, arp_world, n):
    import torch

    pair, keys, rt = arp_world
    rng = np.random.default_rng(2500 + n)
    frames, dsts, select, forced, names = K.mixed_batch(rng, keys, n)
    data, offs, lens = K.pack(rng, frames)
    rids = rt.FindRoute(torch.from_numpy(dsts.view(np.int32)).to(dev)).cpu().numpy().view(np.uint32).copy()
    for i, frc in enumerate(forced):
        if frc is not None:
            rids[i] = frc
    d_rids, d_sel = _t(dev, rids.view(np.int32)), _t(dev, select)
    for in_netif in (0, 1):
        outs = []
        for call in ("encap", "via_null", "via_no_override"):
            d, o, ln = _up(dev, data, offs, lens)
            if call == "encap":
                res, counts, miss = pair.t.encap(d, o, ln, d_rids, in_netif, select=d_sel)
            else:  # NULL, and a via array without one OVERRIDE (the via kernel itself)
                d_via = None if call == "via_null" else torch.zeros((n, 8), dtype=torch.uint8, device=dev)
                if d_via is not None:
                    d_via[:, 0] = torch.arange(n, device=dev).to(torch.uint8) % 3  # NONE, MISS, HIT
                    d_via[:, 1:] = 0x5A  # ignored fields
                res, counts, miss = pair.t.encap_via(d, o, ln, d_rids, in_netif, d_via, select=d_sel)
            torch.cuda.synchronize()
            outs.append((res.cpu().numpy().tobytes(), d.cpu().numpy().tobytes(), counts.cpu().numpy().tobytes(),
                         int(miss.cpu()[0])))
        assert outs[0] == outs[1] == outs[2]


def test_drop_then_egress_leaves_the_frame_out(dev, arp_world):
    import torch

    from halo_amd import PortMappingFlowTable, egress_arp
    from halo_amd._lib import ARP_RESULT_DTYPE

    pair, keys, rt = arp_world
    n = 300
    rng = np.random.default_rng(77)
    frames = [K.ipv4_frame(rng, 60 + i % 9, keys[i % len(keys)][1]) for i in range(n)]
    data, offs, lens = K.pack(rng, frames)
    dsts = np.array([keys[i % len(keys)][1] for i in range(n)], np.uint32)
    d, o, ln = _up(dev, data, offs, lens)
    d_rids = rt.FindRoute(_t(dev, dsts.view(np.int32)))
    res, _, _ = pair.t.encap(d, o, ln, d_rids, 0)
    before = res.cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE).copy()
    assert (before["verdict"] == AM.HIT).all()
    drop = np.array([0, 63, 64, 255, 256, 299], np.int32)
    tail = torch.full((4, 8), FILL, dtype=torch.uint8, device=dev)
    both = torch.cat([res, tail])  # the edit touches the listed results only
    PortMappingFlowTable.drop(both, _t(dev, drop))
    PortMappingFlowTable.drop(both, torch.zeros(0, dtype=torch.int32, device=dev))  # k == 0 is OK
    eg = egress_arp(d, o, ln, both[:n], 3, 64 * 1024, index_cap=n)
    torch.cuda.synchronize()
    after = both.cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE)
    want = before.copy()
    want[drop] = (AM.NONE, 0xFF, 0, 0)
    assert np.array_equal(after[:n], want) and (both[n:].cpu().numpy() == FILL).all()
    sent = np.concatenate([eg.index(p) for p in range(3)])
    assert sorted(sent.tolist()) == sorted(set(range(n)) - set(drop.tolist()))
    assert int(eg.ports["frames"].sum()) == n - len(drop) and eg.n_skipped == 0
    # bytes 0-11 of a dropped frame were already rewritten and stay so
    got = d.cpu().numpy()
    k = int(drop[1])
    assert bytes(got[4 * int(offs[k]):4 * int(offs[k]) + 12]) != frames[k][:12]


# ---- the chain on a dual-WAN router ----------------------------------------------------------------
class _Router:
    """LAN, WAN1 (the default route), WAN2 (a port mapping to the LAN server), and the server's
    return route preferring WAN1."""

    def __init__(self, dev, pm_capacity=64):
        from halo_amd import ArpTable, NatTable, PortMappingFlowTable
        from halo_amd.route import RouteTable

        self.dev = dev
        self.netifs = C.lib_netifs()[:3]
        self.rt = RouteTable(0)
        for q in range(3):
            self.rt.AddRoute(RouteTable.entry(C.IPS[q] & 0xFFFFFF00, 0xFFFFFF00, 0, q))
        self.rt.AddRoute(RouteTable.entry(0, 0, C.GATEWAYS[C.WAN1], C.WAN1))
        self.rt.sync()
        self.arp = ArpTable(self.netifs, 16)
        self.arp_m = AM.Model(C.model_netifs()[:3], 16)
        for nif, ip, mac in ((C.LAN, C.SERVER, C.SERVER_MAC), (C.WAN1, C.GATEWAYS[C.WAN1], C.GW_MAC[C.WAN1]),
                             (C.WAN2, C.GATEWAYS[C.WAN2], C.GW_MAC[C.WAN2])):
            self.arp.SetArpCache(nif, ip, mac, 10)
            self.arp_m.set(nif, ip, mac, 10)
        self.arp.sync(self.rt)
        self.nat = {q: NatTable(C.IPS[q]) for q in (C.WAN1, C.WAN2)}
        self.maps = [(8080, C.SERVER, 80, 6), (5353, C.SERVER, 53, 17)]
        for m in self.maps:
            self.nat[C.WAN2].add_port_mapping(*m)
        for t in self.nat.values():
            t.sync()
        self.pm = PortMappingFlowTable(self.netifs, C.GATEWAYS[:3], pm_capacity)
        self.pm_m = PM.Model(C.model_netifs()[:3], C.GATEWAYS[:3], pm_capacity)
        self.pm.sync(self.rt)

    def close(self):
        for x in (self.pm, self.arp, self.rt, *self.nat.values()):
            x.close()

    def route_of(self, dst):
        """FindRoute restated for this table: the LAN / WAN subnets direct, else the default route."""
        for q in range(3):
            if dst & 0xFFFFFF00 == C.IPS[q] & 0xFFFFFF00:
                return (0, q)
        return (C.GATEWAYS[C.WAN1], C.WAN1)


def _clients(k):
    """k first packets to WAN2's mapped ports: (remote ip, remote port, mapping index)."""
    return [(0x08080000 + 3 * j + 1, 20000 + j, j % 2) for j in range(k)]


def _inbound(r, clients, now, dev):
    """A batch arrives on WAN2: parse -> lookup_wan -> route -> fixup -> encap -> record_device. Returns
    the device tensors and the items listed."""
    import torch

    from halo_amd import protocol
    from halo_amd.pmflow import items_of

    frames = []
    for rip, rport, mi in clients:
        wan_port, _lip, _lport, proto = r.maps[mi]
        frames.append(C.l4_frame(proto, rip, rport, C.IPS[C.WAN2], wan_port, C.MACS[C.WAN2]))
    data, offs, lens = C.pack(frames)
    d, o, ln = _up(dev, data, offs, lens)
    n = len(frames)
    recs = protocol.parse_frames_batch(d, o, ln, netif=r.netifs[C.WAN2])
    ops = _t(dev, protocol.tx_ops(n, TX_TTL | TX_RECALC).view(np.uint8).reshape(n, 16))
    ops, verdict, ref, miss = r.nat[C.WAN2].lookup_wan(recs, now, ops=ops)
    rids = r.rt.FindRoute(ops.view(torch.int32)[:, 1].contiguous())  # the post-DNAT destination
    res = torch.zeros(n, dtype=torch.uint8, device=dev)
    protocol.tx_fixup_batch(d, o, ln, ops.reshape(-1), result=res)
    results, _, _ = r.arp.encap(d, o, ln, rids, C.WAN2, select=res & 1)
    items, count = r.pm.record_device(C.WAN2, recs, verdict, ops, results, now)
    torch.cuda.synchronize()
    assert (verdict.cpu().numpy() == NAT_V_MAPPING).all()
    return frames, (d, o, ln), results, items_of(items, count)


def _want_items(r, clients):
    out = []
    for rip, rport, mi in clients:
        wan_port, lip, lport, proto = r.maps[mi]
        out.append((rip, rport, lip, lport, proto, wan_port))
    return out


def _replies(r, clients):
    frames = []
    for rip, rport, mi in clients:
        _wan_port, lip, lport, proto = r.maps[mi]
        frames.append(C.l4_frame(proto, lip, lport, rip, rport, C.MACS[C.LAN], payload=b"reply-%d" % rport))
    return frames


def _want_streams(r, frames, now, stamp=True):
    """The model's egress of the server's replies: per NetIf, the ring records in frame order."""
    streams = {q: b"" for q in range(3)}
    for f in frames:
        tup = PM.five_tuple(f, C.MACS[C.LAN], C.IPS[C.LAN])
        route = r.route_of(tup[2])
        v, wan, port, hop, snat = r.pm_m.lookup(tup, route, now, stamp=stamp)
        steps = TX_TTL | TX_RECALC | (TX_NAT_SRC if snat else 0)
        after, res = PM.snat_frame(f, steps, *(snat or (0, 0)))
        via = (v, wan, port, hop)
        verdict, out, tx, target, sent = PM.encap_via(r.arp_m, after, route, via, C.LAN, bool(res & 1))
        if verdict == AM.HIT:
            body = sent + bytes(tx - len(sent))
            streams[out] += tx.to_bytes(4, "little") + body + bytes(-(4 + tx) % 4)
    return streams


def _host_lookup(r, recs_np, rids, now):
    """What halo_pmflow_lookup_device replaces: halo_pmflow_get per record on the host, giving the
    same ops / via / hit."""
    from halo_amd._lib import PMFLOW_VIA_DTYPE, TX_OP_DTYPE

    n = len(recs_np)
    ops = np.zeros(n, TX_OP_DTYPE)
    ops["steps"] = TX_TTL | TX_RECALC
    via, hit = np.zeros(n, PMFLOW_VIA_DTYPE), np.zeros(n, np.uint8)
    for i, rec in enumerate(recs_np):
        via[i] = (PM.V_NONE if rec["ip_proto"] == 0xFF else PM.V_MISS, 0xFF, 0, 0)
        if rec["ip_proto"] not in (6, 17):
            continue
        e = r.pm.get(int(rec["dst_ip"]), int(rec["dport"]), int(rec["src_ip"]), int(rec["sport"]), int(rec["ip_proto"]), now=now)
        if e is None:
            continue
        wan = int(e["wan_netif"])
        rid = int(rids[i])
        same = rid == AM.ROUTE_PANIC_ID or (rid != AM.ROUTE_NONE and int(r.rt.get(rid)[0]["netif"]) == wan)
        via[i] = (PM.V_HIT if same else PM.V_OVERRIDE, wan, int(e["wan_port"]), C.GATEWAYS[wan])
        hit[i] = 1
        if C.NAT[wan]:
            ops[i]["steps"] |= TX_NAT_SRC
            ops[i]["src_ip"], ops[i]["src_port"] = C.IPS[wan], int(e["wan_port"])
    return ops, via, hit


def _egress(r, d, o, ln, results):
    from halo_amd import egress_arp

    eg = egress_arp(d, o, ln, results, 3, 64 * 1024, index_cap=int(ln.shape[0]))
    return {q: eg.stream(q).tobytes() for q in range(3)}, eg


def test_chain_returns_through_the_wan_it_came_in_on(dev):
    import torch

    from halo_amd import forward_return_flows, protocol

    r = _Router(dev)
    try:
        clients = _clients(40)
        now = 500
        # ---- first packets arrive on WAN2 ----
        frames_in, (d, o, ln), results, items = _inbound(r, clients, now, dev)
        want = _want_items(r, clients)
        assert items.tobytes() == C.item_array(want).tobytes()  # none known yet: all listed, in frame order
        dropped, added = r.pm.record(C.WAN2, items, now)
        assert added == 40 and not dropped.any() and r.pm_m.record(C.WAN2, want, now) == ([0] * 40, 40)
        streams, _ = _egress(r, d, o, ln, results)
        assert streams[C.WAN1] == streams[C.WAN2] == b"" and streams[C.LAN].count(C.SERVER_MAC + C.MACS[C.LAN]) == 40
        # ---- the server's replies, before the sync: the device misses, halo_pmflow_get answers ----
        replies = _replies(r, clients)
        data, offs, lens = C.pack(replies)
        now = 503
        want_streams = _want_streams(r, replies, now)
        assert want_streams[C.WAN1] == b"" and want_streams[C.LAN] == b"" and len(want_streams[C.WAN2]) > 40 * 64
        d, o, ln = _up(dev, data, offs, lens)
        assert r.pm.dirty
        pre = forward_return_flows(d, o, ln, netif=r.netifs[C.LAN], in_netif=C.LAN, now=now, pmflow=r.pm, routes=r.rt,
                                   arp=r.arp, nat=r.nat[C.WAN1], steps=TX_TTL | TX_RECALC)
        torch.cuda.synchronize()
        assert list(pre.pm_counts.cpu().numpy()) == [0, 40, 0, 0]  # all MISS: recorded since the last sync
        d, o, ln = _up(dev, data, offs, lens)
        recs = protocol.parse_frames_batch(d, o, ln, netif=r.netifs[C.LAN])
        rids = r.rt.FindRouteRecords(recs)
        h_ops, h_via, h_hit = _host_lookup(r, protocol.records(recs), rids.cpu().numpy().view(np.uint32), now)
        assert (h_via["verdict"] == PM.V_OVERRIDE).all() and h_hit.all()
        ops = _t(dev, h_ops.view(np.uint8).reshape(-1, 16))
        ops, nv, _, nmiss = r.nat[C.WAN1].lookup_lan(recs, now, ops=ops, skip=_t(dev, h_hit))
        res = torch.zeros(40, dtype=torch.uint8, device=dev)
        protocol.tx_fixup_batch(d, o, ln, ops.reshape(-1), result=res)
        results, _, _ = r.arp.encap_via(d, o, ln, rids, C.LAN, _t(dev, h_via.view(np.uint8).reshape(-1, 8)), select=res & 1)
        host_streams, _ = _egress(r, d, o, ln, results)
        assert int(nmiss.cpu()[0]) == 0 and (nv.cpu().numpy() == 1).all()  # HALO_NAT_V_SKIP: left alone (:205-207)
        assert host_streams == want_streams
        # ---- sync, then the same replies through the device lookup: identical ----
        r.pm.sync(r.rt)
        assert not r.pm.dirty
        now = 506
        want_streams2 = _want_streams(r, replies, now)
        assert want_streams2 == want_streams
        d, o, ln = _up(dev, data, offs, lens)
        out = forward_return_flows(d, o, ln, netif=r.netifs[C.LAN], in_netif=C.LAN, now=now, pmflow=r.pm, routes=r.rt,
                                   arp=r.arp, nat=r.nat[C.WAN1], steps=TX_TTL | TX_RECALC)
        dev_streams, eg = _egress(r, d, o, ln, out.results)
        assert list(out.pm_counts.cpu().numpy()) == [0, 0, 0, 40]
        assert dev_streams == want_streams and eg.ports["frames"].tolist() == [0, 0, 40]
        # device == host: the lookup's outputs equal the host restatement's
        assert out.via.cpu().numpy().tobytes() == h_via.tobytes() and out.hit.cpu().numpy().tobytes() == h_hit.tobytes()
        assert out.ops.cpu().numpy().tobytes() == h_ops.tobytes()
        first = want_streams[C.WAN2][4:4 + 64]
        assert first[:6] == C.GW_MAC[C.WAN2] and first[6:12] == C.MACS[C.WAN2]
        assert first[26:30] == C.IPS[C.WAN2].to_bytes(4, "big") and first[34:36] == (8080).to_bytes(2, "big")
        # the stamps of both paths, and a second batch of the same clients: known-identical, only stamped
        assert r.pm.TableClear(now) == 0 == r.pm_m.expire(now)
        assert C.listing_of(r.pm.List()) == r.pm_m.listing()
        _, _, _, items2 = _inbound(r, clients, 520, dev)
        assert len(items2) == 0
        for f in r.pm_m.flows.values():
            f[2] = 520
        assert r.pm.TableClear(520 + 60) == 0 and C.listing_of(r.pm.List()) == r.pm_m.listing()
        assert r.pm.TableClear(520 + 61) == 40 and len(r.pm.List()) == 0
    finally:
        r.close()


def test_chain_with_the_table_full_drops_the_first_packets(dev):
    import torch

    r = _Router(dev, pm_capacity=2)
    try:
        clients = _clients(5)
        frames_in, (d, o, ln), results, items = _inbound(r, clients, 700, dev)
        assert len(items) == 5
        dropped, added = r.pm.record(C.WAN2, items, 700)
        assert list(dropped) == [0, 0, 1, 1, 1] and added == 2
        idx = items["index"][dropped == 1].astype(np.int32)
        r.pm.drop(results, _t(dev, idx))
        streams, eg = _egress(r, d, o, ln, results)
        torch.cuda.synchronize()
        assert eg.index(C.LAN).tolist() == [0, 1] and eg.ports["frames"].tolist() == [2, 0, 0]
        listed = C.listing_of(r.pm.List())
        assert [x[1:3] for x in listed] == [(c[0], c[1]) for c in clients[:2]]  # the dropped ones are recorded nowhere
        # their replies take the route's WAN and its own NAT: no return flow exists
        assert r.pm.get(clients[3][0], clients[3][1], C.SERVER, 80, 6) is None
    finally:
        r.close()
