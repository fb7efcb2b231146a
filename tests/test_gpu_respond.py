"""GPU: the local responders on the device (halo_amd/csrc/tx_respond.hip through
halo_amd.respond) against tests/respond_model.py, which works from frame bytes — descriptors,
sources, destination addresses, count, kind counts and actions bit for bit, each output with its
sentinel — at the batch sizes around a wavefront and a tile, with no reply, replies at both sides
of a wave and a tile boundary, the crafted mix and a reply for every frame; `cap` below the count
and one workspace used for two calls; past the tile and the scan pass (tests/respond_cases.py);
device == host; TxIpv4's route / ARP step (ArpTable.encap_tx) against its restatement over the
forced 16-slot table; and one chain from parse to the egress streams."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import ref_py as R
from tests import arp_cases as K
from tests import arp_model as M
from tests import respond_cases as C
from tests import respond_model as RM

pytestmark = pytest.mark.gpu
FILL = C.FILL


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


def _device(dev, recs, offs, lens, nat_enable, *, nat=None, steps=None, result=None, ports=None, cap=None, l3=False,
            kc0=9, ws=None):
    """halo_tx_respond_device into 0xA5-filled device outputs, straight through ctypes: the raw
    arrays downloaded, as tests/respond_cases.check_outputs takes them. `recs` is the cuda record
    tensor, `offs` / `lens` numpy."""
    import torch

    from halo_amd import _lib
    from halo_amd.respond import tcp_port_map

    n = len(lens)
    cap = n if cap is None else cap
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=dev)  # noqa: E731
    a5 = int(np.array(0xA5A5A5A5, np.uint32).view(np.int32))
    desc, src = full((cap + 2, 40), FILL, torch.uint8), full((cap + 2, 8), FILL, torch.uint8)
    dst_ip, count = full((cap + 2,), a5, torch.int32), full((2,), a5, torch.int32)
    kinds, actions = full((5,), kc0, torch.int32), full((n + 2,), FILL, torch.uint8)
    d_offs, d_lens = _t(dev, offs, np.int32), _t(dev, lens, np.int16)
    d_nat = None if nat is None else _t(dev, nat)
    d_ops = None if steps is None else _t(dev, C.ops_array(steps).view(np.uint8).reshape(-1, 16))
    d_res = None if steps is None else _t(dev, result)
    d_pm = None if ports is None else _t(dev, tcp_port_map(ports), np.int32)
    wsb = int(_lib.lib.halo_tx_respond_workspace(n))
    if ws is None:
        ws = full((wsb // 4 + 1,), a5, torch.int32)
    rc = _lib.lib.halo_tx_respond_device(
        _lib.ptr(d_offs), _lib.ptr(d_lens), _lib.ptr(recs), n, _lib.HALO_RX_L3_START if l3 else 0, C.lib_netif(nat_enable),
        _lib.ptr(d_nat), _lib.ptr(d_ops), _lib.ptr(d_res), _lib.ptr(d_pm), _lib.ptr(desc), _lib.ptr(src), _lib.ptr(dst_ip), cap,
        _lib.ptr(count), _lib.ptr(kinds), _lib.ptr(actions), _lib.ptr(ws), wsb, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    h = lambda x, dt=None: x.cpu().numpy() if dt is None else x.cpu().numpy().view(dt)  # noqa: E731
    o = dict(desc=h(desc), src=h(src), dst_ip=h(dst_ip, np.uint32), count=h(count, np.uint32), kinds=h(kinds, np.uint32),
             actions=h(actions), cap=cap, n=n, kc0=kc0)
    assert int(h(ws, np.uint32)[wsb // 4]) == 0xA5A5A5A5, "the workspace was overrun"
    return o


def _host(recs_h, offs, lens, nat_enable, *, nat=None, steps=None, result=None, ports=None, cap=None, l3=False):
    from halo_amd.respond import respond_host, tcp_port_map

    ops = None if steps is None else C.ops_array(steps)
    pm = None if ports is None else tcp_port_map(ports)
    return respond_host(offs, lens, recs_h, netif=C.lib_netif(nat_enable), nat_verdict=nat, ops=ops, fixup_result=result,
                        tcp_ports=pm, cap=cap, l3_start=l3)


def _same_as_host(o, r):
    w = min(int(o["count"][0]), o["cap"])
    assert r.count == int(o["count"][0])
    assert np.array_equal(r.desc_raw[:w], o["desc"][:w]) and np.array_equal(r.src_raw[:w], o["src"][:w])
    assert np.array_equal(r.dst_ip_raw[:w], o["dst_ip"][:w]) and np.array_equal(r.actions, o["actions"][:o["n"]])
    assert np.array_equal(r.kind_counts, o["kinds"][:4] - o["kc0"])


@pytest.mark.parametrize("density", ["none", "sparse", "mixed", "all"])
@pytest.mark.parametrize("n", C.SIZES)
def test_respond_matches_model(dev, n, density):
    from halo_amd import protocol

    cases = C.batch(900 + n, n, density)
    frames, nat, steps, result = C.columns(cases)
    data, offs, lens = C.pack(n, frames)
    seen = set()
    for nat_enable in (False, True):
        recs = protocol.parse_frames_batch(_t(dev, data), _t(dev, offs, np.int32), _t(dev, lens, np.int16),
                                           netif=C.lib_netif(nat_enable))
        want = RM.respond(frames, offs, C.model_netif(nat_enable), nat=nat, fix=(steps, result), tcp_ports=C.SERVED)
        kw = dict(nat=nat, steps=steps, result=result, ports=C.SERVED)
        o = _device(dev, recs, offs, lens, nat_enable, **kw)
        C.check_outputs(o, want, f"{n} {density} nat_enable={nat_enable}")
        _same_as_host(o, _host(protocol.records(recs), offs, lens, nat_enable, **kw))
        seen |= {(nat_enable, r["kind"]) for _, r in want.replies}
        if want.count > 1:  # a cap below the count: the tail stays as it was, the count is the total
            cap = want.count // 2
            C.check_outputs(_device(dev, recs, offs, lens, nat_enable, cap=cap, **kw), want, f"cap {cap}")
    if density == "none":
        assert not seen
    if density == "all":
        assert want.count == 0 and (False, RM.ECHO) in seen  # a NATing NetIf forwards them; FLOW, so no answer
    if density == "mixed" and n >= 255:
        assert seen >= {(False, k) for k in range(4)} | {(True, RM.ECHO), (True, RM.TTL)}
    if density == "sparse" and n >= 257:
        idx = [i for i, _ in RM.respond(frames, offs, C.model_netif(), nat=nat, fix=(steps, result), tcp_ports=C.SERVED).replies]
        assert idx == sorted({0, 63, 64, 255, 256, n - 1})  # both sides of a wave and of a tile boundary


def test_absent_inputs_and_one_workspace_for_two_calls(dev):
    import torch

    from halo_amd import _lib, protocol

    n = 700
    frames, nat, steps, result = C.columns(C.batch(5, n, "mixed"))
    data, offs, lens = C.pack(6, frames)
    recs = protocol.parse_frames_batch(_t(dev, data), _t(dev, offs, np.int32), _t(dev, lens, np.int16), netif=C.lib_netif())
    ws = torch.full((int(_lib.lib.halo_tx_respond_workspace(n)) // 4 + 1,), -1515870811, dtype=torch.int32, device=dev)
    nif = C.model_netif()
    for given in [(True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False),
                  (True, True, True)]:
        kw = dict(nat=nat if given[0] else None, steps=steps if given[1] else None, result=result if given[1] else None,
                  ports=C.SERVED if given[2] else None)
        want = RM.respond(frames, offs, nif, nat=kw["nat"], fix=(steps, result) if given[1] else None,
                          tcp_ports=C.SERVED if given[2] else ())
        C.check_outputs(_device(dev, recs, offs, lens, False, ws=ws, **kw), want, str(given))


def test_lochan_packets(dev):
    from halo_amd import protocol
    from tests.helpers import strip_ethernet

    frames, nat, steps, result = C.columns(C.batch(8, 300, "mixed"))
    data, offs, lens = C.pack(9, frames)
    pdata, poffs, plens = strip_ethernet(data, offs, lens)
    pkts = [bytes(pdata[4 * int(o):4 * int(o) + int(ln)]) for o, ln in zip(poffs, plens)]
    recs = protocol.parse_ipv4_packets_batch(_t(dev, pdata), _t(dev, poffs, np.int32), _t(dev, plens, np.int16),
                                             netif=C.lib_netif())
    want = RM.respond(pkts, poffs, C.model_netif(True), nat=nat, fix=(steps, result), tcp_ports=C.SERVED, l3=True)
    o = _device(dev, recs, poffs, plens, True, nat=nat, steps=steps, result=result, ports=C.SERVED, l3=True)
    C.check_outputs(o, want, "lo")
    assert want.kind_counts[RM.TTL] == 0 and want.kind_counts[RM.ECHO] > 0 and want.kind_counts[RM.TCP_SYN] > 0


@pytest.mark.parametrize("edge", sorted(C.BOUNDARIES))
def test_past_each_edge(dev, edge):
    """past(edge) + r uniform frames with replies on both sides of the edge, of the edge before it
    and at the ends; the model's vectorised path; device == host."""
    from halo_amd import protocol
    from halo_amd._lib import BUILD_DESC_DTYPE, RESPOND_SRC_DTYPE

    n = C.past(edge, 131)
    e = C.BOUNDARIES[edge]["first_past"] - 1
    at = sorted({0, 63, 64, 255, 256, e - 1, e, e + 1, e + 64, n - 1})
    templates, tid, data, offs, lens = C.uniform_batch(n, at)
    recs = protocol.parse_frames_batch(_t(dev, data), _t(dev, offs, np.int32), _t(dev, lens, np.int16), netif=C.lib_netif(),
                                       max_len_hint=64)
    fields, index, kind, kind_counts, actions = RM.respond_uniform(templates, tid, offs, C.model_netif())
    assert index.tolist() == at
    o = _device(dev, recs, offs, lens, False)
    w = len(at)
    got = o["desc"].reshape(-1).view(BUILD_DESC_DTYPE)
    for f in RM.DESC_FIELDS:
        assert np.array_equal(got[f][:w].astype(np.uint64), fields[f]), f
    assert not got["dst_mac"][:w].any() and not got["mode"][:w].any() and not got["pad"][:w].any()
    s = o["src"].reshape(-1).view(RESPOND_SRC_DTYPE)
    assert np.array_equal(s["index"][:w], index) and np.array_equal(s["kind"][:w], kind) and not s["pad"][:w].any()
    assert np.array_equal(o["dst_ip"][:w].astype(np.uint64), fields["dst_ip"])
    assert int(o["count"][0]) == w and int(o["count"][1]) == 0xA5A5A5A5
    assert np.all(o["desc"][w:] == FILL) and np.all(o["src"][w:] == FILL) and np.all(o["dst_ip"][w:] == 0xA5A5A5A5)
    assert np.array_equal(o["kinds"][:4] - o["kc0"], kind_counts) and int(o["kinds"][4]) == o["kc0"]
    assert np.array_equal(o["actions"][:n], actions) and np.all(o["actions"][n:] == FILL)
    _same_as_host(o, _host(protocol.records(recs), offs, lens, False))


# ---- TxIpv4's route / ARP step ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(dev):
    """tests/test_arp_table.py's forced 16-slot table, synced with the route table that has direct
    and next-hop routes, an emptied list and an ECMP list."""
    pair, keys = K.forced_table(lambda **kw: K.Pair(**kw))
    rt = K.world_routes(keys)
    rt.sync()
    pair.t.sync(rt)
    yield pair, keys, rt
    pair.close()
    rt.close()


def _tx_batch(rng, keys, n):
    """The mixed batch of the forward encap's test with broadcast destinations put in: frames as
    TxIpv4 would hold them after BuildIpv4Pkt."""
    frames, dsts, select, forced, names = K.mixed_batch(rng, keys, n)
    frames, dsts, names = list(frames), dsts.copy(), list(names)
    for i in range(5, n, 11):  # x.x.x.255 on frames of every case, short and unselected ones included
        dsts[i] = (int(dsts[i]) & 0xFFFFFF00) | 0xFF
        f = bytearray(frames[i])
        if len(f) >= 34:
            f[30:34] = M.ip_bytes(int(dsts[i]))
        frames[i] = bytes(f)
        names[i] += "+bcast"
    return frames, dsts, select, forced, names


@pytest.mark.parametrize("n", C.SIZES)
def test_encap_tx_matches_model(dev, world, n):
    import torch

    from halo_amd._lib import ARP_RESULT_DTYPE

    pair, keys, rt = world
    rng = np.random.default_rng(1500 + n)
    frames, dsts, select, forced, names = _tx_batch(rng, keys, n)
    data, offs, lens = K.pack(rng, frames)
    rids = rt.FindRoute(_t(dev, dsts, np.int32)).cpu().numpy().view(np.uint32).copy()
    for i, frc in enumerate(forced):
        if frc is not None:
            rids[i] = frc
    seen = set()
    for self_netif in (0, 1):  # NetIf 1 NATs: a LOOPBACK all the same
        want, want_res = data.copy(), np.zeros(n, ARP_RESULT_DTYPE)
        for i, f in enumerate(frames):
            v, out, tx, target, after = RM.tx_ipv4(pair.m, f, K.route_of(rt, int(rids[i])), self_netif, bool(select[i]))
            want_res[i] = (v, out, tx, target)
            want[4 * int(offs[i]):4 * int(offs[i]) + len(f)] = np.frombuffer(after, np.uint8)
            seen.add((names[i], v, self_netif))
        d = _t(dev, data)
        counts = torch.full((7,), 3, dtype=torch.int32, device=dev)
        miss = torch.full((1,), 5, dtype=torch.int32, device=dev)
        res, counts, miss = pair.t.encap_tx(d, _t(dev, offs, np.int32), _t(dev, lens, np.int16), _t(dev, rids, np.int32),
                                            self_netif, select=_t(dev, select), counts=counts, miss_count=miss)
        torch.cuda.synchronize()
        got_res = res.cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE)
        bad = np.nonzero(got_res != want_res)[0]
        assert bad.size == 0, [(int(i), names[i], got_res[i], want_res[i]) for i in bad[:5]]
        got = d.cpu().numpy()
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
        hit_bytes = set()
        for i in np.nonzero(want_res["verdict"] == M.HIT)[0]:
            hit_bytes.update(range(4 * int(offs[i]), 4 * int(offs[i]) + 12))
        assert set(np.nonzero(got != data)[0].tolist()) <= hit_bytes  # the input except bytes 0-11 of HIT frames
        assert list(counts.cpu().numpy() - 3) == [int((want_res["verdict"] == v).sum()) for v in range(7)]
        assert int(miss.cpu()[0]) - 5 == int((want_res["verdict"] == M.MISS).sum())
    if n >= 255:
        verdicts = {v for _, v, _ in seen}
        assert verdicts == set(range(7)), verdicts  # every verdict
        assert any(c.endswith("+bcast") and v == M.HIT and s == 1 for c, v, s in seen)  # the broadcast HIT
        assert {c for c, v, _ in seen if c.endswith("+bcast") and v == M.HIT} >= {"no_route+bcast", "bad_route_id+bcast"}
        assert ("own_dst", M.LOOPBACK, 1) in seen                              # on a NATing self_netif
        assert {v for c, v, _ in seen if c == "ecmp"} == {M.HIT, M.MISS}       # the ECMP list
        assert ("panic", M.ROUTE_PANIC, 0) in seen                             # the emptied list


# ---- the chain ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_netif", [0, 1])
def test_chain_parse_to_egress(dev, world, self_netif):
    """Frames a NetIf received from its neighbours, from beyond a next hop and from where no route
    leads back: parse -> WAN lookup (NetIf 1, which NATs) -> fixup (some with TTL 1) -> respond ->
    tx_build with the rx batch as payload -> route -> encap_tx -> egress_arp. NetIf 0 answers echo
    requests, dead TTLs and SYNs to its served port; NetIf 1 forwards everything: an echo request
    that misses the NAT table falls back to RxIcmp, a mapped UDP flow whose TTL dies is answered
    with the post-DNAT quote, a SYN that misses gets nothing. Every built frame equals the model's,
    *d_ip_id advances by the number built (replies that then miss ARP included), and the egress
    streams parsed as the peers say OK, for me, and ICMP type 0 / 11 or TCP flags 0x12."""
    import torch

    from halo_amd import egress_arp, protocol
    from halo_amd._lib import ARP_RESULT_DTYPE, NAT_V_FLOW, NAT_V_MISS, TX_R_TTL_ALIVE, TX_RECALC, TX_TTL
    from halo_amd.nat import NatTable
    from halo_amd.respond import build_replies, tcp_port_map

    pair, keys, rt = world
    natting = K.NETIFS[self_netif].nat_enable
    assert natting == (self_netif == 1)
    me, own = K.NETIFS[self_netif], K.lib_netifs()[self_netif]
    peers = [ip for nif, ip in keys if nif == self_netif]           # neighbours the NetIf has in its cache
    assert peers
    # where the replies go: HIT, MISS, a next hop that is a HIT, NO_ROUTE, a next hop that is a MISS
    srcs = peers[:3] + [K.absent(keys, self_netif, 2), K.NH_HIT | 9, 0x08080808, K.NH_MISS | 9]
    lan_host = K.NETIFS[2].ip & 0xFFFFFF00 | 77
    nat = NatTable(wan_ip=me.ip)
    rng = np.random.default_rng(77 + self_netif)
    frames = []
    for k in range(150):
        src_u, kind = srcs[k % len(srcs)], k % 5
        src, own_b, far = M.ip_bytes(src_u), M.ip_bytes(me.ip), M.ip_bytes(lan_host)
        if kind == 0:
            pl = rng.integers(0, 256, int(rng.integers(0, 60)), dtype=np.uint8).tobytes()
            pkt = R.build_ipv4(R.build_icmp(pl, 8, bytes([k, 1]), k), 1, src, own_b)
        elif kind in (1, 3):  # a forwarded UDP flow; kind 1 arrives with TTL 1
            dst, dport = far, 33434
            if natting:       # ... through the NAT: addressed to the WAN address and the flow's WAN port
                flow = nat.AddFlow(lan_host, src_u, 7000 + k, 33434 + k, 17, 100)
                dst, dport = own_b, int(flow["wan_port"])
            pkt = R.build_ipv4(R.build_udp(b"probe" * (k % 7), 33434 + k, dport, src, dst), 17, src, dst,
                               ttl=1 if kind == 1 else 9)
        else:  # a SYN to the served port (wrapping ack) / to an unserved one
            seq = (0xFFFFFFF0 + k) & 0xFFFFFFFF
            pkt = R.build_ipv4(R.build_tcp(b"", 40000 + k, 80 if kind == 2 else 81, src, own_b, seq, 0, 0x02), 6, src, own_b)
        frames.append(R.build_eth(pkt, me.mac, K.mac(900 + k % 7), 0x0800))
    data, offs, lens = K.pack(rng, frames)
    d, o, ln = _t(dev, data), _t(dev, offs, np.int32), _t(dev, lens, np.int16)
    n = len(frames)
    recs = protocol.parse_frames_batch(d, o, ln, netif=own)
    kinds_of = np.arange(n) % 5
    d_verdict, verdict_h = None, None
    if natting:  # the DNAT operands come from the lookup; a packet that missed never reaches the TTL step
        nat.sync()
        d_ops, d_verdict, _ref, _miss = nat.lookup_wan(recs, 100)
        d_ops[:, 0] |= torch.where(d_verdict == NAT_V_FLOW, TX_TTL | TX_RECALC, 0).to(torch.uint8)
        torch.cuda.synchronize()
        verdict_h = d_verdict.cpu().numpy()
        assert np.array_equal(verdict_h, np.where((kinds_of == 1) | (kinds_of == 3), NAT_V_FLOW, NAT_V_MISS))
    else:
        d_ops = _t(dev, protocol.tx_ops(n, TX_TTL | TX_RECALC).view(np.uint8).reshape(-1, 16))
    d_res = torch.empty(n, dtype=torch.uint8, device=dev)
    protocol.tx_fixup_batch(d, o, ln, d_ops, result=d_res)
    builder = protocol.TxBuilder(n, ip_id=0xFFE0)
    rep = build_replies(d, o, ln, recs, netif=own, self_netif=self_netif, builder=builder, routes=rt, arp=pair.t,
                        nat_verdict=d_verdict, ops=d_ops, fixup_result=d_res, tcp_ports=_t(dev, tcp_port_map([80]), np.int32),
                        out_stride=128)
    torch.cuda.synchronize()
    after = d.cpu().numpy()
    res_h, steps_h = d_res.cpu().numpy(), d_ops.cpu().numpy()[:, 0].copy()
    mnif = RM.NetIf(me.mac, me.ip, natting)
    want = RM.respond([bytes(after[4 * int(a):4 * int(a) + int(b)]) for a, b in zip(offs, lens)], offs, mnif, nat=verdict_h,
                      fix=(steps_h, res_h), tcp_ports=(80,))
    # the fixup's verdict is the bytes': TTL 1 died, and the quote is the post-DNAT packet
    dead = [i for i in range(n) if steps_h[i] & TX_TTL and not res_h[i] & TX_R_TTL_ALIVE]
    assert dead == [i for i in range(n) if i % 5 == 1]
    if natting:
        i = dead[0]
        assert bytes(after[4 * int(offs[i]) + 30:4 * int(offs[i]) + 34]) == M.ip_bytes(lan_host)
    n_replies = 60 if natting else 90  # echo and TTL; and the served SYNs where they are local
    assert want.count == n_replies and rep.respond.count == want.count
    assert want.kind_counts.tolist() == [30, 30, 0 if natting else 30, 0]
    assert np.array_equal(rep.respond.kind_counts, want.kind_counts)
    built, ip_end = RM.build_frames(want.replies, after, me.mac, 0xFFE0)
    assert all(res == 0 for res, _ in built) and builder.iph_id == ip_end == (0xFFE0 + n_replies) & 0xFFFF
    got_frames, got_lens = rep.frames.cpu().numpy(), rep.lens.cpu().numpy().view(np.uint16)
    got_res = rep.results.cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE)
    rids = rep.route_ids.cpu().numpy().view(np.uint32)
    verdicts = []
    for k, (res, f) in enumerate(built):
        v, out, tx, target, f2 = RM.tx_ipv4(pair.m, bytes(f), K.route_of(rt, int(rids[k])), self_netif)
        assert int(got_lens[k]) == len(f) and bytes(got_frames[k, :len(f)]) == f2, k
        assert tuple(got_res[k]) == (v, out, tx, target), (k, got_res[k], (v, out, tx, target))
        verdicts.append(v)
    assert np.all(got_lens[n_replies:] == 0) and np.all(got_res["verdict"][n_replies:] == M.NONE)
    assert {M.HIT, M.MISS, M.NO_ROUTE} <= set(verdicts)  # replies were dropped after they took their iphId
    # egress, and the streams as the peers see them
    eg = egress_arp(rep.frames.reshape(-1), rep.offsets_dw, rep.lens, rep.results, n_ports=3, region_bytes=1 << 16,
                    index_cap=n)
    torch.cuda.synchronize()
    seen_aux = set()
    total = 0
    for p in range(3):
        stream, idx = eg.stream(p), eg.index(p)
        pos = 0
        for k in idx:
            tx = int(stream[pos:pos + 4].view(np.uint32)[0])
            frame = bytes(stream[pos + 4:pos + 4 + tx])
            pos += (4 + tx + 3) & ~3
            assert verdicts[k] == M.HIT and int(got_res[k]["out_netif"]) == p
            r = R.rx_frame(frame, frame[0:6], M.ip_of(frame[30:34]))
            hop = pair.m.cache[(p, int(got_res[k]["target_ip"]))][0]
            assert frame[0:6] == hop and r["status"] == "OK" and r["flags"] & 1 and r["src_ip"] == me.ip, (k, r)
            assert (r["ip_proto"], r["l4_aux"]) in ((1, 0), (1, 11), (6, 0x12)), r
            seen_aux.add((r["ip_proto"], r["l4_aux"]))
            total += 1
        assert pos == len(stream)
    assert total == verdicts.count(M.HIT) and seen_aux == ({(1, 0), (1, 11)} if natting else {(1, 0), (1, 11), (6, 0x12)})
    nat.close()
