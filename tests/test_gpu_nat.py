"""GPU: the device-resident NAT flow table (halo_amd/csrc/nat_lookup.hip through
halo_amd.nat.NatTable) against the dict model of the reference semantics (tests/nat_model.py),
bit-exact on verdict, ref, the op fields a lookup owns and the miss count: the inbound and outbound
halves of Ipv4RouteForward over full and compact records, the stamps behind NatTableClear, a
device copy that is stale or being replaced, and the whole NATed chain parse -> deep NAT ->
lookup -> rewrite against the tx oracle."""
from __future__ import annotations

import numpy as np
import pytest

from tests import nat_model as M

pytestmark = pytest.mark.gpu

REMOTE = M.REMOTE
TX_TTL, TX_RECALC = M.TX_TTL, 0x08
_records, _ops = M.records, M.ops  # shared with tests/test_gpu_scale.py


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


def _pair(nat_type, tuples, log2=0, mappings=(), now=100, sync=True):
    from halo_amd.nat import NatTable

    t, m = NatTable(M.WAN_IP, nat_type, capacity_log2=log2), M.NatModel(M.WAN_IP, nat_type)
    for e in mappings:
        t.add_port_mapping(*e)
        m.add_port_mapping(*e)
    M.fill(t, m, tuples, now)
    if sync:
        t.sync()
    return t, m


MAPPINGS = [(8080, 0xC0A80010, 80, 6), (8080, 0xC0A80011, 81, 6), (5353, 0xC0A80012, 53, 17)]


@pytest.fixture(scope="module")
def tables(dev):
    """name -> (NatTable, model), synced. The models are only stamped by the tests that share them."""
    fs, fc = M.FIXTURE_SEED[M.SYMMETRIC], M.FIXTURE_SEED[M.FULL_CONE]
    return {
        "empty": _pair(M.SYMMETRIC, []),
        "one": _pair(M.FULL_CONE, M.random_tuples(1, 1)),
        "forced_sym": _pair(M.SYMMETRIC, M.random_tuples(fs, M.FIXTURE_FLOWS), M.FIXTURE_LOG2, MAPPINGS),
        "forced_cone": _pair(M.FULL_CONE, M.random_tuples(fc, M.FIXTURE_FLOWS), M.FIXTURE_LOG2),
        "5000": _pair(M.SYMMETRIC, M.random_tuples(9, 5000), 0, MAPPINGS),
    }


def _launch(dev, t, direction, recs, now, ops, skip=None, compact=False, stream=None):
    import torch

    from halo_amd._lib import compact_of

    host = compact_of(recs) if compact else recs
    d_recs = torch.from_numpy(np.ascontiguousarray(host).view(np.uint8).reshape(len(recs), -1).copy()).to(dev)
    d_ops = torch.from_numpy(ops.view(np.uint8).reshape(len(ops), 16).copy()).to(dev)
    d_skip = None if skip is None else torch.from_numpy(skip).to(dev)
    fn = t.lookup_wan if direction == M.WAN else t.lookup_lan
    return fn(d_recs, now, ops=d_ops, skip=d_skip, stream=stream), (d_recs, d_skip)


def _fetch(res):
    from halo_amd._lib import TX_OP_DTYPE

    ops, verdict, ref, miss = res[0]
    return (ops.cpu().numpy().reshape(-1).view(TX_OP_DTYPE), verdict.cpu().numpy(), ref.cpu().numpy().view(np.uint32),
            int(miss.cpu().numpy()[0]))


def _check(got, want_ops, want, what=""):
    ops, verdict, ref, miss = got
    w_verdict, w_ref, w_miss = want
    assert np.array_equal(verdict, w_verdict), (what, np.nonzero(verdict != w_verdict)[0][:8])
    assert np.array_equal(ref, w_ref), (what, np.nonzero(ref != w_ref)[0][:8])
    assert ops.tobytes() == want_ops.tobytes(), (what, np.nonzero(ops != want_ops)[0][:8])
    assert miss == w_miss, what


def _lookup(dev, t, m, direction, recs, now, skip=None, compact=False, ops_seed=3):
    import torch

    ops = _ops(len(recs), ops_seed)
    want_ops = ops.copy()
    want = m.lookup(direction, recs, now, want_ops, skip)
    res = _launch(dev, t, direction, recs, now, ops, skip, compact)
    torch.cuda.synchronize()
    got = _fetch(res)
    _check(got, want_ops, want, (direction, len(recs), compact))
    return got


@pytest.mark.parametrize("name", ["empty", "one", "forced_sym", "forced_cone", "5000"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_lookups_match_model(dev, tables, name, n):
    """WAN and LAN, full and compact records, with d_skip on some records, at wavefront and block
    tails, on every table shape."""
    t, m = tables[name]
    for direction in (M.WAN, M.LAN):
        recs = _records(m, direction, n, seed=n + direction)
        skip = (np.random.RandomState(n).randint(0, 5, n) == 0).astype(np.uint8)
        seen = set()
        for compact in (False, True):
            got = _lookup(dev, t, m, direction, recs, 200 + n, skip if n > 1 else None, compact)
            seen |= set(got[1].tolist())
        if n == 1025 and name in ("forced_sym", "5000"):
            assert seen == {M.V_NONE, M.V_SKIP, M.V_MISS, M.V_FLOW, M.V_MAPPING}
        if n == 1025 and name == "empty":
            assert M.V_FLOW not in seen and M.V_MISS in seen


def test_forced_table_is_the_colliding_layout(tables):
    for name in ("forced_sym", "forced_cone"):
        s = tables[name][0].layout_stats()
        assert s["slots"] == 16 and min(s["longest_chain"]) >= 3 and min(s["wrapped"]) >= 1


def test_wan_then_lan_compose_one_op(dev, tables):
    """A WAN lookup on the in-interface's table, then a LAN lookup on a second table over the same
    ops: both step bits, each direction's fields from its own lookup, HALO_TX_TTL kept."""
    import torch

    from halo_amd._lib import TX_OP_DTYPE

    (ta, ma), (tb, mb) = tables["forced_cone"], tables["5000"]
    n = 257
    recs = _records(ma, M.WAN, n, seed=5)
    # the same packets seen by the outbound half: make some of them flows of the second table
    out_recs = _records(mb, M.LAN, n, seed=6)
    keep = recs["ip_proto"] == 0xFF
    for f in ("ip_proto", "src_ip", "dst_ip", "sport", "dport"):
        out_recs[f][keep] = recs[f][keep]
    ops = _ops(n, 11)
    want_ops = ops.copy()
    w1 = ma.lookup(M.WAN, recs, 300, want_ops)
    w2 = mb.lookup(M.LAN, out_recs, 300, want_ops)
    r1, keep1 = _launch(dev, ta, M.WAN, recs, 300, ops)
    d_out = torch.from_numpy(out_recs.view(np.uint8).reshape(n, 32).copy()).to(dev)
    r2 = tb.lookup_lan(d_out, 300, ops=r1[0])
    torch.cuda.synchronize()
    got = r2[0].cpu().numpy().reshape(-1).view(TX_OP_DTYPE)
    assert got.tobytes() == want_ops.tobytes()
    assert np.array_equal(r1[1].cpu().numpy(), w1[0]) and np.array_equal(r2[1].cpu().numpy(), w2[0])
    both = (w1[0] >= M.V_FLOW) & (w2[0] >= M.V_FLOW)
    assert both.sum() > 10 and np.all(got["steps"][both] == (TX_TTL | M.TX_NAT_DST | M.TX_NAT_SRC))


def test_device_stamps_keep_hit_flows_alive(dev):
    """Flows added at 100 and looked up at 130: expire(161) removes exactly the flows never hit,
    and a lookup of a removed flow then misses without an explicit sync()."""
    t, m = _pair(M.SYMMETRIC, M.random_tuples(21, 40), now=100)
    flows = m.list()
    hit = flows[::2]
    from halo_amd._lib import RESULT_DTYPE

    recs = np.zeros(len(flows), RESULT_DTYPE)
    for i, f in enumerate(flows):
        recs[i]["ip_proto"], recs[i]["src_ip"], recs[i]["sport"] = f["proto"], f["remote_ip"], f["remote_port"] or 7
        recs[i]["dst_ip"], recs[i]["dport"] = f["wan_ip"], f["wan_port"]
    half = recs[::2].copy()
    got = _lookup(dev, t, m, M.WAN, half, 130)  # synchronises
    assert np.all(got[1] == M.V_FLOW)
    assert t.TableClear(161) == m.expire(161) == len(flows) - len(hit)
    assert M.sorted_flows(t.ListNat()) == M.sorted_flows(m.list())  # last_alive = 130 came from the device
    assert sorted(int(f["id"]) for f in t.ListNat()) == sorted(f["id"] for f in hit)
    got = _lookup(dev, t, m, M.WAN, recs, 162)  # no sync(): expire republished
    assert np.array_equal(got[1][::2], np.full(len(hit), M.V_FLOW)) and np.all(got[1][1::2] == M.V_MISS)
    assert got[3] == len(flows) - len(hit)


def test_stale_device_copy_is_resolved_on_the_host(dev):
    """A flow added since the last sync misses on the device, resolve_misses turns the miss into
    the model's hit, and after sync() the device hits."""
    t, m = _pair(M.FULL_CONE, M.random_tuples(31, 8), now=100)
    new = M.random_tuples(32, 3)
    M.fill(t, m, new, 105)  # host only
    from halo_amd._lib import RESULT_DTYPE

    recs = np.zeros(len(new) + 2, RESULT_DTYPE)
    for i, (lan_ip, remote_ip, lan_port, remote_port, proto) in enumerate(new):
        recs[i]["ip_proto"], recs[i]["src_ip"], recs[i]["sport"] = proto, lan_ip, lan_port
        recs[i]["dst_ip"], recs[i]["dport"] = remote_ip, remote_port
    recs[len(new):] = recs[0]                 # a brand-new flow, twice in the batch
    recs["sport"][len(new):] = 4242
    import torch

    ops = _ops(len(recs), 1)
    res = _launch(dev, t, M.LAN, recs, 110, ops)
    torch.cuda.synchronize()
    d_ops, verdict, ref, miss = _fetch(res)
    assert np.all(verdict == M.V_MISS) and miss == len(recs) and d_ops.tobytes() == ops.tobytes()
    want_ops = ops.copy()
    want = m.resolve(M.LAN, recs, verdict, 110, want_ops)
    got = t.resolve_misses(M.LAN, recs, verdict, 110, d_ops)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] == 1
    assert d_ops.tobytes() == want_ops.tobytes() and np.all(got[0] == M.V_FLOW)
    assert M.sorted_flows(t.ListNat()) == M.sorted_flows(m.list())
    t.sync()
    got = _lookup(dev, t, m, M.LAN, recs, 111)
    assert np.all(got[1] == M.V_FLOW) and got[3] == 0


def test_resync_between_two_lookups(dev):
    """sync, launch a lookup, add flows, sync again, look up again, synchronise once: each result
    is the model's at its own table state (the first launch reads the generation it was given)."""
    import torch

    t, m = _pair(M.SYMMETRIC, M.random_tuples(41, 300), now=100)
    extra = M.random_tuples(42, 300)
    m2_probe = M.NatModel(M.WAN_IP, M.SYMMETRIC)  # only to build records that will hit after the second sync
    for tup in M.random_tuples(41, 300) + extra:
        m2_probe.add_flow(*tup, 100)
    recs = _records(m2_probe, M.WAN, 1025, seed=8)
    ops1, ops2 = _ops(1025, 1), _ops(1025, 2)
    want_ops1 = ops1.copy()
    want1 = m.lookup(M.WAN, recs, 120, want_ops1)
    res1 = _launch(dev, t, M.WAN, recs, 120, ops1)
    M.fill(t, m, extra, 121)
    t.sync()
    want_ops2 = ops2.copy()
    want2 = m.lookup(M.WAN, recs, 122, want_ops2)
    res2 = _launch(dev, t, M.WAN, recs, 122, ops2)
    torch.cuda.synchronize()
    _check(_fetch(res1), want_ops1, want1, "before the second sync")
    _check(_fetch(res2), want_ops2, want2, "after the second sync")
    assert want2[2] < want1[2]  # flows of the second sync hit only in the second lookup


def test_argument_checks(dev):
    import torch

    from halo_amd import _lib
    from halo_amd.nat import NatTable

    L = _lib.lib
    b = torch.zeros(256, dtype=torch.uint8, device=dev)
    p = b.data_ptr()
    never = NatTable(M.WAN_IP, M.SYMMETRIC)
    assert L.halo_nat_lookup_wan_device(never._t, p, 1, 0, None, p, p, p, p, None) == _lib.HALO_E_INVAL
    assert L.halo_nat_lookup_quote_device(never._t, p, 1, p, None) == _lib.HALO_E_INVAL
    t, _ = _pair(M.SYMMETRIC, M.random_tuples(1, 2))
    for fn in (L.halo_nat_lookup_wan_device, L.halo_nat_lookup_lan_device, L.halo_nat_lookup_wan_compact_device,
               L.halo_nat_lookup_lan_compact_device):
        assert fn(t._t, None, 0, 0, None, p, p, p, p, None) == 0  # n = 0
        assert fn(t._t, p, 1, 0, None, None, p, p, p, None) == _lib.HALO_E_INVAL
        assert fn(t._t, p, 1, 0, None, p, None, p, p, None) == _lib.HALO_E_INVAL
        assert fn(t._t, p, 1, 0, None, p, p, None, p, None) == _lib.HALO_E_INVAL
        assert fn(t._t, p, 1, 0, None, p, p, p, None, None) == _lib.HALO_E_INVAL
        assert fn(t._t, None, 1, 0, None, p, p, p, p, None) == _lib.HALO_E_INVAL
        assert fn(t._t, p + 4, 1, 0, None, p, p, p, p, None) == _lib.HALO_E_INVAL  # misaligned records
    assert L.halo_nat_lookup_quote_device(t._t, None, 0, p, None) == 0
    assert L.halo_nat_lookup_quote_device(t._t, p, 1, None, None) == _lib.HALO_E_INVAL
    assert L.halo_nat_sync_device(t._t, 99) in (_lib.HALO_E_NODEV, _lib.HALO_E_INVAL)
    assert L.halo_nat_sync_device(None, 0) == _lib.HALO_E_INVAL
    torch.cuda.synchronize()


def _pack(frames):
    lens = np.array([len(f) for f in frames], np.uint16)
    sizes = (lens.astype(np.int64) + 3) & ~3
    offs = np.zeros(len(frames), np.int64)
    offs[1:] = np.cumsum(sizes)[:-1]
    data = np.zeros(int(sizes.sum()) + 16, np.uint8)
    for o, f in zip(offs, frames):
        data[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return data, (offs // 4).astype(np.uint32), lens


def _ip(u):
    return bytes([(u >> 24) & 255, (u >> 16) & 255, (u >> 8) & 255, u & 255])


@pytest.mark.parametrize("nat_type", [M.SYMMETRIC, M.FULL_CONE])
def test_end_to_end_chain_vs_tx_oracle(dev, oracle_lib, nat_type):
    """parse -> deep-NAT pass 1 -> lookup_quote -> deep-NAT pass 2 -> lookup_wan(d_skip = d_applied)
    -> tx fixup over a small IMIX synth batch plus hand-built replies and ICMP time-exceeded
    messages for flows of the table: the frames equal the oracle's IcmpTtlDeepNat and tx rewrite
    fed with the model's answers."""
    import torch

    from halo_amd import protocol, synth
    from halo_amd._lib import DEEP_NAT_DTYPE, NetIf
    from oracle import ref_py as R

    netif, onetif = NetIf.make(ip="203.0.113.1", nat_enable=True), oracle_lib.NetIf.make(ip="203.0.113.1", nat_enable=True)
    mac = bytes(netif.mac)
    t, m = _pair(nat_type, M.random_tuples(51, 24), mappings=[(53, 0xC0A80063, 5353, 17)])
    lay = synth.layout(48, size_mode=synth.SIZE_IMIX, proto_mode=synth.PROTO_MIX, mutate_shift=3)
    fr = synth.frames_device(lay, netif, device=dev, fill=0)
    sbytes = fr["bytes"].cpu().numpy()
    frames = [sbytes[4 * int(o):4 * int(o) + int(L)].tobytes() for o, L in zip(lay["offsets_dw"], lay["lens"])]
    rng = np.random.RandomState(77)
    for f in m.list():
        rip = f["remote_ip"] or 0x08080404
        rport = f["remote_port"] or 4444
        pl = bytes(rng.randint(0, 256, rng.randint(1, 90)).astype(np.uint8))
        src, dst = _ip(rip), _ip(M.WAN_IP)
        # the reply to the flow's WAN endpoint ...
        if f["proto"] == 17:
            seg = R.build_udp(pl, rport, f["wan_port"], src, dst)
        elif f["proto"] == 6:
            seg = R.build_tcp(pl, rport, f["wan_port"], src, dst, 1, 2, 0x10)
        else:
            seg = R.build_icmp(pl, 0, f["wan_port"].to_bytes(2, "big"), 3)
        frames.append(R.build_eth(R.build_ipv4(seg, f["proto"], src, dst), mac, bytes(6), 0x0800))
        # ... and a router's time-exceeded message quoting the packet the flow sent out
        if f["proto"] == 17:
            q = R.build_udp(pl, f["wan_port"], rport, dst, src)
        elif f["proto"] == 6:
            q = R.build_tcp(pl, f["wan_port"], rport, dst, src, 1, 2, 0x10)
        else:
            q = R.build_icmp(pl, 8, f["wan_port"].to_bytes(2, "big"), 3)
        inner = R.build_ipv4(q, f["proto"], dst, src)
        msg = R.build_icmp(inner[:max(28, min(len(inner), 20 + rng.randint(8, 40)))], 11, b"\0\0", 0)
        frames.append(R.build_eth(R.build_ipv4(msg, 1, _ip(0xC6336402), dst), mac, bytes(6), 0x0800))
    # one time-exceeded message for a flow that does not exist, one UDP packet for the port mapping
    inner = R.build_ipv4(R.build_udp(b"x" * 12, 40000, 53, _ip(M.WAN_IP), _ip(0x08080404)), 17, _ip(M.WAN_IP), _ip(0x08080404))
    frames.append(R.build_eth(R.build_ipv4(R.build_icmp(inner, 11, b"\0\0", 0), 1, _ip(0xC6336402), _ip(M.WAN_IP)), mac,
                              bytes(6), 0x0800))
    frames.append(R.build_eth(R.build_ipv4(R.build_udp(b"query", 4000, 53, _ip(0x08080404), _ip(M.WAN_IP)), 17,
                                           _ip(0x08080404), _ip(M.WAN_IP)), mac, bytes(6), 0x0800))
    data, offs, lens = _pack(frames)
    n, now = len(frames), 140

    # ---- expected: the oracle fed with the model's answers ----
    recs, _ = oracle_lib.rx_batch(data, lens, onetif, 1, offsets_dw=offs)
    quotes = np.array([oracle_lib.icmp_quote(f, 1) for f in frames])
    answers = m.quote(quotes)
    want = data.copy()
    applied = np.zeros(n, np.uint8)
    for k, f in enumerate(frames):
        wf, ok = oracle_lib.icmp_deep_nat(f, *answers[k][:2], bool(answers[k][2]), 1)
        want[4 * int(offs[k]):4 * int(offs[k]) + len(f)] = np.frombuffer(wf, np.uint8)
        applied[k] = ok
    want_ops = protocol.tx_ops(n, TX_TTL | TX_RECALC)
    w_verdict, w_ref, w_miss = m.lookup(M.WAN, recs, now, want_ops, applied)
    want, want_res = oracle_lib.tx_batch(want, offs, lens, want_ops, flags=1)
    assert applied.sum() == len(m.list()) and (w_verdict == M.V_FLOW).sum() == len(m.list())
    assert (w_verdict == M.V_MAPPING).sum() >= 1 and (w_verdict == M.V_SKIP).sum() == applied.sum()

    # ---- the chain on the device: records never leave HBM ----
    d = torch.from_numpy(data).to(dev)
    o = torch.from_numpy(offs.view(np.int32)).to(dev)
    ln = torch.from_numpy(lens.view(np.int16)).to(dev)
    d_recs = protocol.parse_frames_batch(d, o, ln, netif=netif)
    d_quote = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    protocol.icmp_ttl_deep_nat_batch(d, o, ln, quote=d_quote)
    d_nat = t.lookup_quote(d_quote)
    d_applied = torch.empty(n, dtype=torch.uint8, device=dev)
    protocol.icmp_ttl_deep_nat_batch(d, o, ln, nat=d_nat, quote=d_quote, applied=d_applied)
    d_ops = torch.from_numpy(protocol.tx_ops(n, TX_TTL | TX_RECALC).view(np.uint8).reshape(n, 16)).to(dev)
    d_ops, d_verdict, d_ref, d_miss = t.lookup_wan(d_recs, now, ops=d_ops, skip=d_applied)
    d_res = torch.empty(n, dtype=torch.uint8, device=dev)
    protocol.tx_fixup_batch(d, o, ln, d_ops, result=d_res)
    torch.cuda.synchronize()

    got_nat = d_nat.cpu().numpy().reshape(-1).view(DEEP_NAT_DTYPE)
    assert [(int(x["lan_ip"]), int(x["lan_port"]), int(x["found"])) for x in got_nat] == answers
    assert np.array_equal(d_applied.cpu().numpy(), applied)
    assert np.array_equal(d_verdict.cpu().numpy(), w_verdict)
    assert np.array_equal(d_ref.cpu().numpy().view(np.uint32), w_ref) and int(d_miss.cpu()[0]) == w_miss
    assert d_ops.cpu().numpy().tobytes() == want_ops.tobytes()
    got = d.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ from the oracle (first {bad[:8]})"
    assert np.array_equal(d_res.cpu().numpy(), want_res)
