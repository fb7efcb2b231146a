"""GPU: the NAT miss path (halo_amd/csrc/nat_miss.hip through halo_amd.nat.NatTable): the device
listing byte-identical to halo_nat_collect_misses_host and to the dict model over both record widths,
with the verdicts of real lookups; the central property — collect -> resolve_items -> apply on the
device leaves ops, verdicts, refs and the flow table as halo_nat_resolve_misses leaves a twin; a batch
past one scan pass; apply's untouched records and counts; and forward_return_flows(new_flows=True)
against the tx oracle."""
from __future__ import annotations

import numpy as np
import pytest

from tests import nat_miss_model as X
from tests import nat_model as M
from tests import pmflow_cases as C

pytestmark = pytest.mark.gpu

TX_TTL, TX_RECALC = M.TX_TTL, 0x08


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


def _pair(nat_type, tuples, log2=0, mappings=()):
    from halo_amd.nat import NatTable

    t, m = NatTable(M.WAN_IP, nat_type, capacity_log2=log2), M.NatModel(M.WAN_IP, nat_type)
    for e in mappings:
        t.add_port_mapping(*e)
        m.add_port_mapping(*e)
    M.fill(t, m, tuples, 100)
    t.sync()
    return t, m


@pytest.fixture(scope="module")
def tables(dev):
    """The forced_sym, forced_cone and 5000 tables of tests/test_gpu_nat.py's recipe, synced; nothing
    here adds a flow to them."""
    fs, fc = M.FIXTURE_SEED[M.SYMMETRIC], M.FIXTURE_SEED[M.FULL_CONE]
    return {
        "forced_sym": _pair(M.SYMMETRIC, M.random_tuples(fs, M.FIXTURE_FLOWS), M.FIXTURE_LOG2, X.MAPPINGS),
        "forced_cone": _pair(M.FULL_CONE, M.random_tuples(fc, M.FIXTURE_FLOWS), M.FIXTURE_LOG2),
        "5000": _pair(M.SYMMETRIC, M.random_tuples(9, 5000), 0, X.MAPPINGS),
    }


def _up(dev, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy()).to(dev)


def _records(dev, recs, compact):
    from halo_amd._lib import compact_of

    return _up(dev, compact_of(recs) if compact else recs)


def _lookup(dev, t, direction, recs, now, ops, compact=False):
    """A real device lookup: (d_recs, d_ops, d_verdict, d_ref) and the host copies of the last three."""
    import torch

    from halo_amd._lib import TX_OP_DTYPE

    d_recs = _records(dev, recs, compact)
    fn = t.lookup_wan if direction == M.WAN else t.lookup_lan
    d_ops, d_verdict, d_ref, _ = fn(d_recs, now, ops=_up(dev, ops))
    torch.cuda.synchronize()
    return (d_recs, d_ops, d_verdict, d_ref), (d_ops.cpu().numpy().reshape(-1).view(TX_OP_DTYPE).copy(),
                                               d_verdict.cpu().numpy(), d_ref.cpu().numpy().view(np.uint32))


def _fetch_listing(items, count, pos, cap):
    import torch

    from halo_amd._lib import NAT_MISS_ITEM_DTYPE

    torch.cuda.synchronize()
    k = int(count.cpu().numpy().view(np.uint32)[0])
    return (items.cpu().numpy().reshape(-1).view(NAT_MISS_ITEM_DTYPE)[:min(k, cap)].copy(), k,
            pos.cpu().numpy().view(np.uint32).copy())


def _dev_collect(dev, compact=False, scratch_log2=0):
    def fn(t, direction, recs, verdict, select, cap):
        import torch

        d_sel = None if select is None else torch.from_numpy(np.ascontiguousarray(select, np.uint8)).to(dev)
        out = t.collect_misses(direction, _records(dev, recs, compact), torch.from_numpy(verdict).to(dev), select=d_sel,
                               cap=cap, scratch_log2=scratch_log2)
        return _fetch_listing(*out, len(recs) if cap is None else cap)
    return fn


def _dev_apply(dev, counts=None):
    def fn(direction, pos, answers, ops, verdict, ref):
        import torch

        from halo_amd._lib import TX_OP_DTYPE
        from halo_amd.nat import NatTable

        d_pos = torch.from_numpy(pos.view(np.int32).copy()).to(dev)
        d_ans = torch.from_numpy(answers.view(np.uint8).reshape(-1, 16).copy()).to(dev)
        d_ops, d_verdict = _up(dev, ops), torch.from_numpy(verdict.copy()).to(dev)
        d_ref = torch.from_numpy(ref.view(np.int32).copy()).to(dev)
        NatTable.apply_answers(direction, d_pos, d_ans, d_ops, d_verdict, d_ref, counts=counts)
        torch.cuda.synchronize()
        return (d_ops.cpu().numpy().reshape(-1).view(TX_OP_DTYPE).copy(), d_verdict.cpu().numpy(),
                d_ref.cpu().numpy().view(np.uint32).copy())
    return fn


def _same_listing(got, want, what):
    assert got[1] == want[1], (what, got[1], want[1])
    assert got[0].tobytes() == want[0].tobytes(), what
    assert np.array_equal(got[2], want[2]), (what, np.nonzero(got[2] != want[2])[0][:8])


def _batches(m, direction, nat_type, n):
    """(name, records, select, cap) over one table: the corpus and the named cases' records for this
    direction and NAT type."""
    out = [("corpus", X.corpus(m, direction, n, X.FORCED_SEED), None, None)]
    for case in X.named_cases(n):
        if case.direction == direction and (case.nat_type == nat_type or case.name in ("distinct", "one_key", "gre_flood")):
            out.append((case.name, case.records, case.select, case.cap))
    return out


@pytest.mark.parametrize("name", ["forced_sym", "forced_cone", "5000"])
@pytest.mark.parametrize("n", X.SIZES)
def test_device_listing_equals_the_host_listing(dev, tables, name, n):
    """Both record widths, both directions, the corpus and every named batch, between the NONE, FLOW
    and MAPPING records a real lookup leaves."""
    t, m = tables[name]
    seen, reach = set(), [False, False]
    for direction in (M.LAN, M.WAN):
        for what, recs, select, cap in _batches(m, direction, t.nat_type, n):
            _, (_, verdict, _) = _lookup(dev, t, direction, recs, 200, M.ops(n, 3))
            seen |= set(verdict.tolist())
            want = t.collect_misses_host(direction, recs, verdict, select=select, cap=cap)
            w_items, w_count, w_pos = X.collect(t.nat_type, direction, recs, verdict, select, cap)
            assert X.item_tuples(want[0]) == w_items and want[1] == w_count and np.array_equal(want[2], w_pos)
            far, near = X.wave_and_tile_reach(w_pos)
            reach = [reach[0] | far, reach[1] | near]
            for compact in (False, True):
                got = _dev_collect(dev, compact)(t, direction, recs, verdict, select, cap)
                _same_listing(got, want, (name, n, direction, what, compact))
    if n == 1025:
        assert reach == [True, True]  # duplicates in a later workgroup, and in a later wave of the first one's
        assert {M.V_NONE, M.V_MISS, M.V_FLOW} <= seen and (name == "forced_cone" or M.V_MAPPING in seen)


def test_forced_scratch_table_and_the_one_key_batch(dev, tables):
    """The 2048-slot scratch table with 1025 records (probe chains of three slots and a wrap:
    tests/test_nat_miss_host.py checks the corpus reaches them), and one key 1025 times."""
    for case in X.corpus_cases(1025):
        (t,), m, _ = X.build(case, copies=1, sync=True)
        _, (_, verdict, _) = _lookup(dev, t, case.direction, case.records, 200, M.ops(1025, 3))
        want = t.collect_misses_host(case.direction, case.records, verdict)
        for compact in (False, True):
            got = _dev_collect(dev, compact, X.FORCED_LOG2)(t, case.direction, case.records, verdict, None, None)
            _same_listing(got, want, (case.name, compact))
    t, _ = tables["forced_sym"]
    recs = X.one_key(M.LAN, 1025)
    verdict = np.full(1025, M.V_MISS, np.uint8)
    for log2 in (0, X.FORCED_LOG2):
        items, count, pos = _dev_collect(dev, False, log2)(t, M.LAN, recs, verdict, None, None)
        assert count == 1 and int(items["index"][0]) == 0 and not pos.any()


def test_two_launches_are_identical_and_one_workspace_serves_a_stream(dev, tables):
    import torch

    t, m = tables["5000"]
    a, b = X.corpus(m, M.LAN, 1025, 21), X.corpus(m, M.LAN, 700, 22)
    va = _lookup(dev, t, M.LAN, a, 200, M.ops(1025, 3))[1][1]
    vb = _lookup(dev, t, M.LAN, b, 200, M.ops(700, 3))[1][1]
    from halo_amd import _lib

    ws = torch.empty(int(_lib.lib.halo_nat_miss_workspace(1025, 0)) // 4, dtype=torch.int32, device=dev)
    ws.fill_(0x5A5A5A5A)
    d_a, d_b = _up(dev, a), _up(dev, b)
    d_va, d_vb = torch.from_numpy(va).to(dev), torch.from_numpy(vb).to(dev)
    # back to back on one stream, one workspace, no synchronisation in between
    r1 = t.collect_misses(M.LAN, d_a, d_va, workspace=ws)
    r2 = t.collect_misses(M.LAN, d_b, d_vb, workspace=ws)
    r3 = t.collect_misses(M.LAN, d_a, d_va, workspace=ws)
    g1, g2, g3 = _fetch_listing(*r1, 1025), _fetch_listing(*r2, 700), _fetch_listing(*r3, 1025)
    _same_listing(g1, t.collect_misses_host(M.LAN, a, va), "first")
    _same_listing(g2, t.collect_misses_host(M.LAN, b, vb), "second, same workspace")
    _same_listing(g3, g1, "the same call again")
    assert r1[0].cpu().numpy().tobytes() == r3[0].cpu().numpy().tobytes()  # the whole item buffer


def _property(dev, case, now=110):
    (t, twin), m, first_id = X.build(case, copies=2)
    t.sync()
    _, (ops, verdict, ref) = _lookup(dev, t, case.direction, case.records, now, M.ops(len(case.records), 5))
    X.add_late(case, (t, twin), m)
    return X.check_property(case, t, twin, m, first_id, verdict, ref, ops, now, _dev_collect(dev), _dev_apply(dev))


@pytest.mark.parametrize("n", X.SIZES)
def test_miss_path_equals_the_twin_on_random_traces(dev, n):
    seen = set()
    for case in X.corpus_cases(n):
        seen |= set(_property(dev, case).tolist())
    if n == 1025:
        assert seen == {M.V_NONE, M.V_MISS, M.V_FLOW, M.V_MAPPING, M.V_DROP}


@pytest.mark.parametrize("n", X.SIZES)
def test_miss_path_equals_the_twin_on_the_named_cases(dev, n):
    for case in X.named_cases(n):
        verdict = _property(dev, case)
        if case.name == "cone_trap" and n > 1:
            assert verdict.tolist() == [M.V_DROP] + [M.V_FLOW] * (n - 1)
        if case.name == "exhaustion":
            assert verdict.tolist() == ([M.V_FLOW] * 4 + [M.V_DROP] * n)[:n]
        if case.name == "gre_flood":
            assert np.all(verdict == M.V_DROP)
        if case.name == "wan_late":
            assert np.all(verdict[np.arange(n) % 4 != 0] == M.V_FLOW) and np.all(verdict[::4] == M.V_MISS)


def test_past_one_scan_pass(dev):
    """n = 1024 tiles + 257: keys repeat every 4,099 records, so every representative is in the
    scan's first pass and the duplicates run into its second. Expected values from the C host twin."""
    from halo_amd.nat import NatTable

    n = 1024 * X.TILE + 257
    recs = X.period(n)
    t, twin = NatTable(M.WAN_IP, M.SYMMETRIC), NatTable(M.WAN_IP, M.SYMMETRIC)
    t.sync()
    _, (ops, verdict, ref) = _lookup(dev, t, M.LAN, recs, 110, M.ops(n, 5))
    assert np.all(verdict == M.V_MISS)
    want = t.collect_misses_host(M.LAN, recs, verdict)
    assert want[1] == 4099 and int(want[2][-1]) == (n - 1) % 4099
    for compact in (False, True):
        got = _dev_collect(dev, compact)(t, M.LAN, recs, verdict, None, None)
        _same_listing(got, want, compact)
    answers, added = t.resolve_items(M.LAN, got[0], 110)
    g_ops, g_verdict, g_ref = _dev_apply(dev)(M.LAN, got[2], answers, ops.copy(), verdict.copy(), ref.copy())
    t_ops = ops.copy()
    t_verdict, t_added = twin.resolve_misses(M.LAN, recs, verdict, 110, t_ops)
    assert added == t_added == 4099 and g_ops.tobytes() == t_ops.tobytes() and g_verdict.tobytes() == t_verdict.tobytes()
    assert np.array_equal(g_ref, answers["ref"][got[2]])
    assert M.sorted_flows(t.ListNat()) == M.sorted_flows(twin.ListNat())


@pytest.mark.parametrize("direction", [M.LAN, M.WAN])
def test_apply_leaves_the_rest_untouched_and_counts(dev, direction):
    """Every answer kind; pos none and pos >= k are untouched byte for byte; a DROP leaves its op;
    the counts are incremented by the exact per-verdict numbers."""
    import torch

    from halo_amd._lib import NAT_ANSWER_DTYPE

    n, k = 1025, 40
    rng = np.random.RandomState(5 + direction)
    answers = np.zeros(k, NAT_ANSWER_DTYPE)
    answers["verdict"] = rng.choice([M.V_FLOW, M.V_MAPPING, M.V_DROP, M.V_MISS], k)
    answers["ip"], answers["port"], answers["ref"] = rng.randint(1, 1 << 31, k), rng.randint(1, 65536, k), rng.randint(0, 999, k)
    pos = rng.randint(0, 60, n).astype(np.uint32)  # 40..59: beyond the answers
    pos[rng.randint(0, 4, n) == 0] = M.NO_FLOW
    ops, verdict = M.ops(n, 9), np.full(n, M.V_MISS, np.uint8)
    ref = rng.randint(0, 1 << 31, n).astype(np.uint32)
    w_ops, w_verdict, w_ref, w_counts = ops.copy(), verdict.copy(), ref.copy(), np.arange(6, dtype=np.int64) + 100
    X.apply(direction, pos, answers, w_ops, w_verdict, w_ref, w_counts)
    counts = torch.arange(100, 106, dtype=torch.int32, device=dev)
    g_ops, g_verdict, g_ref = _dev_apply(dev, counts)(direction, pos, answers, ops, verdict, ref)
    assert g_ops.tobytes() == w_ops.tobytes() and g_verdict.tobytes() == w_verdict.tobytes() and np.array_equal(g_ref, w_ref)
    assert counts.cpu().numpy().tolist() == w_counts.tolist() and w_counts[M.V_NONE] == 100 and w_counts[M.V_SKIP] == 101
    left = pos >= k
    drop = ~left & (answers["verdict"][np.minimum(pos, k - 1)] == M.V_DROP)
    assert left.sum() > 100 and drop.sum() > 50
    assert g_ops[left | drop].tobytes() == ops[left | drop].tobytes()
    assert np.array_equal(g_verdict[left], verdict[left]) and np.array_equal(g_ref[left], ref[left])
    assert np.all(g_verdict[drop] == M.V_DROP) and np.all(g_ref[drop] == M.NO_FLOW)


def test_argument_checks_on_the_device(dev, tables):
    import torch

    from halo_amd import _lib
    from halo_amd.nat import NatTable

    L = _lib.lib
    b = torch.zeros(8192, dtype=torch.uint8, device=dev)
    p = b.data_ptr()
    never = NatTable(M.WAN_IP, M.SYMMETRIC)
    t, _ = tables["forced_sym"]
    for fn in (L.halo_nat_collect_misses_device, L.halo_nat_collect_misses_compact_device):
        assert fn(never._t, 0, p, p, None, 1, 0, p, 1, p, p, p, 4096, None) == _lib.HALO_E_INVAL  # before the first sync
        assert fn(never._t, 0, None, None, None, 0, 0, None, 0, p, None, None, 0, None) == _lib.HALO_E_INVAL
        assert fn(t._t, 0, p, p, None, 16, 4, p, 1, p, p, p, 4096, None) == _lib.HALO_E_RANGE
        assert fn(t._t, 0, p + 4, p, None, 1, 0, p, 1, p, p, p, 4096, None) == _lib.HALO_E_INVAL
        b[:4] = 0xEE
        assert fn(t._t, 0, None, None, None, 0, 0, None, 0, p, None, None, 0, None) == 0  # n == 0: *d_count = 0
        torch.cuda.synchronize()
        assert b[:4].cpu().numpy().tolist() == [0, 0, 0, 0]
    assert L.halo_nat_apply_answers_device(0, None, 0, None, 0, None, None, None, None, None) == 0
    assert L.halo_nat_apply_answers_device(0, p, 1, p + 8, 1, p, p, p, None, None) == _lib.HALO_E_INVAL
    assert L.halo_nat_apply_answers_device(0, p, 1, p, 1, p + 8, p, p, None, None) == _lib.HALO_E_INVAL
    items, count, pos = t.collect_misses(M.LAN, b[:0].reshape(0, 32), b[:0])
    torch.cuda.synchronize()
    assert int(count.cpu()[0]) == 0 and pos.numel() == 0


# ---- the chain ----------------------------------------------------------------------------------------
class _Router:
    """LAN (not NATing) and WAN1 (NATing, the default route), with the gateway's neighbour entry."""

    def __init__(self):
        from halo_amd import ArpTable, NatTable, PortMappingFlowTable
        from halo_amd.route import RouteTable

        self.netifs = C.lib_netifs()[:3]
        self.rt = RouteTable(0)
        for q in range(3):
            self.rt.AddRoute(RouteTable.entry(C.IPS[q] & 0xFFFFFF00, 0xFFFFFF00, 0, q))
        self.rt.AddRoute(RouteTable.entry(0, 0, C.GATEWAYS[C.WAN1], C.WAN1))
        self.rt.sync()
        self.arp = ArpTable(self.netifs, 16)
        self.arp.SetArpCache(C.WAN1, C.GATEWAYS[C.WAN1], C.GW_MAC[C.WAN1], 10)
        self.arp.sync(self.rt)
        self.nat = NatTable(C.IPS[C.WAN1])
        self.nat.sync()
        self.pm = PortMappingFlowTable(self.netifs, C.GATEWAYS[:3], 64)
        self.pm.sync(self.rt)
        self.model = M.NatModel(C.IPS[C.WAN1], M.SYMMETRIC)

    def close(self):
        for x in (self.pm, self.arp, self.rt, self.nat):
            x.close()


def _chain_frames():
    """New TCP, UDP and ICMP flows of LAN hosts, each at least three times and interleaved; one key
    whose only packet has TTL 1; and one key NatAddFlow refuses (UDP to port 0), three times."""
    flows = [(6, 0xC0A80115, 40001, 0x08080808, 443), (6, 0xC0A80116, 40002, 0x08080404, 80),
             (17, 0xC0A80115, 5000, 0x08080808, 53), (17, 0xC0A80117, 5001, 0x01010101, 123),
             (1, 0xC0A80118, 77, 0x08080808, 77)]
    refused = (17, 0xC0A80119, 6000, 0x08080808, 0)
    dead = (17, 0xC0A8011A, 7000, 0x08080808, 53)
    frames, kinds = [], []
    for rnd in range(4):
        for k, f in enumerate(flows):
            frames.append(C.l4_frame(*f, C.MACS[C.LAN], payload=b"pkt-%d-%d" % (rnd, k)))
            kinds.append("flow")
        if rnd < 3:
            frames.append(C.l4_frame(*refused, C.MACS[C.LAN]))
            kinds.append("refused")
        if rnd == 1:
            frames.append(C.l4_frame(*dead, C.MACS[C.LAN], ttl=1))
            kinds.append("dead")
    return frames, np.array(kinds), flows, dead


def _run_chain(dev, r, frames, new_flows, now=300):
    import torch

    from halo_amd import forward_return_flows

    data, offs, lens = C.pack(frames)
    d = torch.from_numpy(data).to(dev)
    o = torch.from_numpy(offs.view(np.int32)).to(dev)
    ln = torch.from_numpy(lens.view(np.int16)).to(dev)
    out = forward_return_flows(d, o, ln, netif=r.netifs[C.LAN], in_netif=C.LAN, now=now, pmflow=r.pm, routes=r.rt, arp=r.arp,
                               nat=r.nat, steps=TX_TTL | TX_RECALC, new_flows=new_flows)
    torch.cuda.synchronize()
    return (data, offs, lens), d.cpu().numpy(), out


def test_chain_resolves_new_flows_in_the_batch(dev, oracle_lib):
    from halo_amd import protocol
    from halo_amd._lib import ARP_RESULT_DTYPE, ARP_V, TX_OP_DTYPE

    frames, kinds, flows, dead = _chain_frames()
    n, now = len(frames), 300
    r = _Router()
    try:
        (data, offs, lens), got, out = _run_chain(dev, r, frames, True, now)
        recs = protocol.records(out.records)
        # ---- expected: the model's lookup and resolve feed the tx oracle ----
        want_ops = protocol.tx_ops(n, TX_TTL | TX_RECALC)
        verdict0, ref0, _ = r.model.lookup(M.LAN, recs, now, want_ops)
        assert np.all(verdict0 == M.V_MISS)
        select = (kinds != "dead").astype(np.uint8)
        w_verdict, w_ref, w_added = X.resolve(r.model, M.LAN, recs, verdict0, ref0, now, want_ops, select)
        want, want_res = oracle_lib.tx_batch(data, offs, lens, want_ops, flags=1)
        assert out.nat_new == (len(flows) + 3, len(flows)) and w_added == len(flows)  # the refused key is listed alone, thrice
        assert np.array_equal(out.nat_verdict.cpu().numpy(), w_verdict)
        assert np.array_equal(out.nat_ref.cpu().numpy().view(np.uint32), w_ref)
        assert out.ops.cpu().numpy().tobytes() == want_ops.tobytes()
        assert np.array_equal(out.fixup_result.cpu().numpy(), want_res)
        res = out.results.cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE)
        ops = out.ops.cpu().numpy().reshape(-1).view(TX_OP_DTYPE)
        for i, f in enumerate(frames):
            a = 4 * int(offs[i])
            assert got[a + 14:a + len(f)].tobytes() == want[a + 14:a + len(f)].tobytes(), (i, kinds[i])  # the packet
            if kinds[i] == "flow":  # leaves SNATed in this batch, towards the gateway
                assert w_verdict[i] == M.V_FLOW and ops["steps"][i] & M.TX_NAT_SRC
                assert got[a + 26:a + 30].tobytes() == C.IPS[C.WAN1].to_bytes(4, "big")
                assert res["verdict"][i] == ARP_V["HIT"] and res["out_netif"][i] == C.WAN1
                assert got[a:a + 12].tobytes() == C.GW_MAC[C.WAN1] + C.MACS[C.WAN1]
            else:  # DROP (:214-217) and the TTL-dead packet: nothing is transmitted
                assert w_verdict[i] == (M.V_DROP if kinds[i] == "refused" else M.V_MISS)
                assert res["verdict"][i] == ARP_V["NONE"] and got[a:a + 14].tobytes() == want[a:a + 14].tobytes()
        assert r.nat.GetFlowByHash(dead[3], dead[4], dead[1], dead[2], dead[0]) is None  # the TTL-1 key added no flow
        assert M.sorted_flows(r.nat.ListNat()) == M.sorted_flows(r.model.list()) and len(r.model.list()) == len(flows)
    finally:
        r.close()
    # ---- new_flows=False on an identical batch: what the chain gives today ----
    r = _Router()
    try:
        _, got0, out0 = _run_chain(dev, r, frames, False, now)
        plain = protocol.tx_ops(n, TX_TTL | TX_RECALC)
        want0, want_res0 = oracle_lib.tx_batch(data, offs, lens, plain, flags=1)
        assert out0.nat_new is None and np.all(out0.nat_verdict.cpu().numpy() == M.V_MISS)
        assert int(out0.nat_miss.cpu()[0]) == n and out0.ops.cpu().numpy().tobytes() == plain.tobytes()
        assert np.array_equal(out0.fixup_result.cpu().numpy(), want_res0) and len(r.nat.ListNat()) == 0
        res0 = out0.results.cpu().numpy().reshape(-1).view(ARP_RESULT_DTYPE)
        assert np.all((res0["verdict"] == ARP_V["HIT"]) == (kinds != "dead"))  # no SNAT, and the refused key is sent
        for i, f in enumerate(frames):
            a = 4 * int(offs[i])
            assert got0[a + 14:a + len(f)].tobytes() == want0[a + 14:a + len(f)].tobytes()
    finally:
        r.close()
