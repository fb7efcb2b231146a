"""GPU: the lifecycle of a device-resident table (halo_amd/csrc/device_table.h: sync, fold, publish
after an expiry, destroy) through the three tables that share it — the NAT flow table, the ARP
neighbour cache and the port-mapping return-flow table — at the edges the per-table tests do not
state as such: an expiry before any sync; sync, lookup, an expiry that removes half the entries,
lookup; a second sync naming another device; destroy with a lookup just enqueued on a side stream.
Eight entries in a forced 16-slot table whose layout has a wrapped chain, batches of 64 records;
every expected value comes from the dict models (tests/nat_model.py, arp_model.py, pmflow_model.py)."""
from __future__ import annotations

import numpy as np
import pytest

from tests import arp_cases as AK
from tests import arp_model as AM
from tests import nat_model as NM
from tests import pmflow_cases as PC
from tests import pmflow_model as PM

pytestmark = pytest.mark.gpu

ENTRIES, BATCH = 8, 64
OLD, NEW = 1000, 1070  # when the odd and the even entries are added: an expiry at NEW removes the odd ones


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


def _t(dev, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _targets(which):
    """The entry each of the BATCH records asks for: `which` in turn, and -1 (no entry) for every eighth."""
    return [-1 if j % 8 == 7 else which[(j - j // 8) % len(which)] for j in range(BATCH)]


class Nat:
    """`times[k]`: TimeNow of entry k's NatAddFlow."""

    def __init__(self, seed, times):
        from halo_amd.nat import NatTable

        self.t, self.m = NatTable(NM.WAN_IP, NM.SYMMETRIC, capacity_log2=4), NM.NatModel(NM.WAN_IP, NM.SYMMETRIC)
        for tup, now in zip(NM.random_tuples(seed, ENTRIES), times):
            NM.fill(self.t, self.m, [tup], now)
        self.flows = [dict(f) for f in sorted(self.m.list(), key=lambda f: f["id"])]

    def wrapped(self):
        return int(self.t.layout_stats()["wrapped"].sum())

    def sync(self):
        self.t.sync()

    def sync_rc(self, device):
        from halo_amd import _lib

        return _lib.lib.halo_nat_sync_device(self.t._t, device)

    def expire(self, now):
        return self.t.TableClear(now), self.m.expire(now)

    def listings(self):
        return NM.sorted_flows(self.t.ListNat()), NM.sorted_flows(self.m.list())

    def lookup(self, dev, which, now, stream=None):
        """Enqueues the inbound lookup of a batch: (device results, the model's hits per record, a check)."""
        from halo_amd._lib import RESULT_DTYPE

        recs = np.zeros(BATCH, RESULT_DTYPE)
        for j, k in enumerate(_targets(which)):
            f = self.flows[max(k, 0)]
            recs[j]["ip_proto"], recs[j]["src_ip"], recs[j]["sport"] = f["proto"], f["remote_ip"], f["remote_port"] or 7
            recs[j]["dst_ip"], recs[j]["dport"] = f["wan_ip"], f["wan_port"] if k >= 0 else 9
        want_v, want_ref, want_miss = self.m.lookup(NM.WAN, recs, now, NM.ops(BATCH, 1))
        got = self.t.lookup_wan(_t(dev, recs.view(np.uint8).reshape(-1, 32)), now, stream=stream)

        def check():
            _, verdict, ref, miss = got
            assert np.array_equal(verdict.cpu().numpy(), want_v)
            assert np.array_equal(ref.cpu().numpy().view(np.uint32), want_ref) and int(miss.cpu()[0]) == want_miss

        return want_v == NM.V_FLOW, check

    def destroy_rc(self):
        from halo_amd import _lib

        rc, self.t._t = _lib.lib.halo_nat_table_destroy(self.t._t), None
        return rc

    def close(self):
        self.t.close()


class Arp:
    """`times[k]`: TimeNow of entry k's SetArpCache (ExpTime = that + 300)."""

    AGE = 300

    def __init__(self, seed, times):
        self.p = AK.Pair(capacity=ENTRIES, slots_log2=4)
        rng = np.random.RandomState(seed)
        self.ips = [0x0A000100 + int(x) for x in rng.choice(4096, ENTRIES, replace=False)]
        for k, (ip, now) in enumerate(zip(self.ips, times)):
            self.p.set(0, ip, AK.mac(k + 1), now - self.AGE)  # expires as a flow last alive at `now` + 60 does

    def wrapped(self):
        return int(self.p.t.layout_stats()["wrapped"])

    def sync(self):
        self.p.t.sync()

    def sync_rc(self, device):
        from halo_amd import _lib

        return _lib.lib.halo_arp_sync_device(self.p.t._t, None, device)

    def expire(self, now):  # the flow tables' rule is now - last_alive > 60, ARP's is now > ExpTime
        return self.p.t.ArpTableClear(now - 60), self.p.m.expire(now - 60)

    def listings(self):
        got = sorted((int(e["netif"]), int(e["ip"]), bytes(e["mac"]), int(e["exp_time"])) for e in self.p.t.ListArp())
        return got, self.p.m.listing()

    def lookup(self, dev, which, now, stream=None):
        ips = np.array([self.ips[k] if k >= 0 else 0x0A00FFF0 + j for j, k in enumerate(_targets(which))], np.uint32)
        want = [self.p.m.lookup(0, int(ip)) for ip in ips]
        got = self.p.t.lookup(_t(dev, ips.view(np.int32)), stream=stream)

        def check():
            mac8, verdict, miss = got
            assert list(verdict.cpu().numpy()) == [w[0] for w in want]
            assert [bytes(r) for r in mac8.cpu().numpy()] == [w[1] + b"\0\0" if w[0] == AM.HIT else bytes(8) for w in want]
            assert int(miss.cpu()[0]) == sum(w[0] == AM.MISS for w in want)

        return np.array([w[0] == AM.HIT for w in want]), check

    def destroy_rc(self):
        from halo_amd import _lib

        rc, self.p.t._t = _lib.lib.halo_arp_table_destroy(self.p.t._t), None
        return rc

    def close(self):
        self.p.close()


class Pmflow:
    """`times[k]`: TimeNow of the frame that recorded flow k."""

    def __init__(self, seed, times):
        from halo_amd import PortMappingFlowTable
        from halo_amd.route import RouteTable

        self.t = PortMappingFlowTable(PC.lib_netifs(), PC.GATEWAYS, ENTRIES, 4)
        self.m = PM.Model(PC.model_netifs(), PC.GATEWAYS, ENTRIES)
        rng = np.random.RandomState(seed)
        self.items = [(int(rng.randint(1, 1 << 31)), 1 + k, PC.SERVER + int(rng.randint(0, 4)), int(rng.randint(1, 65536)),
                       int(rng.choice([6, 17])), int(rng.randint(1, 65536))) for k in range(ENTRIES)]
        for it, now in zip(self.items, times):
            dropped, added = self.t.record(PC.WAN2, PC.item_array([it]), now)
            assert added == 1 == self.m.record(PC.WAN2, [it], now)[1] and not dropped.any()
        self.rt = RouteTable(0)  # read on the host by the sync: the NetIf of every route id
        self.rid = self.rt.AddRoute(RouteTable.entry(0, 0, PC.GATEWAYS[PC.WAN1], PC.WAN1))

    def wrapped(self):
        return int(self.t.layout_stats()["wrapped"])

    def sync(self):
        self.t.sync(self.rt)

    def sync_rc(self, device):
        from halo_amd import _lib

        return _lib.lib.halo_pmflow_sync_device(self.t._t, self.rt._t, device)

    def expire(self, now):
        return self.t.TableClear(now), self.m.expire(now)

    def listings(self):
        return PC.listing_of(self.t.List()), self.m.listing()

    def lookup(self, dev, which, now, stream=None):
        from halo_amd._lib import PMFLOW_VIA_DTYPE, RESULT_DTYPE

        recs = np.zeros(BATCH, RESULT_DTYPE)
        recs["ethertype"] = 0x0800
        want = np.zeros(BATCH, PMFLOW_VIA_DTYPE)
        for j, k in enumerate(_targets(which)):  # the LAN host's reply of flow k
            rip, rport, lip, lport, proto, _ = self.items[max(k, 0)]
            recs[j]["dst_ip"], recs[j]["dport"], recs[j]["src_ip"], recs[j]["ip_proto"] = rip, rport, lip, proto
            recs[j]["sport"] = lport if k >= 0 else lport ^ 1
            tup = tuple(int(recs[j][f]) for f in ("ip_proto", "src_ip", "dst_ip", "sport", "dport"))
            want[j] = self.m.lookup(tup, AK.route_of(self.rt, self.rid), now)[:4]
        rids = _t(dev, np.full(BATCH, self.rid, np.uint32).view(np.int32))
        got = self.t.lookup(_t(dev, recs.view(np.uint8).reshape(-1, 32)), now, rids, stream=stream)

        def check():
            _, via, hit, counts = got
            assert np.array_equal(via.cpu().numpy().reshape(-1).view(PMFLOW_VIA_DTYPE), want)
            assert np.array_equal(hit.cpu().numpy(), (want["verdict"] >= PM.V_HIT).astype(np.uint8))
            assert list(counts.cpu().numpy()) == [int((want["verdict"] == v).sum()) for v in range(4)]

        return want["verdict"] >= PM.V_HIT, check

    def destroy_rc(self):
        from halo_amd import _lib

        rc, self.t._t = _lib.lib.halo_pmflow_table_destroy(self.t._t), None
        return rc

    def close(self):
        self.t.close()
        self.rt.close()


TABLES = [Nat, Arp, Pmflow]
ALL = list(range(ENTRIES))
_seeds = {}


def _make(cls, times):
    """A table of ENTRIES entries whose 16-slot layout has a wrapped chain: the first seed that gives
    one (layout statistics are computed on the host), kept for the module."""
    for seed in range(_seeds.get(cls, 0), 64):
        w = cls(seed, times)
        if w.wrapped() >= 1:
            _seeds[cls] = seed
            return w
        w.close()
    raise AssertionError("no seed gives a wrapped chain")


@pytest.mark.parametrize("cls", TABLES)
def test_expire_before_any_sync(dev, cls):
    """No device object yet: the expiry is the host model's and nothing is published."""
    w = _make(cls, [OLD if k % 2 else NEW for k in ALL])
    try:
        got, want = w.expire(NEW)
        assert got == want == ENTRIES // 2
        got, want = w.listings()
        assert got == want and len(got) == ENTRIES // 2
        from halo_amd import _lib

        with pytest.raises(_lib.HaloError) as e:  # still never synced
            w.lookup(dev, ALL, NEW)
        assert e.value.code == _lib.HALO_E_INVAL
    finally:
        w.close()


@pytest.mark.parametrize("cls", TABLES)
def test_sync_lookup_expire_lookup(dev, cls):
    """Every entry is old enough to expire at NEW + 1. The first lookup asks for the even entries: in
    the NAT and return-flow tables that stamps them on the device, and the expiry has to fold those
    stamps before it judges and again before it publishes; in the ARP cache, which has no stamps, the
    even entries were set later. The second lookup, without a sync, misses exactly the odd entries."""
    import torch

    w = _make(cls, [OLD if cls is not Arp or k % 2 else NEW for k in ALL])
    try:
        w.sync()
        hits, check = w.lookup(dev, ALL[::2], OLD + 30)
        torch.cuda.synchronize()
        check()
        assert int(hits.sum()) == BATCH - BATCH // 8
        got, want = w.expire(OLD + 61)
        assert got == want == ENTRIES // 2
        got, want = w.listings()
        assert got == want and len(got) == ENTRIES // 2  # with the stamps the device wrote
        assert set(_targets(ALL)) == set(ALL) | {-1}
        hits, check = w.lookup(dev, ALL, OLD + 62)
        torch.cuda.synchronize()
        check()
        assert [bool(h) for h in hits] == [k >= 0 and k % 2 == 0 for k in _targets(ALL)]
    finally:
        w.close()


@pytest.mark.parametrize("cls", TABLES)
def test_second_sync_names_another_device(dev, cls):
    import torch

    from halo_amd import _lib

    w = _make(cls, [NEW] * ENTRIES)
    try:
        w.sync()
        assert w.sync_rc(1) == _lib.HALO_E_INVAL  # one device per table, judged before the device is looked for
        hits, check = w.lookup(dev, ALL, NEW + 1)
        torch.cuda.synchronize()
        check()
        assert int(hits.sum()) == BATCH - BATCH // 8
        assert w.sync_rc(0) == _lib.HALO_OK
    finally:
        w.close()


@pytest.mark.parametrize("cls", TABLES)
def test_destroy_under_a_queued_lookup(dev, cls):
    """Destroy drains the device before it frees: the lookup enqueued just before it on another
    stream still reads the table it was given."""
    import torch

    from halo_amd import _lib

    w = _make(cls, [NEW] * ENTRIES)
    try:
        w.sync()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            hits, check = w.lookup(dev, ALL, NEW + 1, stream=side)
        assert w.destroy_rc() == _lib.HALO_OK
        side.synchronize()
        check()
        assert int(hits.sum()) == BATCH - BATCH // 8
    finally:
        w.close()
