"""CPU: the host control plane of the port-mapping return-flow table (halo_amd/csrc/pmflow_table.cc)
against tests/pmflow_model.py — random traces of record / get / expire / list, the named corners of
engine/ipv4_engine.go:238-266 and :497-516, the forced 16-slot layout the GPU tests probe, every
argument error of every call (the device calls' included, checked before a device is looked for),
and the batch sizes at which halo_pmflow_record_device changes path, pinned."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import pmflow_cases as C
from tests import pmflow_model as PM


def _table(capacity=64, capacity_log2=0, n=4):
    from halo_amd import PortMappingFlowTable

    return PortMappingFlowTable(C.lib_netifs()[:n], C.GATEWAYS[:n], capacity, capacity_log2)


def _model(capacity=64):
    return PM.Model(C.model_netifs(), C.GATEWAYS, capacity)


def _same(t, m):
    assert C.listing_of(t.List()) == m.listing()


def test_random_traces_match_the_model():
    rng = np.random.RandomState(20)
    for capacity in (5, 40):
        t, m = _table(capacity), _model(capacity)
        now = 0xFFFFFF00  # the trace crosses the uint32 wrap of TimeNow
        keys = [(0x08080000 + int(rng.randint(0, 6)), int(rng.randint(1, 4)), C.SERVER + int(rng.randint(0, 2)),
                 int(rng.choice([80, 443])), int(rng.choice([6, 17]))) for _ in range(60)]
        for step in range(1500):
            now = (now + int(rng.randint(0, 9))) & 0xFFFFFFFF
            op = rng.randint(0, 10)
            if op < 5:
                k = int(rng.randint(1, 6))
                items = [keys[rng.randint(len(keys))] + (int(rng.randint(1, 65536)),) for _ in range(k)]
                nif = int(rng.choice([C.WAN1, C.WAN2]))
                dropped, added = t.record(nif, C.item_array(items), now)
                w_dropped, w_added = m.record(nif, items, now)
                assert list(dropped) == w_dropped and added == w_added
            elif op < 8:
                key = keys[rng.randint(len(keys))]
                stamp = now if rng.randint(2) else None
                got, want = t.get(*key, now=stamp), m.get(key, stamp)
                assert (got is None) == (want is None)
                if got is not None:
                    assert (int(got["wan_netif"]), int(got["wan_port"]), int(got["last_alive"]), int(got["id"])) == tuple(want)
            elif op < 9:
                assert t.TableClear(now) == m.expire(now)
            else:
                _same(t, m)
        _same(t, m)
        assert m.next_id > capacity  # ids kept growing past removals: never reused
        t.close()


def test_full_table_drops_a_new_key_and_still_overwrites_an_existing_one():
    t, m = _table(capacity=2), _model(2)
    a, b, c = (1, 10, C.SERVER, 80, 6), (2, 20, C.SERVER, 80, 6), (3, 30, C.SERVER, 80, 6)
    items = [a + (8080,), b + (8080,), c + (8080,), a + (9090,), c + (8080,)]
    dropped, added = t.record(C.WAN2, C.item_array(items), 50)
    assert list(dropped) == [0, 0, 1, 0, 1] == m.record(C.WAN2, items, 50)[0] and added == 2
    _same(t, m)
    assert int(t.get(*a)["wan_port"]) == 9090 and t.get(*c) is None


def test_key_recorded_again_from_another_wan_netif():
    t, m = _table(), _model()
    key = (0x08080808, 4000, C.SERVER, 80, 6)
    for nif, port, now in ((C.WAN2, 8080, 10), (C.WAN1, 8081, 11)):
        t.record(nif, C.item_array([key + (port,)]), now)
        m.record(nif, [key + (port,)], now)
    e = t.get(*key)
    assert (int(e["wan_netif"]), int(e["wan_port"]), int(e["last_alive"]), int(e["id"])) == (C.WAN1, 8081, 11, 0)
    _same(t, m)
    assert t.dirty  # never synced


def test_expire_at_age_60_and_61_and_across_the_wrap():
    for base in (1000, 0xFFFFFFF0):  # the second: now wraps past zero while the flow ages
        t, m = _table(), _model()
        key = (0x08080808, 4000, C.SERVER, 80, 17)
        t.record(C.WAN2, C.item_array([key + (53,)]), base)
        m.record(C.WAN2, [key + (53,)], base)
        at60, at61 = (base + 60) & 0xFFFFFFFF, (base + 61) & 0xFFFFFFFF
        assert t.TableClear(at60) == 0 == m.expire(at60) and t.get(*key) is not None
        assert t.TableClear(at61) == 1 == m.expire(at61) and t.get(*key) is None
        # a stamp through get keeps it alive
        t.record(C.WAN2, C.item_array([key + (53,)]), base)
        assert t.get(*key, now=at60) is not None and t.TableClear(at61) == 0
        assert int(t.get(*key)["id"]) == 1  # a fresh id for the second insert
        t.close()


def test_forced_16_slot_fixture_has_a_long_and_a_wrapped_chain():
    items, st = C.fixture_items(lambda: _table(capacity=15, capacity_log2=4))
    assert st["slots"] == 16 and st["entries"] == 12 and st["longest_chain"] >= 3 and st["wrapped"] >= 1


def test_entries_at_the_forced_slot_count_are_a_range_error():
    from halo_amd import _lib

    t = _table(capacity=32, capacity_log2=4)
    items = [(k + 1, 7, C.SERVER, 80, 6, 8080) for k in range(16)]
    dropped, added = t.record(C.WAN2, C.item_array(items[:15]), 1)
    assert added == 15 and t.layout_stats()["entries"] == 15
    t.record(C.WAN2, C.item_array(items[15:]), 1)
    out = np.zeros(1, _lib.PMFLOW_LAYOUT_DTYPE)
    assert _lib.lib.halo_pmflow_layout_stats(t._t, _lib.ptr(out)) == _lib.HALO_E_RANGE
    assert len(t.List()) == 16  # the host table itself is not limited by the slot count


def test_argument_errors_leave_the_table_as_it_was():
    from halo_amd import _lib

    L, INVAL, RANGE = _lib.lib, _lib.HALO_E_INVAL, _lib.HALO_E_RANGE
    h = ctypes.c_void_p()
    cfg = _lib.PmflowConfig()
    cfg.n_netifs, cfg.capacity = 2, 4
    assert L.halo_pmflow_table_create(None, ctypes.byref(h)) == INVAL
    assert L.halo_pmflow_table_create(ctypes.byref(cfg), None) == INVAL
    for n_netifs, capacity, log2, rc in ((0, 4, 0, INVAL), (65, 4, 0, INVAL), (2, 0, 0, INVAL), (2, 4, 29, RANGE)):
        bad = _lib.PmflowConfig()
        bad.n_netifs, bad.capacity, bad.capacity_log2 = n_netifs, capacity, log2
        assert L.halo_pmflow_table_create(ctypes.byref(bad), ctypes.byref(h)) == rc and not h.value
    assert L.halo_pmflow_table_destroy(None) == INVAL

    t = _table(capacity=8, n=3)
    good = C.item_array([(1, 2, C.SERVER, 80, 6, 8080)])
    t.record(C.WAN2, good, 5)
    before = C.listing_of(t.List())
    dropped, n32, f32 = np.zeros(4, np.uint8), ctypes.c_uint32(), ctypes.c_uint32()
    e = np.zeros(1, _lib.PMFLOW_ENTRY_DTYPE)
    icmp = C.item_array([(9, 9, C.SERVER, 80, 6, 1), (9, 9, C.SERVER, 80, 1, 1)])  # the second: not TCP / UDP
    assert L.halo_pmflow_record(None, 0, _lib.ptr(good), 1, 5, _lib.ptr(dropped), None) == INVAL
    assert L.halo_pmflow_record(t._t, 3, _lib.ptr(good), 1, 5, _lib.ptr(dropped), None) == RANGE  # n_netifs = 3
    assert L.halo_pmflow_record(t._t, 1, None, 1, 5, _lib.ptr(dropped), None) == INVAL
    assert L.halo_pmflow_record(t._t, 1, _lib.ptr(good), 1, 5, None, None) == INVAL
    assert L.halo_pmflow_record(t._t, 1, _lib.ptr(icmp), 2, 5, _lib.ptr(dropped), None) == INVAL  # nothing applied
    assert L.halo_pmflow_record(t._t, 1, None, 0, 5, None, None) == 0
    assert L.halo_pmflow_get(None, 1, 2, 3, 4, 6, None, _lib.ptr(e), ctypes.byref(f32)) == INVAL
    assert L.halo_pmflow_get(t._t, 1, 2, 3, 4, 6, None, _lib.ptr(e), None) == INVAL
    assert L.halo_pmflow_expire(None, 5, ctypes.byref(n32)) == INVAL
    assert L.halo_pmflow_list(None, _lib.ptr(e), 1, ctypes.byref(n32)) == INVAL
    assert L.halo_pmflow_list(t._t, None, 1, ctypes.byref(n32)) == INVAL
    assert L.halo_pmflow_list(t._t, _lib.ptr(e), 1, None) == INVAL
    assert L.halo_pmflow_layout_stats(None, _lib.ptr(e)) == INVAL and L.halo_pmflow_layout_stats(t._t, None) == INVAL
    assert L.halo_pmflow_dirty(None) == INVAL
    assert L.halo_pmflow_sync_device(None, None, 0) == INVAL and L.halo_pmflow_sync_device(t._t, None, -1) == INVAL

    # the device calls: every check comes before a device is looked for
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data % 16)  # a 16-byte aligned host address stands in for a device one
    lk = lambda **kw: L.halo_pmflow_lookup_device(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("t", t._t), ("recs", p), ("n", 1), ("now", 5), ("rids", p), ("sel", None), ("ops", p), ("via", p), ("hit", p),
        ("counts", None), ("stream", None))])
    assert lk(t=None) == INVAL
    for name in ("recs", "rids", "ops", "via", "hit"):
        assert lk(**{name: None}) == INVAL, name
    assert lk(recs=p + 8) == INVAL and lk(ops=p + 8) == INVAL and lk(via=p + 4) == INVAL
    assert lk(rids=p + 2) == INVAL and lk(counts=p + 2) == INVAL
    wsb = int(L.halo_pmflow_record_workspace(1))
    assert wsb == 8 and int(L.halo_pmflow_record_workspace(0)) == 4 and int(L.halo_pmflow_record_workspace(257)) == 8 + 260
    rd = lambda **kw: L.halo_pmflow_record_device(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("t", t._t), ("nif", 1), ("recs", p), ("wv", p), ("ops", p), ("arp", p), ("n", 1), ("now", 5), ("items", p),
        ("cap", 1), ("count", p), ("ws", p), ("wsb", wsb), ("stream", None))])
    assert rd(t=None) == INVAL and rd(count=None) == INVAL and rd(items=None) == INVAL
    assert rd(nif=3) == RANGE
    for name in ("recs", "wv", "ops", "arp", "ws"):
        assert rd(**{name: None}) == INVAL, name
    assert rd(wsb=wsb - 1) == INVAL
    assert rd(recs=p + 8) == INVAL and rd(ops=p + 8) == INVAL and rd(arp=p + 4) == INVAL
    assert rd(items=p + 2) == INVAL and rd(count=p + 2) == INVAL and rd(ws=p + 2) == INVAL
    assert L.halo_arp_drop_device(None, p, 1, None) == INVAL and L.halo_arp_drop_device(p, None, 1, None) == INVAL
    assert L.halo_arp_drop_device(p + 4, p, 1, None) == INVAL and L.halo_arp_drop_device(p, p + 2, 1, None) == INVAL
    # never synced: the table has no device copy to look anything up in
    assert lk() == INVAL and rd() == INVAL
    assert C.listing_of(t.List()) == before and len(before) == 1


def test_encap_via_argument_errors():
    from halo_amd import ArpTable, _lib

    L = _lib.lib
    arp = ArpTable(C.lib_netifs(), 8)
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data % 16)
    assert L.halo_arp_encap_via_device(None, p, p, p, 1, p, 0, None, p, p, None, p, None) == _lib.HALO_E_INVAL
    assert L.halo_arp_encap_via_device(arp._t, p, p, p, 1, p, 4, None, p, p, None, p, None) == _lib.HALO_E_RANGE
    assert L.halo_arp_encap_via_device(arp._t, p, p, p, 1, p, 0, None, p, p, None, p, None) == _lib.HALO_E_INVAL  # never synced


def test_record_device_boundaries_are_pinned():
    """The sizes tests/test_gpu_pmflow.py derives from the sources, pinned: a moved constant must be
    a decision, and the ARP gather's tile must move with it."""
    c = C.read_constants()
    assert c == {"kRecordTile": 256, "kScanPass": 1024, "kGatherTile": 256}
    assert C.derived(c) == {"record_tile": 257, "record_scan_pass": 262145}


@pytest.mark.parametrize("name", ["pmflow_table.cc", "pmflow_fwd.hip"])
def test_sources_are_built_into_the_library(name):
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("halo_build", os.path.join(C.ROOT, "halo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert name in mod.SOURCES and "pmflow_table.h" in mod.HEADERS
