"""CPU: the host parts of the NAT miss path (halo_amd/csrc/nat_table.cc): halo_nat_collect_misses_host
against the dict model of tests/nat_miss_model.py, and the central property — collect ->
halo_nat_resolve_items -> apply on a table leaves ops, verdicts, refs and the flow table exactly as
halo_nat_resolve_misses leaves a twin table built by the same calls — on random traces and the named
cases, both directions and NAT types; the argument checks the device entry points make before they
look for a device; and the reach of the forced-scratch corpus the GPU test runs."""
from __future__ import annotations

import copy

import numpy as np
import pytest

from halo_amd import _lib
from halo_amd.nat import NatTable
from tests import nat_miss_model as X
from tests import nat_model as M


def _collect_host(t, direction, recs, verdict, select, cap):
    return t.collect_misses_host(direction, recs, verdict, select=select, cap=cap)


def _apply_model(direction, pos, answers, ops, verdict, ref):
    X.apply(direction, pos, answers, ops, verdict, ref)
    return ops, verdict, ref


def _run(case, now=110):
    (t, twin), m, first_id = X.build(case)
    ops = M.ops(len(case.records), 5)
    # what a device lookup of the copy taken here would leave (a copy of the model: the lookup's
    # stamps stay on the device until a fold)
    verdict, ref, _ = copy.deepcopy(m).lookup(case.direction, case.records, now, ops)
    X.add_late(case, (t, twin), m)
    return X.check_property(case, t, twin, m, first_id, verdict, ref, ops, now, _collect_host, _apply_model), (t, m)


@pytest.mark.parametrize("n", X.SIZES)
def test_random_traces_match_the_twin(n):
    seen = set()
    for case in X.corpus_cases(n):
        seen |= set(_run(case)[0].tolist())
    if n == 1025:
        assert seen == {M.V_NONE, M.V_MISS, M.V_FLOW, M.V_MAPPING, M.V_DROP}


@pytest.mark.parametrize("n", X.SIZES)
def test_named_cases_match_the_twin(n):
    for case in X.named_cases(n):
        verdict, (t, m) = _run(case)
        if case.name in ("distinct", "one_key", "gre_flood"):
            _, k, pos = X.collect(case.nat_type, case.direction, case.records, np.full(n, M.V_MISS, np.uint8))
            assert k == (n if case.name == "distinct" else 1)
        if case.name in ("distinct", "one_key"):
            assert np.all(verdict == M.V_FLOW)
        if case.name == "gre_flood":
            assert np.all(verdict == M.V_DROP)
        if case.name == "cone_trap":  # A(dport 0), B, C(dport 0): DROP, FLOW (added), FLOW (hit)
            assert verdict.tolist() == ([M.V_DROP] + [M.V_FLOW] * (n - 1) if n > 1 else [M.V_DROP])
            assert len(t.ListNat()) == (1 if n > 1 else 0)
        if case.name == "sym_dport0":  # symmetric: dport 0 is part of the key, and always refused
            assert np.all(verdict[0::3] == M.V_DROP) and np.all(verdict[2::3] == M.V_DROP) and np.all(verdict[1::3] == M.V_FLOW)
        if case.name == "exhaustion":  # two ports were free: two FLOW pairs, then DROP pairs
            assert verdict.tolist() == ([M.V_FLOW] * 4 + [M.V_DROP] * n)[:n]
        if case.name == "select":
            off = case.select == 0
            assert np.all(verdict[off] == M.V_MISS)
            assert len(t.ListNat()) == len({(int(r["src_ip"]), int(r["sport"])) for r in case.records[~off]})
        if case.name == "wan_late":
            late_reply = np.arange(n) % 4 != 0
            assert np.all(verdict[late_reply] == M.V_FLOW) and np.all(verdict[~late_reply] == M.V_MISS)
        if case.name == "one_key_wan":
            assert np.all(verdict == M.V_MISS)


def test_cap_writes_a_prefix_and_counts_all():
    case = [c for c in X.named_cases(65) if c.name == "cap"][0]
    t = NatTable(M.WAN_IP, case.nat_type)
    verdict = np.full(65, M.V_MISS, np.uint8)
    items, count, pos = t.collect_misses_host(X.LAN, case.records, verdict, cap=case.cap)
    assert count == 33 and len(items) == case.cap == 11 and int(pos.max()) == 32
    full, count0, pos0 = t.collect_misses_host(X.LAN, case.records, verdict, cap=0)
    assert count0 == 33 and len(full) == 0 and np.array_equal(pos0, pos)
    answers, added = t.resolve_items(X.LAN, items, 9)
    assert added == 11 and np.all(answers["verdict"] == M.V_FLOW) and not np.any(answers["pad"])
    assert answers["ref"].tolist() == list(range(11)) and np.all(answers["ip"] == M.WAN_IP)


def test_resolve_items_answers_and_refs():
    """A mapping, an existing flow, a new flow, a refused one, and for WAN a miss that stays MISS."""
    t, m = NatTable(M.WAN_IP, M.SYMMETRIC), M.NatModel(M.WAN_IP, M.SYMMETRIC)
    t.add_port_mapping(*X.MAPPINGS[0])
    t.add_port_mapping(*X.MAPPINGS[2])
    old = t.AddFlow(0xC0A80020, 0x08080808, 1000, 53, 17, 50)
    items = np.zeros(4, _lib.NAT_MISS_ITEM_DTYPE)
    items[0] = (0, 0xC0A80012, 0x08080808, 53, 999, 17, (0, 0, 0))      # the second mapping, LAN side
    items[1] = (3, 0xC0A80020, 0x08080808, 1000, 53, 17, (0, 0, 0))     # the old flow
    items[2] = (5, 0xC0A80021, 0x08080808, 1000, 53, 17, (0, 0, 0))     # new
    items[3] = (9, 0xC0A80021, 0x08080808, 1001, 0, 17, (0, 0, 0))      # remote port 0: nil
    a, added = t.resolve_items(X.LAN, items, 77)
    assert added == 1 and a["verdict"].tolist() == [M.V_MAPPING, M.V_FLOW, M.V_FLOW, M.V_DROP]
    assert a["ref"].tolist() == [1, int(old["id"]), int(old["id"]) + 1, M.NO_FLOW]
    assert a["ip"].tolist() == [M.WAN_IP, M.WAN_IP, M.WAN_IP, 0] and a["port"].tolist() == [5353, 32768, 32769, 0]
    assert sorted(int(f["last_alive"]) for f in t.ListNat()) == [77, 77]
    w = np.zeros(2, _lib.NAT_MISS_ITEM_DTYPE)
    w[0] = (0, 0x08080808, M.WAN_IP, 53, 32769, 17, (0, 0, 0))
    w[1] = (1, 0x08080808, M.WAN_IP, 53, 32770, 17, (0, 0, 0))
    a, added = t.resolve_items(X.WAN, w, 78)
    assert added == 0 and a["verdict"].tolist() == [M.V_FLOW, M.V_MISS] and a["ref"].tolist() == [int(old["id"]) + 1, M.NO_FLOW]
    assert (int(a["ip"][0]), int(a["port"][0])) == (0xC0A80021, 1000) and (int(a["ip"][1]), int(a["port"][1])) == (0, 0)


def test_argument_checks():
    L = _lib.lib
    t = NatTable(M.WAN_IP, M.SYMMETRIC)
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    assert p % 16 == 0
    cnt = np.zeros(1, np.uint32)
    c = cnt.ctypes.data
    # host collect
    assert L.halo_nat_collect_misses_host(None, 0, p, p, None, 1, p, 1, c, p) == _lib.HALO_E_INVAL
    assert L.halo_nat_collect_misses_host(t._t, 2, p, p, None, 1, p, 1, c, p) == _lib.HALO_E_INVAL
    assert L.halo_nat_collect_misses_host(t._t, 0, p, p, None, 1, p, 1, None, p) == _lib.HALO_E_INVAL
    assert L.halo_nat_collect_misses_host(t._t, 0, None, p, None, 1, p, 1, c, p) == _lib.HALO_E_INVAL
    assert L.halo_nat_collect_misses_host(t._t, 0, p, p, None, 1, None, 1, c, p) == _lib.HALO_E_INVAL
    assert L.halo_nat_collect_misses_host(t._t, 0, p, p, None, 1, p, 1, c, None) == _lib.HALO_E_INVAL
    cnt[0] = 7
    assert L.halo_nat_collect_misses_host(t._t, 0, None, None, None, 0, None, 0, c, None) == 0 and cnt[0] == 0
    # resolve_items
    assert L.halo_nat_resolve_items(None, 0, p, 1, 0, p, None) == _lib.HALO_E_INVAL
    assert L.halo_nat_resolve_items(t._t, 3, p, 1, 0, p, None) == _lib.HALO_E_INVAL
    assert L.halo_nat_resolve_items(t._t, 0, None, 1, 0, p, None) == _lib.HALO_E_INVAL
    assert L.halo_nat_resolve_items(t._t, 0, p, 1, 0, None, None) == _lib.HALO_E_INVAL
    assert L.halo_nat_resolve_items(t._t, 0, None, 0, 0, None, None) == 0
    # the device entry points check their arguments before they look for a device
    ws = int(L.halo_nat_miss_workspace(1025, 0))
    assert ws == 4 * (4096 + 5 + 1025) and L.halo_nat_miss_workspace(1025, 11) == 4 * (2048 + 5 + 1025)
    assert L.halo_nat_miss_workspace(1, 0) == 4 * (16 + 1 + 1) and L.halo_nat_miss_workspace(0, 0) == 4 * (16 + 1)
    assert L.halo_nat_miss_workspace(8, 32) == 0 and L.halo_nat_miss_workspace((1 << 30) + 1, 0) == 0
    for fn in (L.halo_nat_collect_misses_device, L.halo_nat_collect_misses_compact_device):
        assert fn(None, 0, p, p, None, 1, 0, p, 1, c, p, p, 4096, None) == _lib.HALO_E_INVAL
        assert fn(t._t, 2, p, p, None, 1, 0, p, 1, c, p, p, 4096, None) == _lib.HALO_E_INVAL
        assert fn(t._t, 0, None, p, None, 1, 0, p, 1, c, p, p, 4096, None) == _lib.HALO_E_INVAL
        assert fn(t._t, 0, p, None, None, 1, 0, p, 1, c, p, p, 4096, None) == _lib.HALO_E_INVAL
        assert fn(t._t, 0, p, p, None, 1, 0, None, 1, c, p, p, 4096, None) == _lib.HALO_E_INVAL
        assert fn(t._t, 0, p, p, None, 1, 0, p, 1, None, p, p, 4096, None) == _lib.HALO_E_INVAL
        assert fn(t._t, 0, p, p, None, 1, 0, p, 1, c, None, p, 4096, None) == _lib.HALO_E_INVAL
        assert fn(t._t, 0, p, p, None, 1, 0, p, 1, c, p, None, 4096, None) == _lib.HALO_E_INVAL
        assert fn(t._t, 0, p + 4, p, None, 1, 0, p, 1, c, p, p, 4096, None) == _lib.HALO_E_INVAL  # misaligned records
        assert fn(t._t, 0, p, p, None, 1, 0, p + 2, 1, c, p, p, 4096, None) == _lib.HALO_E_INVAL  # ... items
        assert fn(t._t, 0, p, p, None, 1, 0, p, 1, c, p, p, 71, None) == _lib.HALO_E_INVAL        # short workspace
        # a forced scratch table must have more slots than records
        assert fn(t._t, 0, p, p, None, 1025, 10, p, 1, c, p, p, 1 << 20, None) == _lib.HALO_E_RANGE
        assert fn(t._t, 0, p, p, None, 2048, 11, p, 1, c, p, p, 1 << 20, None) == _lib.HALO_E_RANGE
        assert fn(t._t, 0, p, p, None, 16, 4, p, 1, c, p, p, 1 << 20, None) == _lib.HALO_E_RANGE
        assert fn(t._t, 0, p, p, None, 1, 32, p, 1, c, p, p, 1 << 20, None) == _lib.HALO_E_RANGE
        # well-formed, on a table that was never synced (or in a process without a device)
        assert fn(t._t, 0, p, p, None, 15, 4, p, 1, c, p, p, 1 << 20, None) in (_lib.HALO_E_INVAL, _lib.HALO_E_NODEV)
    A = L.halo_nat_apply_answers_device
    assert A(2, p, 1, p, 1, p, p, p, None, None) == _lib.HALO_E_INVAL
    assert A(0, None, 1, p, 1, p, p, p, None, None) == _lib.HALO_E_INVAL
    assert A(0, p, 1, None, 1, p, p, p, None, None) == _lib.HALO_E_INVAL
    assert A(0, p, 1, p, 1, None, p, p, None, None) == _lib.HALO_E_INVAL
    assert A(0, p, 1, p, 1, p, None, p, None, None) == _lib.HALO_E_INVAL
    assert A(0, p, 1, p, 1, p, p, None, None, None) == _lib.HALO_E_INVAL
    assert A(0, p, 1, p + 8, 1, p, p, p, None, None) == _lib.HALO_E_INVAL  # answers are 16-byte aligned
    assert A(0, p, 1, p, 1, p + 8, p, p, None, None) == _lib.HALO_E_INVAL  # ... and ops
    assert A(0, p + 2, 1, p, 1, p, p, p, None, None) == _lib.HALO_E_INVAL


def _probe_stats(case, log2):
    """(longest probe chain, insertions that wrapped) of the distinct table keys of the case's
    selected records in a 2^log2-slot table, inserted in index order, hashed by the XXH3 oracle."""
    from oracle import ref_xxh3_py as H

    m = M.NatModel(M.WAN_IP, case.nat_type)
    for e in case.mappings:
        m.add_port_mapping(*e)
    for tup in case.tuples:
        m.add_flow(*tup, 100)
    verdict, _, _ = m.lookup(case.direction, case.records, 110, M.ops(len(case.records), 5))
    mask = (1 << log2) - 1
    taken, seen, longest, wrapped = set(), set(), 0, 0
    for i in np.nonzero(verdict == M.V_MISS)[0]:
        r = case.records[i]
        if X.listed_alone(case.direction, int(r["sport"]), int(r["dport"])):
            continue
        key = H.nat_flow_key({f: int(r[f]) for f in ("src_ip", "dst_ip", "sport", "dport", "ip_proto")}, case.direction,
                             case.nat_type)
        if key in seen:
            continue
        seen.add(key)
        s = home = H.xxh3_64(key) & mask
        steps = 1
        while s in taken:
            s, steps = (s + 1) & mask, steps + 1
        taken.add(s)
        longest = max(longest, steps)
        wrapped += s < home
    return longest, wrapped, len(seen)


def test_forced_scratch_corpus_reaches_chains_and_wrap():
    """The n = 1025 corpus in the forced 2048-slot scratch table: some key probes three slots or
    more, and some probe runs past the last slot to slot 0 (X.FORCED_SEED was picked for this)."""
    stats = [_probe_stats(case, X.FORCED_LOG2) for case in X.corpus_cases(1025)]
    assert max(s[0] for s in stats) >= 3 and sum(s[1] for s in stats) >= 1, stats
    assert all(s[2] < (1 << X.FORCED_LOG2) for s in stats)


def test_corpus_has_duplicates_across_waves_and_workgroups():
    for case in X.corpus_cases(1025):
        m = X.build(case, copies=0)[1]
        verdict, _, _ = m.lookup(case.direction, case.records, 110, M.ops(1025, 5))
        assert X.wave_and_tile_reach(X.collect(case.nat_type, case.direction, case.records, verdict)[2]) == (True, True)
