"""Not a test: the expected answers of the NAT miss-path tests, on top of tests/nat_model.py.

``collect`` is the listing halo_nat_collect_misses_{host,device} must produce: a dict keyed by the
normalised key tuple plus the single-listing rule, no hashing. ``resolve`` is
halo_nat_resolve_misses on the NatModel with the ref each record ends with, ``apply`` is
halo_nat_apply_answers_device in numpy, and the builders make the batches the host, sanitizer and
GPU tests share: a corpus with heavy key reuse, zero ports and protocols without ports between the
hits, mappings and unparsed records of nat_model.records, and the named cases of the miss path.
"""
from __future__ import annotations

import numpy as np

from tests import nat_model as M

LAN, WAN = M.LAN, M.WAN
NO_FLOW = M.NO_FLOW
SIZES = (1, 63, 64, 65, 1025)
TILE = 256  # records per workgroup of the device listing
FORCED_LOG2 = 11  # the forced scratch table of the n = 1025 corpus: 2048 slots
FORCED_SEED = 8   # picked on the CPU: tests/test_nat_miss_host.py::test_forced_scratch_corpus_reaches_chains_and_wrap


def listed_alone(direction, sport, dport) -> bool:
    """NatAddFlow refuses a raw remote port 0 although the normalised key may be shared."""
    return direction == LAN and dport == 0 and sport != 0


def norm_key(nat_type, direction, r) -> tuple:
    proto, src, dst = int(r["ip_proto"]), int(r["src_ip"]), int(r["dst_ip"])
    sport, dport = int(r["sport"]), int(r["dport"])
    rip, rport, lip, lport = (src, sport, dst, dport) if direction == WAN else (dst, dport, src, sport)
    if nat_type != M.SYMMETRIC:
        rip, rport = 0, 0
    if proto == 1:
        rport = 0
    return rip, rport, lip, lport, proto


def collect(nat_type, direction, records, verdict, select=None, cap=None):
    """(items [(index, src_ip, dst_ip, sport, dport, proto)] (the first ``cap``), count, pos u32 [n])."""
    n = len(records)
    first: dict = {}
    items = []
    pos = np.full(n, NO_FLOW, np.uint32)
    for i in range(n):
        if verdict[i] != M.V_MISS or (select is not None and not select[i]):
            continue
        r = records[i]
        alone = listed_alone(direction, int(r["sport"]), int(r["dport"]))
        key = norm_key(nat_type, direction, r)
        if not alone and key in first:
            pos[i] = first[key]
            continue
        if not alone:
            first[key] = len(items)
        pos[i] = len(items)
        items.append((i, int(r["src_ip"]), int(r["dst_ip"]), int(r["sport"]), int(r["dport"]), int(r["ip_proto"])))
    return items[:len(items) if cap is None else cap], len(items), pos


def item_tuples(items) -> list:
    """NAT_MISS_ITEM_DTYPE records as collect()'s tuples; the padding must be zero."""
    assert not np.any(items["pad"])
    return [tuple(int(x[f]) for f in ("index", "src_ip", "dst_ip", "sport", "dport", "proto")) for x in items]


def resolve(m: M.NatModel, direction, records, verdicts, refs, now, ops, select=None):
    """halo_nat_resolve_misses on the model over the selected MISS records, in order:
    (verdicts_out, refs_out, n_added); ``ops`` is updated in place."""
    out, ref = verdicts.copy(), refs.copy()
    added = 0
    for i in np.nonzero(verdicts == M.V_MISS)[0]:
        if select is not None and not select[i]:
            continue
        r = records[i]
        v, rf, ip, port, f = m._find(direction, r)
        if v == M.V_MISS:
            if direction == WAN:
                continue
            f = m.add_flow(int(r["src_ip"]), int(r["dst_ip"]), int(r["sport"]), int(r["dport"]), int(r["ip_proto"]), now)
            if f is None:
                out[i], ref[i] = M.V_DROP, NO_FLOW
                continue
            added += 1
            v, rf, ip, port = M.V_FLOW, f["id"], f["wan_ip"], f["wan_port"]
        if f is not None:
            f["last_alive"] = now & M.M32
        m._apply(direction, ops[i:i + 1], ip, port)
        out[i], ref[i] = v, rf
    return out, ref, added


def apply(direction, pos, answers, ops, verdict, ref, counts=None):
    """halo_nat_apply_answers_device over host arrays, in place."""
    k = len(answers)
    for i in np.nonzero(pos < k)[0]:
        a = answers[int(pos[i])]
        v = int(a["verdict"])
        if counts is not None and v <= M.V_DROP:
            counts[v] += 1
        if v in (M.V_FLOW, M.V_MAPPING):
            m_apply(direction, ops[i:i + 1], int(a["ip"]), int(a["port"]))
            verdict[i], ref[i] = v, int(a["ref"])
        elif v == M.V_DROP:
            verdict[i], ref[i] = v, NO_FLOW


def m_apply(direction, op, ip, port):
    if direction == WAN:
        op["steps"] |= M.TX_NAT_DST
        op["dst_ip"], op["dst_port"] = ip, port
    else:
        op["steps"] |= M.TX_NAT_SRC
        op["src_ip"], op["src_port"] = ip, port


# ---- batches --------------------------------------------------------------------------------------
MAPPINGS = [(8080, 0xC0A80010, 80, 6), (8080, 0xC0A80011, 81, 6), (5353, 0xC0A80012, 53, 17)]


def _rec(r, i, proto, src, sport, dst, dport):
    r["ip_proto"][i], r["src_ip"][i], r["sport"][i], r["dst_ip"][i], r["dport"][i] = proto, src, sport, dst, dport


def blank(n):
    from halo_amd._lib import RESULT_DTYPE

    r = np.zeros(n, RESULT_DTYPE)
    r["l4_seq"] = np.arange(n)  # a field nothing here reads
    return r


def corpus(m: M.NatModel, direction, n, seed):
    """nat_model.records (flow hits, distinct misses, mapping hits, unparsed records) with about half
    the records replaced by draws from a small pool of new keys: every pool key several times, LAN
    keys with dport 0 (listed alone) and sport 0, and proto 47 (no ports at all)."""
    r = M.records(m, direction, n, seed)
    rng = np.random.RandomState(seed + 1000)
    pool = []
    for _ in range(max(3, n // 8)):
        proto = int(rng.choice([1, 6, 17, 17, 6, 47]))
        lan_ip, remote = 0xC0A80100 | int(rng.randint(2, 12)), 0x08090000 | int(rng.randint(1, 6))
        if proto == 47:
            lport = rport = 0
        else:
            lport = 0 if rng.randint(0, 10) == 0 else 2000 + int(rng.randint(0, 24))
            rport = 0 if rng.randint(0, 6) == 0 else 50 + int(rng.randint(0, 4))
        if proto == 1 and lport:
            rport = lport  # an echo id is both ports
        if direction == LAN:
            pool.append((proto, lan_ip, lport, remote, rport))
        else:  # towards the WAN address: a port no flow of the table holds yet, or a mapping's
            pool.append((proto, remote, rport, M.WAN_IP, 40000 + int(rng.randint(0, 24))))
    for i in range(n):
        if rng.randint(0, 2):
            _rec(r, i, *pool[rng.randint(0, len(pool))])
    return r


def all_distinct(direction, n):
    r = blank(n)
    for i in range(n):
        if direction == LAN:
            _rec(r, i, 17, 0xC0A80200 + (i >> 12), 1024 + (i & 0xFFF), 0x08080808, 53)
        else:
            _rec(r, i, 17, 0x08080808, 53, M.WAN_IP, 1024 + i)
    return r


def one_key(direction, n):
    r = blank(n)
    for i in range(n):
        _rec(r, i, 6, 0xC0A80205, 5555, 0x08080808, 443) if direction == LAN else _rec(r, i, 6, 0x08080808, 443, M.WAN_IP, 5555)
    return r


def cone_trap(n):
    """Full cone, LAN: A(dport 0), B(dport 5), C(dport 0), ... of one LAN host and port."""
    r = blank(n)
    for i in range(n):
        _rec(r, i, 17, 0xC0A80207, 6000, 0x08080808, 5 if i % 3 == 1 else 0)
    return r


def gre_flood(n):
    r = blank(n)
    for i in range(n):
        _rec(r, i, 47, 0xC0A80209, 0, 0x08080808, 0)
    return r


def pairs(n, lan_base=0xC0A80300):
    """Distinct new LAN keys towards one remote, each twice in a row."""
    r = blank(n)
    for i in range(n):
        _rec(r, i, 17, lan_base + ((i // 2) >> 12), 1024 + ((i // 2) & 0xFFF), 0x08080808, 53)
    return r


def period(n, p=4099):
    """Keys repeat every ``p`` records."""
    r = blank(n)
    k = np.arange(n) % p
    r["ip_proto"], r["src_ip"], r["sport"] = 17, 0xC0A80400 + (k >> 12), 1024 + (k & 0xFFF)
    r["dst_ip"], r["dport"] = 0x08080808, 53
    return r


def wave_and_tile_reach(pos) -> tuple:
    """(a duplicate whose representative is in an earlier workgroup, a duplicate whose representative
    is in another wave of its own workgroup) of a listing's ``pos``."""
    first: dict = {}
    far = near = False
    for i, p in enumerate(pos):
        if p == NO_FLOW:
            continue
        r = first.setdefault(int(p), i)
        if r != i:
            far |= r // TILE < i // TILE
            near |= r // TILE == i // TILE and r // 64 < i // 64
    return far, near


# ---- tables, the named cases and the property ---------------------------------------------------------
EXHAUST_FREE = 2  # ports the exhaustion case leaves free in the one (full-cone) allocator


class Case:
    """One batch: ``records`` for ``direction`` over tables of ``nat_type`` prefilled with ``tuples`` and
    ``mappings``; ``late`` flows are added after the point a device copy would have been taken;
    ``exhaust`` fills the allocator first; ``select`` / ``cap`` as the collect takes them."""

    def __init__(self, name, nat_type, direction, records, tuples=(), mappings=(), late=(), exhaust=False, select=None,
                 cap=None):
        self.__dict__.update(locals())
        del self.__dict__["self"]


def named_cases(n):
    rng = np.random.RandomState(n)
    sel = (rng.randint(0, 3, n) != 0).astype(np.uint8)
    base, late = M.random_tuples(78, 5), M.random_tuples(77, 6)
    probe = M.NatModel(M.WAN_IP, M.SYMMETRIC)
    for tup in base:
        probe.add_flow(*tup, 100)
    late_flows = [probe.add_flow(*tup, 105) for tup in late]
    wan = blank(n)
    for i in range(n):  # replies to the late flows' WAN endpoints, and every fourth a true miss
        (lan_ip, remote_ip, lan_port, remote_port, proto), f = late[i % 6], late_flows[i % 6]
        _rec(wan, i, proto, remote_ip, remote_port, M.WAN_IP, f["wan_port"] if i % 4 else 20000 + i % 7)
    return [
        Case("distinct", M.SYMMETRIC, LAN, all_distinct(LAN, n)),
        Case("distinct_wan", M.SYMMETRIC, WAN, all_distinct(WAN, n)),
        Case("one_key", M.SYMMETRIC, LAN, one_key(LAN, n)),
        Case("one_key_wan", M.FULL_CONE, WAN, one_key(WAN, n)),
        Case("cone_trap", M.FULL_CONE, LAN, cone_trap(n)),
        Case("sym_dport0", M.SYMMETRIC, LAN, cone_trap(n)),
        Case("gre_flood", M.SYMMETRIC, LAN, gre_flood(n)),
        Case("exhaustion", M.FULL_CONE, LAN, pairs(n), exhaust=True),
        Case("select", M.SYMMETRIC, LAN, pairs(n), mappings=MAPPINGS, select=sel),
        Case("cap", M.FULL_CONE, LAN, pairs(n), cap=max(1, (n // 2 + 1) // 3)),
        Case("wan_late", M.SYMMETRIC, WAN, wan, tuples=base, late=late),
    ]


def corpus_cases(n):
    out = []
    for nat_type in (M.SYMMETRIC, M.FULL_CONE):
        for direction in (LAN, WAN):
            tuples = M.random_tuples(40 + nat_type, 40)
            probe = M.NatModel(M.WAN_IP, nat_type)
            for e in MAPPINGS:
                probe.add_port_mapping(*e)
            for tup in tuples:
                probe.add_flow(*tup, 100)
            out.append(Case(f"corpus_{nat_type}_{direction}", nat_type, direction, corpus(probe, direction, n, FORCED_SEED),
                            tuples=tuples, mappings=MAPPINGS))
    return out


def build(case: Case, copies=2, now=100, sync=False):
    """``copies`` NatTables and the model, built by the same calls; (tables, model, first_id): flows
    with an id below first_id exist in the tables only (the exhaustion fill)."""
    from halo_amd import _lib
    from halo_amd.nat import NatTable

    ts = [NatTable(M.WAN_IP, case.nat_type) for _ in range(copies)]
    m = M.NatModel(M.WAN_IP, case.nat_type)
    first_id = 0
    if case.exhaust:  # as tests/test_nat_table.py::test_port_exhaustion fills one allocator
        first_id = 32768 - EXHAUST_FREE
        out = np.zeros(1, _lib.NAT_FLOW_DTYPE)
        for t in ts:
            for k in range(first_id):
                assert _lib.lib.halo_nat_add_flow(t._t, 0x0A000000 + (k >> 15), 0x08080808, 1 + (k & 0x7FFF), 53, 17, now,
                                                  out.ctypes.data, None) == 0
        m.alloc[0] = set(range(32768, 32768 + first_id))
        m.next_id = first_id
    for e in case.mappings:
        m.add_port_mapping(*e)
        for t in ts:
            t.add_port_mapping(*e)
    for tup in case.tuples:
        m.add_flow(*tup, now)
        for t in ts:
            t.AddFlow(*tup, now)
    if sync:
        for t in ts:
            t.sync()
    return ts, m, first_id


def add_late(case: Case, ts, m, now=105):
    for tup in case.late:
        m.add_flow(*tup, now)
        for t in ts:
            t.AddFlow(*tup, now)


def flows_from(flows, first_id) -> list:
    return M.sorted_flows(f for f in flows if int(f["id"]) >= first_id)


def check_property(case: Case, t, twin, m, first_id, verdict, ref, ops, now, collect_fn, apply_fn):
    """collect -> resolve_items -> apply on ``t`` against halo_nat_resolve_misses on ``twin`` and the
    model, from the ``verdict`` / ``ref`` / ``ops`` a lookup left. ``collect_fn(t, direction, records,
    verdict, select, cap)`` -> (items, count, pos) and ``apply_fn(direction, pos, answers, ops, verdict,
    ref)`` -> (ops, verdict, ref) are the host's or the device's. Returns the verdicts."""
    d, recs, select = case.direction, case.records, case.select
    w_items, w_count, w_pos = collect(case.nat_type, d, recs, verdict, select, case.cap)
    items, count, pos = collect_fn(t, d, recs, verdict, select, case.cap)
    assert count == w_count and item_tuples(items) == w_items, (case.name, count, w_count)
    assert np.array_equal(pos, w_pos), (case.name, np.nonzero(pos != w_pos)[0][:8])
    answers, added = t.resolve_items(d, items, now)
    g_ops, g_verdict, g_ref = apply_fn(d, pos, answers, ops.copy(), verdict.copy(), ref.copy())
    off = (verdict == M.V_MISS) & (np.zeros(len(recs), bool) if select is None else select == 0)
    if count > len(items):  # the cap cut the list: the records still MISS go the old way, in order
        rest = g_verdict.copy()
        rest[off] = M.V_SKIP
        assert np.all(g_verdict[pos >= len(items)] == verdict[pos >= len(items)])
        rest, more = t.resolve_misses(d, recs, rest, now, g_ops)
        rest[off] = M.V_MISS
        g_verdict, added = rest, added + more
    # the twin: the whole batch through halo_nat_resolve_misses
    v2 = verdict.copy()
    v2[off] = M.V_SKIP
    t_ops = ops.copy()
    t_verdict, t_added = twin.resolve_misses(d, recs, v2, now, t_ops)
    t_verdict[off] = M.V_MISS
    # the model
    m_ops = ops.copy()
    m_verdict, m_ref, m_added = resolve(m, d, recs, verdict, ref, now, m_ops, select)
    assert g_ops.tobytes() == t_ops.tobytes() == m_ops.tobytes(), case.name
    assert g_verdict.tobytes() == t_verdict.tobytes() == m_verdict.tobytes(), case.name
    assert added == t_added == m_added, (case.name, added, t_added, m_added)
    assert M.sorted_flows(t.ListNat()) == M.sorted_flows(twin.ListNat()), case.name
    assert flows_from(t.ListNat(), first_id) == flows_from(m.list(), first_id), case.name
    done = pos < len(items)
    assert np.array_equal(g_ref[done], m_ref[done]) and np.array_equal(g_ref[~done], ref[~done]), case.name
    return g_verdict
