"""CPU: the host control plane of the NAT flow table (halo_amd/csrc/nat_table.cc through
halo_amd.nat.NatTable) against the dict model of the reference semantics (tests/nat_model.py):
NatAddFlow with its per-remote sequential port allocation, NatGetFlowByHash / ByWan,
CheckNatPortMapping, the NatTableClear tick in uint32 arithmetic, ListNat, the slow path for
device misses, and the layout statistics of the forced-capacity table the GPU tests use."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from halo_amd import _lib
from halo_amd._lib import RESULT_DTYPE, TX_OP_DTYPE
from halo_amd.nat import NatTable
from tests import nat_model as M

LAN_IPS = [0xC0A80002, 0xC0A80003, 0xC0A80004]
REMOTES = [0x08080808, 0x01010101, 0x09090909]
LAN_PORTS = [0, 1000, 1001, 1002, 1003]
REM_PORTS = [0, 53, 80, 443]
PROTOS = [1, 6, 17]


def _same_state(t: NatTable, m: M.NatModel):
    assert M.sorted_flows(t.ListNat()) == M.sorted_flows(m.list())


def _same_flow(got, want):
    assert (got is None) == (want is None), (got, want)
    if want is not None:
        assert M.flow_tuple(got) == M.flow_tuple(want)


def _records(rng, n, wan_ip, direction):
    r = np.zeros(n, RESULT_DTYPE)
    r["ip_proto"] = rng.choice(PROTOS + [0xFF], n)
    if direction == M.LAN:
        r["src_ip"], r["dst_ip"] = rng.choice(LAN_IPS, n), rng.choice(REMOTES, n)
        r["sport"], r["dport"] = rng.choice(LAN_PORTS, n), rng.choice(REM_PORTS, n)
    else:
        r["src_ip"], r["dst_ip"] = rng.choice(REMOTES, n), wan_ip
        r["sport"], r["dport"] = rng.choice(REM_PORTS, n), rng.choice([32768, 32769, 32770, 32771, 8080], n)
    return r


@pytest.mark.parametrize("nat_type", [M.SYMMETRIC, M.FULL_CONE])
@pytest.mark.parametrize("seed", [1, 2])
def test_random_trace_matches_model(nat_type, seed):
    rng = np.random.RandomState(1000 * nat_type + seed)
    t, m = NatTable(M.WAN_IP, nat_type), M.NatModel(M.WAN_IP, nat_type)
    for tb in (t, m):
        tb.add_port_mapping(8080, LAN_IPS[0], 80, 6)
    now = 0xFFFFFF00  # the trace crosses the uint32 wrap of TimeNow
    for _ in range(400):
        op = rng.randint(0, 10)
        if op < 4:
            a = (int(rng.choice(LAN_IPS)), int(rng.choice(REMOTES)), int(rng.choice(LAN_PORTS)),
                 int(rng.choice(REM_PORTS)), int(rng.choice(PROTOS)))
            _same_flow(t.AddFlow(*a, now), m.add_flow(*a, now))
        elif op < 6:
            a = (int(rng.choice(REMOTES)), int(rng.choice(REM_PORTS)), int(rng.choice(LAN_IPS)),
                 int(rng.choice(LAN_PORTS)), int(rng.choice(PROTOS)))
            _same_flow(t.GetFlowByHash(*a), m.get_lan(*a))
            w = (a[0], a[1], M.WAN_IP, int(rng.choice([32768, 32769, 32770, 32775])), a[4])
            _same_flow(t.GetFlowByWan(*w), m.get_wan(*w))
        elif op < 8:
            direction = int(rng.randint(0, 2))
            recs = _records(rng, 9, M.WAN_IP, direction)
            verd = rng.choice([M.V_MISS, M.V_MISS, M.V_FLOW, M.V_NONE], 9).astype(np.uint8)
            ops_t, ops_m = np.zeros(9, TX_OP_DTYPE), np.zeros(9, TX_OP_DTYPE)
            got = t.resolve_misses(direction, recs, verd, now, ops_t)
            want = m.resolve(direction, recs, verd, now, ops_m)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1]
            assert ops_t.tobytes() == ops_m.tobytes()
        elif op < 9:
            now = (now + int(rng.randint(1, 50))) & M.M32
        else:
            assert t.TableClear(now) == m.expire(now)
        _same_state(t, m)
    assert m.next_id > 50 and len(m.lan) != len(m.wan)  # the trace replaced LAN keys too


@pytest.mark.parametrize("nat_type", [M.SYMMETRIC, M.FULL_CONE])
def test_zero_ports_are_refused(nat_type):
    t = NatTable(M.WAN_IP, nat_type)
    assert t.AddFlow(LAN_IPS[0], REMOTES[0], 0, 53, 17, 1) is None
    assert t.AddFlow(LAN_IPS[0], REMOTES[0], 1000, 0, 17, 1) is None
    assert len(t.ListNat()) == 0
    fid = ctypes.c_uint32(0)
    assert _lib.lib.halo_nat_add_flow(t._t, LAN_IPS[0], REMOTES[0], 0, 53, 17, 1, None, ctypes.byref(fid)) == 0
    assert fid.value == _lib.NAT_NO_FLOW  # nil is data, not a call failure


def test_port_allocators_per_normalised_remote():
    sym, cone = NatTable(M.WAN_IP, M.SYMMETRIC), NatTable(M.WAN_IP, M.FULL_CONE)
    a = sym.AddFlow(LAN_IPS[0], REMOTES[0], 1000, 53, 17, 1)
    b = sym.AddFlow(LAN_IPS[0], REMOTES[1], 1000, 53, 17, 1)
    assert (a["wan_port"], b["wan_port"]) == (32768, 32768)  # one allocator per remote address
    assert (a["remote_ip"], b["remote_ip"]) == (REMOTES[0], REMOTES[1])
    a = cone.AddFlow(LAN_IPS[0], REMOTES[0], 1000, 53, 17, 1)
    b = cone.AddFlow(LAN_IPS[1], REMOTES[1], 1000, 53, 17, 1)
    assert (a["wan_port"], b["wan_port"]) == (32768, 32769)  # every remote normalises to 0
    assert (a["remote_ip"], a["remote_port"], b["remote_ip"]) == (0, 0, 0)


def test_port_exhaustion():
    """32768 flows of one allocator take 32768..65535 in order; the next NatAddFlow is nil."""
    t = NatTable(M.WAN_IP, M.FULL_CONE)
    L = _lib.lib
    out = np.zeros(1, _lib.NAT_FLOW_DTYPE)
    for k in range(32768):
        assert L.halo_nat_add_flow(t._t, 0x0A000000 + (k >> 15), REMOTES[0], 1 + (k & 0x7FFF), 53, 17, 7,
                                   out.ctypes.data, None) == 0
        assert out["wan_port"][0] == 32768 + k, k
    assert t.AddFlow(0x0A000009, REMOTES[0], 9, 53, 17, 7) is None
    assert len(t.ListNat()) == 32768
    # a freed port is the next one taken
    assert t.TableClear(7 + 61) == 32768 and len(t.ListNat()) == 0
    assert t.AddFlow(0x0A000009, REMOTES[0], 9, 53, 17, 100)["wan_port"] == 32768


def test_expire_frees_the_port_for_reuse():
    t = NatTable(M.WAN_IP, M.FULL_CONE)
    a = t.AddFlow(LAN_IPS[0], REMOTES[0], 1000, 53, 17, 10)
    b = t.AddFlow(LAN_IPS[1], REMOTES[0], 1000, 53, 17, 40)
    assert (a["wan_port"], b["wan_port"]) == (32768, 32769)
    assert t.TableClear(70) == 0      # 70 - 10 = 60 is not > 60
    assert t.TableClear(71) == 1      # a leaves, b stays
    assert [int(f["id"]) for f in t.ListNat()] == [int(b["id"])]
    assert t.GetFlowByWan(0, 0, M.WAN_IP, 32768, 17) is None
    c = t.AddFlow(LAN_IPS[2], REMOTES[0], 1000, 53, 17, 71)
    assert c["wan_port"] == 32768 and c["id"] == 2  # the port is reused, the id is not


def test_expire_just_past_the_uint32_wrap():
    t, m = NatTable(M.WAN_IP, M.SYMMETRIC), M.NatModel(M.WAN_IP, M.SYMMETRIC)
    for tb, add in ((t, t.AddFlow), (m, m.add_flow)):
        add(LAN_IPS[0], REMOTES[0], 1000, 53, 17, 0xFFFFFFF0)  # 16 ticks before the wrap
        add(LAN_IPS[1], REMOTES[0], 1000, 53, 17, 0xFFFFFFC0)  # 64 ticks before the wrap
        add(LAN_IPS[2], REMOTES[0], 1000, 53, 17, 5)           # "later" than now = 2: now - 5 wraps to huge
    assert t.TableClear(2) == m.expire(2) == 2  # ages 18 (stays), 66 (goes), 0xFFFFFFFD (goes)
    _same_state(t, m)
    assert [int(f["lan_ip"]) for f in t.ListNat()] == [LAN_IPS[0]]


@pytest.mark.parametrize("nat_type", [M.SYMMETRIC, M.FULL_CONE])
def test_icmp_key_has_remote_port_zero(nat_type):
    t = NatTable(M.WAN_IP, nat_type)
    f = t.AddFlow(LAN_IPS[0], REMOTES[0], 0x1234, 0x1234, 1, 1)  # NatGetSrcDstPort: the echo id twice
    assert f["remote_port"] == 0 and f["proto"] == 1
    # any remote port finds it, by either index
    assert t.GetFlowByHash(REMOTES[0], 0x9999, LAN_IPS[0], 0x1234, 1)["id"] == f["id"]
    assert t.GetFlowByWan(REMOTES[0], 0x7777, M.WAN_IP, int(f["wan_port"]), 1)["id"] == f["id"]


def test_port_mapping_first_match_and_no_icmp():
    t, m = NatTable(M.WAN_IP, M.SYMMETRIC), M.NatModel(M.WAN_IP, M.SYMMETRIC)
    for tb in (t, m):
        tb.add_port_mapping(8080, LAN_IPS[0], 80, 6)
        tb.add_port_mapping(8080, LAN_IPS[1], 81, 6)   # same WAN port: never reached inbound
        tb.add_port_mapping(8081, LAN_IPS[1], 81, 17)
    recs = np.zeros(4, RESULT_DTYPE)
    recs["src_ip"], recs["dst_ip"], recs["sport"] = REMOTES[0], M.WAN_IP, 5555
    recs["ip_proto"] = [6, 17, 1, 6]
    recs["dport"] = [8080, 8081, 8080, 8081]  # TCP 8080 -> entry 0; UDP 8081 -> entry 2; ICMP, TCP 8081 -> none
    verd = np.full(4, M.V_MISS, np.uint8)
    ops_t, ops_m = np.zeros(4, TX_OP_DTYPE), np.zeros(4, TX_OP_DTYPE)
    got, _ = t.resolve_misses(M.WAN, recs, verd, 1, ops_t)
    want, _ = m.resolve(M.WAN, recs, verd, 1, ops_m)
    assert list(got) == list(want) == [M.V_MAPPING, M.V_MAPPING, M.V_MISS, M.V_MISS]
    assert ops_t.tobytes() == ops_m.tobytes()
    assert (ops_t["dst_ip"][0], ops_t["dst_port"][0]) == (LAN_IPS[0], 80)
    # outbound: the second entry matches its own LAN host and restores the shared WAN port
    out = np.zeros(2, RESULT_DTYPE)
    out["src_ip"], out["sport"], out["dst_ip"], out["dport"] = LAN_IPS[1], 81, REMOTES[0], 5555
    out["ip_proto"] = [6, 1]
    ops_t, ops_m = np.zeros(2, TX_OP_DTYPE), np.zeros(2, TX_OP_DTYPE)
    got, added = t.resolve_misses(M.LAN, out, np.full(2, M.V_MISS, np.uint8), 1, ops_t)
    want, _ = m.resolve(M.LAN, out, np.full(2, M.V_MISS, np.uint8), 1, ops_m)
    assert list(got) == list(want) == [M.V_MAPPING, M.V_FLOW] and added == 1  # ICMP ignores mappings: a new flow
    assert ops_t.tobytes() == ops_m.tobytes()
    assert (ops_t["src_ip"][0], ops_t["src_port"][0]) == (M.WAN_IP, 8080)
    # the cap
    for k in range(253):
        t.add_port_mapping(9000 + k, LAN_IPS[0], 1, 6)
    assert _lib.lib.halo_nat_port_mapping_add(t._t, 1, 1, 1, 6) == _lib.HALO_E_RANGE


def test_resolve_misses_adds_once_in_ascending_order():
    t = NatTable(M.WAN_IP, M.FULL_CONE)
    recs = np.zeros(4, RESULT_DTYPE)
    recs["ip_proto"], recs["dst_ip"], recs["dport"] = 17, REMOTES[0], 53
    recs["src_ip"] = [LAN_IPS[1], LAN_IPS[0], LAN_IPS[1], LAN_IPS[2]]
    recs["sport"] = [1000, 1000, 1000, 0]  # records 0 and 2 are the same new flow; record 3 cannot be added
    ops = np.zeros(4, TX_OP_DTYPE)
    ops["steps"], ops["dst_ip"], ops["dst_port"] = _lib.TX_TTL, 0xDEADBEEF, 0xBEEF
    verd, added = t.resolve_misses(M.LAN, recs, np.full(4, M.V_MISS, np.uint8), 9, ops)
    assert added == 2 and list(verd) == [M.V_FLOW, M.V_FLOW, M.V_FLOW, M.V_DROP]
    assert ops[0].tobytes() == ops[2].tobytes()
    assert list(ops["src_port"]) == [32768, 32769, 32768, 0]  # ports follow packet order
    assert np.all(ops["steps"][:3] == _lib.TX_TTL | _lib.TX_NAT_SRC) and ops["steps"][3] == _lib.TX_TTL
    assert np.all(ops["dst_ip"] == 0xDEADBEEF) and np.all(ops["dst_port"] == 0xBEEF)  # not this direction's
    assert np.all(ops["src_ip"][:3] == M.WAN_IP)
    assert len(t.ListNat()) == 2 and np.all(t.ListNat()["last_alive"] == 9)


def test_list_with_a_short_cap_and_bad_arguments():
    t = NatTable(M.WAN_IP, M.SYMMETRIC)
    M.fill(t, M.NatModel(M.WAN_IP, M.SYMMETRIC), M.random_tuples(3, 10), 1)
    assert len(t.ListNat(cap=4)) == 4 and len(t.ListNat()) == 10
    L = _lib.lib
    assert L.halo_nat_table_create(None, None) == _lib.HALO_E_INVAL
    h = ctypes.c_void_p()
    assert L.halo_nat_table_create(ctypes.byref(_lib.NatConfig(1, 0, 29, 0)), ctypes.byref(h)) == _lib.HALO_E_RANGE
    assert L.halo_nat_list(t._t, None, 3, ctypes.byref(ctypes.c_uint32())) == _lib.HALO_E_INVAL
    assert L.halo_nat_expire(None, 0, None) == _lib.HALO_E_INVAL
    assert L.halo_nat_resolve_misses(t._t, 2, None, None, 0, 0, None, None, None) == _lib.HALO_E_INVAL
    # a lookup before any sync is refused before any device call
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    assert L.halo_nat_lookup_wan_device(t._t, p, 1, 0, None, p, p, p, p, None) == _lib.HALO_E_INVAL
    assert L.halo_nat_lookup_quote_device(t._t, p, 1, p, None) == _lib.HALO_E_INVAL


@pytest.mark.parametrize("nat_type", [M.SYMMETRIC, M.FULL_CONE])
def test_forced_fixture_exercises_collisions_and_wrap(nat_type):
    """The 16-slot / 12-flow table of tests/test_gpu_nat.py has, in both indexes, a probe chain of
    at least 3 slots and a chain that wraps past the last slot; a table that does not fit is
    HALO_E_RANGE."""
    t = NatTable(M.WAN_IP, nat_type, capacity_log2=M.FIXTURE_LOG2)
    tuples = M.random_tuples(M.FIXTURE_SEED[nat_type], 16)
    m = M.NatModel(M.WAN_IP, nat_type)
    M.fill(t, m, tuples[:M.FIXTURE_FLOWS], 100)
    s = t.layout_stats()
    assert s["slots"] == 16 and list(s["entries"]) == [12, 12]
    assert min(s["longest_chain"]) >= 3 and min(s["wrapped"]) >= 1, s
    M.fill(t, m, tuples[12:15], 100)  # 15 of 16: the chains still end
    assert t.layout_stats()["entries"][0] == 15
    t.AddFlow(*tuples[15], 100)
    with pytest.raises(_lib.HaloError) as e:
        t.layout_stats()
    assert e.value.code == _lib.HALO_E_RANGE
    auto = NatTable(M.WAN_IP, nat_type)
    M.fill(auto, M.NatModel(M.WAN_IP, nat_type), M.random_tuples(5, 100), 1)
    assert auto.layout_stats()["slots"] == 256  # load <= 0.5
