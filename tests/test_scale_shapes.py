"""CPU: what tests/test_gpu_scale.py rests on. The grid caps and scan widths of the .hip sources
still give the thresholds of tests/scale_cases.BOUNDARIES (so the GPU tests cannot silently stop
crossing the edge they exist for); the dict models answer a repeated item the same, which is what
lets a period's answer stand for millions of items; and the automatic ARP table of the scale test
is, on the host, the table the model describes."""
from __future__ import annotations

import numpy as np
import pytest

from tests import arp_cases as K
from tests import arp_model as AM
from tests import nat_model as NM
from tests import scale_cases as S

N_EQ = 3 * S.P + 17


def test_boundaries_follow_the_sources():
    c = S.read_constants()
    got = S.derived(c)
    assert set(got) == set(S.BOUNDARIES)
    for name, row in S.BOUNDARIES.items():
        assert got[name] == row["first_past"], (name, row["kernels"], got[name], row["first_past"], c)
        assert set(row["constants"]) <= set(c), name
        assert row["test"], name
    # one period must not line up with a wave: a case's lane shifts from repeat to repeat
    assert S.P % 64 and N_EQ % S.P


def test_tile_frames_layout():
    rng = np.random.default_rng(1)
    frames = [K.ipv4_frame(rng, int(n), 0x0A000005) for n in rng.integers(34, 120, 10)]
    data, offs, lens = K.pack(rng, frames)
    big, o, ln = S.tile_frames(data, offs, lens, 27)
    assert len(big) == 3 * len(data) and len(o) == len(ln) == 27
    for j in range(27):
        assert big[4 * int(o[j]):4 * int(o[j]) + int(ln[j])].tobytes() == frames[j % 10]
    want = data.copy()
    for k, f in enumerate(frames):
        want[4 * int(offs[k])] ^= 0xFF  # "the kernel" flips every frame's first byte
    exp = S.tile_frames_expected(data, want, offs, 27)
    ref = big.copy()
    ref[4 * o.astype(np.int64)] ^= 0xFF
    assert np.array_equal(exp, ref)
    assert np.array_equal(S.tile_frames_expected(data, want, offs, 20), np.tile(want, 2))


@pytest.fixture(scope="module")
def world(oracle_lib):
    """The forced ARP table (host only) with the route table of the device tests, the latter also in
    the C oracle: it stands in for the device's FindRoute here."""
    pair, keys = K.forced_table(lambda **kw: K.Pair(**kw))
    rt = K.world_routes(keys)
    o = oracle_lib.RouteTable()
    for what, r in K.world_route_ops(keys):
        (o.add if what == "add" else o.delete)(r)
    yield pair, keys, rt, o
    pair.close()
    rt.close()


def test_arp_lookup_tiling_equals_the_model(world):
    pair, keys, _, _ = world
    nifs, ips = K.lookup_mix(np.random.default_rng(5), keys, S.P)
    verdict, mac8 = S.arp_lookup_model(pair.m, nifs, ips)
    assert set(verdict.tolist()) == {AM.NONE, AM.OWN_IP, AM.MISS, AM.HIT}
    full_v, full_m = S.arp_lookup_model(pair.m, S.tiled(nifs, N_EQ), S.tiled(ips, N_EQ))
    assert np.array_equal(full_v, S.tiled(verdict, N_EQ)) and np.array_equal(full_m, S.tiled(mac8, N_EQ))


@pytest.mark.parametrize("in_netif", [0, 1])
def test_arp_encap_tiling_equals_the_model(world, in_netif):
    pair, keys, rt, o = world
    per = S.arp_encap_period(keys, o.find_batch)
    assert int(per["lens"].max()) == 1514 and int((per["lens"] == 1514).sum()) == 1
    res, want = S.arp_encap_model(pair.m, rt, per["frames"], per["rids"], per["select"], in_netif, per["data"], per["offs"])
    assert set(res["verdict"].tolist()) == set(range(7)) - ({AM.LOOPBACK} if in_netif else set())
    big, offs, lens = S.tile_frames(per["data"], per["offs"], per["lens"], N_EQ)
    idx = S.tile_index(N_EQ)
    frames = [per["frames"][k] for k in idx]
    full_res, full_want = S.arp_encap_model(pair.m, rt, frames, per["rids"][idx], per["select"][idx], in_netif, big, offs)
    assert np.array_equal(lens, per["lens"][idx])
    assert np.array_equal(full_res, res[idx])
    assert np.array_equal(full_want, S.tile_frames_expected(per["data"], want, per["offs"], N_EQ))


@pytest.mark.parametrize("direction", [NM.WAN, NM.LAN])
@pytest.mark.parametrize("name", ["forced_sym", "5000"])
def test_nat_tiling_equals_the_model(name, direction):
    """Verdicts, refs, ops and the LastAliveTime stamps (`now` is fixed within a call)."""
    nat_type, tuples, _, maps = S.nat_tables()[name]
    m1, m2 = S.nat_model(nat_type, tuples, maps), S.nat_model(nat_type, tuples, maps)
    per = S.nat_period(m1, direction, 130, seed=40 + direction)
    assert set(per["verdict"].tolist()) == {NM.V_NONE, NM.V_SKIP, NM.V_MISS, NM.V_FLOW, NM.V_MAPPING}
    ops = S.tiled(per["ops"], N_EQ)
    verdict, ref, miss = m2.lookup(direction, S.tiled(per["recs"], N_EQ), 130, ops, S.tiled(per["skip"], N_EQ))
    assert np.array_equal(verdict, S.tiled(per["verdict"], N_EQ)) and np.array_equal(ref, S.tiled(per["ref"], N_EQ))
    assert ops.tobytes() == S.tiled(per["want_ops"], N_EQ).tobytes()
    assert miss == int((S.tiled(per["verdict"], N_EQ) == NM.V_MISS).sum())
    assert NM.sorted_flows(m1.list()) == NM.sorted_flows(m2.list())
    assert 0 < sum(f["last_alive"] == 130 for f in m1.list()) <= len(tuples)


def test_arp_auto_table_on_the_host():
    """The automatic-slot-count table of test_gpu_scale.py: GetArpCache agrees with the model for
    every lookup of the device test, and the layout is one the forced 16-slot table cannot show."""
    pair, keys, nifs, ips = S.arp_auto_table(lambda **kw: K.Pair(**kw))
    try:
        st = pair.t.layout_stats()
        assert int(st["entries"]) == len(keys) >= 19_000 and int(st["slots"]) > 16 and int(st["longest_chain"]) >= 3
        verdict, mac8 = S.arp_lookup_model(pair.m, nifs, ips)
        counts = np.bincount(verdict, minlength=7)
        assert counts[AM.HIT] == len(keys) and min(counts[AM.NONE], counts[AM.OWN_IP], counts[AM.MISS]) >= len(keys) // 5
        for a, ip, v, m in zip(nifs.tolist(), ips.tolist(), verdict.tolist(), mac8):
            if a >= len(K.NETIFS):
                continue  # the host entry point takes a NetIf of the table only
            found, e = pair.t.GetArpCache(a, ip)
            assert found == {AM.HIT: AM.GET_FOUND, AM.MISS: AM.GET_ABSENT, AM.OWN_IP: AM.GET_OWN_IP}[v], (a, ip)
            if v == AM.HIT:
                assert bytes(e["mac"]) == bytes(m[:6])
    finally:
        pair.close()
