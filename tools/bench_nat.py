"""Measure the device NAT lookup (DESIGN.md "NAT flow table"): python tools/bench_nat.py [--flows N]
[--records N] [--runs K].

Data resident, HIP events around each launch, warm-up, then the median of K runs:
  (a) halo_nat_lookup_wan_device over N records against an N-flow table (every record hits)
  (b) the same over compact records
  (c) halo_route_lookup_records_device over the same records in the same run (the same
      gather-bound class: (a) is stated as a ratio to it)
  (d) the wall time of one halo_nat_sync_device at N flows
  (e) the host probe the lookup replaces, on one core over the same records: the C loop of
      halo_nat_resolve_misses(WAN) (probe + op write per record) and halo_nat_get_flow_wan called
      per record through ctypes on a subsample (the call overhead included)
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=int, default=1 << 20)
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch

    from halo_amd import _lib
    from halo_amd._lib import RESULT_DTYPE, TX_OP_DTYPE, compact_of
    from halo_amd.nat import NatTable
    from halo_amd.route import RouteTable, ip_u

    dev = torch.device("cuda:0")
    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    rng = np.random.default_rng(1)
    wan_ip = ip_u("203.0.113.1")
    t = NatTable(wan_ip, _lib.NAT_SYMMETRIC)
    # N distinct outbound packets through the slow path: one NatAddFlow each, in one C call
    out = np.zeros(a.flows, RESULT_DTYPE)
    out["ip_proto"] = rng.choice([6, 17], a.flows)
    out["src_ip"] = 0x0A000000 + np.arange(a.flows, dtype=np.uint32)
    out["sport"] = rng.integers(1024, 65536, a.flows)
    out["dst_ip"] = rng.integers(1 << 24, 0xDF000000, a.flows, dtype=np.uint64).astype(np.uint32)
    out["dport"] = rng.integers(1, 65536, a.flows)
    t0 = time.perf_counter()
    _, added = t.resolve_misses(_lib.FLOW_NAT_LAN, out, np.full(a.flows, _lib.NAT_V_MISS, np.uint8), 100,
                                np.zeros(a.flows, TX_OP_DTYPE))
    add_s = time.perf_counter() - t0
    assert added == a.flows
    t0 = time.perf_counter()
    t.sync()
    first_sync_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    t.sync()
    sync_s = time.perf_counter() - t0
    flows = t.ListNat()
    pick = rng.integers(0, len(flows), a.records)
    recs = np.zeros(a.records, RESULT_DTYPE)
    recs["ip_proto"], recs["src_ip"], recs["sport"] = flows["proto"][pick], flows["remote_ip"][pick], flows["remote_port"][pick]
    recs["dst_ip"], recs["dport"] = flows["wan_ip"][pick], flows["wan_port"][pick]
    d_full = torch.from_numpy(recs.view(np.uint8).reshape(-1, 32)).to(dev)
    d_comp = torch.from_numpy(compact_of(recs).view(np.uint8).reshape(-1, 16)).to(dev)
    d_ops = torch.zeros((a.records, 16), dtype=torch.uint8, device=dev)
    rt = RouteTable()
    rt.AddRoute(rt.entry(0, 0, ip_u("10.0.0.1"), 1))
    rt.AddRoute(rt.entry(ip_u("10.0.0.0"), ip_u("255.0.0.0"), 0, 2))
    rt.AddRoute(rt.entry(ip_u("203.0.113.0"), ip_u("255.255.255.128"), 0, 3))
    rt.sync()
    d_rid = torch.empty(a.records, dtype=torch.int32, device=dev)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    res = {}
    last = {}

    def wan_full():
        last["full"] = t.lookup_wan(d_full, 101, ops=d_ops)

    def wan_comp():
        last["comp"] = t.lookup_wan(d_comp, 101, ops=d_ops)

    res["a_wan_full_ms"] = timed(wan_full)
    res["b_wan_compact_ms"] = timed(wan_comp)
    res["c_route_records_ms"] = timed(lambda: rt.FindRouteRecords(d_full, out=d_rid))
    torch.cuda.synchronize()
    for k in ("full", "comp"):
        assert int((last[k][1] == _lib.NAT_V_FLOW).sum()) == a.records and int(last[k][3][0]) == 0
    res["a_over_c"] = res["a_wan_full_ms"][0] / res["c_route_records_ms"][0]
    res["a_mlookups_per_s"] = a.records / res["a_wan_full_ms"][0] / 1e3
    res["d_sync_wall_s"] = {"first": first_sync_s, "steady": sync_s, "host_add_flows_s": add_s}
    ops = np.zeros(a.records, TX_OP_DTYPE)
    t0 = time.perf_counter()
    verd, _ = t.resolve_misses(_lib.FLOW_NAT_WAN, recs, np.full(a.records, _lib.NAT_V_MISS, np.uint8), 101, ops)
    res["e_host_probe_c_loop_ms"] = (time.perf_counter() - t0) * 1e3
    assert np.all(verd == _lib.NAT_V_FLOW)
    sub = min(a.records, 100_000)
    f = _lib.lib.halo_nat_get_flow_wan
    src, sp, dst, dp, pr = (recs[k][:sub].tolist() for k in ("src_ip", "sport", "dst_ip", "dport", "ip_proto"))
    flow = np.zeros(1, _lib.NAT_FLOW_DTYPE)
    fp = flow.ctypes.data
    t0 = time.perf_counter()
    for i in range(sub):
        f(t._t, src[i], sp[i], dst[i], dp[i], pr[i], fp, None)
    res["e_host_get_flow_wan_ctypes_ns_per_record"] = (time.perf_counter() - t0) / sub * 1e9
    res["flows"], res["records"], res["runs"] = a.flows, a.records, a.runs
    res["layout"] = {k: np.asarray(t.layout_stats()[k]).tolist() for k in ("slots", "entries", "longest_chain", "wrapped")}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
