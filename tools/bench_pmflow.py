"""Measure the port-mapping return-flow calls (DESIGN.md "Port-mapping return flows"):
python tools/bench_pmflow.py [--flows N] [--records N] [--rounds K] [--warmup W] [--dry].

One MI355X, data resident, HIP events around each C entry point with preallocated outputs, W warm-up
rounds, then K interleaved rounds with one call of each line per round; median (min - max) in µs.
  lookup   halo_pmflow_lookup_device beside halo_nat_lookup_lan_device over the same records and a
           table of the same size, all hits and all misses
  record   halo_pmflow_record_device at 0 %, 0.1 % and 100 % candidates (first packets: none known)
           beside halo_arp_gather_device at the same fractions of ARP frames
  encap    halo_arp_encap_via_device with d_via == NULL and with a via array without an OVERRIDE,
           beside halo_arp_encap_device on the same batch, the order rotated every round
  replaces the D2H copy of the records, halo_pmflow_get per record on one core (ctypes, a
           subsample), the H2D copy of the ops: what the lookup call replaces
--dry builds the host side at a small size and stops before the first device call.
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes
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
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    if a.dry:
        a.flows = a.records = 4096

    from halo_amd import _lib
    from halo_amd._lib import (ARP_RESULT_DTYPE, NAT_V_MAPPING, NAT_V_MISS, PMFLOW_ITEM_DTYPE, PMFLOW_VIA_DTYPE, RESULT_DTYPE,
                               TX_OP_DTYPE, NetIf)
    from halo_amd.arp import ArpTable
    from halo_amd.nat import NatTable
    from halo_amd.pmflow import PortMappingFlowTable
    from halo_amd.route import RouteTable, ip_u

    L = _lib.lib
    rng = np.random.default_rng(1)
    nf, n = a.flows, a.records
    netifs = [NetIf.make("02:00:00:00:00:01", "192.168.1.1", False), NetIf.make("02:00:00:00:00:02", "203.0.113.1", True),
              NetIf.make("02:00:00:00:00:03", "198.51.100.1", True)]
    gateways = [0, ip_u("203.0.113.254"), ip_u("198.51.100.254")]
    # nf distinct (LAN host, remote) pairs: the NAT table learns them as outbound flows of WAN1, the
    # return-flow table as connections that came in on WAN2 — the same key in both
    lan_ip = (0x0A000000 + np.arange(nf, dtype=np.uint32))
    lan_port = rng.integers(1024, 65536, nf).astype(np.uint16)
    rip = rng.integers(1 << 24, 0xDF000000, nf, dtype=np.uint64).astype(np.uint32)
    rport = rng.integers(1, 65536, nf).astype(np.uint16)
    proto = rng.choice([6, 17], nf).astype(np.uint8)
    out = np.zeros(nf, RESULT_DTYPE)
    out["ip_proto"], out["src_ip"], out["sport"], out["dst_ip"], out["dport"] = proto, lan_ip, lan_port, rip, rport
    nat = NatTable(netifs[1].ip, _lib.NAT_SYMMETRIC)
    _, added = nat.resolve_misses(_lib.FLOW_NAT_LAN, out, np.full(nf, NAT_V_MISS, np.uint8), 100, np.zeros(nf, TX_OP_DTYPE))
    assert added == nf
    pm = PortMappingFlowTable(netifs, gateways, nf)
    items = np.zeros(nf, PMFLOW_ITEM_DTYPE)
    items["index"], items["remote_ip"], items["lan_ip"] = np.arange(nf), rip, lan_ip
    items["remote_port"], items["lan_port"], items["wan_port"], items["proto"] = rport, lan_port, 8080, proto
    t0 = time.perf_counter()
    dropped, added = pm.record(2, items, 100)
    record_host_s = time.perf_counter() - t0
    assert added == nf and not dropped.any()
    pick = rng.integers(0, nf, n)
    hit = out[pick].copy()
    miss = hit.copy()
    miss["sport"] ^= 1  # one key field off: absent from both tables
    # the WAN-side batch: first packets from new remotes to the mapped port
    first = np.zeros(n, RESULT_DTYPE)
    first["ip_proto"], first["src_ip"], first["sport"] = 6, rng.integers(1 << 24, 0xDF000000, n, dtype=np.uint64), 4000
    first["dst_ip"], first["dport"] = netifs[2].ip, 8080
    wan_ops = np.zeros(n, TX_OP_DTYPE)
    wan_ops["steps"], wan_ops["dst_ip"], wan_ops["dst_port"] = 0x03, ip_u("192.168.1.20"), 80
    arp_hit = np.zeros(n, ARP_RESULT_DTYPE)
    arp_hit["verdict"], arp_hit["out_netif"], arp_hit["tx_len"] = 6, 0, 64
    fracs = {"0": 0, "0.1": max(1, n // 1000), "100": n}

    def marked(k):
        m = np.zeros(n, bool)
        m[rng.choice(n, k, replace=False)] = True
        return m

    wv = {f: np.where(marked(k), NAT_V_MAPPING, NAT_V_MISS).astype(np.uint8) for f, k in fracs.items()}
    arp_recs = {}
    for f, k in fracs.items():
        r = np.zeros(n, RESULT_DTYPE)
        r["ethertype"], r["flags"] = 0x0800, 1
        r["ethertype"][marked(k)] = 0x0806
        arp_recs[f] = r
    # 64-byte IPv4 frames to 1,024 known neighbours of NetIf 1, packed
    neigh = ip_u("203.0.113.0") + 2 + (np.arange(1024, dtype=np.uint32) % 250)
    neigh = np.unique(neigh)
    frames = np.zeros((n, 64), np.uint8)
    frames[:, 12], frames[:, 13] = 0x08, 0x00
    dst = neigh[rng.integers(0, len(neigh), n)]
    for b in range(4):
        frames[:, 30 + b] = (dst >> (24 - 8 * b)) & 0xFF
    if a.dry:
        print(json.dumps({"dry": True, "flows": nf, "records": n, "layout": [int(x) for x in pm.layout_stats()]}))
        return

    import torch

    dev = torch.device("cuda:0")
    _lib.check("halo_rx_init", L.halo_rx_init(0))
    rt = RouteTable()
    rt.AddRoute(rt.entry(0, 0, gateways[1], 1))
    rt.AddRoute(rt.entry(ip_u("203.0.113.0"), ip_u("255.255.255.0"), 0, 1))
    rt.AddRoute(rt.entry(ip_u("192.168.1.0"), ip_u("255.255.255.0"), 0, 0))
    rt.sync()
    arp = ArpTable(netifs, 2048)
    for k, ip in enumerate(neigh):
        arp.SetArpCache(1, int(ip), bytes([2, 0x5A, 0, 0, k >> 8, k & 255]), 10)
    arp.sync(rt)
    nat.sync()
    t0 = time.perf_counter()
    pm.sync(rt)
    sync_s = time.perf_counter() - t0
    up = lambda x, w: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1, w)).to(dev)  # noqa: E731
    d_hit, d_miss, d_first = up(hit, 32), up(miss, 32), up(first, 32)
    d_rids = rt.FindRouteRecords(d_hit)
    d_ops = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
    d_via = torch.empty((n, 8), dtype=torch.uint8, device=dev)
    d_hitb = torch.empty(n, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(4, dtype=torch.int32, device=dev)
    d_verd = torch.empty(n, dtype=torch.uint8, device=dev)
    d_ref = torch.empty(n, dtype=torch.int32, device=dev)
    d_nmiss = torch.zeros(1, dtype=torch.int32, device=dev)
    d_wv = {f: torch.from_numpy(v).to(dev) for f, v in wv.items()}
    d_wops, d_arp = up(wan_ops, 16), up(arp_hit, 8)
    d_items = torch.empty((n, 20), dtype=torch.uint8, device=dev)
    d_count = torch.zeros(1, dtype=torch.int32, device=dev)
    wsb = int(L.halo_pmflow_record_workspace(n))
    d_ws = torch.empty(wsb // 4 + 1, dtype=torch.int32, device=dev)
    d_arecs = {f: up(r, 32) for f, r in arp_recs.items()}
    d_frames = torch.from_numpy(frames).to(dev).reshape(-1)
    d_offs = (torch.arange(n, dtype=torch.int32, device=dev) * 16).contiguous()
    d_lens = torch.full((n,), 64, dtype=torch.int16, device=dev)
    d_msgs = torch.empty((n, 40), dtype=torch.uint8, device=dev)
    gwsb = int(L.halo_arp_gather_workspace(n))
    d_gws = torch.empty(gwsb // 4 + 1, dtype=torch.int32, device=dev)
    d_erids = rt.FindRoute(torch.from_numpy(dst.view(np.int32)).to(dev))
    d_res = torch.empty((n, 8), dtype=torch.uint8, device=dev)
    d_ecnt = torch.zeros(7, dtype=torch.int32, device=dev)
    d_emiss = torch.zeros(1, dtype=torch.int32, device=dev)
    via_plain = np.zeros(n, PMFLOW_VIA_DTYPE)
    via_plain["verdict"], via_plain["wan_netif"] = 1, 0xFF  # all MISS: the via kernel, no override taken
    d_vplain = up(via_plain, 8)
    s = torch.cuda.current_stream().cuda_stream
    P = _lib.ptr

    def pm_lookup(recs, counts=True):
        return lambda: L.halo_pmflow_lookup_device(pm._t, P(recs), n, 101, P(d_rids), None, P(d_ops), P(d_via), P(d_hitb),
                                                   P(d_cnt) if counts else None, s)

    def nat_lookup(recs):
        return lambda: L.halo_nat_lookup_lan_device(nat._t, P(recs), n, 101, None, P(d_ops), P(d_verd), P(d_ref), P(d_nmiss), s)

    def record(f):
        return lambda: L.halo_pmflow_record_device(pm._t, 2, P(d_first), P(d_wv[f]), P(d_wops), P(d_arp), n, 101, P(d_items), n,
                                                   P(d_count), P(d_ws), wsb, s)

    def gather(f):
        return lambda: L.halo_arp_gather_device(P(d_frames), P(d_offs), P(d_lens), P(d_arecs[f]), n, 1, P(d_msgs), n, P(d_count),
                                                P(d_gws), gwsb, s)

    def encap(via):
        if via == "plain":
            return lambda: L.halo_arp_encap_device(arp._t, P(d_frames), P(d_offs), P(d_lens), n, P(d_erids), 0, None, P(d_res),
                                                   P(d_ecnt), P(d_emiss), s)
        v = None if via == "null" else P(d_vplain)
        return lambda: L.halo_arp_encap_via_device(arp._t, P(d_frames), P(d_offs), P(d_lens), n, P(d_erids), 0, None, v,
                                                   P(d_res), P(d_ecnt), P(d_emiss), s)

    lines = {"lookup_hit": pm_lookup(d_hit), "nat_lan_hit": nat_lookup(d_hit), "lookup_miss": pm_lookup(d_miss),
             "nat_lan_miss": nat_lookup(d_miss), "lookup_hit_no_counts": pm_lookup(d_hit, False),
             "lookup_miss_no_counts": pm_lookup(d_miss, False)}
    for f in fracs:
        lines[f"record_{f}"] = record(f)
        lines[f"gather_{f}"] = gather(f)
    enc = {"encap": encap("plain"), "encap_via_null": encap("null"), "encap_via_array": encap("array")}
    us = {k: [] for k in list(lines) + list(enc)}

    def one(name, fn, keep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn()
        e1.record()
        e1.synchronize()
        assert rc == 0, (name, rc)
        if keep:
            us[name].append(e0.elapsed_time(e1) * 1e3)

    for rnd in range(a.warmup + a.rounds):
        keep = rnd >= a.warmup
        for name, fn in lines.items():
            one(name, fn, keep)
        names = list(enc)
        for j in range(3):  # the order of the three encap lines rotates every round
            name = names[(j + rnd) % 3]
            one(name, enc[name], keep)
    torch.cuda.synchronize()
    # what was computed, checked once after the timed rounds
    pm_lookup(d_hit)()
    torch.cuda.synchronize()
    assert int((d_via[:, 0] >= 2).sum()) == n and int(d_hitb.sum()) == n
    pm_lookup(d_miss)()
    torch.cuda.synchronize()
    assert int((d_via[:, 0] == 1).sum()) == n
    for f, k in fracs.items():
        record(f)()
        torch.cuda.synchronize()
        assert int(d_count[0]) == k, (f, int(d_count[0]))
    assert int((d_res[:, 0] == 6).sum()) == n  # every encap line ended with all HIT

    stat = lambda v: [round(float(np.median(v)), 1), round(float(min(v)), 1), round(float(max(v)), 1)]  # noqa: E731
    res = {"us_median_min_max": {k: stat(v) for k, v in us.items()}}
    med = {k: float(np.median(v)) for k, v in us.items()}
    res["ratios"] = {"lookup_hit_over_nat_lan_hit": round(med["lookup_hit"] / med["nat_lan_hit"], 3),
                     "lookup_miss_over_nat_lan_miss": round(med["lookup_miss"] / med["nat_lan_miss"], 3),
                     **{f"record_over_gather_{f}": round(med[f"record_{f}"] / med[f"gather_{f}"], 3) for f in fracs},
                     "encap_via_null_over_encap": round(med["encap_via_null"] / med["encap"], 3),
                     "encap_via_array_over_encap": round(med["encap_via_array"] / med["encap"], 3)}
    # bytes per record at 8 TB/s. lookup: 32 B record + 4 B route id + 32 B slot + 4 B stamp + 16 B op
    # read and written + 8 B via + 1 B hit (+ 16 B NetIf word, cached); a miss: no stamp, no op
    res["bound_us_at_8TBps"] = {"lookup_hit": round(n * (32 + 4 + 32 + 4 + 32 + 8 + 1) / 8e6, 1),
                                "lookup_miss": round(n * (32 + 4 + 32 + 8 + 1) / 8e6, 1),
                                "record_0": round(n * (1 + 8 + 1 + 1) / 8e6, 1),
                                "record_100": round(n * (1 + 8 + 32 + 16 + 32 + 1 + 1 + 32 + 16 + 20) / 8e6, 1)}
    # what the lookup replaces, on the host clock
    pinned = torch.empty((n, 32), dtype=torch.uint8).pin_memory()
    ops_host = torch.zeros((n, 16), dtype=torch.uint8).pin_memory()
    rep = {"d2h_records_us": [], "h2d_ops_us": []}
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pinned.copy_(d_hit)
        torch.cuda.synchronize()
        rep["d2h_records_us"].append((time.perf_counter() - t0) * 1e6)
        t0 = time.perf_counter()
        d_ops.copy_(ops_host)
        torch.cuda.synchronize()
        rep["h2d_ops_us"].append((time.perf_counter() - t0) * 1e6)
    sub = min(n, 100_000)
    f = L.halo_pmflow_get
    cols = [hit[k][:sub].tolist() for k in ("dst_ip", "dport", "src_ip", "sport", "ip_proto")]
    e = np.zeros(1, _lib.PMFLOW_ENTRY_DTYPE)
    found, now = ctypes.c_uint32(), ctypes.c_uint32(101)
    ep, fp, npn = e.ctypes.data, ctypes.byref(found), ctypes.byref(now)
    t0 = time.perf_counter()
    hits = 0
    for i in range(sub):
        f(pm._t, cols[0][i], cols[1][i], cols[2][i], cols[3][i], cols[4][i], npn, ep, fp)
        hits += found.value
    per = (time.perf_counter() - t0) / sub
    assert hits == sub
    res["replaces"] = {"d2h_records_us": round(float(np.median(rep["d2h_records_us"])), 1),
                       "host_get_ns_per_record_ctypes": round(per * 1e9, 1), "host_get_subsample": sub,
                       "host_get_us_for_all_records": round(per * n * 1e6, 1),
                       "h2d_ops_us": round(float(np.median(rep["h2d_ops_us"])), 1)}
    res["host"] = {"record_all_flows_s": round(record_host_s, 3), "sync_wall_s": round(sync_s, 3)}
    res["flows"], res["records"], res["rounds"], res["warmup"] = nf, n, a.rounds, a.warmup
    res["layout"] = {k: int(pm.layout_stats()[k]) for k in ("slots", "entries", "longest_chain", "wrapped")}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
