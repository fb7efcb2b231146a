"""Measure the ARP neighbour cache's device side: python tools/bench_arp.py
[--frames N] [--rounds K] [--warmup W] [--log PATH].

N frames of 64 B resident in HBM, every one routed directly out of NetIf 1:
  hit_1k / hit_1m     destinations drawn from 1,024 / 2^20 neighbours the table holds (all HIT)
  miss_1k / miss_1m   destinations the same tables do not hold (all MISS)
HIP events around each call. The four halo_arp_encap_device shapes, the neighbouring steps of the
chain over the same frames (halo_route_lookup_records_device, halo_tx_fixup_batch_device) and
halo_arp_gather_device with 0.1 % and 100 % ARP frames are timed in interleaved rounds — one call
of each per round — after warm-up rounds, and the median, minimum and maximum over the rounds are
reported, with Mpps, the bytes the L2 step must move per frame against the 8 TB/s HBM roofline, and
the host alternative the step replaces: halo_route_get + halo_arp_get per record in a C loop on
one core (tools/bench_arp_host.c). Prints one JSON line and, with --log, writes it there. Kernel
times come from a profiler run of their own: --profile runs ten calls of every line, untimed, under
rocprofv3 --kernel-trace --stats."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# Bytes per frame the L2 step needs, with 64-byte frames: the frame's first 64 B line read and (on a
# HIT) written back, 6 B of offset and length, the 4 B route id, one 8 B route entry, one 16 B slot
# and the 8 B result.
ALGO_BYTES_PER_FRAME = 64 + 64 + 6 + 4 + 8 + 16 + 8
HBM_BYTES_PER_S = 8e12
HIT_BASE, MISS_BASE = 0x0B000000, 0x0C000000  # 11.0.0.0/8 and 12.0.0.0/8, both direct out of NetIf 1


def host_lib():
    """tools/libhalo_arp_host.so, built from bench_arp_host.c against the product library."""
    out = os.path.join(ROOT, "tools", "libhalo_arp_host.so")
    src = os.path.join(ROOT, "tools", "bench_arp_host.c")
    libdir = os.path.join(ROOT, "halo_amd", "lib")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        subprocess.run(["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-I" + os.path.join(ROOT, "include"), src,
                        "-L" + libdir, "-lhalo_rx", "-Wl,-rpath," + libdir, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.bench_arp_fill.restype = ctypes.c_int
    lib.bench_arp_fill.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    lib.bench_arp_host_loop.restype = ctypes.c_uint32
    lib.bench_arp_host_loop.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                        ctypes.POINTER(ctypes.c_uint32)]
    return lib


def udp_frames(dst_ips: np.ndarray, own_mac: bytes) -> np.ndarray:
    """n x 64 B IPv4/UDP frames addressed to `own_mac`, valid up to the IPv4 header checksum."""
    n = len(dst_ips)
    f = np.zeros((n, 64), np.uint8)
    f[:, 0:6] = np.frombuffer(own_mac, np.uint8)
    f[:, 6:12] = [0x02, 0x77, 0, 0, 0, 1]
    f[:, 12:14] = [0x08, 0x00]
    f[:, 14:24] = [0x45, 0, 0, 50, 0, 1, 0x40, 0, 255, 17]  # total length 50, DF, TTL 255, UDP
    f[:, 26:30] = [10, 0, 0, 200]
    for b in range(4):
        f[:, 30 + b] = (dst_ips >> (8 * (3 - b))) & 0xFF
    f[:, 34:42] = [0x10, 0x00, 0x20, 0x00, 0, 30, 0, 0]  # ports 4096 -> 8192, length 30
    w = f[:, 14:34].astype(np.uint32)
    s = ((w[:, 0::2] << 8) | w[:, 1::2]).sum(axis=1)
    s = (s & 0xFFFF) + (s >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    c = (~s) & 0xFFFF
    f[:, 24], f[:, 25] = c >> 8, c & 0xFF
    return f


def arp_frames(n: int, own_mac: bytes) -> np.ndarray:
    f = np.zeros((n, 64), np.uint8)
    f[:, 0:6] = np.frombuffer(own_mac, np.uint8)
    f[:, 6:12] = [0x02, 0x77, 0, 0, 0, 2]
    f[:, 12:22] = [0x08, 0x06, 0, 1, 8, 0, 6, 4, 0, 1]
    f[:, 22:28] = [0x02, 0x77, 0, 0, 0, 2]
    f[:, 28:32] = [10, 0, 0, 9]
    f[:, 38:42] = [10, 0, 0, 1]
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=5, help="timed host loops per shape")
    ap.add_argument("--log", default=None, help="also write the JSON line to this file")
    ap.add_argument("--profile", action="store_true",
                    help="run ten calls of everything, untimed, and exit (under rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    import torch

    from halo_amd import _lib, protocol
    from halo_amd._lib import ARP_V, NetIf, TX_RECALC, TX_TTL
    from halo_amd.arp import ArpTable
    from halo_amd.route import RouteTable

    assert torch.cuda.is_available(), "bench_arp needs a GPU"
    dev = torch.device("cuda:0")
    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    H = host_lib()
    n = a.frames
    rng = np.random.default_rng(1)
    netifs = [NetIf.make("02:00:00:00:00:01", "10.0.0.1"), NetIf.make("02:00:00:00:00:02", "10.1.0.1")]
    own_mac = bytes(netifs[0].mac)
    rt = RouteTable(0)
    rt.AddRoute(RouteTable.entry(HIT_BASE, 0xFF000000, 0, 1))
    rt.AddRoute(RouteTable.entry(MISS_BASE, 0xFF000000, 0, 1))
    rt.sync()
    d_offs = torch.from_numpy((np.arange(n, dtype=np.uint32) * 16).view(np.int32)).to(dev)
    d_lens = torch.from_numpy(np.full(n, 64, np.uint16).view(np.int16)).to(dev)
    tables = {}
    for tag, neighbours in (("1k", 1024), ("1m", 1 << 20)):
        t = ArpTable(netifs, neighbours)
        _lib.check("bench_arp_fill", H.bench_arp_fill(t._t, 1, HIT_BASE, neighbours, 100))
        t.sync(rt)
        tables[tag] = (t, neighbours)
    shapes = {}
    for name, tag, base in (("hit_1k", "1k", HIT_BASE), ("miss_1k", "1k", MISS_BASE), ("hit_1m", "1m", HIT_BASE),
                            ("miss_1m", "1m", MISS_BASE)):
        t, neighbours = tables[tag]
        dst = (base + rng.integers(0, neighbours, n)).astype(np.uint32)
        d_bytes = torch.from_numpy(udp_frames(dst, own_mac).ravel()).to(dev)
        recs = protocol.parse_frames_batch(d_bytes, d_offs, d_lens, netif=netifs[0], max_len_hint=64)
        rids = rt.FindRouteRecords(recs)
        shapes[name] = dict(t=t, dst=dst, d_bytes=d_bytes, recs=recs, rids=rids,
                            res=torch.empty((n, 8), dtype=torch.uint8, device=dev),
                            counts=torch.zeros(7, dtype=torch.int32, device=dev),
                            miss=torch.zeros(1, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream

    def encap(name):  # the C entry point with preallocated outputs: no allocation inside the timed region
        s = shapes[name]
        _lib.check("halo_arp_encap_device", _lib.lib.halo_arp_encap_device(
            s["t"]._t, _lib.ptr(s["d_bytes"]), _lib.ptr(d_offs), _lib.ptr(d_lens), n, _lib.ptr(s["rids"]), 0, None,
            _lib.ptr(s["res"]), _lib.ptr(s["counts"]), _lib.ptr(s["miss"]), stream))

    s0 = shapes["hit_1k"]
    rid_out = torch.empty(n, dtype=torch.int32, device=dev)
    d_ops = torch.from_numpy(protocol.tx_ops(n, TX_TTL | TX_RECALC).view(np.uint8).reshape(n, 16)).to(dev)
    d_res = torch.empty(n, dtype=torch.uint8, device=dev)
    gathers = {}
    for name, every in (("gather_0.1pct", 1000), ("gather_100pct", 1)):
        arr = udp_frames(s0["dst"], own_mac)
        arr[::every] = arp_frames(len(arr[::every]), own_mac)
        g_bytes = torch.from_numpy(arr.ravel()).to(dev)
        g_recs = protocol.parse_frames_batch(g_bytes, d_offs, d_lens, netif=netifs[0], max_len_hint=64)
        wsb = int(_lib.lib.halo_arp_gather_workspace(n))
        gathers[name] = dict(d_bytes=g_bytes, recs=g_recs, want=len(arr[::every]), wsb=wsb,
                             msgs=torch.empty((n, 40), dtype=torch.uint8, device=dev),
                             count=torch.zeros(1, dtype=torch.int32, device=dev),
                             ws=torch.empty(wsb // 4, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()

    def gather(name):  # the C entry point with preallocated outputs: no allocation inside the timed region
        g = gathers[name]
        _lib.check("halo_arp_gather_device", _lib.lib.halo_arp_gather_device(
            _lib.ptr(g["d_bytes"]), _lib.ptr(d_offs), _lib.ptr(d_lens), _lib.ptr(g["recs"]), n, 0, _lib.ptr(g["msgs"]), n,
            _lib.ptr(g["count"]), _lib.ptr(g["ws"]), g["wsb"], torch.cuda.current_stream().cuda_stream))

    fns = {**{k: (lambda k=k: encap(k)) for k in shapes},
           "route_lookup_records": lambda: rt.FindRouteRecords(s0["recs"], out=rid_out),
           "tx_fixup": lambda: protocol.tx_fixup_batch(s0["d_bytes"], d_offs, d_lens, d_ops, max_len_hint=64, result=d_res),
           **{k: (lambda k=k: gather(k)) for k in gathers}}
    if a.profile:  # for a kernel trace: ten untimed calls of everything
        for _ in range(10):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        print(json.dumps({"profiled": list(fns), "calls": 10}))
        return
    for _ in range(a.warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(a.rounds):  # interleaved: one call of each per round
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    res = {"frames": n, "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for k, v in ms.items():
        med = float(np.median(v))
        res[k] = {"us_median": med * 1e3, "us_min": float(min(v)) * 1e3, "us_max": float(max(v)) * 1e3, "mpps": n / med / 1e3}
    for k, s in shapes.items():
        res[k]["ratio_to_route_lookup"] = res[k]["us_median"] / res["route_lookup_records"]["us_median"]
        res[k]["ratio_to_tx_fixup"] = res[k]["us_median"] / res["tx_fixup"]["us_median"]
        res[k]["algo_bytes_per_frame"] = ALGO_BYTES_PER_FRAME
        res[k]["roofline_us"] = n * ALGO_BYTES_PER_FRAME / HBM_BYTES_PER_S * 1e6
        res[k]["share_of_hbm_roofline"] = res[k]["roofline_us"] / res[k]["us_median"]
        v = s["res"].cpu().numpy()[:, 0]
        res[k]["verdicts"] = {name: int((v == code).sum()) for name, code in ARP_V.items() if (v == code).any()}
        assert res[k]["verdicts"] == {"HIT" if k.startswith("hit") else "MISS": n}, res[k]["verdicts"]
        res[k]["layout"] = {f: int(s["t"].layout_stats()[f]) for f in ("slots", "entries", "longest_chain", "wrapped")}
    for k, g in gathers.items():
        res[k]["arp_frames"] = int(g["count"].cpu()[0])
        assert res[k]["arp_frames"] == g["want"]
    # the host alternative: one core, a C loop of halo_route_get + halo_arp_get per record
    for k, s in shapes.items():
        rids = np.ascontiguousarray(s["rids"].cpu().numpy().view(np.uint32))
        sink = ctypes.c_uint32()
        dts = []
        for _ in range(a.host_rounds):
            t0 = time.perf_counter()
            hits = H.bench_arp_host_loop(s["t"]._t, rt._t, rids.ctypes.data, s["dst"].ctypes.data, n, ctypes.byref(sink))
            dts.append(time.perf_counter() - t0)
        assert hits == (n if k.startswith("hit") else 0)
        dt = float(np.median(dts))
        res[k]["host_one_core_us"] = {"median": dt * 1e6, "min": min(dts) * 1e6, "max": max(dts) * 1e6, "rounds": a.host_rounds}
        res[k]["host_mpps"] = n / dt / 1e6
        res[k]["speedup_over_host"] = dt * 1e6 / res[k]["us_median"]
    line = json.dumps(res)
    print(line)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
