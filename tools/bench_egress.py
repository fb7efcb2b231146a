"""Measure the egress step: python tools/bench_egress.py [--frames N] [--rounds K]
[--warmup W] [--log PATH] [--profile].

Frames resident in HBM, back to back, with preallocated outputs:
  arp_1 / arp_4 / arp_64   N x 64 B, ARP kind, every frame a HIT, spread over 1 / 4 / 64 ports
  switch_flood3            N x 64 B, switch kind, every frame a FLOOD to 3 ports of 4
  big_1                    N / 4 x 1500 B, ARP kind, one port
HIP events around each C entry point. In the same interleaved rounds — one call of each line per
round, after warm-up rounds — a hipMemcpyAsync device-to-device copy of exactly each line's output
bytes (copy_<line>) and halo_arp_encap_device over the same 64 B frames (arp_encap). The median with
minimum and maximum over the rounds is reported, with the ratio to the copy line and to the bound
computed from shapes: per frame its bytes read, 6 B of offset and length, the result, the record
written and 4 B of index, at 8 TB/s. Separately: halo_tx_egress_host on one core, and the device
call, over a ladder of batch sizes (the crossing of the two lines is reported). Prints one JSON line
and, with --log, writes it there. --profile runs ten untimed calls of every egress line and exits,
for a rocprofv3 --kernel-trace --stats run of its own."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
HIT_BASE = 0x0B000000  # 11.0.0.0/8, direct out of NetIf 1
LADDER = [64, 256, 1024, 4096, 16384, 65536]


def hip_memcpy_async():
    """hipMemcpyAsync of the HIP runtime this process already has (halo_amd._lib loaded it)."""
    with open("/proc/self/maps") as fh:  # the copy that is mapped, not a second one
        paths = sorted({ln.split()[-1] for ln in fh if "libamdhip64" in ln})
    assert len(paths) == 1, paths
    fn = ctypes.CDLL(paths[0]).hipMemcpyAsync
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=5)
    ap.add_argument("--log", default=None, help="also write the JSON line to this file")
    ap.add_argument("--profile", action="store_true",
                    help="run ten calls of every egress line, untimed, and exit (under rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    import torch

    from halo_amd import _lib
    from halo_amd import egress as E
    from halo_amd._lib import ARP_RESULT_DTYPE, ARP_V, SW_RESULT_DTYPE, SW_V, NetIf
    from halo_amd.arp import ArpTable
    from halo_amd.route import RouteTable
    from tools.bench_arp import udp_frames

    assert torch.cuda.is_available(), "bench_egress needs a GPU"
    dev = torch.device("cuda:0")
    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    L = _lib.lib
    n = a.frames
    rng = np.random.default_rng(1)
    stream = torch.cuda.current_stream().cuda_stream
    memcpy = hip_memcpy_async()

    # the 64 B frames: IPv4/UDP to 1,024 neighbours NetIf 1 holds, so that the encap line is all HIT
    netifs = [NetIf.make("02:00:00:00:00:01", "10.0.0.1"), NetIf.make("02:00:00:00:00:02", "10.1.0.1")]
    rt = RouteTable(0)
    rt.AddRoute(RouteTable.entry(HIT_BASE, 0xFF000000, 0, 1))
    rt.sync()
    table = ArpTable(netifs, 1024)
    for k in range(1024):
        table.SetArpCache(1, HIT_BASE + k, bytes([2, 0x5A, 0, 0, k >> 8, k & 255]), 100)
    table.sync(rt)
    dst = (HIT_BASE + rng.integers(0, 1024, n)).astype(np.uint32)
    small = udp_frames(dst, bytes(netifs[0].mac))
    d_small = torch.from_numpy(small.ravel()).to(dev)
    d_offs = torch.from_numpy((np.arange(n, dtype=np.uint32) * 16).view(np.int32)).to(dev)
    d_lens = torch.from_numpy(np.full(n, 64, np.uint16).view(np.int16)).to(dev)
    rids = rt.FindRoute(torch.from_numpy(dst.view(np.int32)).to(dev))
    enc_res = torch.empty((n, 8), dtype=torch.uint8, device=dev)
    enc_counts = torch.zeros(7, dtype=torch.int32, device=dev)
    enc_miss = torch.zeros(1, dtype=torch.int32, device=dev)
    nb = n // 4
    d_big = torch.from_numpy(rng.integers(0, 256, nb * 1500, dtype=np.uint8)).to(dev)
    d_big_offs = torch.from_numpy((np.arange(nb, dtype=np.uint32) * 375).view(np.int32)).to(dev)
    d_big_lens = torch.from_numpy(np.full(nb, 1500, np.uint16).view(np.int16)).to(dev)

    def arp_results(count, ports):
        r = np.zeros(count, ARP_RESULT_DTYPE)
        r["verdict"], r["tx_len"] = ARP_V["HIT"], 64
        r["out_netif"] = rng.integers(0, ports, count)
        return r

    lines = {}

    def add(name, kind, frames, offs, lens, count, length, sel_host, ports, flood=0):
        rec = E.record_size(length)
        per_port = np.bincount(sel_host["out_netif"], minlength=ports) if kind == E.EGRESS_KIND_ARP else None
        most = int(per_port.max()) if per_port is not None else count
        region = (most * rec + 15) & ~15
        copies = count * (bin(flood).count("1") if kind == E.EGRESS_KIND_SWITCH else 1)
        cfg = _lib.EgressConfig()
        cfg.n_ports, cfg.flags, cfg.region_bytes, cfg.index_cap = ports, 0, region, most
        wsb = E.workspace_bytes(count, ports)
        sel_bytes = sel_host.view(np.uint8).reshape(count, -1)
        lines[name] = dict(
            kind=kind, cfg=cfg, frames=frames, offs=offs, lens=lens, n=count, ports=ports, flood=flood, wsb=wsb,
            sel=torch.from_numpy(sel_bytes).to(dev), out=torch.empty(ports * region, dtype=torch.uint8, device=dev),
            summary=torch.empty((ports, 24), dtype=torch.uint8, device=dev),
            index=torch.empty((ports, most), dtype=torch.int32, device=dev),
            skipped=torch.zeros(1, dtype=torch.int32, device=dev), ws=torch.empty(wsb // 8, dtype=torch.int64, device=dev),
            out_bytes=copies * rec, records=copies,
            bound_bytes=count * (length + 6 + sel_host.dtype.itemsize) + copies * (rec + 4),
            copy_src=torch.empty(copies * rec, dtype=torch.uint8, device=dev),
            copy_dst=torch.empty(copies * rec, dtype=torch.uint8, device=dev))

    add("arp_1", E.EGRESS_KIND_ARP, d_small, d_offs, d_lens, n, 64, arp_results(n, 1), 1)
    add("arp_4", E.EGRESS_KIND_ARP, d_small, d_offs, d_lens, n, 64, arp_results(n, 4), 4)
    add("arp_64", E.EGRESS_KIND_ARP, d_small, d_offs, d_lens, n, 64, arp_results(n, 64), 64)
    sw = np.zeros(n, SW_RESULT_DTYPE)
    sw["verdict"], sw["out_port"], sw["tx_len"] = SW_V["FLOOD"], 0xFF, 64
    add("switch_flood3", E.EGRESS_KIND_SWITCH, d_small, d_offs, d_lens, n, 64, sw, 4, flood=0b1110)
    big_res = arp_results(nb, 1)
    big_res["tx_len"] = 1500
    add("big_1", E.EGRESS_KIND_ARP, d_big, d_big_offs, d_big_lens, nb, 1500, big_res, 1)
    torch.cuda.synchronize()

    def egress(name, count=None):  # the C entry point with preallocated outputs: no allocation inside the timed region
        s = lines[name]
        m = s["n"] if count is None else count
        args = [ctypes.byref(s["cfg"]), _lib.ptr(s["frames"]), _lib.ptr(s["offs"]), _lib.ptr(s["lens"]), m, _lib.ptr(s["sel"])]
        if s["kind"] == E.EGRESS_KIND_SWITCH:
            _lib.check("halo_tx_egress_switch_device", L.halo_tx_egress_switch_device(
                *args, s["flood"], _lib.ptr(s["out"]), _lib.ptr(s["summary"]), _lib.ptr(s["index"]), _lib.ptr(s["skipped"]),
                _lib.ptr(s["ws"]), s["wsb"], stream))
        else:
            _lib.check("halo_tx_egress_arp_device", L.halo_tx_egress_arp_device(
                *args, _lib.ptr(s["out"]), _lib.ptr(s["summary"]), _lib.ptr(s["index"]), _lib.ptr(s["skipped"]),
                _lib.ptr(s["ws"]), s["wsb"], stream))

    def copy(name):
        s = lines[name]
        assert memcpy(_lib.ptr(s["copy_dst"]), _lib.ptr(s["copy_src"]), s["out_bytes"], 3, stream) == 0  # device to device

    def encap():
        _lib.check("halo_arp_encap_device", L.halo_arp_encap_device(
            table._t, _lib.ptr(d_small), _lib.ptr(d_offs), _lib.ptr(d_lens), n, _lib.ptr(rids), 0, None, _lib.ptr(enc_res),
            _lib.ptr(enc_counts), _lib.ptr(enc_miss), stream))

    fns = {**{k: (lambda k=k: egress(k)) for k in lines}, **{"copy_" + k: (lambda k=k: copy(k)) for k in lines},
           "arp_encap": encap}
    if a.profile:
        for _ in range(10):
            for k in lines:
                egress(k)
        torch.cuda.synchronize()
        print(json.dumps({"profiled": list(lines), "calls": 10}))
        return

    def timed(fn_map, rounds, warmup):
        for _ in range(warmup):
            for f in fn_map.values():
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in fn_map}
        for _ in range(rounds):  # interleaved: one call of each per round
            for k, f in fn_map.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        return {k: {"us_median": float(np.median(v)) * 1e3, "us_min": float(min(v)) * 1e3, "us_max": float(max(v)) * 1e3}
                for k, v in ms.items()}

    res = {"frames": n, "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    res.update(timed(fns, a.rounds, a.warmup))
    for k, s in lines.items():
        summ = s["summary"].cpu().numpy().reshape(-1).view(_lib.EGRESS_PORT_DTYPE)
        assert int(summ["frames"].sum()) == int(summ["frames_written"].sum()) == s["records"], (k, summ)
        assert int(summ["bytes_written"].sum()) == s["out_bytes"] and int(s["skipped"].cpu()[0]) == 0
        r = res[k]
        r["records"], r["out_bytes"], r["ports"] = s["records"], s["out_bytes"], s["ports"]
        r["mpps_in"] = s["n"] / r["us_median"]
        r["ratio_to_copy"] = r["us_median"] / res["copy_" + k]["us_median"]
        r["bound_bytes"] = s["bound_bytes"]
        r["bound_us"] = s["bound_bytes"] / HBM_BYTES_PER_S * 1e6
        r["ratio_to_bound"] = r["us_median"] / r["bound_us"]
        res["copy_" + k]["gbytes_per_s"] = s["out_bytes"] / res["copy_" + k]["us_median"] / 1e3
    # host and device over a ladder of batch sizes, one port, 64 B frames
    s = lines["arp_1"]
    h_sel = np.ascontiguousarray(s["sel"].cpu().numpy()).reshape(-1).view(ARP_RESULT_DTYPE)
    h_offs = np.ascontiguousarray(d_offs.cpu().numpy().view(np.uint32))
    h_lens = np.ascontiguousarray(d_lens.cpu().numpy().view(np.uint16))
    ladder = [m for m in LADDER if m <= n] + [n]
    dev_ladder = timed({m: (lambda m=m: egress("arp_1", m)) for m in ladder}, a.rounds, a.warmup)
    out_h = np.zeros(int(s["cfg"].region_bytes), np.uint8)
    ports_h = np.zeros(1, _lib.EGRESS_PORT_DTYPE)
    index_h = np.zeros(int(s["cfg"].index_cap), np.uint32)
    res["ladder"] = {}
    for m in ladder:
        dts = []
        for _ in range(a.host_rounds + 1):
            t0 = time.perf_counter()
            rc = L.halo_tx_egress_host(ctypes.byref(s["cfg"]), E.EGRESS_KIND_ARP, _lib.ptr(small), _lib.ptr(h_offs),
                                       _lib.ptr(h_lens), m, _lib.ptr(h_sel), 0, _lib.ptr(out_h), _lib.ptr(ports_h),
                                       _lib.ptr(index_h), None)
            dts.append(time.perf_counter() - t0)
            assert rc == 0 and int(ports_h[0]["frames_written"]) == m
        dts = dts[1:]  # the first touches the pages
        res["ladder"][str(m)] = {"host_us_median": float(np.median(dts)) * 1e6, "host_us_min": min(dts) * 1e6,
                                 "host_us_max": max(dts) * 1e6, "device": dev_ladder[m]}
    cross = [m for m in ladder if res["ladder"][str(m)]["device"]["us_median"] < res["ladder"][str(m)]["host_us_median"]]
    res["device_faster_from_frames"] = cross[0] if cross else None
    line = json.dumps(res)
    print(line)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
