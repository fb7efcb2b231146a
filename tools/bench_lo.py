"""Measure the loopback gather: python tools/bench_lo.py [--frames N] [--rounds K]
[--warmup W] [--log PATH] [--profile].

Frames resident in HBM, back to back, with preallocated outputs:
  lo_64      N x 64 B, every frame LOOPBACK to one NetIf
  lo_1500    N / 4 x 1500 B, every frame LOOPBACK to one NetIf
  lo_mix64   N x 64 B, one frame in 64 LOOPBACK (the realistic share), the rest HIT
  lo_tx_64   N x 64 B, tx mode (totalLen 50), every frame LOOPBACK to one NetIf
HIP events around each C entry point. In the same interleaved rounds — one call of each line per
round, after warm-up rounds — a hipMemcpyAsync device-to-device copy of exactly each line's output
bytes (copy_<line>) and halo_tx_egress_arp_device over the same batch to one port with HIT where the
line has LOOPBACK (egress_<line>), the nearest existing kernel. The median with minimum and maximum
over the rounds is reported, with the ratio to the copy line, to the egress line and to the bound
computed from shapes: per frame its 8 B result and 2 B length, per selected frame 4 B of offset, its
bytes read from the packet's first dword on, the packet written and 10 B of per-packet entries, at
8 TB/s. Separately: halo_lo_gather_host on one core plus the upload of what it wrote, and the device
call, over a ladder of batch sizes (the crossing of the two lines is reported). Prints one JSON line
and, with --log, writes it there. --profile runs ten untimed calls of every gather line, each beside
its egress line, and exits, for a counter or kernel-trace run of its own."""
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
LADDER = [64, 256, 1024, 4096, 16384, 65536]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=5)
    ap.add_argument("--log", default=None, help="also write the JSON line to this file")
    ap.add_argument("--profile", action="store_true", help="run ten calls of every gather line, untimed, and exit")
    a = ap.parse_args()
    import torch

    from halo_amd import _lib
    from halo_amd import egress as E
    from halo_amd import loopback as LO
    from halo_amd._lib import ARP_RESULT_DTYPE, ARP_V
    from tools.bench_egress import hip_memcpy_async

    assert torch.cuda.is_available(), "bench_lo needs a GPU"
    dev = torch.device("cuda:0")
    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    L = _lib.lib
    n = a.frames
    rng = np.random.default_rng(1)
    stream = torch.cuda.current_stream().cuda_stream
    memcpy = hip_memcpy_async()

    small = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    small[:, 16], small[:, 17] = 0, 50  # totalLen 50, for the tx line
    d_small = torch.from_numpy(small.ravel()).to(dev)
    d_offs = torch.from_numpy((np.arange(n, dtype=np.uint32) * 16).view(np.int32)).to(dev)
    d_lens = torch.from_numpy(np.full(n, 64, np.uint16).view(np.int16)).to(dev)
    nb = n // 4
    d_big = torch.from_numpy(rng.integers(0, 256, nb * 1500, dtype=np.uint8)).to(dev)
    d_big_offs = torch.from_numpy((np.arange(nb, dtype=np.uint32) * 375).view(np.int32)).to(dev)
    d_big_lens = torch.from_numpy(np.full(nb, 1500, np.uint16).view(np.int16)).to(dev)

    lines = {}

    def add(name, frames, offs, lens, count, length, every, tx=False):
        plen = 50 if tx else length - 14
        size = LO.packet_size(plen)
        res = np.zeros(count, ARP_RESULT_DTYPE)
        res["verdict"], res["out_netif"], res["tx_len"] = ARP_V["HIT"], 0, max(length, 60)
        res["verdict"][::every] = ARP_V["LOOPBACK"]
        res["out_netif"][::every] = 1
        sel = len(res["verdict"][::every])
        region = (sel * size + 15) & ~15
        cfg = LO._config(2, region, sel, tx, False)
        wsb = LO.workspace_bytes(count, 2)
        # the egress line: the same frames, HIT where the line has LOOPBACK, everything else nowhere
        eres = np.zeros(count, ARP_RESULT_DTYPE)
        eres["out_netif"] = 0xFF
        eres["verdict"][::every], eres["out_netif"][::every], eres["tx_len"][::every] = ARP_V["HIT"], 0, max(length, 60)
        rec = E.record_size(length)
        ecfg = _lib.EgressConfig()
        ecfg.n_ports, ecfg.flags, ecfg.region_bytes, ecfg.index_cap = 1, 0, (sel * rec + 15) & ~15, sel
        ewsb = E.workspace_bytes(count, 1)
        lines[name] = dict(
            cfg=cfg, frames=frames, offs=offs, lens=lens, n=count, wsb=wsb, sel=sel, size=size,
            res=torch.from_numpy(res.view(np.uint8).reshape(count, 8)).to(dev), res_host=res,
            out=torch.empty(2 * region, dtype=torch.uint8, device=dev),
            summary=torch.empty((2, 24), dtype=torch.uint8, device=dev),
            pkt_off=torch.empty((2, sel), dtype=torch.int32, device=dev),
            pkt_len=torch.empty((2, sel), dtype=torch.int16, device=dev),
            index=torch.empty((2, sel), dtype=torch.int32, device=dev),
            skipped=torch.zeros(1, dtype=torch.int32, device=dev), ws=torch.empty(wsb // 8, dtype=torch.int64, device=dev),
            out_bytes=sel * size,
            bound_bytes=count * 10 + sel * (4 + (length - 12 if not tx else plen + 2) + size + 10),
            copy_src=torch.empty(sel * size, dtype=torch.uint8, device=dev),
            copy_dst=torch.empty(sel * size, dtype=torch.uint8, device=dev),
            ecfg=ecfg, ewsb=ewsb, eres=torch.from_numpy(eres.view(np.uint8).reshape(count, 8)).to(dev),
            eout=torch.empty(int(ecfg.region_bytes), dtype=torch.uint8, device=dev),
            esummary=torch.empty((1, 24), dtype=torch.uint8, device=dev),
            eindex=torch.empty((1, sel), dtype=torch.int32, device=dev),
            ews=torch.empty(ewsb // 8, dtype=torch.int64, device=dev))

    add("lo_64", d_small, d_offs, d_lens, n, 64, 1)
    add("lo_1500", d_big, d_big_offs, d_big_lens, nb, 1500, 1)
    add("lo_mix64", d_small, d_offs, d_lens, n, 64, 64)
    add("lo_tx_64", d_small, d_offs, d_lens, n, 64, 1, tx=True)
    torch.cuda.synchronize()

    def gather(name, count=None):  # the C entry point with preallocated outputs: no allocation inside the timed region
        s = lines[name]
        m = s["n"] if count is None else count
        _lib.check("halo_lo_gather_device", L.halo_lo_gather_device(
            ctypes.byref(s["cfg"]), _lib.ptr(s["frames"]), _lib.ptr(s["offs"]), _lib.ptr(s["lens"]), m, _lib.ptr(s["res"]),
            _lib.ptr(s["out"]), _lib.ptr(s["summary"]), _lib.ptr(s["pkt_off"]), _lib.ptr(s["pkt_len"]), _lib.ptr(s["index"]),
            _lib.ptr(s["skipped"]), _lib.ptr(s["ws"]), s["wsb"], stream))

    def egress(name):
        s = lines[name]
        _lib.check("halo_tx_egress_arp_device", L.halo_tx_egress_arp_device(
            ctypes.byref(s["ecfg"]), _lib.ptr(s["frames"]), _lib.ptr(s["offs"]), _lib.ptr(s["lens"]), s["n"], _lib.ptr(s["eres"]),
            _lib.ptr(s["eout"]), _lib.ptr(s["esummary"]), _lib.ptr(s["eindex"]), _lib.ptr(s["skipped"]), _lib.ptr(s["ews"]),
            s["ewsb"], stream))

    def copy(name):
        s = lines[name]
        assert memcpy(_lib.ptr(s["copy_dst"]), _lib.ptr(s["copy_src"]), s["out_bytes"], 3, stream) == 0  # device to device

    fns = {**{k: (lambda k=k: gather(k)) for k in lines}, **{"copy_" + k: (lambda k=k: copy(k)) for k in lines},
           **{"egress_" + k: (lambda k=k: egress(k)) for k in lines if k != "lo_tx_64"}}
    if a.profile:
        for _ in range(10):
            for k in lines:
                gather(k)
                if k != "lo_tx_64":
                    egress(k)  # beside it in the trace: the same batch through the egress kernels
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
        assert int(summ[1]["frames"]) == int(summ[1]["frames_written"]) == s["sel"] and int(summ[0]["frames"]) == 0, (k, summ)
        assert int(summ[1]["bytes_written"]) == s["out_bytes"] and int(s["skipped"].cpu()[0]) == 0
        r = res[k]
        r["packets"], r["out_bytes"] = s["sel"], s["out_bytes"]
        r["mpps_in"] = s["n"] / r["us_median"]
        r["ratio_to_copy"] = r["us_median"] / res["copy_" + k]["us_median"]
        if "egress_" + k in res:
            r["ratio_to_egress"] = r["us_median"] / res["egress_" + k]["us_median"]
        r["bound_bytes"] = s["bound_bytes"]
        r["bound_us"] = s["bound_bytes"] / HBM_BYTES_PER_S * 1e6
        r["ratio_to_bound"] = r["us_median"] / r["bound_us"]
        res["copy_" + k]["gbytes_per_s"] = s["out_bytes"] / res["copy_" + k]["us_median"] / 1e3
    # host (plus the upload of what it wrote) and device over a ladder of batch sizes, one NetIf, 64 B frames
    s = lines["lo_64"]
    h_offs = np.ascontiguousarray(d_offs.cpu().numpy().view(np.uint32))
    h_lens = np.ascontiguousarray(d_lens.cpu().numpy().view(np.uint16))
    ladder = [m for m in LADDER if m <= n] + [n]
    dev_ladder = timed({m: (lambda m=m: gather("lo_64", m)) for m in ladder}, a.rounds, a.warmup)
    region = int(s["cfg"].region_bytes)
    out_h = np.zeros(2 * region, np.uint8)
    ports_h = np.zeros(2, _lib.EGRESS_PORT_DTYPE)
    off_h, len_h, idx_h = np.zeros((2, s["sel"]), np.uint32), np.zeros((2, s["sel"]), np.uint16), np.zeros((2, s["sel"]), np.uint32)
    small_flat = small.ravel()
    res["ladder"] = {}
    for m in ladder:
        dts, ups = [], []
        for _ in range(a.host_rounds + 1):
            t0 = time.perf_counter()
            rc = L.halo_lo_gather_host(ctypes.byref(s["cfg"]), _lib.ptr(small_flat), _lib.ptr(h_offs), _lib.ptr(h_lens), m,
                                       _lib.ptr(s["res_host"]), _lib.ptr(out_h), _lib.ptr(ports_h), _lib.ptr(off_h),
                                       _lib.ptr(len_h), _lib.ptr(idx_h), None)
            t1 = time.perf_counter()
            assert rc == 0 and int(ports_h[1]["frames_written"]) == m
            wrote = int(ports_h[1]["bytes_written"])
            s["out"][region:region + wrote].copy_(torch.from_numpy(out_h[region:region + wrote]))
            s["pkt_off"][1, :m].copy_(torch.from_numpy(off_h[1, :m].view(np.int32)))
            s["pkt_len"][1, :m].copy_(torch.from_numpy(len_h[1, :m].view(np.int16)))
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            dts.append(t1 - t0)
            ups.append(t2 - t1)
        dts, ups = dts[1:], ups[1:]  # the first touches the pages
        res["ladder"][str(m)] = {"host_us_median": float(np.median(dts)) * 1e6, "host_us_min": min(dts) * 1e6,
                                 "host_us_max": max(dts) * 1e6, "upload_us_median": float(np.median(ups)) * 1e6,
                                 "host_plus_upload_us_median": float(np.median(np.add(dts, ups))) * 1e6,
                                 "device": dev_ladder[m]}
    cross = [m for m in ladder
             if res["ladder"][str(m)]["device"]["us_median"] < res["ladder"][str(m)]["host_plus_upload_us_median"]]
    res["device_faster_from_frames"] = cross[0] if cross else None
    line = json.dumps(res)
    print(line)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
