"""Measure the L2 switch's device mode (DESIGN.md "L2 switch"): python tools/bench_switch.py
[--frames N] [--rounds K] [--warmup W].

N frames of 64 B resident in HBM, three traffic shapes:
  known_1k    sources and destinations drawn from 1,024 MACs the table already holds
  known_64k   the same over 65,536 MACs
  flood_1m    N all-new source MACs against capacity 65,536 (a MAC flood): the steady state, with
              the table full, and the first call into an empty table (an expiry tick in between)
HIP events around each call. The shapes and the parse kernel over the same frames
(halo_rx_parse_batch_device, the yardstick) are timed in interleaved rounds — one call of each per
round — and the median, minimum and maximum over the rounds are reported, with Mpps, the host mode
on one core over the same frames, and the bytes the algorithm must move per frame against the
8 TB/s HBM roofline. Prints one JSON line. Per-kernel shares come from a profiler run of this
script: --profile-shape runs ten calls of one shape, untimed, under rocprofv3 --kernel-trace, and
--trace-summary prints the per-kernel medians of the trace it leaves."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# Bytes per frame the algorithm needs, with 64-byte frames: the 64 B line that holds bytes 0..13 and
# 6 B of offset and length (learn), the 4 B result, and one 32 B scratch sector for each of the
# source and the destination (32 B is the smallest HBM access). The stash and the table probes come on top.
ALGO_BYTES_PER_FRAME = 64 + 6 + 4 + 32 + 32
HBM_BYTES_PER_S = 8e12


def frames_of(src_ids, dst_ids):
    n = len(src_ids)
    arr = np.zeros((n, 64), np.uint8)
    for ids, base in ((dst_ids, 0), (src_ids, 6)):
        arr[:, base] = 0x02
        for b in range(4):
            arr[:, base + 2 + b] = (ids >> (8 * (3 - b))) & 0xFF
    arr[:, 12] = 0x08
    arr[:, 14:] = np.arange(50, dtype=np.uint8)
    return arr


def trace_summary(path, last=10):
    """Per switch kernel, the median duration (us) of its last `last` dispatches in a rocprofv3
    --kernel-trace CSV — the 2^20-frame calls of --profile-shape; the pre-learning call comes first —
    and its share of their sum."""
    import csv
    import re

    dur = {}
    for r in csv.DictReader(open(path)):
        m = re.search(r"sw_(\w+)_kernel", r["Kernel_Name"])
        if m:
            dur.setdefault(m.group(1), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    med = {k: float(np.median(v[-last:])) for k, v in dur.items()}
    total = sum(med.values())
    return {"calls": last, "sum_us": total, "kernels": {k: {"us_median": x, "share": x / total} for k, x in med.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=7, help="timed host-mode calls per shape")
    ap.add_argument("--trace-summary", default=None, metavar="CSV",
                    help="print the per-kernel medians of the last 10 calls in a rocprofv3 kernel trace and exit")
    ap.add_argument("--profile-shape", default=None, help="run 10 calls of one shape and exit (for a kernel trace)")
    a = ap.parse_args()
    if a.trace_summary:
        print(json.dumps(trace_summary(a.trace_summary)))
        return
    import torch

    from halo_amd import _lib, protocol
    from halo_amd._lib import SW_V, NetIf
    from halo_amd.switch import Switch

    assert torch.cuda.is_available(), "bench_switch needs a GPU"
    dev = torch.device("cuda:0")
    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    n = a.frames
    rng = np.random.default_rng(1)
    offs = np.arange(n, dtype=np.uint32) * 16
    lens = np.full(n, 64, np.uint16)
    d_offs = torch.from_numpy(offs.view(np.int32)).to(dev)
    d_lens = torch.from_numpy(lens.view(np.int16)).to(dev)
    shapes = {}
    for name, macs, cap in (("known_1k", 1024, 2048), ("known_64k", 65536, 131072), ("flood_1m", n, 65536)):
        if macs == n:
            src, dst = rng.permutation(n).astype(np.uint32), rng.integers(0, n, n).astype(np.uint32)
        else:
            src, dst = (rng.integers(0, macs, n).astype(np.uint32) for _ in range(2))
        arr = frames_of(src, dst)
        sw = Switch([1, 1, 1, 1], cap, max_batch=n, device=0)
        d_bytes = torch.from_numpy(arr.ravel()).to(dev)
        if macs != n:  # the table learns every MAC from port 1 first
            ids = np.arange(macs, dtype=np.uint32)
            pre = frames_of(ids, ids)
            sw.forward(1, torch.from_numpy(pre.ravel()).to(dev), d_offs[:macs], d_lens[:macs], 1)
        shapes[name] = dict(sw=sw, arr=arr, d_bytes=d_bytes, res=torch.empty((n, 4), dtype=torch.uint8, device=dev),
                            counts=torch.zeros(6, dtype=torch.int32, device=dev), cap=cap)

    def call(name, now=100):
        s = shapes[name]
        s["sw"].forward(0, s["d_bytes"], d_offs, d_lens, now, results=s["res"], counts=s["counts"])

    if a.profile_shape:
        for _ in range(10):
            call(a.profile_shape)
        torch.cuda.synchronize()
        print(json.dumps({"profiled": a.profile_shape, "calls": 10}))
        return

    parse_out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    netif = NetIf.make()

    def parse():
        protocol.parse_frames_batch(shapes["known_1k"]["d_bytes"], d_offs, d_lens, netif=netif, max_len_hint=64, out=parse_out)

    fns = {**{k: (lambda k=k: call(k)) for k in shapes}, "parse": parse}
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
    res = {"frames": n, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    for k, v in ms.items():
        med = float(np.median(v))
        res[k] = {"us_median": med * 1e3, "us_min": float(min(v)) * 1e3, "us_max": float(max(v)) * 1e3,
                  "mpps": n / med / 1e3}
    for k in shapes:
        res[k]["ratio_to_parse"] = res[k]["us_median"] / res["parse"]["us_median"]
        res[k]["algo_bytes_per_frame"] = ALGO_BYTES_PER_FRAME
        res[k]["roofline_us"] = n * ALGO_BYTES_PER_FRAME / HBM_BYTES_PER_S * 1e6
        res[k]["share_of_hbm_roofline"] = res[k]["roofline_us"] / res[k]["us_median"]
    # the first call of a MAC flood into an empty table (an expiry tick empties it; not timed)
    fill = []
    s = shapes["flood_1m"]
    for r in range(5):
        s["sw"].expire(100000 * (r + 1))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call("flood_1m", now=100000 * (r + 1))
        e1.record()
        e1.synchronize()
        fill.append(e0.elapsed_time(e1))
    res["flood_1m"]["first_call_us_median"] = float(np.median(fill)) * 1e3
    # what the calls computed (the last timed call of each shape)
    for k, s in shapes.items():
        v = s["res"].cpu().numpy()[:, 0]
        res[k]["verdicts"] = {name: int((v == code).sum()) for name, code in SW_V.items()}
        res[k]["entries"] = int(s["sw"].layout_stats()["entries"])
    assert res["known_1k"]["verdicts"]["UNICAST"] == n and res["known_64k"]["verdicts"]["UNICAST"] == n
    assert res["flood_1m"]["entries"] == 65536 and res["flood_1m"]["verdicts"]["TABLE_FULL"] == n - 65536
    # the host mode on one core over the same frames (a fresh switch per shape, the same pre-learning)
    for k, s in shapes.items():
        hs = Switch([1, 1, 1, 1], s["cap"], max_batch=n)
        if k != "flood_1m":
            macs = s["cap"] // 2
            ids = np.arange(macs, dtype=np.uint32)
            hs.forward(1, frames_of(ids, ids).ravel(), offs[:macs], lens[:macs], 1)
        data = s["arr"].ravel()
        hres, hcnt = hs.forward(0, data, offs, lens, 100)  # the steady state, as on the device
        dts = []
        for _ in range(a.host_rounds):
            t0 = time.perf_counter()
            hs.forward(0, data, offs, lens, 100, results=hres, counts=hcnt)
            dts.append(time.perf_counter() - t0)
        dt = float(np.median(dts))
        res[k]["host_one_core_us"] = {"median": dt * 1e6, "min": min(dts) * 1e6, "max": max(dts) * 1e6,
                                      "rounds": a.host_rounds}
        res[k]["host_mpps"] = n / dt / 1e6
        res[k]["speedup_over_host"] = dt * 1e6 / res[k]["us_median"]
        hs.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
