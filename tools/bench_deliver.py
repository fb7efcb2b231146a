"""Measure local delivery: python tools/bench_deliver.py [--frames N] [--rounds K]
[--warmup W] [--log PATH].

Frames resident in HBM, back to back, records from the device parse (checksums off: the served
port is patched into a template frame), outputs preallocated:
  udp64_all    N x 64 B UDP frames, all to one served port
  udp64_1in16  the same frames, every 16th to the served port
  udp1500_all  N / 4 x 1500 B UDP frames, all served
Per workload, in interleaved rounds after warm-up rounds — one call of each line per round, so that
the variants alternate in one process — with HIP events around each:
  (a) deliver     halo_rx_deliver_device
  (b) copy_d2d    hipMemcpyAsync device to device of exactly bytes_written
  (d) stream_d2h  hipMemcpyAsync of the stream alone to pinned host memory
and, by the host's clock with the stream synchronised, the path the device call replaces:
  (c) download_host  the batch bytes, offsets, lengths and records copied to pinned host memory,
                     then halo_rx_deliver_host on one core
The median with minimum and maximum over the rounds is reported, with (a)/(b) and (c)/((a)+(d)).
Then a ladder of batch sizes over the 64 B all-served frames, both sides by the host's clock: (c)
against (a) followed by (d) and a synchronise; the largest size at which (c) still wins is
reported. Prints one JSON line and, with --log, writes it there."""
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

LADDER = [16, 64, 256, 1024, 4096, 16384, 65536, 262144]
SERVED, UNSERVED = 8192, 8193
D2H, D2D = 2, 3  # hipMemcpyKind


def frames_of(n: int, length: int, served_every: int) -> np.ndarray:
    """n x length IPv4/UDP frames to 192.168.100.100, dport SERVED at every served_every-th frame."""
    from oracle import ref_py as R

    src, dst = bytes([192, 168, 100, 7]), bytes([192, 168, 100, 100])
    payload = bytes(k % 251 for k in range(length - 42))
    t = R.build_eth(R.build_ipv4(R.build_udp(payload, 4096, UNSERVED, src, dst), 17, src, dst), bytes([0xAA] * 6),
                    bytes([2, 0x77, 0, 0, 0, 1]), 0x0800)
    assert len(t) == length
    f = np.tile(np.frombuffer(t, np.uint8), (n, 1))
    f[::served_every, 36:38] = [SERVED >> 8, SERVED & 0xFF]
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=20)
    ap.add_argument("--log", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert a.rounds >= 20 and a.host_rounds >= 20, "at least 20 runs per line"
    import torch

    from halo_amd import _lib, protocol
    from halo_amd.deliver import port_map, workspace_bytes
    from tools.bench_egress import hip_memcpy_async

    assert torch.cuda.is_available(), "bench_deliver needs a GPU"
    dev = torch.device("cuda:0")
    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    L = _lib.lib
    stream = torch.cuda.current_stream().cuda_stream
    memcpy = hip_memcpy_async()
    netif = _lib.NetIf.make("AA:AA:AA:AA:AA:AA", "192.168.100.100")
    pm_h = port_map([SERVED])
    pm_d = torch.from_numpy(pm_h.view(np.int32)).to(dev)
    pinned = lambda nbytes: torch.empty(max(nbytes, 16), dtype=torch.uint8).pin_memory()  # noqa: E731

    lines = {}

    def add(name, n, length, served_every):
        f = frames_of(n, length, served_every)
        d = torch.from_numpy(f.reshape(-1)).to(dev)
        offs = torch.from_numpy((np.arange(n, dtype=np.uint32) * (length // 4)).view(np.int32)).to(dev)
        lens = torch.from_numpy(np.full(n, length, np.uint16).view(np.int16)).to(dev)
        recs = protocol.parse_frames_batch(d, offs, lens, netif=netif, check_sum_enable=False)
        served = (n + served_every - 1) // served_every
        rec = 24 + ((length - 42 + 3) & ~3)
        region = (served * rec + 15) & ~15
        cfg = _lib.DeliverConfig()
        cfg.flags, cfg.index_cap, cfg.region_bytes = 0, served, region
        wsb = workspace_bytes(n)
        lines[name] = dict(
            n=n, length=length, served=served, out_bytes=served * rec, cfg=cfg, d=d, offs=offs, lens=lens, recs=recs, wsb=wsb,
            out=torch.empty(region, dtype=torch.uint8, device=dev), summary=torch.empty(5, dtype=torch.int64, device=dev),
            index=torch.empty((served, 2), dtype=torch.int32, device=dev), ws=torch.empty(wsb // 8, dtype=torch.int64, device=dev),
            copy_dst=torch.empty(region, dtype=torch.uint8, device=dev),
            h_stream=pinned(region), h_bytes=pinned(n * length), h_offs=pinned(4 * n), h_lens=pinned(2 * n), h_recs=pinned(32 * n),
            h_out=np.zeros(region, np.uint8), h_summary=np.zeros(40, np.uint8), h_index=np.zeros((served, 8), np.uint8))

    add("udp64_all", a.frames, 64, 1)
    add("udp64_1in16", a.frames, 64, 16)
    add("udp1500_all", a.frames // 4, 1500, 1)
    torch.cuda.synchronize()

    def deliver(s, m=None):
        m = s["n"] if m is None else m
        _lib.check("halo_rx_deliver_device", L.halo_rx_deliver_device(
            ctypes.byref(s["cfg"]), _lib.ptr(s["d"]), _lib.ptr(s["offs"]), _lib.ptr(s["lens"]), _lib.ptr(s["recs"]), m, netif,
            _lib.ptr(pm_d), None, _lib.ptr(s["out"]), _lib.ptr(s["summary"]), _lib.ptr(s["index"]), _lib.ptr(s["ws"]), s["wsb"],
            stream))

    def copy(dst, src, nbytes, kind):
        assert memcpy(_lib.ptr(dst), _lib.ptr(src), nbytes, kind, stream) == 0

    def download_host(s, m=None):
        """(c): the batch and its records to the host, then the host loop."""
        m = s["n"] if m is None else m
        copy(s["h_bytes"], s["d"], m * s["length"], D2H)
        copy(s["h_offs"], s["offs"], 4 * m, D2H)
        copy(s["h_lens"], s["lens"], 2 * m, D2H)
        copy(s["h_recs"], s["recs"], 32 * m, D2H)
        torch.cuda.synchronize()
        rc = L.halo_rx_deliver_host(ctypes.byref(s["cfg"]), _lib.ptr(s["h_bytes"]), _lib.ptr(s["h_offs"]), _lib.ptr(s["h_lens"]),
                                    _lib.ptr(s["h_recs"]), m, netif, _lib.ptr(pm_h), None, _lib.ptr(s["h_out"]),
                                    _lib.ptr(s["h_summary"]), _lib.ptr(s["h_index"]))
        assert rc == 0

    def stat(v, scale):
        return {"us_median": float(np.median(v)) * scale, "us_min": float(min(v)) * scale, "us_max": float(max(v)) * scale}

    def timed_events(fn_map, rounds, warmup):
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
        return {k: stat(v, 1e3) for k, v in ms.items()}

    def timed_clock(fn_map, rounds, warmup):
        for _ in range(warmup):
            for f in fn_map.values():
                f()
        torch.cuda.synchronize()
        dt = {k: [] for k in fn_map}
        for _ in range(rounds):
            for k, f in fn_map.items():
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                dt[k].append(time.perf_counter() - t0)
        return {k: stat(v, 1e6) for k, v in dt.items()}

    res = {"frames": a.frames, "rounds": a.rounds, "host_rounds": a.host_rounds, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "workloads": {}}
    for name, s in lines.items():
        ev = timed_events({"deliver": lambda s=s: deliver(s), "copy_d2d": lambda s=s: copy(s["copy_dst"], s["out"], s["out_bytes"], D2D),
                           "stream_d2h": lambda s=s: copy(s["h_stream"], s["out"], s["out_bytes"], D2H)}, a.rounds, a.warmup)
        summ = s["summary"].cpu().numpy().view(np.uint8).view(_lib.DELIVER_SUMMARY_DTYPE)[0]
        assert int(summ["records"]) == int(summ["records_written"]) == s["served"], (name, summ)
        assert int(summ["bytes_written"]) == s["out_bytes"] and int(summ["skipped"]) == 0
        ck = timed_clock({"download_host": lambda s=s: download_host(s)}, a.host_rounds, 2)
        host = s["h_summary"].view(_lib.DELIVER_SUMMARY_DTYPE)[0]
        assert host == summ and np.array_equal(s["h_out"][:s["out_bytes"]], s["h_stream"].numpy()[:s["out_bytes"]])
        w = {"n": s["n"], "frame_bytes": s["length"], "records": s["served"], "out_bytes": s["out_bytes"], **ev, **ck}
        w["deliver_over_copy_d2d"] = ev["deliver"]["us_median"] / ev["copy_d2d"]["us_median"]
        w["download_host_over_deliver_plus_d2h"] = ck["download_host"]["us_median"] / (
            ev["deliver"]["us_median"] + ev["stream_d2h"]["us_median"])
        w["mpps_in"] = s["n"] / ev["deliver"]["us_median"]
        w["out_gbytes_per_s"] = s["out_bytes"] / ev["deliver"]["us_median"] / 1e3
        res["workloads"][name] = w
    # the ladder: 64 B frames, all served, both sides by the host's clock
    s = lines["udp64_all"]
    rec = s["out_bytes"] // s["served"]

    def device_side(m):
        deliver(s, m)
        copy(s["h_stream"], s["out"], m * rec, D2H)

    res["ladder"] = {}
    for m in [m for m in LADDER if m <= s["n"]]:
        r = timed_clock({"download_host": lambda m=m: download_host(s, m), "deliver_then_d2h": lambda m=m: device_side(m)},
                        a.host_rounds, 3)
        res["ladder"][str(m)] = r
    wins = [int(m) for m, r in res["ladder"].items() if r["download_host"]["us_median"] < r["deliver_then_d2h"]["us_median"]]
    res["download_host_wins_up_to_frames"] = max(wins) if wins else None
    line = json.dumps(res)
    print(line)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
