"""Measure the tx ring producer: python tools/bench_txring.py [--frames N]
[--rounds K] [--warmup W] [--log PATH] [--profile].

One port's egress stream, resident in HBM as whole records, published into an empty registered
ring large enough to take it:
  small    N x 64 B frames (68-byte records)
  big      N / 4 x 1500 B frames (1504-byte records)
  ladder   64 ... 65,536 x 64 B frames
For every line, in the same interleaved rounds (one call of each per round, after warm-up rounds):
  dev        halo_tx_ring_write_span_device (16-byte stores aligned on the ring), HIP events
  dev_dword  the same with the plain 4-byte copy kernel (halo_tx_ring_debug_copy_mode)
  d2h_ring   (b) a bare hipMemcpyAsync device-to-host of the span's bytes straight into the ring's
             data area: the practical ceiling of a device-to-host write; HIP events
  replaced   (a) the path the device write replaces: hipMemcpyAsync device-to-host into pinned
             memory, a synchronise, halo_ring_write_span on one core; wall clock
  dev_wall   the device write enqueued and synchronised, wall clock, to set beside `replaced`
and (c) the bound: the span's bytes at the 63 GB/s PCIe Gen5 x16 spec figure. The ladder also times
the host pair halo_tx_egress_host + halo_ring_write_span on one core and reports where the device
line crosses it. Before every write the host empties the ring (tail = head). Median with minimum
and maximum over the rounds; one JSON line, also written to --log. --profile runs ten untimed device
writes of `small` and `big` and exits, for a rocprofv3 --kernel-trace --stats run of its own."""
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

PCIE_BYTES_PER_S = 63e9
LADDER = [64, 256, 1024, 4096, 16384, 65536]


def records(rng, n, length):
    """n records of one length, back to back: (span uint8, record size)."""
    rec = (4 + length + 3) & ~3
    a = rng.integers(0, 256, (n, rec), dtype=np.uint8)
    a[:, :4] = np.frombuffer(np.uint32(length).tobytes(), np.uint8)
    a[:, 4 + length:] = 0
    return a.reshape(-1), rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log", default=None, help="also write the JSON line to this file")
    ap.add_argument("--profile", action="store_true",
                    help="run ten device writes of the two large lines, untimed, and exit (under rocprofv3 --kernel-trace)")
    a = ap.parse_args()
    import torch

    from halo_amd import _lib
    from halo_amd import egress as E
    from halo_amd.ring import RingBuffer, RingProducer
    from tools.bench_egress import hip_memcpy_async

    assert torch.cuda.is_available(), "bench_txring needs a GPU"
    dev = torch.device("cuda:0")
    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    L = _lib.lib
    rng = np.random.default_rng(1)
    stream = torch.cuda.current_stream().cuda_stream
    memcpy = hip_memcpy_async()
    n = a.frames
    shapes = {"small": (n, 64), "big": (max(n // 4, 1), 1500)}
    shapes.update({f"ladder_{m}": (m, 64) for m in LADDER if m <= n})

    lines, prods = {}, []
    try:
        for name, (count, length) in shapes.items():
            span, rec = records(rng, count, length)
            size = max(4096, 1 << (span.nbytes - 1).bit_length())
            ring = RingBuffer(size)
            prod = RingProducer(ring)  # registers the ring: d2h_ring then writes pinned memory too
            prods.append(prod)
            wsb = RingProducer.workspace_bytes(span.nbytes)
            lines[name] = dict(
                n=count, length=length, bytes=span.nbytes, ring=ring, prod=prod, span=span, wsb=wsb,
                d_span=torch.from_numpy(span).to(dev), ws=torch.empty(wsb, dtype=torch.uint8, device=dev),
                res=torch.empty(24, dtype=torch.uint8, device=dev),
                pinned=torch.empty(span.nbytes, dtype=torch.uint8, pin_memory=True))
        torch.cuda.synchronize()

        def empty(s):  # the consumer has read everything
            s["ring"].mem[64:72].view(np.uint64)[0] = s["ring"].head

        def dev_write(name, mode=0):
            s = lines[name]
            empty(s)
            _lib.check("copy_mode", L.halo_tx_ring_debug_copy_mode(s["prod"]._h, mode))
            _lib.check("halo_tx_ring_write_span_device", L.halo_tx_ring_write_span_device(
                s["prod"]._h, _lib.ptr(s["d_span"]), s["bytes"], _lib.ptr(s["res"]), _lib.ptr(s["ws"]), s["wsb"], stream))

        def d2h_ring(name):
            s = lines[name]
            assert memcpy(s["ring"].data.ctypes.data, _lib.ptr(s["d_span"]), s["bytes"], 2, stream) == 0  # device to host

        def replaced(name):
            s = lines[name]
            empty(s)
            assert memcpy(_lib.ptr(s["pinned"]), _lib.ptr(s["d_span"]), s["bytes"], 2, stream) == 0
            torch.cuda.synchronize()
            taken = ctypes.c_uint64()
            rc = L.halo_ring_write_span(s["ring"].mem.ctypes.data, _lib.ptr(s["pinned"]), s["bytes"], None, ctypes.byref(taken))
            assert rc == 0 and taken.value == s["bytes"], (rc, taken.value)

        def dev_wall(name):
            dev_write(name)
            torch.cuda.synchronize()

        if a.profile:
            for _ in range(10):
                for k in ("small", "big"):
                    dev_write(k)
                    torch.cuda.synchronize()  # the host empties the ring before the next write: head must be there
            print(json.dumps({"profiled": ["small", "big"], "calls": 10}))
            return

        event_fns, wall_fns = {}, {}
        for k in lines:
            event_fns["dev_" + k] = lambda k=k: dev_write(k)
            event_fns["dev_dword_" + k] = lambda k=k: dev_write(k, 1)
            event_fns["d2h_ring_" + k] = lambda k=k: d2h_ring(k)
            wall_fns["replaced_" + k] = lambda k=k: replaced(k)
            wall_fns["dev_wall_" + k] = lambda k=k: dev_wall(k)
        ms = {k: [] for k in list(event_fns) + list(wall_fns)}
        for r in range(a.warmup + a.rounds):  # interleaved: one call of each per round
            keep = r >= a.warmup
            for k, f in event_fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                if keep:
                    ms[k].append(e0.elapsed_time(e1))
            for k, f in wall_fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                if keep:
                    ms[k].append((time.perf_counter() - t0) * 1e3)
        res = {"frames": n, "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
        for k, v in ms.items():
            res[k] = {"us_median": float(np.median(v)) * 1e3, "us_min": float(min(v)) * 1e3, "us_max": float(max(v)) * 1e3}
        for k, s in lines.items():  # the last write of every line took the whole span
            dev_write(k)
            torch.cuda.synchronize()
            out = RingProducer.read_result(s["res"])
            assert (int(out["status"]), int(out["records"]), int(out["bytes"])) == (0, s["n"], s["bytes"]), (k, out)
            idx = ((int(out["head"]) - s["bytes"]) % s["ring"].size + np.arange(min(s["bytes"], 1 << 16))) % s["ring"].size
            assert np.array_equal(s["ring"].data[idx], s["span"][:idx.size]), k
            d = res["dev_" + k]
            d["records"], d["bytes"] = s["n"], s["bytes"]
            d["gbytes_per_s"] = s["bytes"] / d["us_median"] / 1e3
            d["bound_us"] = s["bytes"] / PCIE_BYTES_PER_S * 1e6
            d["ratio_to_bound"] = d["us_median"] / d["bound_us"]
            d["ratio_to_d2h_ring"] = d["us_median"] / res["d2h_ring_" + k]["us_median"]
            d["dword_over_aligned"] = res["dev_dword_" + k]["us_median"] / d["us_median"]
            d["replaced_over_dev_wall"] = res["replaced_" + k]["us_median"] / res["dev_wall_" + k]["us_median"]
        # the host pair on one core over the ladder: halo_tx_egress_host, then halo_ring_write_span
        res["host_pair"] = {}
        for m in [m for m in LADDER if m <= n]:
            s = lines[f"ladder_{m}"]
            frames = rng.integers(0, 256, (m, 64), dtype=np.uint8)
            offs = (np.arange(m, dtype=np.uint32) * 16)
            lens = np.full(m, 64, np.uint16)
            masks = np.ones(m, np.uint64)
            cfg = _lib.EgressConfig()
            cfg.n_ports, cfg.flags, cfg.region_bytes, cfg.index_cap = 1, 0, s["bytes"], 0
            out_h = np.zeros(s["bytes"], np.uint8)
            ports_h = np.zeros(1, _lib.EGRESS_PORT_DTYPE)
            dts = []
            for _ in range(a.rounds + 1):
                empty(s)
                t0 = time.perf_counter()
                rc = L.halo_tx_egress_host(ctypes.byref(cfg), E.EGRESS_KIND_MASKS, _lib.ptr(frames), _lib.ptr(offs),
                                           _lib.ptr(lens), m, _lib.ptr(masks), 0, _lib.ptr(out_h), _lib.ptr(ports_h), None, None)
                rc2 = L.halo_ring_write_span(s["ring"].mem.ctypes.data, _lib.ptr(out_h), s["bytes"], None, None)
                dts.append(time.perf_counter() - t0)
                assert rc == 0 and rc2 == 0 and int(ports_h[0]["bytes_written"]) == s["bytes"]
            dts = dts[1:]  # the first touches the pages
            res["host_pair"][str(m)] = {"us_median": float(np.median(dts)) * 1e6, "us_min": min(dts) * 1e6,
                                        "us_max": max(dts) * 1e6}
        cross = [m for m in LADDER if m <= n and
                 res[f"dev_wall_ladder_{m}"]["us_median"] < res["host_pair"][str(m)]["us_median"]]
        res["device_faster_than_host_pair_from_frames"] = cross[0] if cross else None
        line = json.dumps(res)
        print(line)
        if a.log:
            os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
            with open(a.log, "w") as fh:
                fh.write(line + "\n")
    finally:
        torch.cuda.synchronize()
        for p in prods:
            p.close()


if __name__ == "__main__":
    main()
