"""Measure the local responders: python tools/bench_respond.py [--frames N]
[--rounds K] [--warmup W] [--log PATH].

N frames of 64 B resident in HBM, parsed, addressed to the NetIf: plain UDP with 0 %, 0.1 % and
100 % ICMP echo requests among them. HIP events around the C entry points with preallocated
outputs, timed in interleaved rounds — one call of each line per round — after warm-up rounds;
median, minimum and maximum over the rounds:
  respond_*        halo_tx_respond_device (records, offsets, lengths; actions and kind counts on)
  gather_*         halo_arp_gather_device with the same fractions of ARP frames: the same
                   three-launch shape, re-measured here as the yardstick
  encap / encap_tx halo_arp_encap_device and halo_arp_encap_tx_device over the replies
                   halo_tx_build_batch_device built from the 100 % batch (128-byte slots, all HIT)
and what the device call replaces, per fraction, on the host clock: the D2H copy of the records,
halo_tx_respond_host on one core, the H2D copy of the descriptors. The bound is computed from the
shapes at 8 TB/s: per frame the bytes each pass reads (count: the 32 B record; scatter: record, 4 B
offset, 2 B length) and the action byte written, per reply the 52 B written. Prints one JSON line
and, with --log, writes it there. Kernel times come from a profiler run of their own: --profile
runs ten calls of every line, untimed, under rocprofv3 --kernel-trace --stats."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_arp import HIT_BASE, arp_frames, host_lib, udp_frames  # noqa: E402

HBM_BYTES_PER_S = 8e12
FRAME_BYTES_READ = 32 + (32 + 4 + 2)  # count pass; scatter pass
FRAME_BYTES_WRITTEN = 1              # the action byte
REPLY_BYTES_WRITTEN = 40 + 8 + 4
OWN_IP = 0x0A000001


def _csum(rows: np.ndarray) -> np.ndarray:
    """RFC 1071 over each row of an even number of bytes."""
    w = rows.astype(np.uint32)
    s = ((w[:, 0::2] << 8) | w[:, 1::2]).sum(axis=1)
    s = (s & 0xFFFF) + (s >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    return (~s) & 0xFFFF


def echo_frames(src_ips: np.ndarray, own_mac: bytes) -> np.ndarray:
    """n x 64 B ICMP echo requests from src_ips to the NetIf: 22 payload bytes, valid checksums."""
    n = len(src_ips)
    f = np.zeros((n, 64), np.uint8)
    f[:, 0:6] = np.frombuffer(own_mac, np.uint8)
    f[:, 6:12] = [0x02, 0x77, 0, 0, 0, 1]
    f[:, 12:14] = [0x08, 0x00]
    f[:, 14:24] = [0x45, 0, 0, 50, 0, 1, 0x40, 0, 64, 1]  # total length 50, DF, TTL 64, ICMP
    for b in range(4):
        f[:, 26 + b] = (src_ips >> (8 * (3 - b))) & 0xFF
        f[:, 30 + b] = (OWN_IP >> (8 * (3 - b))) & 0xFF
    c = _csum(f[:, 14:34])
    f[:, 24], f[:, 25] = c >> 8, c & 0xFF
    f[:, 34] = 8
    seq = np.arange(n)
    f[:, 38:42] = np.stack([np.full(n, 0x12), np.full(n, 0x34), (seq >> 8) & 0xFF, seq & 0xFF], axis=1)
    f[:, 42:64] = np.arange(22)
    c = _csum(f[:, 34:64])
    f[:, 36], f[:, 37] = c >> 8, c & 0xFF
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=5, help="timed host loops per fraction")
    ap.add_argument("--log", default=None, help="also write the JSON line to this file")
    ap.add_argument("--profile", action="store_true",
                    help="run ten calls of everything, untimed, and exit (under rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    import torch

    from halo_amd import _lib, protocol
    from halo_amd._lib import ARP_V, NetIf
    from halo_amd.arp import ArpTable
    from halo_amd.route import RouteTable

    assert torch.cuda.is_available(), "bench_respond needs a GPU"
    dev = torch.device("cuda:0")
    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    H = host_lib()
    n = a.frames
    rng = np.random.default_rng(1)
    netifs = [NetIf.make("02:00:00:00:00:01", "10.0.0.1"), NetIf.make("02:00:00:00:00:02", "10.1.0.1")]
    own, own_mac = netifs[0], bytes(netifs[0].mac)
    neighbours = 1024
    peers = (HIT_BASE + rng.integers(0, neighbours, n)).astype(np.uint32)  # whom the echo requests come from
    d_offs = torch.from_numpy((np.arange(n, dtype=np.uint32) * 16).view(np.int32)).to(dev)
    d_lens = torch.from_numpy(np.full(n, 64, np.uint16).view(np.int16)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    plain = udp_frames(np.full(n, OWN_IP, np.uint32), own_mac)
    cases = {}
    for tag, every in (("0pct", 0), ("0.1pct", 1000), ("100pct", 1)):
        c = {}
        for what, special in (("respond", echo_frames), ("gather", lambda ips, mac: arp_frames(len(ips), mac))):
            arr = plain.copy()
            if every:
                arr[::every] = special(peers[::every], own_mac)
            d_bytes = torch.from_numpy(arr.ravel()).to(dev)
            c[what] = dict(d_bytes=d_bytes, want=len(arr[::every]) if every else 0,
                           recs=protocol.parse_frames_batch(d_bytes, d_offs, d_lens, netif=own, max_len_hint=64))
        wsb = int(_lib.lib.halo_tx_respond_workspace(n))
        c["respond"].update(wsb=wsb, ws=torch.empty(wsb // 4, dtype=torch.int32, device=dev),
                            desc=torch.zeros((n, 40), dtype=torch.uint8, device=dev),
                            src=torch.empty((n, 8), dtype=torch.uint8, device=dev),
                            dst_ip=torch.empty(n, dtype=torch.int32, device=dev),
                            count=torch.zeros(1, dtype=torch.int32, device=dev),
                            kinds=torch.zeros(4, dtype=torch.int32, device=dev),
                            actions=torch.empty(n, dtype=torch.uint8, device=dev))
        gwsb = int(_lib.lib.halo_arp_gather_workspace(n))
        c["gather"].update(wsb=gwsb, ws=torch.empty(gwsb // 4, dtype=torch.int32, device=dev),
                           msgs=torch.empty((n, 40), dtype=torch.uint8, device=dev),
                           count=torch.zeros(1, dtype=torch.int32, device=dev))
        cases[tag] = c
    torch.cuda.synchronize()

    def respond(tag):
        r = cases[tag]["respond"]
        _lib.check("halo_tx_respond_device", _lib.lib.halo_tx_respond_device(
            _lib.ptr(d_offs), _lib.ptr(d_lens), _lib.ptr(r["recs"]), n, 0, own, None, None, None, None, _lib.ptr(r["desc"]),
            _lib.ptr(r["src"]), _lib.ptr(r["dst_ip"]), n, _lib.ptr(r["count"]), _lib.ptr(r["kinds"]), _lib.ptr(r["actions"]),
            _lib.ptr(r["ws"]), r["wsb"], stream))

    def gather(tag):
        g = cases[tag]["gather"]
        _lib.check("halo_arp_gather_device", _lib.lib.halo_arp_gather_device(
            _lib.ptr(g["d_bytes"]), _lib.ptr(d_offs), _lib.ptr(d_lens), _lib.ptr(g["recs"]), n, 0, _lib.ptr(g["msgs"]), n,
            _lib.ptr(g["count"]), _lib.ptr(g["ws"]), g["wsb"], stream))

    # the replies of the 100 % batch, built into 128-byte slots, for the two encap lines
    rt = RouteTable(0)
    rt.AddRoute(RouteTable.entry(HIT_BASE, 0xFF000000, 0, 1))
    rt.sync()
    table = ArpTable(netifs, neighbours)
    _lib.check("bench_arp_fill", H.bench_arp_fill(table._t, 1, HIT_BASE, neighbours, 100))
    table.sync(rt)
    respond("100pct")
    r100 = cases["100pct"]["respond"]
    stride = 128
    builder = protocol.TxBuilder(n)
    frames, out_lens, _ = builder.build(r100["desc"], r100["d_bytes"], netif=own, out_stride=stride, max_payload_hint=22)
    rids = rt.FindRoute(r100["dst_ip"])
    slot_offs = torch.arange(n, dtype=torch.int32, device=dev) * (stride // 4)
    enc = {k: dict(res=torch.empty((n, 8), dtype=torch.uint8, device=dev), counts=torch.zeros(7, dtype=torch.int32, device=dev),
                   miss=torch.zeros(1, dtype=torch.int32, device=dev)) for k in ("encap", "encap_tx")}
    torch.cuda.synchronize()

    def encap(name):
        e = enc[name]
        fn = _lib.lib.halo_arp_encap_device if name == "encap" else _lib.lib.halo_arp_encap_tx_device
        _lib.check(name, fn(table._t, _lib.ptr(frames), _lib.ptr(slot_offs), _lib.ptr(out_lens), n, _lib.ptr(rids), 0, None,
                            _lib.ptr(e["res"]), _lib.ptr(e["counts"]), _lib.ptr(e["miss"]), stream))

    fns = {**{f"respond_{t}": (lambda t=t: respond(t)) for t in cases}, **{f"gather_{t}": (lambda t=t: gather(t)) for t in cases},
           "encap": lambda: encap("encap"), "encap_tx": lambda: encap("encap_tx")}
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
    res = {"frames": n, "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "note": "measured once on one machine"}
    for k, v in ms.items():
        med = float(np.median(v))
        res[k] = {"us_median": med * 1e3, "us_min": float(min(v)) * 1e3, "us_max": float(max(v)) * 1e3, "mpps": n / med / 1e3}
    for tag, c in cases.items():
        r, k = c["respond"], f"respond_{tag}"
        got = int(r["count"].cpu()[0])
        assert got == r["want"] and int(c["gather"]["count"].cpu()[0]) == c["gather"]["want"], (tag, got)
        assert int((r["actions"] == 9).sum()) == got  # LOCAL_ICMP
        bound = (n * (FRAME_BYTES_READ + FRAME_BYTES_WRITTEN) + got * REPLY_BYTES_WRITTEN) / HBM_BYTES_PER_S * 1e6
        res[k].update(replies=got, bound_us=bound, ratio_to_bound=res[k]["us_median"] / bound,
                      ratio_to_gather=res[k]["us_median"] / res[f"gather_{tag}"]["us_median"])
        # what the call replaces: records down, the loop on one core, descriptors up
        h_recs = torch.empty((n, 32), dtype=torch.uint8).pin_memory()
        desc = np.zeros((max(got, 1), 40), np.uint8)
        src, dst = np.zeros((max(got, 1), 8), np.uint8), np.zeros(max(got, 1), np.uint32)
        cnt, acts = np.zeros(1, np.uint32), np.zeros(n, np.uint8)
        offs_h, lens_h = d_offs.cpu().numpy(), d_lens.cpu().numpy()
        parts = {"d2h_records": [], "host_loop": [], "h2d_desc": []}
        for _ in range(a.host_rounds):
            t0 = time.perf_counter()
            h_recs.copy_(r["recs"])
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            _lib.check("halo_tx_respond_host", _lib.lib.halo_tx_respond_host(
                _lib.ptr(offs_h), _lib.ptr(lens_h), h_recs.data_ptr(), n, 0, own, None, None, None, None, _lib.ptr(desc),
                _lib.ptr(src), _lib.ptr(dst), got, _lib.ptr(cnt), None, _lib.ptr(acts)))
            t2 = time.perf_counter()
            r["desc"][:max(got, 1)].copy_(torch.from_numpy(desc))
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            for name, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2)):
                parts[name].append(dt * 1e6)
        assert int(cnt[0]) == got
        res[k]["host_path_us"] = {name: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for name, v in parts.items()}
        total = sum(res[k]["host_path_us"][name]["median"] for name in parts)
        res[k]["host_path_us"]["total_median"] = total
        res[k]["speedup_over_host_path"] = total / res[k]["us_median"]
    for k, e in enc.items():
        v = e["res"].cpu().numpy()[:, 0]
        res[k]["verdicts"] = {name: int((v == code).sum()) for name, code in ARP_V.items() if (v == code).any()}
        assert res[k]["verdicts"] == {"HIT": n}, res[k]["verdicts"]
    res["encap_tx"]["ratio_to_encap"] = res["encap_tx"]["us_median"] / res["encap"]["us_median"]
    line = json.dumps(res)
    print(line)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
