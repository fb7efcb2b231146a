"""Measure KCP ingest: python tools/bench_kcp.py [--scale S] [--rounds K]
[--warmup W] [--log PATH].

A delivery stream resident in HBM (made here record by record: 24-byte header, one UDP payload to
the served port, padding), its summary and index, outputs and workspace preallocated:
  ack      2^20 datagrams of one empty-payload ACK segment each
  push     2^18 datagrams of one 1,368-byte PUSH segment (a full 1,400-byte MTU segment)
  mix8     2^18 datagrams of 8 small segments: ACK, PUSH 24 B, ACK, PUSH 60 B, WASK, PUSH 120 B, WINS, PUSH 200 B
each in disabled, CRC32 and XXH3 mode (the hash fields are right, so every datagram returns 0).
Per workload and mode, in interleaved rounds after warm-up rounds — one call of each line per
round — with HIP events around each:
  (a) ingest     halo_kcp_ingest_device
  (b) copy_d2d   hipMemcpyAsync device to device of the stream bytes the call must read (the whole
                 stream when it hashes; the record and segment headers when it does not)
  (d) out_d2h    hipMemcpyAsync of the written dgram and seg arrays to pinned host memory
and, by the host's clock:
  (c) host       halo_kcp_ingest_host on one core over the same stream already in pinned host
                 memory — what a caller does today after the download it needs anyway
The median with minimum and maximum over the rounds is reported, with (a)/(b) and (c)/((a)+(d)).
Then, for mix8 in each mode, a ladder of datagram counts from 16 to 262,144, both sides by the
host's clock: (c) against (a) followed by (d) and a synchronise; the largest count at which (c)
still wins is reported. Prints one JSON line and, with --log, writes it there."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LADDER = [16, 64, 256, 1024, 4096, 16384, 65536, 262144]
PORT, CONV = 22102, 0x1122334455667788
D2H, D2D = 2, 3  # hipMemcpyKind
MODES = {"disabled": -1, "crc32": 1, "xxh3": 2}
PUSH, ACK, WASK, WINS = 81, 82, 83, 84


def payload_of(segments, mode: int) -> bytes:
    """One datagram: segment.encode (kcp.go:134-155) of each (cmd, data length)."""
    from oracle.ref_xxh3_py import xxh3_64

    out = b""
    for sn, (cmd, n) in enumerate(segments):
        data = bytes((7 * k + sn) % 251 for k in range(n))
        out += struct.pack("<QBBHIIII", CONV, cmd, 0, 256, 1000 + sn, sn, 0, n)
        if mode != -1:
            h = 0 if cmd != PUSH else (zlib.crc32(data) if mode == 1 else xxh3_64(data) & 0xFFFFFFFF)
            out += struct.pack("<I", h)
        out += data
    return out


WORKLOADS = {"ack": (1 << 20, [(ACK, 0)]), "push": (1 << 18, [(PUSH, 1368)]),
             "mix8": (1 << 18, [(ACK, 0), (PUSH, 24), (ACK, 0), (PUSH, 60), (WASK, 0), (PUSH, 120), (WINS, 0), (PUSH, 200)])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1, help="divide every datagram count by this")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=20)
    ap.add_argument("--log", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert a.rounds >= 20 and a.host_rounds >= 20, "at least 20 runs per line"
    import torch

    from halo_amd import _lib
    from tools.bench_egress import hip_memcpy_async

    assert torch.cuda.is_available(), "bench_kcp needs a GPU"
    dev = torch.device("cuda:0")
    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    L = _lib.lib
    stream = torch.cuda.current_stream().cuda_stream
    memcpy = hip_memcpy_async()

    def pinned(x: np.ndarray):
        t = torch.empty(max(x.nbytes, 16), dtype=torch.uint8).pin_memory()
        t.numpy()[:x.nbytes] = x.view(np.uint8).reshape(-1)
        return t

    def copy(dst, src, nbytes, kind):
        assert memcpy(_lib.ptr(dst), _lib.ptr(src), nbytes, kind, stream) == 0

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

    def setup(n, segments, mode):
        p = payload_of(segments, mode)
        rec = struct.pack("<IBBHIHHII", 0, 0, 0, len(p), 0x0A000001, 4000, PORT, 0, 0) + p
        rec += bytes(-len(rec) % 4)
        h_stream = np.tile(np.frombuffer(rec, np.uint8), n)
        h_index = np.zeros((n, 2), np.uint32)
        h_index[:, 0], h_index[:, 1] = np.arange(n), np.arange(n, dtype=np.uint64) * len(rec)
        h_dsum = np.zeros(1, _lib.DELIVER_SUMMARY_DTYPE)
        h_dsum["records"] = h_dsum["records_written"] = n
        h_dsum["bytes"] = h_dsum["bytes_written"] = h_stream.nbytes
        nseg = n * len(segments)
        cfg = _lib.KcpConfig()
        cfg.byte_check_mode, cfg.port, cfg.dgram_cap, cfg.seg_cap = mode, PORT, n, nseg
        wsb = int(L.halo_kcp_ingest_workspace(n, nseg))
        H = 28 if mode == -1 else 32
        must_read = h_stream.nbytes if mode != -1 else n * 24 + nseg * H
        return dict(n=n, per=len(segments), rec=len(rec), cfg=cfg, wsb=wsb, must_read=must_read, stream_bytes=h_stream.nbytes,
                    d_stream=torch.from_numpy(h_stream).to(dev), d_index=torch.from_numpy(h_index.view(np.int32)).to(dev),
                    d_dsum=torch.from_numpy(h_dsum.view(np.int64)).to(dev), h_dsum=h_dsum,
                    dg=torch.empty((n, 5), dtype=torch.int64, device=dev), sg=torch.empty((nseg, 4), dtype=torch.int64, device=dev),
                    sm=torch.empty(12, dtype=torch.int64, device=dev), ws=torch.empty(wsb // 8 + 1, dtype=torch.int64, device=dev),
                    copy_dst=torch.empty(max(must_read, 16), dtype=torch.uint8, device=dev), p_stream=pinned(h_stream),
                    p_index=pinned(h_index), p_out=torch.empty(40 * n + 32 * nseg, dtype=torch.uint8).pin_memory(),
                    h_dg=np.zeros((n, 40), np.uint8), h_sg=np.zeros((max(nseg, 1), 32), np.uint8), h_sm=np.zeros(96, np.uint8))

    def ingest(s, m=None):
        m = s["n"] if m is None else m
        _lib.check("halo_kcp_ingest_device", L.halo_kcp_ingest_device(
            ctypes.byref(s["cfg"]), _lib.ptr(s["d_stream"]), _lib.ptr(s["d_dsum"]), _lib.ptr(s["d_index"]), m, _lib.ptr(s["dg"]),
            _lib.ptr(s["sg"]), _lib.ptr(s["sm"]), _lib.ptr(s["ws"]), s["wsb"], stream))

    def out_d2h(s, m=None):
        m = s["n"] if m is None else m
        copy(s["p_out"], s["dg"], 40 * m, D2H)
        copy(s["p_out"][40 * s["n"]:], s["sg"], 32 * m * s["per"], D2H)

    def host(s, m=None):
        m = s["n"] if m is None else m
        rc = L.halo_kcp_ingest_host(ctypes.byref(s["cfg"]), _lib.ptr(s["p_stream"]), _lib.ptr(s["h_dsum"]), _lib.ptr(s["p_index"]), m,
                                    _lib.ptr(s["h_dg"]), _lib.ptr(s["h_sg"]), _lib.ptr(s["h_sm"]))
        assert rc == 0

    res = {"scale": a.scale, "rounds": a.rounds, "host_rounds": a.host_rounds, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "workloads": {}, "ladder": {}, "host_wins_up_to_dgrams": {}}
    for wname, (n, segments) in WORKLOADS.items():
        n = max(n // a.scale, 16)
        for mname, mode in MODES.items():
            s = setup(n, segments, mode)
            torch.cuda.synchronize()
            ev = timed_events({"ingest": lambda: ingest(s), "copy_d2d": lambda: copy(s["copy_dst"], s["d_stream"], s["must_read"], D2D),
                               "out_d2h": lambda: out_d2h(s)}, a.rounds, a.warmup)
            ck = timed_clock({"host": lambda: host(s)}, a.host_rounds, 1)
            summ = s["sm"].cpu().numpy().view(np.uint8).view(_lib.KCP_SUMMARY_DTYPE)[0]
            assert int(summ["dgrams_written"]) == n and int(summ["segs_written"]) == n * len(segments), (wname, mname, summ)
            assert int(summ["ret_counts"][0]) == n and int(summ["in_segs"]) == n * len(segments), (wname, mname, summ)
            assert summ == s["h_sm"].view(_lib.KCP_SUMMARY_DTYPE)[0], (wname, mname)
            out_d2h(s)
            torch.cuda.synchronize()
            got = s["p_out"].numpy()
            assert np.array_equal(got[:40 * n], s["h_dg"].reshape(-1)) and np.array_equal(got[40 * n:], s["h_sg"].reshape(-1)[:32 * n * len(segments)])
            w = {"dgrams": n, "segs": n * len(segments), "stream_bytes": s["stream_bytes"], "must_read_bytes": s["must_read"],
                 "out_bytes": 40 * n + 32 * n * len(segments), "bytes_hashed": int(summ["bytes_hashed"]), **ev, **ck}
            w["ingest_over_copy_d2d"] = ev["ingest"]["us_median"] / ev["copy_d2d"]["us_median"]
            w["host_over_ingest_plus_d2h"] = ck["host"]["us_median"] / (ev["ingest"]["us_median"] + ev["out_d2h"]["us_median"])
            w["read_gbytes_per_s"] = s["must_read"] / ev["ingest"]["us_median"] / 1e3
            res["workloads"][f"{wname}/{mname}"] = w
            if wname == "mix8":  # the ladder, both sides by the host's clock

                def device_side(m):
                    ingest(s, m)
                    out_d2h(s, m)

                lad = {}
                for m in [m for m in LADDER if m <= n]:
                    s["d_dsum"].view(torch.int32)[0:2] = m  # records = records_written = m
                    s["h_dsum"]["records"] = s["h_dsum"]["records_written"] = m
                    s["cfg"].dgram_cap, s["cfg"].seg_cap = m, m * s["per"]  # capacities sized to the call, as a caller would
                    lad[str(m)] = timed_clock({"host": lambda m=m: host(s, m), "ingest_then_d2h": lambda m=m: device_side(m)},
                                              a.host_rounds, 3)
                res["ladder"][mname] = lad
                wins = [int(m) for m, r in lad.items() if r["host"]["us_median"] < r["ingest_then_d2h"]["us_median"]]
                res["host_wins_up_to_dgrams"][mname] = max(wins) if wins else None
            del s
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
