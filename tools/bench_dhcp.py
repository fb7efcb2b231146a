"""Measure the DHCP decode and reply build: python tools/bench_dhcp.py [--scale S]
[--rounds K] [--warmup W] [--log PATH].

A delivery stream resident in HBM (made here record by record: 24-byte header, one 68 -> 67 DHCP
payload, padding), its summary and index, outputs and workspace preallocated:
  disc20   2^20 minimal DISCOVERs (244 bytes: the fixed 240, option 53, 0xff)
  disc16   2^16 of the same
  mix      2^18 messages cycling through a DISCOVER with an 8-byte hostname, a REQUEST with option
           50 and a 20-byte hostname, a REQUEST with a client id, a parameter list, option 50 and a
           63-byte hostname, and a RELEASE
Per workload, in interleaved rounds after warm-up rounds — one call of each line per round — with
HIP events around each:
  (a) decode      halo_dhcp_decode_device
  (b) copy_d2d    hipMemcpyAsync device to device of HALF the bytes the call must read plus write
                  (a copy of N bytes reads N and writes N): per record the 24 header bytes, the 20
                  bytes of xid, yiaddr, chaddr and cookie and the option bytes up to the end mark,
                  plus the 128 bytes of its message record
  (d) out_d2h     hipMemcpyAsync of the written message records to pinned host memory
  (s) stream_d2h  the same for the whole stream: the download the host path needs first
and, by the host's clock:
  (c) host        halo_dhcp_decode_host on one core over the same stream already in pinned memory
The same for the reply build over 2^20 and 2^16 replies of mixed kinds: (a) build, (b) copy_d2d of
half of (32 + 288 + 40) bytes per reply, (c) halo_dhcp_reply_build_host into pinned memory, (d)
replies_h2d, the upload of the 32-byte descriptors the device path needs, and built_h2d, the upload
of the 328 bytes per reply the host path produces. The median with minimum and maximum over the
rounds is reported, with (a)/(b) and (c)/((a)+(d)). Then two ladders from 16 to 262,144 messages,
both sides by the host's clock: decode_host against decode followed by out_d2h and a synchronise
(mix), and build_host followed by built_h2d against replies_h2d followed by the build, each with a
synchronise; the largest count at which the host side still wins is reported. Prints one JSON
line and, with --log, writes it there."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LADDER = [16, 64, 256, 1024, 4096, 16384, 65536, 262144]
H2D, D2H, D2D = 1, 2, 3  # hipMemcpyKind
MAC = bytes([2, 0, 0, 0, 0, 9])


def message(opts) -> bytes:
    fixed = bytes([1, 1, 6, 0, 1, 2, 3, 4, 0, 0, 0x80, 0]) + bytes(16) + MAC + bytes(10 + 64 + 128) + bytes([0x63, 0x82, 0x53, 0x63])
    return fixed + b"".join(bytes([c, len(d)]) + bytes(d) for c, d in opts) + b"\xff"


MINIMAL = [message([(53, [1])])]
MIX = [message([(53, [1]), (12, b"desk-042")]),
       message([(53, [3]), (50, [192, 168, 1, 77]), (12, b"a-twenty-byte-name-x")]),
       message([(53, [3]), (61, b"\x01" + MAC), (55, [1, 3, 6, 15, 31, 33, 43, 44, 46, 47]), (50, [192, 168, 1, 78]), (12, b"n" * 63)]),
       message([(53, [7])])]
WORKLOADS = {"disc20": (1 << 20, MINIMAL), "disc16": (1 << 16, MINIMAL), "mix": (1 << 18, MIX)}
BUILD_SIZES = {"build20": 1 << 20, "build16": 1 << 16}
REPLY_KINDS = [2, 5, 6, 5, 2, 3, 1, 5]  # OFFER ACK NAK ACK OFFER REQUEST DISCOVER ACK


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1, help="divide every message count by this")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=20)
    ap.add_argument("--log", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert a.rounds >= 20 and a.host_rounds >= 20, "at least 20 runs per line"
    import torch

    from halo_amd import _lib
    from tools.bench_egress import hip_memcpy_async

    assert torch.cuda.is_available(), "bench_dhcp needs a GPU"
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

    def ladder(n, host_fn, device_fn, set_count):
        lad = {}
        for m in [m for m in LADDER if m <= n]:
            set_count(m)
            lad[str(m)] = timed_clock({"host": lambda m=m: host_fn(m), "device": lambda m=m: device_fn(m)}, a.host_rounds, 3)
        wins = [int(m) for m, r in lad.items() if r["host"]["us_median"] < r["device"]["us_median"]]
        return lad, (max(wins) if wins else None)

    # ---- decode ---------------------------------------------------------------------------------
    def setup(n, payloads):
        recs = []
        for p in payloads:
            r = struct.pack("<IBBHIHHII", 0, 2, 0, len(p), 0x0A000001, 68, 67, 0, 0) + p
            recs.append(np.frombuffer(r + bytes(-len(r) % 4), np.uint8))
        reps = n // len(recs)
        assert reps * len(recs) == n
        h_stream = np.tile(np.concatenate(recs), reps)
        sizes = np.tile(np.array([len(r) for r in recs], np.uint64), reps)
        h_index = np.zeros((n, 2), np.uint32)
        h_index[:, 0], h_index[:, 1] = np.arange(n), np.cumsum(sizes) - sizes
        h_dsum = np.zeros(1, _lib.DELIVER_SUMMARY_DTYPE)
        h_dsum["records"] = h_dsum["records_written"] = n
        h_dsum["bytes"] = h_dsum["bytes_written"] = h_stream.nbytes
        wsb = int(L.halo_dhcp_decode_workspace(n))
        must_read = reps * sum(24 + 20 + len(p) - 240 for p in payloads)
        return dict(n=n, wsb=wsb, must_read=must_read, stream_bytes=h_stream.nbytes, d_stream=torch.from_numpy(h_stream).to(dev),
                    d_index=torch.from_numpy(h_index.view(np.int32)).to(dev), d_dsum=torch.from_numpy(h_dsum.view(np.int64)).to(dev),
                    h_dsum=h_dsum, mg=torch.empty((n, 16), dtype=torch.int64, device=dev), sm=torch.empty(8, dtype=torch.int64, device=dev),
                    ws=torch.empty(wsb // 8 + 1, dtype=torch.int64, device=dev),
                    copy_dst=torch.empty(max(h_stream.nbytes, 128 * n), dtype=torch.uint8, device=dev), p_stream=pinned(h_stream),
                    p_index=pinned(h_index), p_out=torch.empty(128 * n, dtype=torch.uint8).pin_memory(),
                    p_down=torch.empty(h_stream.nbytes, dtype=torch.uint8).pin_memory(), h_mg=np.zeros((n, 128), np.uint8),
                    h_sm=np.zeros(64, np.uint8))

    def decode(s, m=None):
        m = s["n"] if m is None else m
        _lib.check("halo_dhcp_decode_device", L.halo_dhcp_decode_device(
            _lib.ptr(s["d_stream"]), _lib.ptr(s["d_dsum"]), _lib.ptr(s["d_index"]), m, _lib.ptr(s["mg"]), m, _lib.ptr(s["sm"]),
            _lib.ptr(s["ws"]), s["wsb"], stream))

    def decode_host(s, m=None):
        m = s["n"] if m is None else m
        assert L.halo_dhcp_decode_host(_lib.ptr(s["p_stream"]), _lib.ptr(s["h_dsum"]), _lib.ptr(s["p_index"]), m, _lib.ptr(s["h_mg"]), m,
                                       _lib.ptr(s["h_sm"])) == 0

    res = {"scale": a.scale, "rounds": a.rounds, "host_rounds": a.host_rounds, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "decode": {}, "build": {}, "ladder": {}, "host_wins_up_to": {}}
    for wname, (n, payloads) in WORKLOADS.items():
        n = max(n // a.scale, 16)
        s = setup(n, payloads)
        torch.cuda.synchronize()
        moved = s["must_read"] + 128 * n
        ev = timed_events({"decode": lambda: decode(s), "copy_d2d": lambda: copy(s["copy_dst"], s["d_stream"], moved // 2, D2D),
                           "out_d2h": lambda: copy(s["p_out"], s["mg"], 128 * n, D2H),
                           "stream_d2h": lambda: copy(s["p_down"], s["d_stream"], s["stream_bytes"], D2H)}, a.rounds, a.warmup)
        ck = timed_clock({"host": lambda: decode_host(s)}, a.host_rounds, 1)
        summ = s["sm"].cpu().numpy().view(np.uint8).view(_lib.DHCP_SUMMARY_DTYPE)[0]
        assert int(summ["msgs_written"]) == n == int(summ["status_counts"][0]), (wname, summ)
        assert summ == s["h_sm"].view(_lib.DHCP_SUMMARY_DTYPE)[0], wname
        copy(s["p_out"], s["mg"], 128 * n, D2H)
        torch.cuda.synchronize()
        assert np.array_equal(s["p_out"].numpy(), s["h_mg"].reshape(-1)), wname
        w = {"msgs": n, "stream_bytes": s["stream_bytes"], "must_read_bytes": s["must_read"], "out_bytes": 128 * n, **ev, **ck}
        w["decode_over_copy_d2d"] = ev["decode"]["us_median"] / ev["copy_d2d"]["us_median"]
        w["host_over_decode_plus_d2h"] = ck["host"]["us_median"] / (ev["decode"]["us_median"] + ev["out_d2h"]["us_median"])
        w["moved_gbytes_per_s"] = moved / ev["decode"]["us_median"] / 1e3
        res["decode"][wname] = w
        if wname == "mix":  # the ladder, both sides by the host's clock

            def set_count(m):
                s["d_dsum"].view(torch.int32)[0:2] = m  # records = records_written = m
                s["h_dsum"]["records"] = s["h_dsum"]["records_written"] = m

            def device_side(m):
                decode(s, m)
                copy(s["p_out"], s["mg"], 128 * m, D2H)

            res["ladder"]["decode"], res["host_wins_up_to"]["decode"] = ladder(n, lambda m: decode_host(s, m), device_side, set_count)
        del s
        torch.cuda.empty_cache()

    # ---- reply build ----------------------------------------------------------------------------
    cfg = _lib.DhcpConfig()
    cfg.ip, cfg.network_mask, cfg.dns = 0xC0A80101, 0xFFFFFF00, 0x08080808
    for bname, n in BUILD_SIZES.items():
        n = max(n // a.scale, 16)
        r = np.zeros(n, _lib.DHCP_REPLY_DTYPE)
        r["kind"] = np.resize(np.array(REPLY_KINDS, np.uint8), n)
        r["xid"] = np.arange(4 * n, dtype=np.uint32).reshape(n, 4) & 0xFF
        r["yiaddr"], r["req_ip"], r["server_id"] = 0xC0A80100 + np.arange(n) % 250, 0xC0A80142, 0xC0A80101
        r["chaddr"][:] = list(MAC)
        p_replies = pinned(r)
        d_replies = torch.from_numpy(r.view(np.int64)).to(dev)
        d_payload = torch.empty(36 * n, dtype=torch.int64, device=dev)
        d_descs = torch.empty(5 * n, dtype=torch.int64, device=dev)
        p_built = torch.empty(328 * n, dtype=torch.uint8).pin_memory()
        d_up = torch.empty(328 * n, dtype=torch.uint8, device=dev)
        copy_dst = torch.empty(180 * n, dtype=torch.uint8, device=dev)

        def build(m=n):
            _lib.check("halo_dhcp_reply_build_device", L.halo_dhcp_reply_build_device(
                ctypes.byref(cfg), _lib.ptr(d_replies), m, _lib.ptr(d_payload), _lib.ptr(d_descs), stream))

        def build_host(m=n):
            assert L.halo_dhcp_reply_build_host(ctypes.byref(cfg), _lib.ptr(p_replies), m, _lib.ptr(p_built), _lib.ptr(p_built) + 288 * n) == 0

        ev = timed_events({"build": build, "copy_d2d": lambda: copy(copy_dst, d_payload, 180 * n, D2D),
                           "replies_h2d": lambda: copy(d_replies, p_replies, 32 * n, H2D),
                           "built_h2d": lambda: copy(d_up, p_built, 328 * n, H2D)}, a.rounds, a.warmup)
        ck = timed_clock({"host": build_host}, a.host_rounds, 1)
        torch.cuda.synchronize()
        got = np.concatenate([d_payload.cpu().numpy().view(np.uint8), d_descs.cpu().numpy().view(np.uint8)])
        assert np.array_equal(got, p_built.numpy()), bname
        w = {"replies": n, "in_bytes": 32 * n, "out_bytes": 328 * n, **ev, **ck}
        w["build_over_copy_d2d"] = ev["build"]["us_median"] / ev["copy_d2d"]["us_median"]
        w["host_plus_h2d_over_h2d_plus_build"] = (ck["host"]["us_median"] + ev["built_h2d"]["us_median"]) / (
            ev["replies_h2d"]["us_median"] + ev["build"]["us_median"])
        w["moved_gbytes_per_s"] = 360 * n / ev["build"]["us_median"] / 1e3
        res["build"][bname] = w
        if bname == "build20":

            def host_side(m):
                build_host(m)
                copy(d_up, p_built, 288 * m, H2D)
                copy(d_up[288 * n:], p_built[288 * n:], 40 * m, H2D)

            def device_side(m):
                copy(d_replies, p_replies, 32 * m, H2D)
                build(m)

            res["ladder"]["build"], res["host_wins_up_to"]["build"] = ladder(n, host_side, device_side, lambda m: None)
        del d_replies, d_payload, d_descs, d_up, copy_dst
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
