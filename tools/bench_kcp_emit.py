"""Measure KCP emit: python tools/bench_kcp_emit.py [--scale S] [--rounds K]
[--warmup W] [--log PATH].

A flush batch resident in HBM — entries, segment descriptors and the payload the descriptors point
into (each session's data one byte further on than a multiple of its size, so source alignments
rotate) — outputs and workspace preallocated:
  ack      2^20 sessions of one empty ACK segment each
  push     2^18 sessions of one 1,368-byte PUSH segment (a full 1,400-byte MTU datagram)
  mix8     2^18 sessions of 8 small segments: ACK, PUSH 24 B, ACK, PUSH 60 B, WASK, PUSH 120 B, WINS, PUSH 200 B
each in disabled, CRC32 and XXH3 mode, mtu 1400. Per workload and mode, in interleaved rounds after
warm-up rounds — one call of each line per round — with HIP events around each:
  (a) emit       halo_kcp_emit_device
  (b) copy_d2d   hipMemcpyAsync device to device of HALF the bytes the call must read plus write
                 (entries, descriptors and data in; stream, records, descriptors and status out), so
                 that the copy moves as many bytes as the call must
  (d) up_h2d     hipMemcpyAsync of the host-built stream, records and descriptors from pinned memory
and, by the host's clock:
  (c) host       halo_kcp_emit_host on one core over the same batch in pinned host memory
The median with minimum and maximum over the rounds is reported, with (a)/(b) and ((c)+(d))/(a).
Then, for mix8 in each mode, a ladder of session counts from 16 to 262,144, both sides by the
host's clock: (c) followed by (d) and a synchronise against (a) and a synchronise; the largest
count at which the host side still wins is reported. Prints one JSON line and, with --log, writes
it there."""
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
PORT, CONV, MTU = 22102, 0x1122334455667788, 1400
H2D, D2D = 1, 3  # hipMemcpyKind
MODES = {"disabled": -1, "crc32": 1, "xxh3": 2}
PUSH, ACK, WASK, WINS = 81, 82, 83, 84
WORKLOADS = {"ack": (1 << 20, [(ACK, 0)]), "push": (1 << 18, [(PUSH, 1368)]),
             "mix8": (1 << 18, [(ACK, 0), (PUSH, 24), (ACK, 0), (PUSH, 60), (WASK, 0), (PUSH, 120), (WINS, 0), (PUSH, 200)])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1, help="divide every session count by this")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=20)
    ap.add_argument("--log", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert a.rounds >= 20 and a.host_rounds >= 20, "at least 20 runs per line"
    import torch

    from halo_amd import _lib
    from tools.bench_egress import hip_memcpy_async

    assert torch.cuda.is_available(), "bench_kcp_emit needs a GPU"
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
        per = len(segments)
        H = 28 if mode == -1 else 32
        data_per = sum(ln for _, ln in segments)
        stride = data_per + 1  # the next session's data starts one byte further on
        k = np.arange(n, dtype=np.uint64)
        ss = np.zeros(n, _lib.KCP_OUT_SESSION_DTYPE)
        ss["conv"], ss["first_seg"], ss["n_segs"], ss["mtu"] = CONV + k, k * per, per, MTU
        ss["dst_ip"], ss["dst_port"] = 0x0A000000 + (k & 0xFFFFFF), 4000 + (k & 0xFFF)
        sg = np.zeros((n, per), _lib.KCP_SEG_DTYPE)
        at = 0
        for i, (cmd, ln) in enumerate(segments):
            sg["cmd"][:, i], sg["wnd"][:, i], sg["ts"][:, i], sg["sn"][:, i], sg["len"][:, i] = cmd, 256, 1000 + i, k * per + i, ln
            sg["data_off"][:, i] = k * stride + at
            at += ln
        pay_bytes = n * stride
        rng = np.random.default_rng(7)
        pay = np.tile(rng.integers(0, 256, 65521, dtype=np.uint8), pay_bytes // 65521 + 1)[:(pay_bytes + 3) & ~3].copy()
        size = per * H + data_per
        assert size <= MTU  # one datagram per session
        nd, out_stream = n, n * ((size + 3) & ~3)
        cfg = _lib.KcpEmitConfig()
        cfg.byte_check_mode, cfg.src_ip, cfg.src_port, cfg.dgram_cap, cfg.stream_cap = mode, 0x0A0000FE, PORT, nd, out_stream
        wsb = int(L.halo_kcp_emit_workspace(n, n * per))
        must_read = 40 * n + 32 * n * per + n * data_per
        must_write = out_stream + 56 * nd + n
        return dict(n=n, per=per, cfg=cfg, wsb=wsb, must_read=must_read, must_write=must_write, out_stream=out_stream, size=size,
                    pay_bytes=pay_bytes, d_ss=torch.from_numpy(ss.view(np.int64)).to(dev),
                    d_sg=torch.from_numpy(sg.reshape(-1).view(np.int64)).to(dev), d_pay=torch.from_numpy(pay.view(np.int32)).to(dev),
                    d_out=torch.empty(out_stream // 4 + 2, dtype=torch.int32, device=dev),
                    d_dg=torch.empty((nd, 2), dtype=torch.int64, device=dev), d_ds=torch.empty((nd, 5), dtype=torch.int64, device=dev),
                    d_st=torch.empty(n, dtype=torch.uint8, device=dev), sm=torch.empty(11, dtype=torch.int64, device=dev),
                    ws=torch.empty(wsb // 8 + 1, dtype=torch.int64, device=dev),
                    copy_src=torch.empty((must_read + must_write) // 2 + 16, dtype=torch.uint8, device=dev),
                    copy_dst=torch.empty((must_read + must_write) // 2 + 16, dtype=torch.uint8, device=dev),
                    p_ss=pinned(ss), p_sg=pinned(sg.reshape(-1)), p_pay=pinned(pay),
                    p_out=torch.empty(out_stream + 16, dtype=torch.uint8).pin_memory(), p_dg=torch.empty(16 * nd, dtype=torch.uint8).pin_memory(),
                    p_ds=torch.empty(40 * nd, dtype=torch.uint8).pin_memory(), h_st=np.zeros(n, np.uint8), h_sm=np.zeros(88, np.uint8))

    def emit(s, m=None):
        m = s["n"] if m is None else m
        _lib.check("halo_kcp_emit_device", L.halo_kcp_emit_device(
            ctypes.byref(s["cfg"]), _lib.ptr(s["d_ss"]), m, _lib.ptr(s["d_sg"]), m * s["per"], _lib.ptr(s["d_pay"]), s["pay_bytes"],
            _lib.ptr(s["d_out"]), _lib.ptr(s["d_dg"]), _lib.ptr(s["d_ds"]), _lib.ptr(s["d_st"]), _lib.ptr(s["sm"]), _lib.ptr(s["ws"]),
            s["wsb"], stream))

    def host(s, m=None):
        m = s["n"] if m is None else m
        rc = L.halo_kcp_emit_host(ctypes.byref(s["cfg"]), _lib.ptr(s["p_ss"]), m, _lib.ptr(s["p_sg"]), m * s["per"], _lib.ptr(s["p_pay"]),
                                  s["pay_bytes"], _lib.ptr(s["p_out"]), _lib.ptr(s["p_dg"]), _lib.ptr(s["p_ds"]), _lib.ptr(s["h_st"]),
                                  _lib.ptr(s["h_sm"]))
        assert rc == 0

    def up_h2d(s, m=None):
        m = s["n"] if m is None else m
        copy(s["d_out"], s["p_out"], m * ((s["size"] + 3) & ~3), H2D)
        copy(s["d_dg"], s["p_dg"], 16 * m, H2D)
        copy(s["d_ds"], s["p_ds"], 40 * m, H2D)

    res = {"scale": a.scale, "rounds": a.rounds, "host_rounds": a.host_rounds, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "workloads": {}, "ladder": {}, "host_wins_up_to_sessions": {}}
    for wname, (n, segments) in WORKLOADS.items():
        n = max(n // a.scale, 16)
        for mname, mode in MODES.items():
            s = setup(n, segments, mode)
            torch.cuda.synchronize()
            half = (s["must_read"] + s["must_write"]) // 2
            ck = timed_clock({"host": lambda: host(s)}, a.host_rounds, 1)  # first: up_h2d uploads what it built
            ev = timed_events({"emit": lambda: emit(s), "copy_d2d": lambda: copy(s["copy_dst"], s["copy_src"], half, D2D),
                               "up_h2d": lambda: up_h2d(s)}, a.rounds, a.warmup)
            emit(s)
            torch.cuda.synchronize()
            summ = s["sm"].cpu().numpy().view(np.uint8).view(_lib.KCP_EMIT_SUMMARY_DTYPE)[0]
            assert int(summ["dgrams_written"]) == n and int(summ["segs_written"]) == n * len(segments), (wname, mname, summ)
            assert int(summ["bytes_written"]) == s["out_stream"] and summ == s["h_sm"].view(_lib.KCP_EMIT_SUMMARY_DTYPE)[0], (wname, mname)
            got = s["d_out"].cpu().numpy().view(np.uint8)[:s["out_stream"]]
            assert np.array_equal(got, s["p_out"].numpy()[:s["out_stream"]]), (wname, mname, "stream")
            assert np.array_equal(s["d_dg"].cpu().numpy().view(np.uint8).reshape(-1), s["p_dg"].numpy())
            assert np.array_equal(s["d_ds"].cpu().numpy().view(np.uint8).reshape(-1), s["p_ds"].numpy())
            w = {"sessions": n, "segs": n * len(segments), "must_read_bytes": s["must_read"], "must_write_bytes": s["must_write"],
                 "copy_bytes": half, "bytes_hashed": int(summ["bytes_hashed"]), **ev, **ck}
            w["emit_over_copy_d2d"] = ev["emit"]["us_median"] / ev["copy_d2d"]["us_median"]
            w["host_plus_h2d_over_emit"] = (ck["host"]["us_median"] + ev["up_h2d"]["us_median"]) / ev["emit"]["us_median"]
            w["moved_gbytes_per_s"] = (s["must_read"] + s["must_write"]) / ev["emit"]["us_median"] / 1e3
            res["workloads"][f"{wname}/{mname}"] = w
            print(f"{wname}/{mname}: emit {ev['emit']['us_median']:.0f} us, copy {ev['copy_d2d']['us_median']:.0f} us, "
                  f"host {ck['host']['us_median']:.0f} us, h2d {ev['up_h2d']['us_median']:.0f} us", file=sys.stderr, flush=True)
            if wname == "mix8":  # the ladder, both sides by the host's clock

                def host_side(m):
                    host(s, m)
                    up_h2d(s, m)

                lad = {}
                for m in [m for m in LADDER if m <= n]:
                    s["cfg"].dgram_cap, s["cfg"].stream_cap = m, m * ((s["size"] + 3) & ~3)  # capacities sized to the call
                    lad[str(m)] = timed_clock({"host_then_h2d": lambda m=m: host_side(m), "emit": lambda m=m: emit(s, m)}, a.host_rounds, 3)
                res["ladder"][mname] = lad
                wins = [int(m) for m, r in lad.items() if r["host_then_h2d"]["us_median"] < r["emit"]["us_median"]]
                res["host_wins_up_to_sessions"][mname] = max(wins) if wins else None
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
