"""Measure the NAT miss path: python tools/bench_nat_miss.py [--flows N] [--sizes ...]
[--runs K] [--warmup W].

A symmetric table of N flows, synced; batches of n LAN records that hit it, with four miss mixes:
no misses, 1 % new distinct flows, all-new distinct flows, one new key n times. Data resident, HIP
events for device time, wall time (synchronised) for the round trips, W warm-ups, then the median of
K runs with min-max. Per n and mix, one JSON line:
  (a) today's path: D2H of records, verdicts and ops, halo_nat_resolve_misses, H2D of the ops
  (b) resolve_misses_device, and its parts: collect, D2H of the count and the items,
      halo_nat_resolve_items, H2D of the answers, apply
  (c) collect alone, beside a device copy of the bytes it must read (records and verdicts) and the
      lookup_lan of the same records
Flows a run added are expired again before the next run (not timed), so every run meets the same
table; that expiry republishes the device copy, so the round trips that add flows at n > 65536 take
--big-runs runs after 2 warm-ups (the line's "wall_runs"). The one-key mix is the figure with the
i < o test; a build without the test is not kept, so it has no line here.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BASE_NOW, NEW_NOW, EXPIRE_NOW = 160, 100, 165  # 165 - 100 > 60: only the flows a run added leave


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=int, default=1 << 20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 4096, 1 << 20])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--big-runs", type=int, default=7, help="runs (2 warm-ups) of a round trip that adds flows at n > 65536")
    a = ap.parse_args()
    import torch

    from halo_amd import _lib
    from halo_amd._lib import NAT_MISS_ITEM_DTYPE, RESULT_DTYPE, TX_OP_DTYPE
    from halo_amd.nat import NatTable
    from halo_amd.route import ip_u

    dev = torch.device("cuda:0")
    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    rng = np.random.default_rng(1)
    LAN = _lib.FLOW_NAT_LAN
    t = NatTable(ip_u("203.0.113.1"), _lib.NAT_SYMMETRIC)
    base = np.zeros(a.flows, RESULT_DTYPE)
    base["ip_proto"] = rng.choice([6, 17], a.flows)
    base["src_ip"] = 0x0A000000 + np.arange(a.flows, dtype=np.uint32)
    base["sport"] = rng.integers(1024, 65536, a.flows)
    base["dst_ip"] = rng.integers(1 << 24, 0xDF000000, a.flows, dtype=np.uint64).astype(np.uint32)
    base["dport"] = rng.integers(1, 65536, a.flows)
    _, added = t.resolve_misses(LAN, base, np.full(a.flows, _lib.NAT_V_MISS, np.uint8), BASE_NOW, np.zeros(a.flows, TX_OP_DTYPE))
    assert added == a.flows
    t.sync()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "flows": a.flows, "runs": a.runs, "warmup": a.warmup}), flush=True)

    def stats(ms):
        return [round(float(np.median(ms)), 4), round(float(min(ms)), 4), round(float(max(ms)), 4)]

    def reset():
        torch.cuda.synchronize()
        t.TableClear(EXPIRE_NOW)

    def events(fn, mutate=False):
        ms = []
        for r in range(a.warmup + a.runs):
            if mutate:
                reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return stats(ms)

    def wall(fn, mutate=False):
        """fn returns a dict of part -> ms (or None); the total is measured around it, synchronised."""
        tot, parts = [], {}
        warm, runs = (2, a.big_runs) if mutate and n > 65536 else (a.warmup, a.runs)
        for r in range(warm + runs):
            if mutate:
                reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p = fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= warm:
                tot.append(dt)
                for k, v in (p or {}).items():
                    parts.setdefault(k, []).append(v)
        return stats(tot), {k: stats(v) for k, v in parts.items()}

    for n in a.sizes:
        pick = rng.integers(0, a.flows, n)
        hits = base[pick].copy()
        fresh = np.zeros(n, RESULT_DTYPE)
        fresh["ip_proto"], fresh["src_ip"], fresh["sport"] = 17, 0x0B000000 + np.arange(n, dtype=np.uint32), 2000
        fresh["dst_ip"], fresh["dport"] = rng.integers(1 << 24, 0xDF000000, n, dtype=np.uint64).astype(np.uint32), 53
        one = fresh.copy()
        one[:] = fresh[0]
        some = hits.copy()
        at = rng.choice(n, max(1, n // 100), replace=False)
        some[at] = fresh[at]
        for mix, recs in (("none", hits), ("1pct_new", some), ("all_new", fresh), ("one_key", one)):
            mutate = mix != "none"
            d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1, 32).copy()).to(dev)
            d_ops0 = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
            d_ops0[:, 0] = 0x02
            d_ops, d_verdict, d_ref, _ = t.lookup_lan(d_recs, BASE_NOW, ops=d_ops0.clone())
            torch.cuda.synchronize()
            misses = int((d_verdict == _lib.NAT_V_MISS).sum())
            ws = torch.empty(int(_lib.lib.halo_nat_miss_workspace(n, 0)) // 4, dtype=torch.int32, device=dev)
            line = {"n": n, "mix": mix, "misses": misses, "wall_runs": a.big_runs if mutate and n > 65536 else a.runs}

            # (a) today's path
            def today():
                ops = d_ops.clone()
                h_recs = d_recs.cpu().numpy().reshape(-1).view(RESULT_DTYPE)
                h_verdict = d_verdict.cpu().numpy()
                h_ops = ops.cpu().numpy().reshape(-1).view(TX_OP_DTYPE)
                t0 = time.perf_counter()
                t.resolve_misses(LAN, h_recs, h_verdict, NEW_NOW, h_ops)
                host = (time.perf_counter() - t0) * 1e3
                ops.copy_(torch.from_numpy(h_ops.view(np.uint8).reshape(-1, 16)))
                return {"resolve_misses_ms": host}

            line["a_today_wall_ms"], line["a_parts"] = wall(today, mutate)

            # (b) the miss path, whole and in parts
            def device_path():
                ops, verdict, ref = d_ops.clone(), d_verdict.clone(), d_ref.clone()
                t.resolve_misses_device(LAN, d_recs, ops, verdict, ref, NEW_NOW)

            line["b_device_wall_ms"], _ = wall(device_path, mutate)

            def device_parts():
                ops, verdict, ref = d_ops.clone(), d_verdict.clone(), d_ref.clone()
                torch.cuda.synchronize()
                p = {}
                t0 = time.perf_counter()
                items, count, pos = t.collect_misses(LAN, d_recs, verdict, workspace=ws)
                torch.cuda.synchronize()
                p["collect_ms"] = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                k = int(count.cpu().numpy().view(np.uint32)[0])
                host = items[:k].cpu().numpy().reshape(-1).view(NAT_MISS_ITEM_DTYPE)
                p["d2h_items_ms"] = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                answers, _ = t.resolve_items(LAN, host, NEW_NOW)
                p["resolve_items_ms"] = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                d_ans = torch.from_numpy(answers.view(np.uint8).reshape(-1, 16)).to(dev)
                torch.cuda.synchronize()
                p["h2d_answers_ms"] = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                if k:
                    t.apply_answers(LAN, pos, d_ans, ops, verdict, ref)
                torch.cuda.synchronize()
                p["apply_ms"] = (time.perf_counter() - t0) * 1e3
                p["items"] = k
                return p

            _, line["b_parts_wall"] = wall(device_parts, mutate)

            # (c) collect alone (device time), beside a copy of its input bytes and the lookup
            line["c_collect_ms"] = events(lambda: t.collect_misses(LAN, d_recs, d_verdict, workspace=ws))
            r2, v2 = torch.empty_like(d_recs), torch.empty_like(d_verdict)

            def copy_inputs():
                r2.copy_(d_recs)
                v2.copy_(d_verdict)

            line["c_copy_inputs_ms"] = events(copy_inputs)
            scratch_ops = d_ops0.clone()
            line["c_lookup_lan_ms"] = events(lambda: t.lookup_lan(d_recs, BASE_NOW, ops=scratch_ops))
            pos1 = t.collect_misses(LAN, d_recs, d_verdict, workspace=ws)[2]
            k1 = max(1, misses if mix != "one_key" else 1)
            ans1 = torch.zeros((k1, 16), dtype=torch.uint8, device=dev)  # verdict 0: nothing is written
            v1, f1 = d_verdict.clone(), d_ref.clone()
            line["c_apply_ms"] = events(lambda: t.apply_answers(LAN, pos1, ans1, scratch_ops, v1, f1))
            reset()
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
