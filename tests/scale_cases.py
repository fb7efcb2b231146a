"""Not a test: where each forwarding kernel changes behaviour with the batch size, and how the
scale tests (tests/test_scale_shapes.py on the CPU, tests/test_gpu_scale.py on the device) get
their shapes and their expected values.

BOUNDARIES is the table: per kernel the source file, the constants its launch code derives the edge
from, and the first `n` past the edge. `read_constants` takes those constants out of the .hip
sources with plain regular expressions and `derived` recomputes every threshold from them, so a
moved cap fails the CPU suite until the table and the shapes move with it. Every shape of the GPU
tests is `past(name) + r` with a small r that is no multiple of 64 or of 4: the second trip ends
in a partial wave (and, for lpm_kernel, in the n % 4 tail loop).

The ARP and NAT references are Python dict models, far too slow for 0.5-4 M items. Those kernels
are stateless per item, so the device input is a period of P = 1000 items (no multiple of 64: a
case's lane and block position shifts from one repeat to the next) repeated q times plus its first
r items, and the expectation is the model's answer for the period repeated the same way.
tests/test_scale_shapes.py checks on the CPU that the models do answer a repeated item the same."""
from __future__ import annotations

import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo_amd", "csrc")
P = 1000  # items per period

# kernel(s) -> file, the constants the boundary follows from, the first n past it (as the launch
# code gives it today), and the test of tests/test_gpu_scale.py that crosses it (or why none does)
BOUNDARIES = {
    "arp_scan_lane": dict(kernels="arp_scan_kernel: second lane", file="arp_fwd.hip",
                          constants=("kGatherTile", "arp_pass"), first_past=1_025, test="test_arp_gather[300 tiles]"),
    "arp_scan_wave": dict(kernels="arp_scan_kernel: second wave", file="arp_fwd.hip",
                          constants=("kGatherTile", "arp_pass"), first_past=65_537, test="test_arp_gather[second wave]"),
    "arp_scan_pass": dict(kernels="arp_scan_kernel: second pass", file="arp_fwd.hip",
                          constants=("kGatherTile", "arp_pass"), first_past=262_145, test="test_arp_gather[second pass]"),
    "arp_trip": dict(kernels="arp_lookup_kernel, arp_encap_kernel", file="arp_fwd.hip", constants=("arp_blocks",),
                     first_past=524_289, test="test_arp_lookup_second_trip, test_arp_encap_second_trip"),
    "sw_scan_pass": dict(kernels="sw_scan_kernel", file="switch_fwd.hip", constants=("kTile", "sw_pass"),
                         first_past=262_145, test="test_switch_scale[new_macs], [differential]"),
    "sw_resolve_trip": dict(kernels="sw_resolve_kernel", file="switch_fwd.hip", constants=("kTile", "sw_resolve_cap"),
                            first_past=524_289, test="test_switch_scale[differential]"),
    "sw_rebuild_trip": dict(kernels="sw_rebuild_kernel (table slots)", file="switch_fwd.hip", constants=("sw_rebuild_cap",),
                            first_past=524_289, test="test_switch_scale[rebuild]"),
    "nat_trip": dict(kernels="nat_lookup_kernel<KIND,COMPACT>, nat_quote_kernel", file="nat_lookup.hip",
                     constants=("nat_blocks",), first_past=4_194_305, test="test_nat_lookup_second_trip, test_nat_quote_second_trip"),
    "lpm_trip": dict(kernels="lpm_kernel (4 addresses per lane)", file="route_lpm.hip", constants=("lpm_blocks",),
                     first_past=16_777_217, test="test_route_second_trip"),
    "lpm_records_trip": dict(kernels="lpm_records_kernel", file="route_lpm.hip", constants=("lpm_blocks",),
                             first_past=4_194_305, test="test_route_records_second_trip"),
    "flow_hash_trip": dict(kernels="flow_hash_kernel<COMPACT>", file="flow_hash.hip", constants=("blocks_for",),
                           first_past=4_194_305, test="test_flow_hash_second_trip"),
    "tx_g16_trip": dict(kernels="tx_fixup_kernel<16>", file="tx_fixup.hip", constants=("tx_waves",), first_past=262_145,
                        test="test_tx_fixup_second_trip[hint 0]"),
    "tx_g8_trip": dict(kernels="tx_fixup_kernel<8>", file="tx_fixup.hip", constants=("tx_waves",), first_past=524_289,
                       test="test_tx_fixup_second_trip[hint 4000]"),
    "tx_g4_trip": dict(kernels="tx_fixup_kernel<4>", file="tx_fixup.hip", constants=("tx_waves",), first_past=1_048_577,
                       test="test_tx_fixup_second_trip[hint 1000]"),
    "tx_g1_trip": dict(kernels="tx_fixup_kernel<1>", file="tx_fixup.hip", constants=("tx_waves",), first_past=4_194_305,
                       test="test_tx_fixup_second_trip[hint 64]"),
    # halo_tx_build_batch_device: HALO_TXB_MAX_BLOCKS (= HALO_TXB_G1_WAVES * 256) blocks of kBlock / 64 waves, a
    # 64-descriptor tile per wave and trip whatever the lanes per frame (with HALO_TXB_SPLIT waves per
    # tile the 16-lane build's cap grows by the same factor)
    "txb_g1_trip": dict(kernels="tx_build_kernel<1,4>", file="tx_build.hip",
                        constants=("txb_g1_waves", "txb_blocks_per_wave", "txb_kBlock", "txb_kTile"), first_past=262_145,
                        test="test_tx_build_second_trip[G1]"),
    "txb_g4_trip": dict(kernels="tx_build_kernel<4,4>", file="tx_build.hip",
                        constants=("txb_g1_waves", "txb_blocks_per_wave", "txb_kBlock", "txb_kTile"), first_past=262_145,
                        test="test_tx_build_second_trip[G4]"),
    "txb_g8_trip": dict(kernels="tx_build_kernel<8,4>", file="tx_build.hip",
                        constants=("txb_g1_waves", "txb_blocks_per_wave", "txb_kBlock", "txb_kTile"), first_past=262_145,
                        test="test_tx_build_second_trip[G8]"),
    "txb_g16_trip": dict(kernels="tx_build_kernel<16,4>", file="tx_build.hip",
                         constants=("txb_g1_waves", "txb_blocks_per_wave", "txb_kBlock", "txb_kTile", "txb_split"),
                         first_past=262_145, test="test_tx_build_second_trip[G16]"),
    # tx_finish_kernel's full path: every block scans the tile counts txb_finish_pass at a time
    "txb_finish_pass": dict(kernels="tx_finish_kernel: second scan pass", file="tx_build.hip",
                            constants=("txb_finish_pass", "txb_kTile"), first_past=65_537,
                            test="tests/test_gpu_tx_build.py::test_build_rejections_then_clean_launch (n = 70,000); "
                                 "test_tx_build_second_trip (five passes)"),
    # tx_build_pair_kernel has no grid-stride loop and no cap: the grid is ceil(n / 512) * 64 blocks of
    # four waves, a pair of frames per wave. No edge today; its case runs at the grid-stride kernels' n
    # so that a cap put on that grid meets a test.
    "txb_pair_grid": dict(kernels="tx_build_pair_kernel<3> (no grid-stride loop: grid = ceil(n / 512) * 64 blocks)",
                          file="tx_build.hip", constants=("txb_pair_run", "txb_pair_run_blocks", "txb_kBlock"),
                          first_past=None, test="test_tx_build_second_trip[pair]"),
    # halo_xxh3_64_batch_device launches xxh3_run_kernel alone: one 64-lane block per window of kRunWin
    # strings, no grid-stride loop and no cap (grid = ceil(n / kRunWin)). No edge today; the named tests
    # cross a window edge (20,000 strings: 79 windows, the last one 32 strings), and the launch
    # expression is matched in read_constants so that a cap put on that grid meets a test.
    "xxh3_run_grid": dict(kernels="xxh3_run_kernel (no grid-stride loop: grid = ceil(n / kRunWin) one-wave blocks)",
                          file="flow_hash.hip", constants=("kRunWin",), first_past=None,
                          test="tests/test_gpu_flow_hash.py::test_xxh3_random_batches_vs_oracle (n = 20,000), "
                               "test_xxh3_canonical_every_length"),
}


def _product(expr: str) -> int:
    """'256ull * 8 * 8' -> 16384."""
    out = 1
    for f in expr.split("*"):
        out *= int(re.fullmatch(r"\s*(\d+)(?:ull|u)?\s*", f).group(1))
    return out


def _src(name: str) -> str:
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _one(pattern: str, text: str, flags=0) -> str:
    found = re.findall(pattern, text, flags)
    assert len(found) == 1, (pattern, found)
    return found[0]


def scan_pass(hip: str, kernel: str) -> int:
    """The tiles per pass of `kernel`'s one-workgroup scan: the kernel of file `hip` calls
    scan_tiles, and scan_tiles' one loop (tile_scan.h) advances by the one kScanPass."""
    hdr, text = _src("tile_scan.h"), _src(hip)
    _one(r"__global__ void __launch_bounds__\(256\) %s\([^)]*\) \{\s*const uint32_t \w+ = scan_tiles\(" % kernel, text)
    assert len(re.findall(r"scan_tiles\(", text)) == 1 and "t0 +=" not in text, hip  # no scan loop of the file's own
    assert _one(r"t0 < n_tiles; t0 \+= (\w+)\)", hdr) == "kScanPass"
    return int(_one(r"constexpr uint32_t kScanPass = (\d+);", hdr))


def read_constants() -> dict:
    """The named constants of the launch code, as the sources have them now."""
    arp, sw, nat = _src("arp_fwd.hip"), _src("switch_fwd.hip"), _src("nat_lookup.hip")
    lpm, fh, tx, arp_h = _src("route_lpm.hip"), _src("flow_hash.hip"), _src("tx_fixup.hip"), _src("arp_table.h")

    def kmax(text, fn):  # `const uint64_t kMax = <product>;` inside fn
        return _product(_one(r"uint32_t %s\(uint64_t \w+\) \{[^}]*?const uint64_t kMax = ([^;]+);" % fn, text))

    resolve = _one(r"n_tiles < (\d+)u \? n_tiles : (\d+)u", sw)
    rebuild = _one(r"s->slots / 256u < (\d+)u \? s->slots / 256u : (\d+)u", sw)
    assert resolve[0] == resolve[1] and rebuild[0] == rebuild[1]
    txb = _src("tx_build.hip")
    # the pair kernel's grid: dim3((uint32_t)(((uint64_t)n + 511u) / 512u * 64u))
    pair = _one(r"tx_build_pair_kernel<HALO_TXB_BIG_U>\),\s*dim3\(\(uint32_t\)\(\(\(uint64_t\)n \+ (\d+)u\) / (\d+)u \* (\d+)u\)\)",
                txb)
    assert int(pair[0]) == int(pair[1]) - 1
    # the build launch's cap, and that the launch code applies it (times the waves per tile)
    _one(r"cap = HALO_TXB_MAX_BLOCKS \* split;\s*const dim3 grid\(blocks < cap \? blocks : cap\)", txb)
    # the XXH3 launch: a block of one wave per window, the window being kRunWin, nothing else in the grid
    _one(r"const uint32_t win = halo::kRunWin;\s*p\.win = win;\s*hipLaunchKernelGGL\(halo::xxh3_run_kernel, "
         r"dim3\(\(n \+ win - 1\) / win\), dim3\(64\), 0, s, p\);", fh)
    return {
        "txb_g1_waves": int(_one(r"#define HALO_TXB_G1_WAVES (\d+)", txb)),
        "txb_blocks_per_wave": int(_one(r"#define HALO_TXB_MAX_BLOCKS \(HALO_TXB_G1_WAVES \* (\d+)u\)", txb)),
        "txb_split": int(_one(r"#define HALO_TXB_SPLIT (\d+)", txb)),
        "txb_kTile": int(_one(r"constexpr uint32_t kTile = (\d+);", txb)),
        "txb_kBlock": int(_one(r"constexpr uint32_t kBlock = (\d+);", txb)),
        "txb_finish_pass": int(_one(r"t0 \+= (\d+)\)", txb)),
        "txb_pair_run": int(pair[1]),
        "txb_pair_run_blocks": int(pair[2]),
        "arp_blocks": kmax(arp, "arp_blocks"),
        "nat_blocks": kmax(nat, "nat_blocks"),
        "lpm_blocks": kmax(lpm, "lpm_blocks"),
        "blocks_for": kmax(fh, "blocks_for"),
        # tx_grid's kMaxBlocks is <product> / wpb workgroups of wpb waves: the product is the cap in waves
        "tx_waves": _product(_one(r"const uint64_t kMaxBlocks = ([^;/]+)/ wpb;", tx)),
        "sw_resolve_cap": int(resolve[0]),
        "sw_rebuild_cap": int(rebuild[0]),
        "arp_pass": scan_pass("arp_fwd.hip", "arp_scan_kernel"),
        "sw_pass": scan_pass("switch_fwd.hip", "sw_scan_kernel"),
        "kTile": int(_one(r"constexpr uint32_t kTile = (\d+);", sw)),
        "kGatherTile": int(_one(r"constexpr uint32_t kGatherTile = (\d+);", arp_h)),
        "kRunWin": int(_one(r"constexpr uint32_t kRunWin = (\d+);", fh)),
    }


def derived(c: dict) -> dict:
    """name -> first n past the boundary, from the constants. Fixed by the kernels' shape and not
    read from the sources: 256 lanes per workgroup, 64 per wave, so a scan pass of `pass` tiles
    gives a lane pass / 256 tiles; 4 addresses per lane in lpm_kernel; 64 / G frames per wave in
    tx_fixup_kernel<G>; 256 slots per workgroup and trip in sw_rebuild_kernel. The build launch
    (tx_build.hip) is the exception: its block size and tile are read from the source."""
    per_lane = c["arp_pass"] // 256
    # the build launch: cap blocks of kBlock / 64 waves, a wave per tile (G >= 16: split waves per
    # tile under a cap split times as large), kTile descriptors per tile
    txb_waves = c["txb_g1_waves"] * c["txb_blocks_per_wave"] * (c["txb_kBlock"] // 64)
    txb_trip = txb_waves * c["txb_kTile"] + 1
    # the pair kernel's grid holds a wave for every pair of frames of every run: nothing to cross
    assert c["txb_pair_run_blocks"] * (c["txb_kBlock"] // 64) * 2 == c["txb_pair_run"]
    # the XXH3 windows of the named tests' 20,000 strings: more than one, the last one partial
    assert 20_000 > c["kRunWin"] and 20_000 % c["kRunWin"] and c["kRunWin"] % 64 == 0
    return {
        "txb_g1_trip": txb_trip,
        "txb_g4_trip": txb_trip,
        "txb_g8_trip": txb_trip,
        "txb_g16_trip": (txb_waves * c["txb_split"]) // c["txb_split"] * c["txb_kTile"] + 1,  # cap x split waves, split per tile
        "txb_finish_pass": c["txb_finish_pass"] * c["txb_kTile"] + 1,
        "txb_pair_grid": None,
        "arp_scan_lane": c["kGatherTile"] * per_lane + 1,
        "arp_scan_wave": c["kGatherTile"] * per_lane * 64 + 1,
        "arp_scan_pass": c["kGatherTile"] * c["arp_pass"] + 1,
        "arp_trip": c["arp_blocks"] * 256 + 1,
        "sw_scan_pass": c["kTile"] * c["sw_pass"] + 1,
        "sw_resolve_trip": c["sw_resolve_cap"] * c["kTile"] + 1,
        "sw_rebuild_trip": c["sw_rebuild_cap"] * 256 + 1,
        "nat_trip": c["nat_blocks"] * 256 + 1,
        "lpm_trip": c["lpm_blocks"] * 256 * 4 + 1,
        "lpm_records_trip": c["lpm_blocks"] * 256 + 1,
        "flow_hash_trip": c["blocks_for"] * 256 + 1,
        "tx_g16_trip": c["tx_waves"] * (64 // 16) + 1,
        "tx_g8_trip": c["tx_waves"] * (64 // 8) + 1,
        "tx_g4_trip": c["tx_waves"] * (64 // 4) + 1,
        "tx_g1_trip": c["tx_waves"] * 64 + 1,
        "xxh3_run_grid": None,
    }


def past(name: str, r: int) -> int:
    """The shape of a GPU test: the last n of the first trip / pass plus r (a partial wave; the
    tests of per-lane kernels also choose r off a multiple of 4)."""
    assert 65 <= r <= 300 and r % 64, r
    return BOUNDARIES[name]["first_past"] - 1 + r


# ---- tiling --------------------------------------------------------------------------------------
def tile_index(n: int, period: int = P) -> np.ndarray:
    """Item j of the tiled input is item j % period of the period."""
    return np.arange(n, dtype=np.int64) % period


def tiled(a: np.ndarray, n: int) -> np.ndarray:
    return np.ascontiguousarray(a[tile_index(n, len(a))])


def tile_frames(data: np.ndarray, offs_dw: np.ndarray, lens: np.ndarray, n: int):
    """A packed period (bytes with their gap garbage, dword offsets, lengths) repeated to n frames:
    every repeat is a whole copy of the period's buffer and its offsets are shifted by the buffer's
    size. Returns (bytes, offsets_dw u32, lens u16)."""
    period, size = len(lens), len(data)
    assert size % 4 == 0
    reps = -(-n // period)
    j = np.arange(n, dtype=np.int64)
    offs = offs_dw.astype(np.int64)[j % period] + (j // period) * (size // 4)
    assert int(offs[-1]) < 1 << 32
    return np.tile(data, reps), offs.astype(np.uint32), np.ascontiguousarray(lens[j % period])


def tile_frames_expected(data: np.ndarray, want: np.ndarray, offs_dw: np.ndarray, n: int) -> np.ndarray:
    """The buffer tile_frames' first n frames leave behind when one period's frames turn `data`
    into `want`: whole repeats of `want`, and a last repeat in which only the first n % period
    frames were there to be touched."""
    period = len(offs_dw)
    q, r = divmod(n, period)
    parts = [np.tile(want, q)]
    if r:
        cut = 4 * int(offs_dw[r])  # frames are packed in order: frame r and everything behind it is input
        parts.append(np.concatenate([want[:cut], data[cut:]]))
    return np.concatenate(parts)


# ---- ARP -----------------------------------------------------------------------------------------
SCALE_LENS_POOL = [34, 60, 61, 62, 63, 64, 100, 72]  # the period's one 1514-byte frame is set apart
LONG_AT = 16 * 33  # a hit_direct position of arp_cases.mixed_batch


def arp_encap_period(keys, find_route, seed: int = 77, period: int = P):
    """One period of the L2 step's mixed batch. `find_route(dsts u32) -> route ids u32`.
    Returns dict(frames, data, offs, lens, rids, select, names)."""
    from tests import arp_cases as K

    rng = np.random.default_rng(seed)
    frames, dsts, select, forced, names = K.mixed_batch(rng, keys, period, lens_pool=SCALE_LENS_POOL)
    if period > LONG_AT:
        assert names[LONG_AT] == "hit_direct"
        frames[LONG_AT] = K.ipv4_frame(rng, 1514, int(dsts[LONG_AT]))
    data, offs, lens = K.pack(rng, frames)
    rids = np.array(find_route(dsts), np.uint32)
    for i, frc in enumerate(forced):
        if frc is not None:
            rids[i] = frc
    return dict(frames=frames, data=data, offs=offs, lens=lens, rids=rids, select=select, names=names)


def arp_encap_model(model, rt, frames, rids, select, in_netif, data, offs):
    """arp_model.Model.encap over frames: (results ARP_RESULT_DTYPE, the buffer afterwards)."""
    from halo_amd._lib import ARP_RESULT_DTYPE
    from tests import arp_cases as K

    want = data.copy()
    res = np.zeros(len(frames), ARP_RESULT_DTYPE)
    routes = {}
    for i, f in enumerate(frames):
        rid = int(rids[i])
        if rid not in routes:
            routes[rid] = K.route_of(rt, rid)
        v, out, tx, target, after = model.encap(f, routes[rid], in_netif, bool(select[i]))
        res[i] = (v, out, tx, target)
        want[4 * int(offs[i]):4 * int(offs[i]) + len(f)] = np.frombuffer(after, np.uint8)
    return res, want


def arp_lookup_model(model, nifs, ips):
    """arp_model.Model.lookup over (netif, ip) pairs: (verdict u8, mac8 u8 [n, 8])."""
    from tests import arp_model as AM

    verdict = np.zeros(len(ips), np.uint8)
    mac8 = np.zeros((len(ips), 8), np.uint8)
    for i, (a, b) in enumerate(zip(nifs, ips)):
        v, m = model.lookup(int(a), int(b))
        verdict[i] = v
        if v == AM.HIT:
            mac8[i, :6] = np.frombuffer(m, np.uint8)
    return verdict, mac8


def arp_auto_table(make_pair, entries: int = 20_000, seed: int = 31):
    """An automatic-slot-count table (slots_log2 = 0) of about `entries` neighbours over the three
    NetIfs, and the lookups of the scale test: every key plus as many absent addresses, own
    addresses and unknown NetIfs. Returns (pair, keys, netifs u8, ips u32)."""
    from tests import arp_cases as K

    rng = np.random.default_rng(seed)
    pair = make_pair(capacity=entries + 16, slots_log2=0)
    nif = rng.integers(0, 3, entries)
    host = rng.integers(2, 1 << 16, entries)
    seen, keys = set(), []
    for a, h in zip(nif.tolist(), host.tolist()):
        ip = (K.NETIFS[a].ip & 0xFFFF0000) | h
        if (a, ip) not in seen and ip != K.NETIFS[a].ip:
            seen.add((a, ip))
            keys.append((a, ip))
    for k, (a, ip) in enumerate(keys):
        pair.set(a, ip, K.mac(5000 + k), 50)
    q_nif, q_ip = [a for a, _ in keys], [ip for _, ip in keys]
    for k in range(len(keys)):
        kind = k % 4
        a = k % 3
        if kind == 0 or kind == 1:  # absent: outside the hosts' range, or a key of another NetIf
            ip = (K.NETIFS[a].ip & 0xFFFF0000) | 0x10000 | k if kind == 0 else keys[k][1]
            a = a if kind == 0 else (keys[k][0] + 1) % 3
            if (a, ip) in seen:
                ip ^= 0x40000000
        elif kind == 2:
            ip = K.NETIFS[a].ip
        else:
            a, ip = [3, 64, 255][(k // 4) % 3], keys[k][1]
        q_nif.append(a)
        q_ip.append(ip & 0xFFFFFFFF)
    return pair, keys, np.array(q_nif, np.uint8), np.array(q_ip, np.uint32)


# ---- NAT -----------------------------------------------------------------------------------------
NAT_MAPPINGS = [(8080, 0xC0A80010, 80, 6), (8080, 0xC0A80011, 81, 6), (5353, 0xC0A80012, 53, 17)]


def nat_model(nat_type, tuples, mappings=(), now=100):
    from tests import nat_model as NM

    m = NM.NatModel(NM.WAN_IP, nat_type)
    for e in mappings:
        m.add_port_mapping(*e)
    for tup in tuples:
        m.add_flow(*tup, now)
    return m


def nat_tables():
    """name -> (nat type, tuples, capacity_log2, mappings) of the scale tests' tables: the forced
    16-slot layout and the 5000-flow table of tests/test_gpu_nat.py."""
    from tests import nat_model as NM

    return {"forced_sym": (NM.SYMMETRIC, NM.random_tuples(NM.FIXTURE_SEED[NM.SYMMETRIC], NM.FIXTURE_FLOWS), NM.FIXTURE_LOG2,
                           NAT_MAPPINGS),
            "5000": (NM.SYMMETRIC, NM.random_tuples(9, 5000), 0, NAT_MAPPINGS)}


def nat_period(m, direction, now, seed, period: int = P, skip_share: int = 5):
    """One period of lookup records with ops and a skip array, and the model's answer for it (the
    model's hit flows are stamped `now`). Returns dict(recs, ops, skip, want_ops, verdict, ref)."""
    from tests import nat_model as NM

    recs = NM.records(m, direction, period, seed)
    skip = (np.random.RandomState(seed + 1).randint(0, skip_share, period) == 0).astype(np.uint8)
    ops = NM.ops(period, seed + 2)
    want_ops = ops.copy()
    verdict, ref, _ = m.lookup(direction, recs, now, want_ops, skip)
    return dict(recs=recs, ops=ops, skip=skip, want_ops=want_ops, verdict=verdict, ref=ref)
