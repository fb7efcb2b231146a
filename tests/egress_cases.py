"""Not a test: shared by tests/test_egress_host.py and tests/test_gpu_egress.py — the mixed batch
of the egress tests (every length edge against every kind of mask, packed with garbage in the gaps)
and, in the manner of tests/scale_cases.py, where the egress kernels change behaviour with the
batch size: the tile, the scan pass and the grid cap, read out of the sources by regular expression
so that a moved constant moves the shapes."""
from __future__ import annotations

import os
import re

import numpy as np

from tests import arp_cases as K
from tests import switch_model as SWM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo_amd", "csrc")

LENS = [0, 13, 14, 41, 42, 59, 60, 61, 62, 63, 64, 65, 100, 1514, 1515]
JUMBO_LENS = LENS + [9014, 9015]
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
ALL = (1 << 64) - 1


def mask_pool(n_ports: int):
    """No port, one bit, the last port, bit 63, all bits, a bit at or above n_ports alone and
    beside a real port."""
    above = 1 << (n_ports if n_ports < 64 else 63)
    return [0, 1, 1 << (n_ports - 1), 1 << 63, ALL, above, above | 1 << (n_ports // 2)]


def mixed(seed: int, n: int, n_ports: int, jumbo: bool = False):
    """n frames: frame i has length lens[i % 15 (17)] and mask pool[i % 7] — 15 and 17 are coprime
    to 7, so a batch of 105 (119) frames holds every pairing. Returns (frames, data, offsets_dw,
    lens, masks)."""
    rng = np.random.default_rng(seed)
    lens_pool, pool = (JUMBO_LENS if jumbo else LENS), mask_pool(n_ports)
    first = int(rng.integers(0, 1000))
    frames = [rng.integers(0, 256, lens_pool[(first + i) % len(lens_pool)], dtype=np.uint8).tobytes() for i in range(n)]
    masks = np.array([pool[(first + i) % len(pool)] for i in range(n)], np.uint64)
    data, offs, lens = K.pack(rng, frames)
    return frames, data, offs, lens, masks


def region_for(want_bytes: int) -> int:
    """A region that holds the largest stream and leaves sentinel bytes behind it: a multiple of 16."""
    return (int(want_bytes) + 64 + 15) & ~15


# ---- the switch kind's batch ------------------------------------------------------------------
def switch_batch():
    """A 4-port, 2-VLAN switch (ports 0-2 in VLAN 10, port 3 in VLAN 20), ingress port 0: UNICAST
    (one back to the ingress port), FLOOD, and every drop verdict. Returns (warm-up calls, frames)."""
    A, B, C3, D = SWM.mac(1), SWM.mac(2), SWM.mac(3), SWM.mac(4)
    bcast, mcast = b"\xff" * 6, bytes([0x01, 0x00, 0x5E, 0x00, 0x00, 0x01])
    warm = [(1, [SWM.frame(bcast, B)], 1), (2, [SWM.frame(bcast, C3), SWM.frame(bcast, SWM.mac(9))], 1)]
    frames = [SWM.frame(A, A, 64),            # UNICAST back to the ingress port
              SWM.frame(B, A, 42),            # UNICAST to port 1, padded
              SWM.frame(D, A, 61),            # unknown: FLOOD to ports 1 and 2
              SWM.frame(B, A, 41),            # ETH_LEN
              SWM.frame(B, A, 1515),          # ETH_LEN
              SWM.frame(B, A, 64, 0x8100),    # ETH_TYPE
              SWM.frame(B, mcast, 64),        # SRC_MCAST
              SWM.frame(C3, A, 1514),         # UNICAST to port 2
              SWM.frame(bcast, A, 60),        # FLOOD
              SWM.frame(B, SWM.mac(7), 100),   # TABLE_FULL (capacity 4: A, B, C, mac 9)
              SWM.frame(C3, A, 63)]
    return warm, frames


# ---- past the edges ------------------------------------------------------------------------------
# edge -> the constants it follows from and the first n past it, as the launch code gives it today
BOUNDARIES = {
    "egress_tile": dict(kernels="port_count_kernel, port_scatter_kernel of the egress stages: second tile", constants=("kTile",),
                        first_past=257),
    "egress_scan_pass": dict(kernels="port_scan_kernel: second pass", constants=("kTile", "kScanPass"),
                             first_past=262_145),
    "egress_grid": dict(kernels="port_count_kernel, port_scatter_kernel of the egress stages: second trip",
                        constants=("kTile", "egress_blocks"), first_past=524_289),
}


def _one(pattern: str, text: str) -> str:
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def read_port_streams(stage: str) -> dict:
    """What tx_egress.hip and lo_gather.hip (`stage`, without suffix) take from port_streams.h: the
    stage's own kTile pinned to the shared tile, the grid cap of the count and scatter kernels, the
    scan's pass and a lane's tiles in it. tests/lo_cases.py reads through this too."""
    def src(name):
        with open(os.path.join(CSRC, name)) as fh:
            return fh.read()

    hip, hdr = src(stage + ".hip"), src(stage + ".h")
    ps, tile, stream = src("port_streams.h"), src("tile_scan.h"), src("stream_scan.h")
    k_tile = int(_one(r"constexpr uint32_t kTile = (\d+);", hdr))
    assert k_tile == int(_one(r"constexpr uint32_t kPortTile = (\d+);", ps))
    _one(r"static_assert\(\w+::kTile == kPortTile &&", hip)
    kmax = _one(r"uint32_t port_stream_blocks\(uint64_t \w+\) \{[^}]*?const uint64_t kMax = ([^;]+);", ps)
    blocks = 1
    for f in kmax.split("*"):
        blocks *= int(re.fullmatch(r"\s*(\d+)(?:ull|u)?\s*", f).group(1))
    # the stage's kernels are port_streams.h's, launched by its one launch function with that grid;
    # port_scan_kernel calls the streams' fused scan (stream_scan.h), whose one loop advances by
    # tile_scan.h's pass, a lane taking consecutive tiles; neither file has a scan loop of its own
    assert '#include "port_streams.h"' in hip and "<<<" not in hip and len(re.findall(r"launch_port_streams<", hip)) >= 2
    _one(r"const uint32_t grid = port_stream_blocks\(q\.n_tiles\);\s*port_count_kernel<Stage><<<dim3\(grid\), dim3\(kPortTile\)[^;]*;"
         r"\s*port_scan_kernel<[^;]*;\s*port_scatter_kernel<Stage><<<dim3\(grid\), dim3\(kPortTile\)", ps)
    assert '#include "stream_scan.h"' in ps and "t0 +=" not in hip + ps and "kScanPass =" not in hip + ps + stream
    _one(r"__global__ void __launch_bounds__\(256\) port_scan_kernel\([^)]*\) \{[^}]*?=\s*scan_stream_tiles\(", ps)
    assert len(re.findall(r"scan_stream_tiles\(", hip + ps)) == 1 and '#include "tile_scan.h"' in stream
    assert _one(r"t0 < n_tiles; t0 \+= (\w+),", stream) == "kScanPass"
    per_lane = int(_one(r"const uint32_t t = t0 \+ (\d+) \* threadIdx\.x;\s*uint32_t c\[", stream))
    k_pass = int(_one(r"constexpr uint32_t kScanPass = (\d+);", tile))
    assert k_pass == per_lane * 256
    return {"kTile": k_tile, "kScanPass": k_pass, "tiles_per_lane": per_lane, "port_stream_blocks": blocks}


def read_constants() -> dict:
    c = read_port_streams("tx_egress")
    return {"kTile": c["kTile"], "kScanPass": c["kScanPass"], "egress_blocks": c["port_stream_blocks"]}


def derived(c: dict) -> dict:
    return {"egress_tile": c["kTile"] + 1,
            "egress_scan_pass": c["kTile"] * c["kScanPass"] + 1,
            "egress_grid": c["kTile"] * c["egress_blocks"] + 1}


def past(name: str, r: int) -> int:
    assert 65 <= r <= 300 and r % 64, r
    return BOUNDARIES[name]["first_past"] - 1 + r


def uniform_batch(seed: int, n: int, length: int = 64):
    """n frames of one length, back to back: (frames2d uint8 [n, length], data, offsets_dw, lens)."""
    assert length % 4 == 0
    rng = np.random.default_rng(seed)
    frames2d = rng.integers(0, 256, (n, length), dtype=np.uint8)
    return (frames2d, frames2d.reshape(-1), (np.arange(n, dtype=np.int64) * (length // 4)).astype(np.uint32),
            np.full(n, length, np.uint16))
