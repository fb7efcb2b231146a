"""Not a test: shared by tests/test_lo_host.py, tests/test_gpu_lo.py and tests/test_gpu_lo_chain.py —
the seeded corpus of the loopback gather (every length edge against every verdict and every kind of
out NetIf, packed with garbage in the gaps; in tx mode every relation of totalLen to the frame) and,
in the manner of tests/scale_cases.py, where the gather's scan changes behaviour with the batch
size: one lane's tiles, one wave's, one pass and one grid, read out of the sources by regular expression so
that a moved constant moves the shapes."""
from __future__ import annotations

import numpy as np

from tests import arp_cases as K
from tests import arp_model as AM
from tests import egress_cases as E

ARP_RESULT_DTYPE = np.dtype([("verdict", "u1"), ("out_netif", "u1"), ("tx_len", "<u2"), ("target_ip", "<u4")])
LENS = [0, 17, 33, 34, 35, 36, 37, 60, 64, 100, 1514, 1515]          # pkt_len % 4 in {0, 1, 2, 3}; both caps
JUMBO_LENS = LENS + [9014, 9015]
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 513]
FILL = 0xA5
# tx mode: totalLen relative to len - 14
TOTAL_LEN_KINDS = ["equal", "below_1", "below_3", "min_20", "under_19", "above_1", "zero", "huge"]


def netif_pool(n_netifs: int):
    """NetIf 0, the last, one in the middle, the first above n_netifs, 0xFF."""
    return [0, n_netifs - 1, n_netifs // 2, min(n_netifs, 0xFE), 0xFF]


def total_len_of(kind: str, length: int) -> int:
    room = max(length - 14, 0)
    return {"equal": room, "below_1": max(room - 1, 0), "below_3": max(room - 3, 0), "min_20": 20, "under_19": 19,
            "above_1": room + 1, "zero": 0, "huge": 0xFFFF}[kind]


def mixed(seed: int, n: int, n_netifs: int, tx: bool = False, jumbo: bool = False, loopback_share: int = 2):
    """n frames: frame i has length pool[i % 12 (14)], verdict i % 7 — except that `loopback_share`
    of every three frames are LOOPBACK whatever i says — and out NetIf pool[i % 5]; 12, 7 and 5 are
    pairwise coprime, so a few hundred frames hold every pairing (tests/test_lo_host.py asserts
    what is reached). In tx mode bytes 16-17 carry totalLen by TOTAL_LEN_KINDS, one kind per three
    frames. The cycles start at a seeded offset. Returns (frames, data, offsets_dw, lens, results)."""
    rng = np.random.default_rng(seed)
    lens_pool, pool = (JUMBO_LENS if jumbo else LENS), netif_pool(n_netifs)
    first = int(rng.integers(0, 1000))
    frames = []
    results = np.zeros(n, ARP_RESULT_DTYPE)
    for i in range(n):
        j = first + i
        length = lens_pool[j % len(lens_pool)]
        f = bytearray(rng.integers(0, 256, length, dtype=np.uint8).tobytes())
        if tx and length >= 18:
            t = total_len_of(TOTAL_LEN_KINDS[(j // 3) % len(TOTAL_LEN_KINDS)], length)
            f[16], f[17] = (t >> 8) & 255, t & 255
        frames.append(bytes(f))
        verdict = AM.LOOPBACK if (j % 3) < loopback_share else j % 7
        results[i] = (verdict, pool[j % len(pool)], int(rng.integers(0, 1 << 16)), int(rng.integers(0, 1 << 32)))
    data, offs, lens = K.pack(rng, frames) if n else (np.zeros(16, np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint16))
    return frames, data, offs, lens, results


def region_for(want_bytes: int) -> int:
    """A region that holds the largest NetIf's packets and leaves sentinel bytes behind: a multiple of 16."""
    return (int(want_bytes) + 64 + 15) & ~15


# ---- past the edges ------------------------------------------------------------------------------
# edge -> the constants it follows from and the first n past it, as the sources give it today
BOUNDARIES = {
    "lo_scan_lane": dict(kernels="port_scan_kernel: a second lane of scan_stream_tiles", constants=("kTile", "tiles_per_lane"),
                         first_past=1_025),
    "lo_scan_wave": dict(kernels="port_scan_kernel: a second wave", constants=("kTile", "tiles_per_lane"), first_past=65_537),
    "lo_scan_pass": dict(kernels="port_scan_kernel: a second pass", constants=("kTile", "kScanPass"), first_past=262_145),
    "lo_grid": dict(kernels="port_count_kernel, port_scatter_kernel of the gather's stages: second trip",
                    constants=("kTile", "port_stream_blocks"), first_past=524_289),
}


def read_constants() -> dict:
    """The gather's kernels are port_streams.h's: tests/egress_cases.py reads them for both stages."""
    return E.read_port_streams("lo_gather")


def derived(c: dict) -> dict:
    return {"lo_scan_lane": c["kTile"] * c["tiles_per_lane"] + 1,
            "lo_scan_wave": c["kTile"] * c["tiles_per_lane"] * 64 + 1,
            "lo_scan_pass": c["kTile"] * c["kScanPass"] + 1,
            "lo_grid": c["kTile"] * c["port_stream_blocks"] + 1}


def past(name: str, r: int) -> int:
    assert 1 <= r <= 300 and r % 4, r
    return BOUNDARIES[name]["first_past"] - 1 + r


def periodic_batch(seed: int, n: int, period: int = 1000, length: int = 64):
    """n frames of one length, back to back, repeating `period` random templates: (templates uint8
    [period, length], tid [n], data, offsets_dw, lens)."""
    assert length % 4 == 0
    rng = np.random.default_rng(seed)
    templates = rng.integers(0, 256, (period, length), dtype=np.uint8)
    tid = (np.arange(n) % period).astype(np.int64)
    data = np.tile(templates.reshape(-1), n // period + 1)[:n * length] if n else np.zeros(16, np.uint8)
    return (templates, tid, np.ascontiguousarray(data), (np.arange(n, dtype=np.int64) * (length // 4)).astype(np.uint32),
            np.full(n, length, np.uint16))
