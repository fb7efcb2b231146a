"""Not a test: shared by tests/test_txring_host.py and tests/test_gpu_txring.py — spans of whole
ring records built from lists of frame lengths, the malformed spans, and, in the manner of
tests/egress_cases.py, where the copy kernel of halo_amd/csrc/tx_ring.hip changes behaviour with the
span size: its workgroup cap and its bytes per workgroup and pass, read out of the source by regular
expression so that a moved constant moves the shape."""
from __future__ import annotations

import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo_amd", "csrc")

LENS = [60, 61, 63, 64, 100, 570, 1514]
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
MAX_RECORD = 16376  # HALO_TXRING_MAX_RECORD


def record_size(length: int) -> int:
    return (4 + int(length) + 3) & ~3


def span_of(frames) -> np.ndarray:
    """The frames as ring records, back to back: u32 length, the bytes, zeros to a 4-byte boundary."""
    parts = []
    for f in frames:
        f = bytes(f)
        parts.append(np.uint32(len(f)).tobytes() + f + b"\0" * (record_size(len(f)) - 4 - len(f)))
    return np.frombuffer(b"".join(parts), np.uint8).copy() if parts else np.zeros(0, np.uint8)


def frames_of(seed: int, lens) -> list:
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lens]


def mixed_lens(seed: int, n: int, pool=LENS) -> list:
    """n lengths that run through the pool from a seeded start (every length by n = 7)."""
    first = int(np.random.default_rng(seed).integers(0, 1000))
    return [pool[(first + i) % len(pool)] for i in range(n)]


def mixed_span(seed: int, n: int, pool=LENS):
    """(frames, span) of n records with lengths mixed from the pool."""
    frames = frames_of(seed, mixed_lens(seed, n, pool))
    return frames, span_of(frames)


def ends_of(frames) -> np.ndarray:
    """Span offset of the end of each record (ascending)."""
    return np.cumsum([record_size(len(f)) for f in frames]).astype(np.int64)


def raw_record(length_field: int, payload_bytes: int) -> np.ndarray:
    """A record whose length field says `length_field` and that holds `payload_bytes` bytes."""
    return np.frombuffer(np.uint32(length_field).tobytes() + b"\x11" * payload_bytes, np.uint8).copy()


def bad_span(kind: str, ring_size: int) -> np.ndarray:
    """Three good records, then the malformed one (and, for the lengths, a good one behind it)."""
    good = span_of(frames_of(5, [60, 100, 64]))
    tail = span_of(frames_of(6, [60]))
    if kind == "zero":
        return np.concatenate([good, raw_record(0, 60), tail])
    if kind == "half_plus_4":
        return np.concatenate([good, raw_record(ring_size // 2 + 4, 64), tail])
    if kind == "past_end":  # the last record says 100 bytes and holds 64
        return np.concatenate([good, raw_record(100, 64)])
    if kind == "walk_capacity":  # whole and well-formed; the host takes it in a ring of >= 2 * 16380
        return np.concatenate([good, span_of(frames_of(7, [MAX_RECORD + 4])), tail])
    raise KeyError(kind)


# ---- past the copy grid ------------------------------------------------------------------------
# edge -> the constants it follows from and the first span size past it (bytes), as the launch code
# gives it today: one more byte-group than the capped grid copies in one pass
BOUNDARIES = {
    "txring_copy_grid": dict(kernels="txring_copy_kernel: second trip of the grid-stride loop",
                             constants=("kCopyThreads", "kCopyUnroll", "copy_blocks"), first_past=4_194_308),
}


def _one(pattern: str, text: str) -> str:
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def read_constants() -> dict:
    with open(os.path.join(CSRC, "tx_ring.hip")) as fh:
        hip = fh.read()
    kmax = _one(r"uint32_t copy_blocks\(uint64_t \w+\) \{[^}]*?const uint64_t kMax = (\d+);", hip)
    assert _one(r"constexpr uint32_t kCopyBlockBytes = ([^;]+);", hip) == "kCopyThreads * kCopyUnroll * 16"
    return {"kCopyThreads": int(_one(r"constexpr uint32_t kCopyThreads = (\d+);", hip)),
            "kCopyUnroll": int(_one(r"constexpr uint32_t kCopyUnroll = (\d+);", hip)),
            "copy_blocks": int(kmax)}


def block_bytes(c: dict) -> int:
    """A workgroup's bytes per pass."""
    return c["kCopyThreads"] * c["kCopyUnroll"] * 16


def derived(c: dict) -> dict:
    return {"txring_copy_grid": block_bytes(c) * c["copy_blocks"] + 4}


def past(name: str, r: int) -> int:
    """A span size r bytes past the edge's last in-pass byte: r a multiple of 4, not of 16."""
    assert 68 <= r <= 4096 and r % 4 == 0 and r % 16, r
    return BOUNDARIES[name]["first_past"] - 4 + r
