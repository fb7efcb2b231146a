"""Far placements: one batch spread over a buffer of FAR_BYTES = 8 GiB + 64 MiB, for the tests
that take every frame-addressing entry past byte 4 GiB (where 32-bit byte arithmetic wraps) and
byte 8 GiB (dword offset 2^31, the first that is negative as the int32 the wrappers carry).

A frame's answer does not depend on where it lies, so the expected result of every row is the
existing model's or oracle's over the frames themselves; only the placement is new.

`place(frames, order)` packs the frames on dword boundaries inside four dense bands:

    N   from byte 0
    X4  a run in which one frame (the band's middle one, or the first after it of 34 bytes or more)
        starts at byte 2^32 - 20: its Ethernet header lies below the 4 GiB mark and its IPv4 header
        above it; at least 64 frames of the run lie before it and 64 after it
    X8  the same at byte 2^33: that frame and the ones after it have dword offsets >= 2^31
    T   a run whose last (padded) frame ends at the buffer's last byte

in one of three orders: `banded` (index order is memory order, a quarter of the batch per band),
`interleaved` (frame i in band i mod 4: every 64-frame window and 256-frame tile holds neighbours
4 and 8 GiB apart, in rising and falling steps) and `first_far` (lane 0 of every 64-frame window in
T, the rest in N: every other frame of the window lies far below its first one).

Each band has a 64-byte guard of GUARD before and after it (none before byte 0 and none after the
last byte), and the alignment bytes between frames hold GAP. `to_host` / `to_device` write a band
(guards, frames, gaps) with one slice copy and `read_bands` reads it back the same way, so the
buffer is never filled or downloaded whole: a numpy buffer commits only the pages of the bands
(about 30 MiB resident), a device buffer is a `torch.empty` of FAR_BYTES.

Device memory: the far buffer is 8.06 GiB and the far-output rows of test_gpu_far_offsets.py add a
12 GiB output, so that file peaks at about 20 GiB; its module fixture frees both at teardown.
"""
from __future__ import annotations

import numpy as np

FAR_BYTES = (8 << 30) + (64 << 20)
MARK4 = 1 << 32
MARK8 = 1 << 33
X4_PIVOT = MARK4 - 20  # the pivot frame's start: 14 B of Ethernet + 6 B of the IPv4 header below the mark
GUARD_BYTES = 64
GUARD = 0x5C
GAP = 0xC3
ORDERS = ("banded", "interleaved", "first_far")
BAND_NAMES = ("N", "X4", "X8", "T")
N_FRAMES = 1024  # 16 windows of 64, 4 tiles of 256: every band and straddle holds whole windows


class Band:
    """One dense run: `members` (batch indices in memory order) occupy bytes [lo, hi); the span that
    is written and read back, guards included, is [span_lo, span_hi)."""

    def __init__(self, name, members, lo, hi):
        self.name, self.members, self.lo, self.hi = name, members, lo, hi
        self.span_lo = max(lo - GUARD_BYTES, 0)
        self.span_hi = min(hi + GUARD_BYTES, FAR_BYTES)

    def __repr__(self):
        return f"Band({self.name}, {len(self.members)} frames, [{self.lo:#x}, {self.hi:#x}))"


def _lens_of(frames) -> np.ndarray:
    if isinstance(frames, np.ndarray) and frames.ndim == 1 and frames.dtype != object:
        return frames.astype(np.int64)
    return np.array([len(f) for f in frames], np.int64)


def band_of(n: int, order: str) -> np.ndarray:
    """The band (index into BAND_NAMES) of each of n frames."""
    i = np.arange(n)
    if order == "banded":
        return np.minimum(i * 4 // max(n, 1), 3)
    if order == "interleaved":
        return i % 4
    if order == "first_far":
        return np.where(i % 64 == 0, 3, 0)
    raise ValueError(order)


def place(frames, order: str):
    """(offsets_dw u32[n], lens u16[n], bands) of `frames` (a list of byte strings, or their lengths)
    in the given order. offsets_dw are dword offsets into a buffer of FAR_BYTES."""
    lens = _lens_of(frames)
    n = len(lens)
    size = (lens + 3) & ~3
    which = band_of(n, order)
    start = np.zeros(n, np.int64)
    bands = []
    for b, name in enumerate(BAND_NAMES):
        m = np.flatnonzero(which == b)
        if m.size == 0:
            continue
        rel = np.concatenate([[0], np.cumsum(size[m])])  # rel[k]: member k's start inside the run
        if name == "N":
            lo = 0
        elif name == "T":
            lo = FAR_BYTES - int(rel[-1])
        else:
            # the middle frame, or the first one after it long enough for its IPv4 header to cross the mark
            pivot = next((k for k in range(m.size // 2, m.size) if lens[m[k]] >= 34), m.size // 2)
            assert pivot >= 64 and m.size - 1 - pivot >= 64, f"band {name}: {m.size} frames do not give 64 each side"
            lo = (X4_PIVOT if name == "X4" else MARK8) - int(rel[pivot])
        start[m] = lo + rel[:-1]
        bands.append(Band(name, m, lo, lo + int(rel[-1])))
    for a, b in zip(bands, bands[1:]):
        assert a.span_hi <= b.span_lo, (a, b)
    assert bands[-1].hi <= FAR_BYTES and np.all(start % 4 == 0)
    return (start // 4).astype(np.uint32), lens.astype(np.uint16), bands


def byte_offsets(offsets_dw) -> list:
    """The frames' byte offsets as Python integers."""
    return [4 * int(o) for o in offsets_dw]


def frames_of(data: np.ndarray, offsets_dw, lens) -> list:
    """The frames of a compact batch as byte strings."""
    return [data[4 * int(o):4 * int(o) + int(ln)].tobytes() for o, ln in zip(offsets_dw, lens)]


def image(band: Band, offsets_dw, frames) -> np.ndarray:
    """What the span of `band` holds when `frames` lie at offsets_dw: guards, frames, gaps."""
    img = np.full(band.span_hi - band.span_lo, GAP, np.uint8)
    img[:band.lo - band.span_lo] = GUARD
    img[band.hi - band.span_lo:] = GUARD
    for i in band.members:
        f = frames[i]
        at = 4 * int(offsets_dw[i]) - band.span_lo
        img[at:at + len(f)] = np.frombuffer(f, np.uint8) if not isinstance(f, np.ndarray) else f
    return img


def new_host_buffer() -> np.ndarray:
    return np.empty(FAR_BYTES, np.uint8)  # untouched pages are never committed


def to_host(placement, frames, buf: np.ndarray | None = None) -> np.ndarray:
    """Write the placement into a numpy buffer of FAR_BYTES (a new one when none is given)."""
    offsets_dw, _, bands = placement
    if buf is None:
        buf = new_host_buffer()
    assert buf.nbytes == FAR_BYTES
    for b in bands:
        buf[b.span_lo:b.span_hi] = image(b, offsets_dw, frames)
    return buf


def to_device(placement, frames, buf):
    """Write the placement into a cuda uint8 tensor of FAR_BYTES: one slice copy per band."""
    import torch

    offsets_dw, _, bands = placement
    assert buf.numel() == FAR_BYTES and buf.dtype == torch.uint8
    for b in bands:
        buf[b.span_lo:b.span_hi].copy_(torch.from_numpy(image(b, offsets_dw, frames)))
    return buf


def read_bands(placement, buf) -> list:
    """Each band's span (guards included) as a numpy array, from a numpy or cuda buffer."""
    out = []
    for b in placement[2]:
        s = buf[b.span_lo:b.span_hi]
        out.append(s.cpu().numpy() if hasattr(s, "cpu") else s.copy())
    return out


def assert_bands(placement, buf, frames, what="") -> None:
    """The buffer's bands hold exactly `frames` at the placement, with guards and gaps unchanged."""
    offsets_dw, _, bands = placement
    for b, got in zip(bands, read_bands(placement, buf)):
        want = image(b, offsets_dw, frames)
        bad = np.flatnonzero(got != want)
        if bad.size:
            at = int(bad[0]) + b.span_lo
            inside = [int(i) for i in b.members if 4 * int(offsets_dw[i]) <= at < 4 * int(offsets_dw[i]) + len(frames[i])]
            raise AssertionError(f"{what}: band {b.name}: {bad.size} bytes differ, first at byte {at:#x} "
                                 f"({'frame %d' % inside[0] if inside else 'guard or gap'})")


def device_offsets(placement, dev):
    """(offsets_dw as int32, lens as int16) cuda tensors; offsets >= 2^31 are negative int32."""
    import torch

    offsets_dw, lens, _ = placement
    return (torch.from_numpy(offsets_dw.view(np.int32).copy()).to(dev), torch.from_numpy(lens.view(np.int16).copy()).to(dev))


def describe(placement) -> dict:
    """Counts a test asserts on, so that a placement that lost its far frames cannot pass."""
    offsets_dw, lens, bands = placement
    o = offsets_dw.astype(np.int64) * 4
    end = o + lens.astype(np.int64)
    return {"beyond_4g": int((o >= MARK4).sum()), "beyond_8g": int((o >= MARK8).sum()),
            "straddle_4g": int(((o < MARK4) & (end > MARK4)).sum()), "at_8g": int((o == MARK8).sum()),
            "last_end": int(((end + 3) & ~3).max()), "bands": [b.name for b in bands]}
