"""Not a test: which build kernel halo_tx_build_batch_device launches for a max_payload_hint, the
descriptor batches of the transmit-build tests, and their comparison with the C oracle.

`read_ladder` takes the dispatch ladder out of halo_amd/csrc/tx_build.hip with plain regular
expressions (as scale_cases.read_constants does for the grid caps) and `variant_of` restates it, so
a moved threshold fails tests/test_build_cases.py on the CPU until HINTS moves with it. Every GPU
test of the build takes its hint from HINTS (or EDGE_HINTS) and asserts through `variant_of` the
kernel it names.

`sweep(order)` is the length sweep: every payload length at every start alignment for every
protocol and both modes, once in runs of one (protocol, mode) with rising lengths (whole waves
uniform: the scalar arms) and once shuffled (every wave mixes protocols, modes, 60- and 1514-byte
frames and rejections). `second_trip_batch(n)` is the batch of tests/test_gpu_scale.py's build case.
`assert_slots` compares a device result with the oracle's when the frames buffer was prefilled with
a marker byte: a stray store past a frame's last dword, or into a rejected descriptor's slot, shows."""
from __future__ import annotations

import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TX_BUILD_HIP = os.path.join(ROOT, "halo_amd", "csrc", "tx_build.hip")

VARIANTS = ("G1", "G4", "G8", "G16", "pair")
# variant -> the hint its tests pass. 100 is what an honest caller of the local responders passes
# for an ordinary echo reply; 1472 is the benchmark's large-frame hint.
HINTS = {"G1": 22, "G4": 100, "G8": 300, "G16": 500, "pair": 1472}
# the last hint of every rung and the first of the next, and the two spellings of the default
EDGE_HINTS = ((1, "G1"), (22, "G1"), (23, "G4"), (214, "G4"), (215, "G8"), (470, "G8"), (471, "G16"), (982, "G16"),
              (983, "pair"), (0, "pair"))
# test_build_golden_fixtures: every variant's HINTS entry, every edge, and the hints 10 and 0 the
# test passed before it had the right names
GOLDEN_HINTS = tuple(sorted({(v, h) for h, v in EDGE_HINTS} | {(v, h) for v, h in HINTS.items()} | {("G1", 10)},
                            key=lambda vh: (VARIANTS.index(vh[0]), vh[1] or 1 << 20)))
FILL = 0xEE  # the frames buffer's prefill: no byte the build may leave behind by accident (it pads with 0)
MAC = bytes.fromhex("020000000001")


# ---- the ladder ----------------------------------------------------------------------------------
def _one(pattern: str, text: str):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


@functools.lru_cache(maxsize=None)
def read_ladder(path: str = TX_BUILD_HIP) -> dict:
    """The dispatch of halo_tx_build_batch_device as the source has it now: the default hint, the
    chunk-count expression, the `chunks <= N` rungs with the kernel beside each, and what takes the
    rest."""
    with open(path) as fh:
        src = fh.read()
    add_a, add_b, div = _one(r"const uint32_t chunks = \(h \+ (\d+)u \+ (\d+)u\) / (\d+)u;", src)
    rungs = re.findall(r"if \(chunks <= (\d+)\) hipLaunchKernelGGL\(\(halo::tx_build_kernel<(\d+), (\d+)>\)", src)
    return {
        "default": int(_one(r"const uint32_t h = max_payload_hint \? max_payload_hint : (\d+)u;", src)),
        "add": int(add_a) + int(add_b),
        "headers": int(add_a),
        "div": int(div),
        "rungs": tuple((int(lim), int(g), int(u)) for lim, g, u in rungs),
        "pair": int(_one(r"#define HALO_TXB_PAIR (\d+)", src)),
        "big_g": int(_one(r"#define HALO_TXB_BIG_G (\d+)", src)),
    }


def variant_of(hint: int, ladder: dict | None = None) -> str:
    """The build kernel a max_payload_hint selects: "G<lanes per frame>" or "pair"."""
    lad = ladder or read_ladder()
    h = hint if hint else lad["default"]
    chunks = (h + lad["add"]) // lad["div"]
    for lim, g, _u in lad["rungs"]:
        if chunks <= lim:
            return f"G{g}"
    return "pair" if lad["pair"] else f"G{lad['big_g']}"


# ---- descriptors ---------------------------------------------------------------------------------
UNKNOWN_PROTOS = (99, 0, 58, 255, 2)
UNKNOWN_EVERY = 89


def frame_len(desc: np.ndarray) -> np.ndarray:
    """The Build* chain's frame length of each descriptor (from its fields alone)."""
    l4 = np.where(desc["proto"] == 6, 20, 8) + desc["payload_len"].astype(np.int64)
    return np.where(desc["mode"] == 1, 20 + l4, np.maximum(60, 34 + l4))


def _random_fields(rng, desc: np.ndarray) -> None:
    n = len(desc)
    desc["aux"] = rng.integers(0, 256, n)
    icmp = np.flatnonzero(desc["proto"] == 1)
    desc["aux"][icmp] = np.array([8, 0, 11], np.uint8)[np.arange(len(icmp)) % 3]
    for f in ("src_port", "dst_port"):
        desc[f] = rng.integers(0, 1 << 16, n)
    for f in ("src_ip", "dst_ip", "seq", "ack"):
        desc[f] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    desc["dst_mac"] = rng.integers(0, 256, (n, 6))
    desc["dst_mac"][rng.random(n) < 0.02] = 0xFF  # a few broadcasts


def _place_payloads(rng, desc: np.ndarray, align: np.ndarray) -> np.ndarray:
    """Each payload in a cell of its own at the given start alignment, cells 0..3 dwords apart, in a
    buffer of random bytes: whatever a wrong mask or shift pulls in is a neighbour's byte. Sets
    payload_off; returns the buffer (with room behind the last payload)."""
    plen = desc["payload_len"].astype(np.int64)
    cell = ((align + plen + 3) & ~3) + 4 * rng.integers(0, 4, len(desc))
    start = np.concatenate([[0], np.cumsum(cell)[:-1]])
    desc["payload_off"] = start + align
    return rng.integers(0, 256, int(start[-1] + cell[-1]) + 64, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _sweep_sorted():
    from halo_amd._lib import BUILD_DESC_DTYPE

    rng = np.random.default_rng(0x5EE9)
    cols = []
    for proto in (17, 6, 1):
        past = (1460 if proto == 6 else 1472) + 1  # one past the Go limit
        for mode in (0, 1):
            ln = np.repeat(np.arange(past + 1), 4)
            cols.append(np.stack([np.full(len(ln), proto), np.full(len(ln), mode), ln, np.tile(np.arange(4), past + 1)]))
    proto, mode, plen, align = np.concatenate(cols, axis=1)
    n = len(proto)
    while n - n // UNKNOWN_EVERY < len(proto):
        n += 1
    unk = np.arange(n) % UNKNOWN_EVERY == UNKNOWN_EVERY - 1  # one unknown protocol in every 89
    src = np.cumsum(~unk) - 1  # the product's item in front of (or at) each position
    desc = np.zeros(n, BUILD_DESC_DTYPE)
    desc["proto"], desc["mode"], desc["payload_len"] = proto[src], mode[src], plen[src]
    al = align[src].astype(np.int64)
    k = np.flatnonzero(unk)
    desc["proto"][k] = np.array(UNKNOWN_PROTOS, np.uint8)[np.arange(len(k)) % len(UNKNOWN_PROTOS)]
    desc["payload_len"][k] = rng.integers(0, 200, len(k))
    al[k] = rng.integers(0, 4, len(k))
    _random_fields(rng, desc)
    payload = _place_payloads(rng, desc, al)
    desc.setflags(write=False)
    payload.setflags(write=False)
    return desc, payload


@functools.lru_cache(maxsize=None)
def sweep(order: str):
    """(descriptors, payload bytes) of the length sweep, read-only and shared. order "sorted": runs
    of one (protocol, mode) with rising lengths, four alignments per length; "shuffled": a seeded
    permutation of the same descriptors over the same payload buffer."""
    desc, payload = _sweep_sorted()
    if order == "sorted":
        return desc, payload
    assert order == "shuffled", order
    out = desc[np.random.default_rng(0x5F1E).permutation(len(desc))]
    out.setflags(write=False)
    return out, payload


TRIP_STRIDE = 156       # a multiple of 4 and not of 16
TRIP_MAX_PAYLOAD = 100  # TCP over Ethernet: 14 + 20 + 20 + 100 = 154 <= 156
TRIP_SLOT_PAYLOAD = 103  # TCP over Ethernet: 157 > 156, the smallest frame the slot refuses


@functools.lru_cache(maxsize=None)
def second_trip_batch(n: int):
    """(descriptors, payload bytes) of the build's second-trip case, read-only: payloads of 0..100
    bytes (every 61st at 100) at any alignment, protocols and modes mixed, every 97th descriptor an
    unknown protocol, a handful of 100-byte TCP payloads over Ethernet (154 of the slot's 156 bytes).
    In the last, partial tile one TCP payload of 101 bytes over Ethernet (155 bytes: the longest
    frame that fits) and one of 103 (157 bytes: HALO_TX_B_SLOT; with a 156-byte slot 101 is not yet
    refused, 14 + 40 + 101 = 155)."""
    from halo_amd._lib import BUILD_DESC_DTYPE

    rng = np.random.default_rng(0x7219)
    desc = np.zeros(n, BUILD_DESC_DTYPE)
    desc["proto"] = rng.choice(np.array([17, 6, 1], np.uint8), n)
    desc["mode"] = rng.random(n) < 0.3
    desc["payload_len"] = rng.integers(0, TRIP_MAX_PAYLOAD + 1, n)
    desc["payload_len"][::61] = TRIP_MAX_PAYLOAD
    desc["proto"][::97] = 99
    full = np.arange(61 * 7, n, 61 * 1013)  # multiples of 61: already at 100 bytes
    desc["proto"][full], desc["mode"][full] = 6, 0
    last = (n - 1) // 64 * 64  # the first descriptor of the last tile
    assert n - last >= 10 and np.all(full % 97) and full[-1] < last
    for at, plen in ((last + 5, TRIP_MAX_PAYLOAD + 1), (last + 9, TRIP_SLOT_PAYLOAD)):
        assert at % 97 and at % 61
        desc["proto"][at], desc["mode"][at], desc["payload_len"][at] = 6, 0, plen
    _random_fields(rng, desc)
    payload = _place_payloads(rng, desc, rng.integers(0, 4, n))
    desc.setflags(write=False)
    payload.setflags(write=False)
    return desc, payload


# ---- comparison ----------------------------------------------------------------------------------
def expected_slots(wf: np.ndarray, wl: np.ndarray, wr: np.ndarray, fill: int = FILL) -> np.ndarray:
    """The frames buffer a build leaves behind in a buffer prefilled with `fill`, from the oracle's
    frames (untouched bytes 0), lengths and results: a built frame's dwords [0, ceil(len / 4)) are
    the oracle's (zeros past len: the last dword is stored whole), every other byte is the prefill."""
    col = np.arange(wf.shape[1])
    written = (col[None, :] < ((wl.astype(np.int64) + 3) & ~3)[:, None]) & (wr == 0)[:, None]
    return np.where(written, wf, np.uint8(fill))


def assert_slots(got, want_slots: np.ndarray, want, what: str, desc: np.ndarray | None = None) -> None:
    """got = (frames, lens, results, final iphId) of the device, want = the oracle's, want_slots =
    expected_slots(...) of it. Bit-exact; a difference names the descriptor and the first byte."""
    frames, lens, res, end = got
    _wf, wl, wr, we = want
    bad = np.flatnonzero(np.asarray(res) != wr)
    assert bad.size == 0, f"{what}: {bad.size} results differ, first at descriptor {bad[0]}: got {res[bad[0]]} want {wr[bad[0]]}"
    bad = np.flatnonzero(np.asarray(lens) != wl)
    assert bad.size == 0, f"{what}: {bad.size} lengths differ, first at descriptor {bad[0]}: got {lens[bad[0]]} want {wl[bad[0]]}"
    assert frames.shape == want_slots.shape, (what, frames.shape, want_slots.shape)
    if not np.array_equal(frames, want_slots):
        rows = np.flatnonzero(np.any(frames != want_slots, axis=1))
        i = int(rows[0])
        at = int(np.flatnonzero(frames[i] != want_slots[i])[0])
        zone = "the frame" if wr[i] == 0 and at < wl[i] else "the last dword's padding" if wr[i] == 0 and at < (
            (int(wl[i]) + 3) & ~3) else "slot bytes the build must not touch"
        raise AssertionError(
            f"{what}: {rows.size} slots differ (first {rows[:8].tolist()}); descriptor {i}"
            f"{' ' + str(desc[i]) if desc is not None else ''} result {wr[i]} len {wl[i]}: first at byte {at} ({zone}): "
            f"got {frames[i, at:at + 8].tobytes().hex()} want {want_slots[i, at:at + 8].tobytes().hex()}")
    assert end == we, f"{what}: final iphId {end:#x}, want {we:#x}"
