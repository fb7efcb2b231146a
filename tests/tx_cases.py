"""Not a test: which kernel halo_tx_fixup_batch_device launches for a max_len_hint, the plan the
kernel makes for a frame, and the case table of the transmit-rewrite sweep.

`read_ladder` takes the hint ladder and the loop constants out of halo_amd/csrc/tx_fixup.hip with
plain regular expressions (as build_cases.read_ladder does for the build) and `width_of` restates
it, so a moved rung fails tests/test_tx_cases.py on the CPU until HINTS moves with it. Every GPU
test of the sweep takes its hint from HINTS and asserts through `width_of` the width it names.

`plan_of(frame, steps, en)` restates apply_steps' plan (ip_hi, go_hi, dp_hi and the two L4 ranges
l4a / l4b of tx_frame) and names the path the frame takes. It only proves what the table reaches
(tests/test_tx_cases.py); it is never an expected value: those come from the C oracle.

`sweep()` is the table: IPv4 frames with real options (IHL 5..15), four protocols, L4 lengths on
both sides of every edge of the header copy and of every iteration of the kernel's two loops at
every width, five relations between the total-length field and the frame, nine step sets each.
`ordered(name)` gives it as generated ("mixed": neighbours differ in step set, every wave mixes
plans) or stably sorted by path class ("uniform": whole waves take one path, the ballot-guarded
arms of ip_header_sum / l4_header_sum). `layout(cases, rng)` lays the frames 0..3 dwords apart in
a buffer of random bytes, so that a stray or over-wide store, or a mask that pulls in a
neighbour's byte, shows in a whole-buffer compare; `first_difference` names the case it shows in."""
from __future__ import annotations

import functools
import os
import re
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TX_FIXUP_HIP = os.path.join(ROOT, "halo_amd", "csrc", "tx_fixup.hip")

WIDTHS = (1, 4, 8, 16)
# lanes per frame -> the hint its tests pass (0: unknown, the widest)
HINTS = {1: 64, 4: 1000, 8: 4000, 16: 0}

NAT_DST, TTL, NAT_SRC, RECALC, DPDK_FILL = 0x01, 0x02, 0x04, 0x08, 0x10


# ---- the ladder ----------------------------------------------------------------------------------
def _one(pattern: str, text: str):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


@functools.lru_cache(maxsize=None)
def read_ladder(path: str = TX_FIXUP_HIP) -> dict:
    """The dispatch of halo_tx_fixup_batch_device as the source has it now: what hint 0 stands for,
    the `h <= N` rungs with the lanes per frame beside each, what takes the rest; and the constants
    the sweep's lengths are built around: kHdrDw (dwords of the header copy), U0 and U (16-byte
    chunks per lane in the first and the later load rounds)."""
    with open(path) as fh:
        src = fh.read()
    launch = r"hipLaunchKernelGGL\(halo::tx_fixup_kernel<(\d+)>"
    g1_max = int(_one(r"#define HALO_TX_G1_MAX (\d+)", src))
    first = int(_one(r"\n    if \(h <= HALO_TX_G1_MAX\) " + launch, src))
    rungs = re.findall(r"else if \(h <= (\d+)\) " + launch, src)
    return {
        "default": int(_one(r"const uint32_t h = max_len_hint \? max_len_hint : (\d+)u;", src)),
        "rungs": ((g1_max, first),) + tuple((int(lim), int(g)) for lim, g in rungs),
        "rest": int(_one(r"\n    else " + launch, src)),
        "kHdrDw": int(_one(r"constexpr uint32_t kHdrDw = (\d+);", src)),
        "U0": int(_one(r"constexpr int U0 = (\d+);", src)),
        "U": int(_one(r"constexpr int U = (\d+);", src)),
    }


def width_of(hint: int, ladder: dict | None = None) -> int:
    """The lanes per frame a max_len_hint selects."""
    lad = ladder or read_ladder()
    h = hint if hint else lad["default"]
    for lim, g in lad["rungs"]:
        if h <= lim:
            return g
    return lad["rest"]


# ---- the plan ------------------------------------------------------------------------------------
HDR = 52  # bytes of the header copy (4 * kHdrDw); test_tx_cases.py holds it against the source


def plan_of(frame, steps: int, en) -> dict:
    """The checksum plan the kernel makes for `frame` under `steps` and CheckSumEnable `en`:
    ip_hi (the IPv4 sum covers [14, ip_hi)), go_hi (the Go L4 recalculation, [34, go_hi)), dp_hi
    (the DPDK fill's L4 sum, [34, dp_hi)), each 0 when not summed; l4a / l4b, the L4 ranges of the
    kernel's first and second pass; and "cls", the name of the path: which arm the IPv4 sum takes
    (ip0 none, ip34 the constant form, ipgen the masked header sum, iptail past the header copy),
    whose range pass 1 sums (go / dp, "<52" when it ends inside the header copy: the masked arm of
    l4_header_sum), and whether a second range follows ("+dp<=52" from the header copy alone,
    "+dp>52" through the pass-2 loop)."""
    L = len(frame)
    h = bytes(bytearray(frame[:HDR])).ljust(HDR, b"\0")
    steps &= 0xFF
    ip_hi = go_hi = dp_hi = 0
    if L >= 14:
        n = L - 14  # len(pkt)
        proto = h[23]
        ip_go, l4_go = False, 0

        def recalc_l4():
            need = {1: 24, 6: 38, 17: 28}.get(proto)
            return proto if need is not None and n >= need else 0

        alive = True
        if steps & NAT_DST and n >= 26:
            ip_go = True
            l4_go = recalc_l4() or l4_go
        if steps & TTL:
            if n < 9 or h[22] <= 1:
                alive = False
            elif n >= 20:
                ip_go = True
        if alive:
            if steps & NAT_SRC and n >= 26:
                ip_go = True
                l4_go = recalc_l4() or l4_go
            if steps & RECALC:
                ip_go = ip_go or n >= 20
                if n >= 10:
                    l4_go = recalc_l4() or l4_go
        if ip_go and en:
            ip_hi = 34
        if l4_go == 1 or (l4_go and en):
            go_hi = L
        if alive and steps & DPDK_FILL and h[12:14] == b"\x08\x00" and L >= 34:
            ihl4 = (h[14] & 15) * 4
            ip_hi = 14 + ihl4 if 14 + ihl4 <= L else 0
            if proto in (17, 6):
                field = 40 if proto == 17 else 50
                if field + 2 <= L:
                    if ip_hi <= field:
                        go_hi = 0  # the Go value is overwritten before any sum sees it
                    l3 = (h[16] << 8) | h[17]
                    if l3 >= ihl4 and 34 + l3 - ihl4 <= L:
                        dp_hi = 34 + l3 - ihl4
    l4a = go_hi or dp_hi
    l4b = dp_hi if go_hi else 0
    ip = "ip0" if not ip_hi else "ip34" if ip_hi == 34 else "ipgen" if ip_hi <= HDR else "iptail"
    a = "-" if not l4a else ("go" if go_hi else "dp") + ("<52" if l4a < HDR else "")
    b = "" if not l4b else "+dp<=52" if l4b <= HDR else "+dp>52"
    return {"L": L, "ip_hi": ip_hi, "go_hi": go_hi, "dp_hi": dp_hi, "l4a": l4a, "l4b": l4b, "cls": f"{ip}/{a}{b}"}


# ---- the table -----------------------------------------------------------------------------------
IHLS = (5, 6, 7, 9, 10, 11, 15)
PROTOS = (17, 6, 1, 2)
TTLS = (1, 2, 64, 255)
# total-length field against the frame: exact; exact with 3 bytes of non-zero padding behind; 5
# short (the fill's L4 range ends at an odd byte inside the frame); 4 long (at IHL 5 past the frame:
# OVERRUN); long by the options' length, 4 * (IHL - 5), so that the fill's L4 range ends at the
# frame's end (dp_hi == L)
RELATIONS = ("exact", "padded", "short5", "long4", "long_options")
STEP_SETS = (0x1F, 0x17, 0x15, 0x19, 0x10, 0x08, 0x03, 0x06)  # and one seeded random value per frame
MAX_FRAME = 1514
ITER_BYTES = 64  # one iteration of either loop covers ITER_BYTES * G bytes: U chunks of 16 bytes per lane


def l4_lengths() -> tuple:
    """Bytes behind the IPv4 header: the header-copy edges, both sides of every iteration edge of
    both loops at every width (64 G + d; d = -35..-33 puts the L4 range's end, 34 + length, at the
    edge), and two full-size lengths. The lengths 2, 3, 5, 6, 12 and 13 are there for the rare
    path classes (a range that ends inside the header copy, before or behind a second one): with
    them every class fills two 64-frame waves in the uniform order."""
    edges = [*range(0, 7), 8, 9, 12, 13, *range(17, 21), *range(29, 35), *range(50, 54)]
    loops = [ITER_BYTES * g + d for g in WIDTHS for d in (-35, -34, -33, -2, -1, 0, 1, 2, 3, 5)]
    return tuple(sorted(set(edges + loops + [1440, 1441])))


def _subset(c, idx):
    idx = np.asarray(idx)
    out = SimpleNamespace(blob=c.blob, **{k: getattr(c, k)[idx] for k in _PER_CASE})
    for k in _PER_CASE:
        getattr(out, k).setflags(write=False)
    return out


_PER_CASE = ("start", "lens", "ops", "proto", "ihl", "l4len", "rel", "total_len", "steps", "ident")


@functools.lru_cache(maxsize=None)
def sweep(seed: int = 0x7F1C5):
    """The case table, read-only and shared: `blob` holds the frames back to back, and per case
    `start` (into blob), `lens`, `ops` (halo_tx_op_t), the parameters it was made from (`proto`,
    `ihl`, `l4len`, `rel` as an index into RELATIONS, `total_len`, `steps`) and `ident`, its
    position in this order. Frames whose length would exceed 1514 bytes are left out."""
    from oracle.oracle import TX_OP_DTYPE

    rng = np.random.default_rng(seed)
    per_frame = len(STEP_SETS) + 1
    rows = []
    for ihl in IHLS:
        for proto in PROTOS:
            for l4 in l4_lengths():
                for r, rel in enumerate(RELATIONS):
                    L = 14 + 4 * ihl + l4 + (3 if rel == "padded" else 0)
                    if L > MAX_FRAME:
                        continue
                    tl = 4 * ihl + l4 + {"short5": -5, "long4": 4, "long_options": 4 * (ihl - 5)}.get(rel, 0)
                    rows.append((ihl, proto, l4, r, tl, L))
    ihl, proto, l4, rel, tl, L = (np.repeat(np.array(col, np.int64), per_frame) for col in zip(*rows))
    n = len(L)
    steps = np.tile(np.array(STEP_SETS + (0,), np.int64), n // per_frame)
    rand = np.arange(n) % per_frame == per_frame - 1
    steps[rand] = rng.integers(0, 32, int(rand.sum()))
    start = np.concatenate([[0], np.cumsum(L)[:-1]])
    blob = rng.integers(0, 256, int(L.sum()), dtype=np.uint8)  # MACs, header fields, options, payload
    blob[start + 12], blob[start + 13] = 0x08, 0x00
    blob[start + 14] = 0x40 | ihl
    blob[start + 16], blob[start + 17] = tl >> 8, tl & 0xFF
    blob[start + 22] = np.array(TTLS, np.uint8)[rng.integers(0, len(TTLS), n)]
    blob[start + 23] = proto
    pad = np.flatnonzero(rel == RELATIONS.index("padded"))
    for back in (1, 2, 3):
        at = start[pad] + L[pad] - back
        blob[at] = np.where(blob[at] == 0, 0xA5, blob[at])
    ops = np.zeros(n, TX_OP_DTYPE)
    ops["steps"] = steps
    for f in ("dst_ip", "src_ip"):
        ops[f] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for f in ("dst_port", "src_port"):
        ops[f] = rng.integers(0, 1 << 16, n)
    blob.setflags(write=False)
    c = SimpleNamespace(blob=blob, start=start, lens=L.astype(np.uint16), ops=ops, proto=proto.astype(np.uint8),
                        ihl=ihl.astype(np.uint8), l4len=l4.astype(np.uint16), rel=rel.astype(np.uint8),
                        total_len=tl.astype(np.uint16), steps=steps.astype(np.uint8), ident=np.arange(n))
    return _subset(c, np.arange(n))


def frame_of(c, i: int) -> np.ndarray:
    s = int(c.start[i])
    return c.blob[s:s + int(c.lens[i])]


@functools.lru_cache(maxsize=None)
def plans(flag: int) -> tuple:
    """plan_of for every case of sweep(), in its order, under CheckSumEnable = flag."""
    c = sweep()
    raw = c.blob.tobytes()
    return tuple(plan_of(raw[s:s + n], st, flag)
                 for s, n, st in zip(c.start.tolist(), c.lens.tolist(), c.steps.tolist()))


ORDERS = ("mixed", "uniform")


@functools.lru_cache(maxsize=None)
def ordered(order: str):
    """sweep() as generated ("mixed"), or stably sorted by the path class it takes with
    CheckSumEnable on ("uniform")."""
    c = sweep()
    if order == "mixed":
        return c
    assert order == "uniform", order
    names = sorted({p["cls"] for p in plans(1)})
    key = np.array([names.index(p["cls"]) for p in plans(1)])
    return _subset(c, np.argsort(key, kind="stable"))


def layout(c, rng):
    """(data, offsets_dw, lens): the cases' frames in their order at 4-byte aligned starts, 0..3
    dwords apart, in a buffer of random bytes (64 of them behind the last frame)."""
    L = c.lens.astype(np.int64)
    cell = ((L + 3) & ~3) + 4 * rng.integers(0, 4, len(L))
    offs = np.concatenate([[0], np.cumsum(cell)[:-1]])
    data = rng.integers(0, 256, int(offs[-1] + cell[-1]) + 64, dtype=np.uint8)
    for o, s, n in zip(offs.tolist(), c.start.tolist(), L.tolist()):
        data[o:o + n] = c.blob[s:s + n]
    return data, (offs // 4).astype(np.uint32), c.lens


def describe(c, i: int, flag: int) -> str:
    p = plans(flag)[int(c.ident[i])]
    return (f"case {i} (table row {int(c.ident[i])}): proto {int(c.proto[i])} IHL {int(c.ihl[i])} L {int(c.lens[i])} "
            f"total length {int(c.total_len[i])} ({RELATIONS[int(c.rel[i])]}) steps {int(c.steps[i]):#04x} "
            f"flag {flag}; plan {p}")


def first_difference(c, flag: int, got, want, offsets_dw, got_res=None, want_res=None, what: str = "") -> None:
    """Bit-exact compare of a whole buffer (and the result bytes); a difference names the case, its
    plan and the first differing offset inside its frame (or the gap behind it)."""
    if got_res is not None:
        bad = np.flatnonzero(np.asarray(got_res) != np.asarray(want_res))
        if bad.size:
            i = int(bad[0])
            raise AssertionError(f"{what}: {bad.size} result bytes differ; first got {int(got_res[i])} want "
                                 f"{int(want_res[i])} at {describe(c, i, flag)}")
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    at = int(bad[0])
    byte_off = offsets_dw.astype(np.int64) * 4
    i = int(np.searchsorted(byte_off, at, side="right")) - 1
    rel = at - int(byte_off[i])
    where = f"frame offset {rel}" if rel < int(c.lens[i]) else f"{rel - int(c.lens[i])} bytes behind the frame (gap)"
    frames = np.unique(np.searchsorted(byte_off, bad, side="right") - 1)
    raise AssertionError(f"{what}: {bad.size} buffer bytes differ in {frames.size} cases (first {frames[:8].tolist()}); "
                         f"first at buffer byte {at}, {where}: got {got[at:at + 8].tobytes().hex()} want "
                         f"{want[at:at + 8].tobytes().hex()}; {describe(c, i, flag)}")
