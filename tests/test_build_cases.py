"""CPU: what the transmit-build tests on the device rest on (tests/build_cases.py). The dispatch
ladder of halo_tx_build_batch_device as tx_build.hip has it still gives the hint ranges the GPU
tests' hints were chosen for; the length sweep holds what it is meant to hold; the C oracle, which
is the expectation of every GPU comparison, equals the Python restatement of the Build* chain
(oracle/ref_tx_py.py) on the sweep; and the slot comparison does see a stray store."""
from __future__ import annotations

import numpy as np
import pytest

from tests import build_cases as B

LADDER = {"default": 1472, "headers": 42, "add": 42 + 15, "div": 16, "pair": 1, "big_g": 32,
          "rungs": ((4, 1, 4), (16, 4, 4), (32, 8, 4), (64, 16, 4))}
# variant -> the hints that select it (0 stands for the default)
RANGES = {"G1": (1, 22), "G4": (23, 214), "G8": (215, 470), "G16": (471, 982), "pair": (983, 1 << 16)}


def test_ladder_follows_the_source():
    """The ladder found in tx_build.hip is the one the hints were chosen for: every rung, the
    chunk expression, the default and HALO_TXB_PAIR; and it gives the ranges 1..22, 23..214,
    215..470, 471..982, 983.. with 0 equal to 1472."""
    assert B.read_ladder() == LADDER
    for hint, name in B.EDGE_HINTS:
        assert B.variant_of(hint) == name, (hint, name)
    assert B.variant_of(0) == B.variant_of(1472) == "pair"
    assert set(B.HINTS) == set(B.VARIANTS) == set(RANGES)
    for name, hint in B.HINTS.items():
        assert B.variant_of(hint) == name and RANGES[name][0] <= hint <= RANGES[name][1]
    for name, (lo, hi) in RANGES.items():
        assert {B.variant_of(h) for h in range(lo, min(hi, 4000) + 1)} == {name}
    assert {B.variant_of(h) for h in (1 << 16, (1 << 32) - 1)} == {"pair"}
    assert {v for v, _ in B.GOLDEN_HINTS} == set(B.VARIANTS)
    assert {h for _, h in B.GOLDEN_HINTS} >= {22, 23, 214, 215, 470, 471, 982, 983, 0, 10} | set(B.HINTS.values())
    assert all(B.variant_of(h) == v for v, h in B.GOLDEN_HINTS)


@pytest.mark.parametrize("old,new,moved", [
    ("if (chunks <= 4)", "if (chunks <= 5)", 23), ("if (chunks <= 16)", "if (chunks <= 17)", 215),
    ("if (chunks <= 32)", "if (chunks <= 31)", 470), ("if (chunks <= 64)", "if (chunks <= 65)", 983),
    ("(h + 42u + 15u) / 16u", "(h + 54u + 15u) / 16u", 214), ("max_payload_hint : 1472u", "max_payload_hint : 900u", 0),
    ("tx_build_kernel<4, 4>", "tx_build_kernel<8, 4>", 100), ("#define HALO_TXB_PAIR 1", "#define HALO_TXB_PAIR 0", 1472)])
def test_an_edited_rung_is_noticed(tmp_path, old, new, moved):
    """An edit of any rung of a copy of the source changes the ladder read from it and the variant
    of a hint the GPU tests use: test_ladder_follows_the_source would fail on such a tree."""
    with open(B.TX_BUILD_HIP) as fh:
        src = fh.read()
    assert src.count(old) == 1, old
    path = tmp_path / "tx_build.hip"
    path.write_text(src.replace(old, new))
    lad = B.read_ladder(str(path))
    assert lad != LADDER and B.variant_of(moved, lad) != B.variant_of(moved)


def _tiles(a: np.ndarray, count=None):
    n = len(a) // 64 if count is None else count
    return a[:64 * n].reshape(n, 64)


@pytest.fixture(scope="module")
def sweep_oracle(oracle_lib):
    """(flags, start) -> the C oracle's answer for the sorted sweep (shared, read-only)."""
    desc, payload = B.sweep("sorted")
    return {flags: oracle_lib.tx_build_batch(desc, payload, B.MAC, flags, 1516, 0xFF00) for flags in (1, 0)}


def test_sweep_holds_what_it_claims(oracle_lib, sweep_oracle):
    srt, payload = B.sweep("sorted")
    shf, payload2 = B.sweep("shuffled")
    assert payload is payload2 and 35_000 <= len(srt) <= 36_000
    # one multiset, two orders
    key = lambda d: np.sort(np.ascontiguousarray(d).view(np.dtype((np.void, d.dtype.itemsize))))  # noqa: E731
    assert np.array_equal(key(srt), key(shf)) and srt.tobytes() != shf.tobytes()
    # every payload length 0 .. one past the limit, at all four start alignments, for every
    # protocol and both modes
    known = np.isin(srt["proto"], (17, 6, 1))
    for proto in (17, 6, 1):
        for mode in (0, 1):
            m = (srt["proto"] == proto) & (srt["mode"] == mode)
            past = (1460 if proto == 6 else 1472) + 1
            got = set(zip(srt["payload_len"][m].tolist(), (srt["payload_off"][m] & 3).tolist()))
            assert got == {(ln, a) for ln in range(past + 1) for a in range(4)}, (proto, mode)
    icmp = srt[srt["proto"] == 1]
    assert set(icmp["aux"].tolist()) == {8, 0, 11} and np.any(np.all(srt["dst_mac"] == 0xFF, axis=1))
    assert np.array_equal(np.flatnonzero(~known), np.arange(B.UNKNOWN_EVERY - 1, len(srt), B.UNKNOWN_EVERY))
    # payloads lie apart, inside the buffer with room for the last dword's read
    end = srt["payload_off"].astype(np.int64) + srt["payload_len"]
    assert np.all(srt["payload_off"][1:] >= end[:-1]) and int(end.max()) + 4 <= len(payload)
    # every result code but SLOT (1516-byte slots hold every frame), many tiles with a rejection
    _wf, wl, wr, _we = sweep_oracle[1]
    assert set(wr.tolist()) == {0, 1, 2}
    assert np.array_equal(wl[wr == 0], B.frame_len(srt)[wr == 0]) and not wl[wr != 0].any()
    for d in (srt, shf):
        rejected = ~np.isin(d["proto"], (17, 6, 1)) | (d["payload_len"] > np.where(d["proto"] == 6, 1460, 1472))
        assert int(rejected.sum()) == 400 + 6 * 4 and int(_tiles(rejected).any(1).sum()) > 250  # of 557 tiles
    # every chunk count a variant can meet: 4..95 over Ethernet (60..1514 bytes) and 2..94 as
    # loopback packets (28..1500 bytes: the longest packet is 14 bytes short of a 95th chunk)
    ok = wr == 0
    chunks = (B.frame_len(srt) + 15) // 16
    assert set(chunks[ok & (srt["mode"] == 0)].tolist()) == set(range(4, 96))
    assert set(chunks[ok & (srt["mode"] == 1)].tolist()) == set(range(2, 95))
    # sorted: tiles of one protocol and one mode whose frames differ by a few chunks (and a whole
    # tile of frames <= 64 bytes for the lane kernel's uniform arm); shuffled: none of the first 100
    def uniform(d, count=None):
        p, m = _tiles(d["proto"], count), _tiles(d["mode"], count)
        return (p == p[:, :1]).all(1) & (m == m[:, :1]).all(1)

    u = uniform(srt)
    ch = _tiles(chunks)
    assert int(u.sum()) > 100 and int((ch[u].max(1) - ch[u].min(1)).max()) <= 2
    assert np.any(u & (_tiles(B.frame_len(srt)).max(1) <= 64))
    assert not uniform(shf, 100).any()
    big = _tiles(B.frame_len(shf), 100)
    assert np.all(big.max(1) > 1300) and np.all(big.min(1) < 300) and np.any(big.min(1) <= 64)  # 5-fold within each wave


@pytest.mark.parametrize("flags", [1, 0])
def test_oracle_equals_python_reference(oracle_lib, sweep_oracle, flags):
    """The C oracle's frames, lengths, results and final iphId on the sorted sweep == the Python
    restatement's (oracle/ref_tx_py.tx_build), on every 7th descriptor and on every descriptor whose
    frame length is within 2 of a multiple of 16, iphId from 0xFF00 (it wraps). The oracle numbers
    the whole batch in order, so the restatement's counter for a chosen descriptor starts at
    0xFF00 + the descriptors built before it. About 14,000 descriptors per flag value: a few seconds
    of per-byte Python checksums."""
    from oracle import ref_tx_py as R

    desc, payload = B.sweep("sorted")
    wf, wl, wr, we = sweep_oracle[flags]
    near = (B.frame_len(desc) + 2) % 16 <= 4
    pick = np.flatnonzero(near | (np.arange(len(desc)) % 7 == 0))
    assert 12_000 < len(pick) < 17_000
    built_before = np.concatenate([[0], np.cumsum(wr == 0)[:-1]])
    names = desc.dtype.names
    raw = payload.tobytes()
    for i in pick.tolist():
        d = {k: (bytes(desc[i][k]) if k == "dst_mac" else int(desc[i][k])) for k in names}
        iph = R.IphId(0xFF00 + int(built_before[i]))
        r, frame = R.tx_build(d, raw[d["payload_off"]:d["payload_off"] + d["payload_len"]], B.MAC, iph, bool(flags))
        assert r == wr[i] and len(frame) == wl[i], (i, d, r, wr[i], len(frame), wl[i])
        assert bytes(wf[i, :len(frame)]) == frame and not wf[i, len(frame):].any(), (i, d)
        assert iph.value == (0xFF00 + int(built_before[i]) + (r == 0)) & 0xFFFF
    assert we == (0xFF00 + int((wr == 0).sum())) & 0xFFFF and we < 0xFF00  # wrapped


def test_slot_comparison_sees_stray_stores(oracle_lib):
    desc, payload = B.sweep("shuffled")
    desc = desc[:129]
    want = oracle_lib.tx_build_batch(desc, payload, B.MAC, 1, 1516, 7)
    wf, wl, wr, we = want
    slots = B.expected_slots(wf, wl, wr)
    assert {0, 2} <= set(wr.tolist())
    B.assert_slots((slots.copy(), wl, wr, we), slots, want, "same")
    i = int(np.flatnonzero((wr == 0) & (wl % 4 == 1) & (wl < 1500))[0])
    assert not slots[i, wl[i]:wl[i] + 3].any() and np.all(slots[i, wl[i] + 3:] == B.FILL)
    j = int(np.flatnonzero(wr != 0)[0])
    assert np.all(slots[j] == B.FILL)
    for row, col, zone in ((i, int(wl[i]) + 3, "must not touch"), (j, 40, "must not touch"), (i, int(wl[i]) + 1, "padding"),
                           (i, 30, "the frame")):
        got = slots.copy()
        got[row, col] ^= 0xEE  # a zero where the prefill was, or a wrong frame byte
        with pytest.raises(AssertionError, match=f"descriptor {row} .*byte {col} .*{zone}"):
            B.assert_slots((got, wl, wr, we), slots, want, "stray", desc)
    with pytest.raises(AssertionError, match="final iphId"):
        B.assert_slots((slots, wl, wr, we + 1), slots, want, "id")
    with pytest.raises(AssertionError, match="results differ"):
        B.assert_slots((slots, wl, np.where(np.arange(129) == j, 0, wr), we), slots, want, "res")
