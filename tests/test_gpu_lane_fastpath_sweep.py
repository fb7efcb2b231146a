"""GPU: the lane kernel's fast path (lane_plain / lane_fast_record) held to the C
oracle by sweep, not by example: every one-bit mutant of eight plain base frames, alone in an
otherwise plain window and back to back; every header field bit the predicate admits, with both
checksums made right again; and a window of frames chosen for their checksum sums. Each batch runs
under the five modes of test_gpu_lane_fastpath.py, with a status histogram and without one. Every
record byte and every count is the oracle's; no test depends on which path a window took.
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import ref_py as R
from tests.gen_golden import udp_frame
from tests.test_gpu_lane_fastpath import MODE_IDS, MODES, check_packed, pack_rows, padded, plain, to_dev

pytestmark = pytest.mark.gpu

LENGTHS = (61, 62, 63, 64)
OK, ETH_TYPE, IP_VER, IP_FRAG, IP_PROTO, IP_HDR_CKSUM = 0, 2, 4, 5, 6, 7
IP_TOTLEN_UNDERFLOW, IP_TOTLEN_OVERRUN, ICMP_TYPE, L4_CKSUM = 8, 9, 11, 13
N_SWEEP = 8 + 2 * 8 * sum(LENGTHS)  # 8 base frames, each with its 8 L one-bit mutants
# the C oracle's statuses of those frames, CheckSumEnable off / on (flags bit 1 changes nothing here)
SWEEP_COUNTS_CSUM_OFF = {OK: 3529, ETH_TYPE: 128, IP_FRAG: 120, IP_TOTLEN_OVERRUN: 95, IP_VER: 64, IP_PROTO: 56,
                         IP_TOTLEN_UNDERFLOW: 8, ICMP_TYPE: 8}
SWEEP_COUNTS_CSUM_ON = {L4_CKSUM: 1552, OK: 1048, IP_HDR_CKSUM: 1040, ETH_TYPE: 128, IP_FRAG: 120, IP_VER: 64,
                        IP_PROTO: 56}
N_COMPENSATED = 1185  # 8 frames x 23 bytes x 8 bits, less the 287 mutants the predicate rejects


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


def base_frames():
    """Per length 61..64: a UDP frame whose segment fills the frame (totalLen = L - 14), and one
    with a 12-byte payload (totalLen = 40) padded to L with varied non-zero bytes. Both to the
    NetIf, both checksums valid."""
    out = []
    for length in LENGTHS:
        out.append(plain(length, length))
        short = udp_frame(payload=bytes((0x31 + 5 * j) & 0xFF for j in range(12)), sport=4000 + length, dport=53)[:54]
        out.append(padded(short, length))
    return out


def rows_of(frames):
    """Frames as the rows of an (n, 64) array, and their lengths."""
    rows = np.zeros((len(frames), 64), np.uint8)
    for i, f in enumerate(frames):
        rows[i, :len(f)] = np.frombuffer(f, np.uint8)
    return rows, np.array([len(f) for f in frames], np.int64)


def bit_sweep():
    """(rows, lens) of the N_SWEEP frames in sweep order: each base frame, then its mutants by
    rising byte and bit."""
    rows, lens = [], []
    for f in base_frames():
        L = len(f)
        m = np.tile(np.frombuffer(padded(f, 64, 0), np.uint8), (8 * L + 1, 1))
        k = np.arange(8 * L)
        m[1 + k, k // 8] ^= (1 << (k % 8)).astype(np.uint8)
        m[:, L:] = 0
        rows.append(m)
        lens.append(np.full(8 * L + 1, L))
    return np.concatenate(rows), np.concatenate(lens)


def is_plain(rows, lens):
    """The fast path's predicate restated (rx_lane.hip, lane_plain and the length ballot), one
    bool per row. Asserted as a population only; never an expected value."""
    tl = rows[:, 16].astype(np.int64) << 8 | rows[:, 17]
    return ((lens >= 61) & (lens <= 64)
            & (rows[:, 12] == 0x08) & (rows[:, 13] == 0x00) & (rows[:, 14] == 0x45)
            & ((rows[:, 20] & 0xBF) == 0) & (rows[:, 21] == 0) & (rows[:, 23] == 0x11)
            & (tl >= 28) & (tl <= lens - 14))


def plain_rows(n):
    """n plain 64 B frames, frame i = plain(i % 64)."""
    base, _ = rows_of([plain(j) for j in range(64)])
    return np.tile(base, ((n + 63) // 64, 1))[:n]


def isolated(rows, lens):
    """Frame k of the sweep at lane k % 64 of window k; plain(j) at every other lane j."""
    n = len(lens)
    at = 64 * np.arange(n) + np.arange(n) % 64
    allr, alll = plain_rows(64 * n), np.full(64 * n, 64)
    allr[at], alll[at] = rows, lens
    return allr, alll, at


def dense(rows, lens, tail=37):
    """The sweep's frames back to back, plain frames up to the next multiple of 64, then a partial
    window of `tail` plain frames."""
    n = len(lens)
    fill = -n % 64 + tail
    return np.concatenate([rows, plain_rows(fill)]), np.concatenate([lens, np.full(fill, 64)]), np.arange(n)


class Batch:
    """One packed batch: on the device once, the oracle's records and counts once per flags."""

    def __init__(self, dev, oracle_lib, rows, lens, at=None):
        self.rows, self.lens = rows, lens
        self.at = np.arange(len(lens)) if at is None else at  # where the frames under test sit
        self.data, self.offs, self.plens = pack_rows(rows, lens)
        self.dev, self.oracle, self._bufs, self._ref = dev, oracle_lib, None, {}

    def ref(self, flags):
        if flags not in self._ref:
            self._ref[flags] = self.oracle.rx_batch(self.data, self.plens, self.oracle.NetIf.make(), flags,
                                                    offsets_dw=self.offs, threads=8)
        return self._ref[flags]

    def run(self, mode, what):
        """Both launches of one mode: with a histogram (a wave of a small grid takes two windows)
        and without (one window)."""
        flags, compact = mode
        if self._bufs is None:
            self._bufs = to_dev(self.dev, self.data, self.offs, self.plens)
        try:
            for with_hist in (True, False):
                check_packed(self.dev, self._bufs, self.ref(flags), flags, compact,
                             f"{what}, {'hist' if with_hist else 'no hist'}", with_hist)
        except AssertionError as e:
            raise AssertionError(f"{e}\n{self.first_bad(flags, compact)}") from None

    def first_bad(self, flags, compact):
        """The bytes of the first frame whose record differs, for the assertion message (a separate
        launch: only reached when a comparison has already failed)."""
        import torch

        from halo_amd import _lib
        from halo_amd._lib import NetIf, compact_of

        d, o, ln = self._bufs
        want = self.ref(flags)[0]
        n, width = len(want), 16 if compact else 32
        out = torch.zeros((n, width), dtype=torch.uint8, device=self.dev)
        word = flags | _lib.variant_flags(1) | (_lib.HALO_RX_RECORD_COMPACT if compact else 0)
        _lib.check("parse", _lib.lib.halo_rx_parse_batch_device(
            d.data_ptr(), o.data_ptr(), ln.data_ptr(), n, word, NetIf.make(), 64, out.data_ptr(), None,
            torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        wb = np.ascontiguousarray(compact_of(want) if compact else want).view(np.uint8).reshape(n, width)
        bad = np.nonzero(np.any(out.cpu().numpy() != wb, axis=1))[0]
        if not bad.size:
            return "(records equal on a second launch without a histogram: the counts differ)"
        i = int(bad[0])
        return (f"first differing frame {i} (lane {i % 64} of window {i // 64}), {int(self.lens[i])} bytes: "
                f"{self.rows[i, :self.lens[i]].tobytes().hex()}")


@pytest.fixture(scope="module")
def sweep():
    return bit_sweep()


@pytest.fixture(scope="module")
def batches(dev, oracle_lib, sweep):
    rows, lens = sweep
    return {"isolated": Batch(dev, oracle_lib, *isolated(rows, lens)),
            "dense": Batch(dev, oracle_lib, *dense(rows, lens))}


def counts(status):
    return {int(s): int(c) for s, c in zip(*np.unique(status, return_counts=True))}


def test_sweep_population(oracle_lib, sweep, batches):
    """What the sweep feeds, by the oracle: how many of its frames the predicate admits, which
    statuses the others carry, and that the dense arrangement holds whole windows of plain frames
    that all fail a checksum (the fast path's histogram branch with no OK lane). Counted here, by the
    C oracle, for base_frames(); the literals are that count."""
    rows, lens = sweep
    assert len(lens) == N_SWEEP == 4008
    pl = is_plain(rows, lens)
    assert (int(pl.sum()), int((~pl).sum())) == (3529, 479)
    for name, b in batches.items():
        off = b.ref(0)[0]["status"][b.at]
        on = b.ref(1)[0]["status"][b.at]
        assert counts(off) == SWEEP_COUNTS_CSUM_OFF, name
        assert counts(on) == SWEEP_COUNTS_CSUM_ON, name
        assert np.array_equal(off == OK, pl), name  # without checksums a plain frame has nothing left to fail
        rest = np.ones(len(b.lens), bool)
        rest[b.at] = False
        assert np.all(b.ref(1)[0]["status"][rest] == OK) and np.all(is_plain(b.rows[rest], b.lens[rest]))
    d = batches["dense"]
    n_win = len(d.lens) // 64
    failing = (d.ref(1)[0]["status"][:64 * n_win] != OK) & is_plain(d.rows[:64 * n_win], d.lens[:64 * n_win])
    assert int(failing.reshape(n_win, 64).all(axis=1).sum()) >= 8  # one or more per base frame
    assert len(d.lens) % 64 != 0 and len(batches["isolated"].lens) == 64 * N_SWEEP


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("arrangement", ["isolated", "dense"])
def test_single_bit_sweep(batches, arrangement, mode):
    """isolated: 4008 windows, each plain but for one lane that holds a sweep frame (the window stays
    fast or exactly one lane forces it general). dense: the sweep back to back (whole windows of
    plain frames failing L4_CKSUM; header mutants mixing both paths in a window; a partial window)."""
    batches[arrangement].run(mode, f"{arrangement} sweep")


def compensated():
    """Every one-bit mutant of bytes 15..41 of the base frames that is outside the checksum fields
    (24-25, 40-41) and that the predicate admits, with the IPv4 header checksum and the UDP checksum
    computed again (oracle.ref_py) over the bytes the reference sums: TOS, totalLen, id, DF, TTL,
    addresses, ports and the UDP length field, each bit, in frames that are valid."""
    out = []
    for f in base_frames():
        L = len(f)
        for byte in [b for b in range(15, 42) if b not in (24, 25, 40, 41)]:
            for bit in range(8):
                m = bytearray(f)
                m[byte] ^= 1 << bit
                r, ln = rows_of([bytes(m)])
                if not is_plain(r, ln)[0]:
                    continue
                m[24:26] = b"\0\0"
                m[24:26] = R.get_checksum(bytes(m[14:34])).to_bytes(2, "big")
                end = 14 + (m[16] << 8 | m[17])
                m[40:42] = b"\0\0"
                fake = bytes(m[26:34]) + b"\x00\x11" + bytes(m[38:40])  # src, dst, 0x0011, the UDP length field
                m[40:42] = R.get_checksum(fake + bytes(m[34:end])).to_bytes(2, "big")
                assert len(m) == L
                out.append(bytes(m))
    return out


@pytest.mark.parametrize("flags", [1, 3])
def test_compensated_field_sweep(dev, oracle_lib, flags):
    """Dense; CheckSumEnable on. Every frame is OK by the oracle: a wrong multiplier or a wrong
    byte select on any header field shows as a failed checksum or a wrong record field."""
    frames = compensated()
    rows, lens = rows_of(frames)
    assert len(frames) == N_COMPENSATED and np.all(is_plain(rows, lens))
    b = Batch(dev, oracle_lib, *dense(rows, lens, tail=11))
    assert np.all(b.ref(flags)[0]["status"] == OK)
    for field, bits in (("src_ip", 32), ("dst_ip", 32), ("sport", 16), ("dport", 16)):  # every bit of each was flipped
        assert len(np.unique(b.ref(flags)[0][field][:len(frames)])) > bits, field
    b.run((flags, False), "compensated field sweep")


def fold_edges():
    """64 valid plain frames chosen for their sums: the largest unfolded sums (addresses
    255.255.255.255, ports 0xFFFF, payload 0xFF), the smallest (payload 0x00, ports 1), a segment
    whose UDP checksum computes to 0x0000, carried as 0xFFFF and as 0x0000 (the oracle decides what
    each means), and 0xFF segments of every parity of totalLen under 0xFx padding that the dword
    mask has to cut off, all at each frame length."""
    ff = b"\xff" * 4
    frames = []
    for L in LENGTHS:
        frames.append(udp_frame(payload=b"\xff" * (L - 42), src=ff, dst_ip=ff, sport=0xFFFF, dport=0xFFFF))
        frames.append(udp_frame(payload=bytes(L - 42), sport=1, dport=1))
        pay = bytearray((0x11 * j) & 0xFF for j in range(L - 42))
        pay[0:2] = b"\0\0"
        s = 0xFFFF ^ R.be16(udp_frame(payload=bytes(pay))[40:42])  # the folded sum with that word at 0
        assert s != 0
        pay[0:2] = (0xFFFF - s).to_bytes(2, "big")
        assert R.be16(udp_frame(payload=bytes(pay))[40:42]) == 0
        frames.append(udp_frame(payload=bytes(pay), udp_csum=0xFFFF))
        frames.append(udp_frame(payload=bytes(pay), udp_csum=0x0000))
        for pay_len in np.linspace(0, L - 43, 12).astype(int):  # totalLen 28 .. L - 15, both parities
            short = udp_frame(payload=b"\xff" * int(pay_len), src=ff, dst_ip=ff, sport=0xFFFF, dport=0xFF00 + L)
            frames.append(padded(short[:42 + int(pay_len)], L, fill=0xF0))
    return frames


def test_fold_and_carry_edges(dev, oracle_lib):
    """The window of fold_edges(), then the same window with one bit flipped in each frame's last
    segment byte (byte 13 + totalLen: its half-word is the one the dword mask cuts through)."""
    frames = fold_edges()
    rows, lens = rows_of(frames)
    assert len(frames) == 64 and np.all(is_plain(rows, lens))
    tl = rows[:, 16].astype(np.int64) << 8 | rows[:, 17]
    assert {int(t) % 2 for t in tl} == {0, 1} and all(np.any(tl[lens == L] % 2 == p) for L in LENGTHS for p in (0, 1))
    good = Batch(dev, oracle_lib, rows, lens)
    assert np.all(good.ref(1)[0]["status"] == OK) and np.all(good.ref(0)[0]["status"] == OK)
    flipped = rows.copy()
    flipped[np.arange(64), 13 + tl] ^= 1 << (np.arange(64) % 8).astype(np.uint8)
    bad = Batch(dev, oracle_lib, flipped, lens)
    assert np.all(is_plain(flipped, lens)) and np.all(bad.ref(1)[0]["status"] == L4_CKSUM)
    for mode, name in zip(MODES, MODE_IDS):
        good.run(mode, f"fold edges {name}")
        bad.run(mode, f"fold edges, last segment byte flipped, {name}")
