"""GPU: the resident consumer (ring_service_kernel) under the lane fast path: it
runs lane_window with the default store policy, in the uniform layout (one length with the request
line, lane_window<2,0>) and the ragged one (<0,0>), and above 4096 frames each of its 64 waves
loops: window k and window k + 64 are one wave's, which reuses its LDS staging between them and
between requests. Batches of plain frames, with and without one deviating frame or failing
checksums, through HostBatcher.set_resident and through a persistent small-poll RingConsumer; every
record byte and every status count == the C oracle's, and every request is counted as served by the
consumer.
"""
from __future__ import annotations

import contextlib

import numpy as np
import pytest

from tests.gen_golden import icmp_frame, tcp_frame
from tests.helpers import assert_records_equal, golden_arrays, strip_ethernet
from tests.test_gpu_lane_fastpath import golden_frame, pack_rows, padded, plain

pytestmark = pytest.mark.gpu

LENGTHS = (61, 62, 63, 64)
SIZES = (64, 65, 128, 4096, 4097, 8256, 16384)  # 4097 and up: some wave takes a second window


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    yield torch.device("cuda:0")
    assert _lib.registered_count() == 0, _lib.registrations()


_packed: dict = {}


def plain_batch(m: int, length: int = 0):
    """m plain frames, packed (data, offsets_dw, lens; 4-byte aligned starts with gaps): frame i =
    plain(i % 64, L), L = `length`, or 61 + i % 4 (a ragged batch) when it is 0. Shared: not to be
    written to."""
    if (m, length) not in _packed:
        if length not in _packed:
            _packed[length] = np.stack([np.frombuffer(padded(plain(j, length or 61 + j % 4), 64, 0), np.uint8)
                                        for j in range(64)])
        rows = np.tile(_packed[length], ((m + 63) // 64, 1))[:m]
        _packed[m, length] = pack_rows(rows, np.full(m, length) if length else 61 + np.arange(m) % 4)
    return _packed[m, length]


def with_frames(packed, frames: dict):
    """The batch with frame i replaced for every (i, frame) given: the new frames lie behind the
    others, and offsets and lengths point there (a batch's frames need no order in memory)."""
    data, offs, lens = packed[0], packed[1].copy(), packed[2].copy()
    tail = [data, np.zeros(-len(data) % 4, np.uint8)]
    pos = len(data) + len(tail[1])
    for i, f in frames.items():
        offs[i], lens[i] = pos // 4, len(f)
        tail.append(np.frombuffer(f + bytes(-len(f) % 4), np.uint8))
        pos += len(tail[-1])
    return np.concatenate(tail + [np.full(64, 0x5A, np.uint8)]), offs, lens


def fit(frame: bytes, length: int) -> bytes:
    """A frame cut or padded to `length` bytes."""
    return frame[:length] if len(frame) >= length else padded(frame, length)


def failing_checksums(packed, window: int = 0):
    """test_gpu_lane_fastpath's three failing frames inside window `window`: a TTL bit in frame 5, a
    payload bit in frame 40, both in frame 41; each still plain by the predicate."""
    data, offs, lens = packed[0].copy(), packed[1], packed[2]
    for i, byte, bit in ((5, 22, 8), (40, 50, 64), (41, 22, 8), (41, 50, 64)):
        data[4 * int(offs[64 * window + i]) + byte] ^= bit
    return data, offs, lens


class Resident:
    """A HostBatcher with a resident consumer for up to 16384 frames; every parse is compared with
    the oracle and counted."""

    def __init__(self, oracle_lib):
        from halo_amd.engine import HostBatcher

        self.oracle, self.requests = oracle_lib, 0
        self.hb = HostBatcher(0)
        self.hb.set_resident(16384, 4 << 20)

    def parse(self, packed, flags, what, out=None):
        from halo_amd._lib import NetIf

        data, offs, lens = packed
        want, whist = self.oracle.rx_batch(data, lens, self.oracle.NetIf.make(), flags, offsets_dw=offs)
        hist = np.zeros(14, np.uint32)
        got = self.hb.parse(data, offs.astype(np.uint64) * 4, lens, NetIf.make(), flags, hist, out=out)[:len(lens)]
        self.requests += 1
        assert_records_equal(got.copy(), want, None, what)
        assert np.array_equal(hist, whist), (what, "histogram")
        return want

    def close(self):
        """Every request went to the consumer: none to the chunked path, none to a plain launch."""
        st = self.hb.stats()
        self.hb.close()
        assert st["resident_calls"] == self.requests and st["calls"] == self.requests, st
        assert st["resident_parked"] == 0 and st["service_launches"] >= 1, st


@pytest.fixture
def resident(dev, oracle_lib):
    r = Resident(oracle_lib)
    yield r
    r.close()


@pytest.mark.parametrize("length", LENGTHS)
def test_uniform_layout(resident, golden, length):
    """All frames of one length L: the request carries p.len = L and a 64 B stride, and the consumer
    reads no offset or length array (lane_window<2,0>). All plain; one deviating frame of the same
    length at lane 0, 31 or 63 of window 0; failing checksums inside a fast window."""
    deviants = [("eth_type_ipv6", fit(golden_frame(golden, "eth_type_ipv6"), length)),
                ("tcp_64B", fit(tcp_frame(payload=b"0123456789"), length)),
                ("ip_frag_mf", fit(golden_frame(golden, "ip_frag_mf"), length))]
    for m in SIZES:
        base = plain_batch(m, length)
        for flags in (0, 1, 3):
            what = f"uniform L={length} m={m} flags={flags}"
            clean = resident.parse(base, flags, what)
            assert np.all(clean["status"] == 0) and np.all(clean["payload_len"] == length - 42)
            for name, frame in deviants:
                for lane in (0, 31, 63):
                    want = resident.parse(with_frames(base, {lane: frame}), flags, f"{what}, {name} at lane {lane}")
                    assert want[lane].tobytes() != clean[lane].tobytes()
            want = resident.parse(failing_checksums(base), flags, f"{what}, failing checksums")
            assert [int(want["status"][i]) for i in (5, 40, 41)] == ([7, 13, 7] if flags & 1 else [0, 0, 0])


def test_ragged_layout(resident):
    """Lengths cycling through 61..64: offsets and lengths come from the arrays (lane_window<0,0>).
    All plain; a 74 B ICMP frame or a 60 B frame at lane 0, 31 or 63 of window 0."""
    deviants = [("icmp_74B", icmp_frame()), ("udp_60B", plain(1, 60))]
    assert [len(f) for _, f in deviants] == [74, 60]
    for m in SIZES:
        base = plain_batch(m)
        for flags in (0, 1, 3):
            what = f"ragged m={m} flags={flags}"
            clean = resident.parse(base, flags, what)
            assert np.all(clean["status"] == 0)
            for name, frame in deviants:
                for lane in (0, 31, 63):
                    resident.parse(with_frames(base, {lane: frame}), flags, f"{what}, {name} at lane {lane}")


@pytest.mark.parametrize("length", [0, 61, 64], ids=["ragged", "uniform61", "uniform64"])
def test_looping_waves(resident, golden, length):
    """Window k and window k + 64 belong to one wave. m = 8256 (129 windows): windows 0 / 64 / 128
    go fast / general / fast and windows 1 / 65 general / fast. m = 16384: window 64 j + 5 general
    for odd j only. The general windows hold one deviating frame, or (still fast, but every record
    different) the three failing checksums."""
    dev_frame = fit(golden_frame(golden, "eth_type_ipv6"), length) if length else icmp_frame()
    base = plain_batch(8256, length)
    for flags in (0, 1, 3):
        clean = resident.parse(base, flags, "8256 plain")
        want = resident.parse(with_frames(base, {64 * 64 + 17: dev_frame, 64 * 1 + 63: dev_frame}), flags,
                              f"8256, windows 64 and 1 general, flags={flags}")
        changed = np.any(want.view(np.uint8).reshape(-1, 32) != clean.view(np.uint8).reshape(-1, 32), axis=1)
        assert np.nonzero(changed)[0].tolist() == [64 * 1 + 63, 64 * 64 + 17]
        resident.parse(failing_checksums(with_frames(base, {64 * 64: dev_frame}), window=128), flags,
                       f"8256, window 64 general, window 128 failing checksums, flags={flags}")
    base = plain_batch(16384, length)
    for flags in (1, 3):
        resident.parse(base, flags, "16384 plain")
        resident.parse(with_frames(base, {64 * (64 * j + 5) + 9 * j: dev_frame for j in (1, 3)}), flags,
                       f"16384, windows 69 and 197 general, flags={flags}")


@pytest.mark.parametrize("registered_out", [False, True], ids=["pageable_out", "registered_out"])
def test_requests_in_sequence(resident, golden, oracle_lib, registered_out):
    """One context, not closed in between: an all-plain uniform request, a LoChan one
    (HALO_RX_L3_START: never fast), a ragged one with a deviating frame, the all-plain one again;
    twice, so that the plain request also follows itself."""
    from halo_amd import _lib
    from halo_amd._lib import HALO_RX_L3_START, RESULT_DTYPE

    meta, blob = golden
    lo = strip_ethernet(*golden_arrays(meta, blob)[:3])
    out = _lib.host_array(4160, RESULT_DTYPE)
    uniform, ragged = plain_batch(4160, 64), with_frames(plain_batch(4160), {64 * 64 + 31: icmp_frame()})
    with contextlib.ExitStack() as regs:
        if registered_out:
            regs.enter_context(_lib.registered(out))
        for rnd in range(2):
            first = resident.parse(uniform, 1, f"round {rnd}: plain uniform", out=out)
            resident.parse(lo, 1 | HALO_RX_L3_START, f"round {rnd}: LoChan", out=out)
            resident.parse(ragged, 1, f"round {rnd}: ragged with a deviant", out=out)
            again = resident.parse(uniform, 1, f"round {rnd}: plain uniform again", out=out)
            assert again.tobytes() == first.tobytes()


@pytest.mark.parametrize("length", [0, 64], ids=["ragged", "uniform"])
def test_ring_polls(dev, oracle_lib, golden, length):
    """A persistent small-poll consumer: polls of 64, 65, 1000 and 4160 frames in a row (4160: 65
    windows, so one wave takes two), all plain and with one deviating frame, CheckSumEnable on and
    off; records == the oracle's after each poll, each poll served by the resident consumer."""
    from halo_amd._lib import NetIf
    from halo_amd.ring import RingBuffer, RingConsumer

    dev_frame = fit(golden_frame(golden, "ip_frag_mf"), 64) if length else icmp_frame()
    ring = RingBuffer(1 << 23)
    cons = RingConsumer(ring, capacity=1514, persistent=True, max_frames=8192, small_poll=16 << 20)
    polls = 0
    try:
        before = cons.stats()
        for csum in (True, False):
            for deviant_at in (None, 0, 31, 63):
                for k in (64, 65, 1000, 4160):
                    data, offs, lens = plain_batch(k, length)
                    if deviant_at is not None:
                        # in the first window, the last (of 65: one frame; of 4160: a wave's second) or the middle one
                        window = {0: 0, 31: (k - 1) // 64, 63: (k - 1) // 128}[deviant_at]
                        at = min(64 * window + deviant_at, k - 1)
                        data, offs, lens = with_frames((data, offs, lens), {at: dev_frame})
                    want, _ = oracle_lib.rx_batch(data, lens, oracle_lib.NetIf.make(), int(csum), offsets_dw=offs)
                    assert ring.write_batch(data, offs.astype(np.uint64) * 4, lens) == k
                    got, info, _ = cons.poll(NetIf.make(), check_sum_enable=csum)
                    polls += 1
                    assert info["n_frames"] == k and info["stop"] == "EMPTY", info
                    assert_records_equal(got.copy(), want, None, f"poll of {k}, deviant at {deviant_at}, csum {csum}")
                    assert deviant_at is not None or not want["status"].any()
                    cons.commit()
        st = cons.stats()
        assert st["service_requests"] - before["service_requests"] == polls == 32, (st, before)
        assert st["small_polls"] - before["small_polls"] == polls, (st, before)
    finally:
        cons.close()
