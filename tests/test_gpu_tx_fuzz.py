"""tx_fixup on the structured fuzz corpus (oracle/halo_fuzz.c): 20,000 frames from 0 to about
9,100 bytes, runt and jumbo frames, every EtherType the generator knows, IHL nibbles 0..15, total
lengths on every side of the frame's, under random step sets. halo_tx_fixup_batch_device against
oracle.tx_batch, bit-exact over the WHOLE buffer (gap bytes random) and the result bytes, at every
lanes-per-frame width; the hint is then often smaller than the frames, which is legal ("any G
handles any length"). Behind the corpus lie UDP_ZERO_ROWS frames whose UDP sum under the fill step
is 0x0000, which DPDK sends as 0xFFFF: one frame in 65,536 has it by chance, the corpus none. The CPU
test proves from the oracle alone what the batch holds."""
from __future__ import annotations

import numpy as np
import pytest

from tests import tx_cases as T
from tests.helpers import random_tx_ops

SEED, N, OPS_SEED = 0x7F1, 20_000, 5
UDP_ZERO_ROWS = 24


def _udp_zero_rows(oracle, rng):
    """(frames, ops): UDP frames of 44 to about 3,000 bytes, odd and even, under step sets that hold
    the fill, with payload bytes 0..1 set so that the fill's UDP sum is 0x0000. The C oracle is the
    solver: with the free word at zero it stores the complement of the rest of the sum; with the
    free word at that value the sum is 0xFFFF, its complement zero, and 0xFFFF is what is sent."""
    from oracle import ref_py as R

    frames, ops = [], np.array(random_tx_ops(UDP_ZERO_ROWS, OPS_SEED + 1))
    for k in range(UDP_ZERO_ROWS):
        ops["steps"][k] = (0x10, 0x1F, 0x15, 0x18)[k % 4]
        src, dst = bytes(rng.integers(0, 256, 4, dtype=np.uint8)), bytes(rng.integers(0, 256, 4, dtype=np.uint8))
        pl = bytearray(rng.integers(0, 256, int((2, 3, 18, 19, 470, 1471, 1472, 2990)[k % 8] + 2 * (k // 8)), dtype=np.uint8))
        sport, dport = int(rng.integers(1, 65536)), int(rng.integers(1, 65536))
        pl[0:2] = b"\0\0"
        for _ in range(2):
            seg = R.build_udp(bytes(pl), sport, dport, src, dst)
            f = R.build_eth(R.build_ipv4(seg, 17, src, dst, ttl=64), bytes(6), bytes(6), 0x0800, pad=False)
            out, _ = oracle.tx_frame(f, ops[k], 1)
            pl[0:2] = out[40:42]
        assert out[40:42] == b"\xff\xff" and pl[0:2] == b"\xff\xff", k  # (the second pass stored the substitute)
        frames.append(f)
    return frames, ops


@pytest.fixture(scope="module")
def fuzz(oracle_lib):
    """The batch with its gap bytes overwritten by random ones, its ops, and flag -> the C oracle's
    buffer and result bytes (one oracle run per flag, shared, not modified)."""
    data, offs, lens = oracle_lib.fuzz_batch(SEED, N, oracle_lib.NetIf.make())
    rng = np.random.default_rng(SEED + 1)
    extra, extra_ops = _udp_zero_rows(oracle_lib, rng)
    at = (data.size + 3) & ~3
    for f in extra:  # behind the corpus, 0..3 dwords apart
        at += 4 * int(rng.integers(0, 4))
        offs, lens = np.append(offs, np.uint32(at // 4)), np.append(lens, np.uint16(len(f)))
        at += (len(f) + 3) & ~3
    data = np.concatenate([data, np.zeros(at + 64 - data.size, np.uint8)])
    for o, f in zip(offs[N:].tolist(), extra):
        data[4 * o:4 * o + len(f)] = np.frombuffer(f, np.uint8)
    gap = np.ones(data.size, bool)
    for o, L in zip((offs.astype(np.int64) * 4).tolist(), lens.tolist()):
        gap[o:o + L] = False
    data[gap] = np.random.default_rng(SEED).integers(1, 256, int(gap.sum()), dtype=np.uint8)
    ops = np.concatenate([np.array(random_tx_ops(N, OPS_SEED)), extra_ops])
    for a in (data, offs, lens, gap):
        a.setflags(write=False)
    wants = {}

    def get(flag):
        if flag not in wants:
            wants[flag] = oracle_lib.tx_batch(data, offs, lens, ops, flags=flag, threads=8)
        return data, offs, lens, ops, gap, wants[flag]

    return get


def _frame_fields(data, offs, lens):
    """Per frame: EtherType, IHL nibble (frames of 15 bytes and more; else -1)."""
    start = offs.astype(np.int64) * 4
    L = lens.astype(np.int64)
    at = lambda k: data[np.minimum(start + k, data.size - 1)].astype(np.int64)  # noqa: E731
    ethertype = np.where(L >= 14, (at(12) << 8) | at(13), -1)
    ihl = np.where(L >= 15, at(14) & 15, -1)
    return ethertype, ihl


def test_fuzz_batch_reaches_the_edges(fuzz):
    """From the oracle's output and the frame bytes: the batch holds every result byte, the fill
    step on malformed IHLs and on foreign EtherTypes, and frames below and above every size the
    kernel's arithmetic assumes."""
    for flag in (0, 1):
        data, offs, lens, ops, gap, (want, res) = fuzz(flag)
        assert gap.sum() > 10_000 and np.array_equal(want[gap], data[gap])
        counts = np.bincount(res, minlength=8)
        assert counts.size == 8 and counts.min() >= 50, counts
        ethertype, ihl = _frame_fields(data, offs, lens)
        fill = (ops["steps"] & T.DPDK_FILL) != 0
        ipv4 = fill & (ethertype == 0x0800) & (lens >= 34)
        assert (ipv4 & (ihl < 5)).sum() >= 100 and (ipv4 & (ihl > 5)).sum() >= 100
        assert (fill & (lens >= 14) & (ethertype != 0x0800)).sum() >= 300
        assert (lens < 34).sum() >= 300 and (lens > 1514).sum() >= 1000
        assert (want != data).sum() > 100_000
        start = offs[N:].astype(np.int64) * 4
        assert len(start) == UDP_ZERO_ROWS and np.all(want[start + 40] == 0xFF) and np.all(want[start + 41] == 0xFF)
        assert {0, 1} == set((lens[N:] & 1).tolist()) and int(lens[N:].max()) > 1514


def _run(dev, data, offs, lens, ops, flag, hint, with_result=True):
    import torch

    from halo_amd import protocol

    d = torch.from_numpy(np.array(data)).to(dev)
    o = torch.from_numpy(np.array(offs, np.uint32).view(np.int32)).to(dev)
    ln = torch.from_numpy(np.array(lens, np.uint16).view(np.int16)).to(dev)
    op = torch.from_numpy(np.ascontiguousarray(ops).view(np.uint8)).to(dev)
    res = torch.full((len(lens) + 1,), 0xEE, dtype=torch.uint8, device=dev) if with_result else None
    protocol.tx_fixup_batch(d, o, ln, op, check_sum_enable=bool(flag), max_len_hint=hint, result=res)
    torch.cuda.synchronize()
    return d.cpu().numpy(), (res.cpu().numpy() if with_result else None)


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


def _compare(data, offs, lens, ops, flag, got, want, res, want_res, what):
    if res is not None:
        assert res[len(lens)] == 0xEE, f"{what}: the result byte behind the last was written"
        bad = np.flatnonzero(res[:len(lens)] != want_res)
        assert bad.size == 0, (f"{what}: {bad.size} result bytes differ; first frame {int(bad[0])}: got {int(res[bad[0]])} "
                               f"want {int(want_res[bad[0]])}, L {int(lens[bad[0]])}, steps {int(ops['steps'][bad[0]]):#04x}")
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    start = offs.astype(np.int64) * 4
    # (zero-length frames share an offset with their neighbour: the last frame at or before the byte)
    i = int(np.searchsorted(start, int(bad[0]), side="right")) - 1
    at, o, L, steps = int(bad[0]), int(start[i]), int(lens[i]), int(ops["steps"][i])
    frames = np.unique(np.searchsorted(start, bad, side="right")).size
    where = f"frame offset {at - o}" if at - o < L else f"{at - o - L} bytes behind it (gap)"
    raise AssertionError(f"{what}: {bad.size} buffer bytes differ in {frames} frames; first in frame {i} at {where}: got "
                         f"{got[at:at + 8].tobytes().hex()} want {want[at:at + 8].tobytes().hex()}; L {L}, steps {steps:#04x}, "
                         f"plan {T.plan_of(data[o:o + L].tobytes(), steps, flag)}, first bytes "
                         f"{data[o:o + min(L, 52)].tobytes().hex()}")


@pytest.mark.gpu
@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("g", [1, 4, 8, 16])
def test_tx_fuzz_every_width(dev, fuzz, g, flag):
    hint = T.HINTS[g]
    assert T.width_of(hint) == g
    data, offs, lens, ops, _, (want, want_res) = fuzz(flag)
    got, res = _run(dev, data, offs, lens, ops, flag, hint)
    _compare(data, offs, lens, ops, flag, got, want, res, want_res, f"GPU tx fuzz G{g} flag={flag}")


@pytest.mark.gpu
def test_tx_fuzz_without_result(dev, fuzz):
    data, offs, lens, ops, _, (want, _) = fuzz(1)
    got, none = _run(dev, data, offs, lens, ops, 1, T.HINTS[16], with_result=False)
    assert none is None
    _compare(data, offs, lens, ops, 1, got, want, None, None, "GPU tx fuzz G16, no result pointer, flag=1")
