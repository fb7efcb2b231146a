"""GPU: every frame-addressing entry with its frames past byte 4 GiB (where 32-bit byte arithmetic
wraps) and byte 8 GiB (dword offset 2^31, negative as the int32 the wrappers and torch carry), and
the far-output entries with regions that start and cross beyond both marks.

The placements are tests/far_cases.py's (bands N, X4, X8 and T of one 8 GiB + 64 MiB buffer; orders
banded, interleaved and first_far); tests/test_far_offsets_host.py proves them and the expectations
on the CPU. A frame's answer does not depend on where it lies, so every row

  1. takes its expected result from the existing oracle or model over the frames themselves,
  2. runs the entry over the far placement,
  3. compares bit for bit, with outputs prefilled with 0xA5,
  4. and, for entries that write frames in place, reads the bands back (guards and gaps included)
     and compares them whole.

ROWS is the table of rows: test -> the entries of include/halo_rx.h it takes far. The completeness
check of tests/test_far_offsets_host.py holds it against the header.

Device memory: the far buffer is 8.06 GiB and the far-output buffer 12 GiB (three regions of
2^32 - 4096 bytes); with both alive the file peaks at about 20 GiB. Neither is ever filled or
downloaded whole, and the module fixtures free them at teardown.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import far_cases as F

pytestmark = pytest.mark.gpu
FILL = 0xA5
N = F.N_FRAMES
REGION = (1 << 32) - 4096  # far outputs: port 1 starts below 4 GiB and crosses it, port 2 crosses 8 GiB
VARIANTS = (0, 1, 4, 8, 16, -1, -2)  # as tests/test_gpu_route.py lists them

ROWS = {
    "test_parse": ("halo_rx_parse_batch_device",),
    "test_parse_flow_and_route": ("halo_rx_parse_flow_batch_device", "halo_rx_parse_route_batch_device"),
    "test_parse_batches": ("halo_rx_parse_batches_device",),
    "test_parse_strided": ("halo_rx_parse_strided_device",),
    "test_synth_frames": ("halo_synth_frames_device",),
    "test_ring_scan_offsets_past_8g": ("halo_rx_ring_scan_device",),
    "test_tx_fixup": ("halo_tx_fixup_batch_device",),
    "test_deep_nat": ("halo_tx_icmp_deep_nat_batch_device",),
    "test_arp_encap": ("halo_arp_encap_device", "halo_arp_encap_tx_device", "halo_arp_encap_via_device"),
    "test_arp_gather": ("halo_arp_gather_device",),
    "test_switch_forward": ("halo_switch_forward",),
    "test_forward_return_flows": ("forward_return_flows", "halo_arp_encap_via_device", "halo_tx_fixup_batch_device"),
    "test_respond_and_build": ("halo_tx_respond_device", "halo_tx_build_batch_device"),
    "test_deliver": ("halo_rx_deliver_device",),
    "test_deliver_largest_region": ("halo_rx_deliver_device",),
    "test_egress_far_source": ("halo_tx_egress_masks_device", "halo_tx_egress_arp_device", "halo_tx_egress_switch_device"),
    "test_lo_gather_far_source": ("halo_lo_gather_device",),
    "test_egress_far_output": ("halo_tx_egress_masks_device",),
    "test_lo_gather_far_output": ("halo_lo_gather_device",),
    "test_tx_build_far_output": ("halo_tx_build_batch_device",),
}


# ---- fixtures and helpers ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def far(dev):
    """The far buffer: allocated once, never filled; every test writes its own bands."""
    import torch

    buf = torch.empty(F.FAR_BYTES, dtype=torch.uint8, device=dev)
    yield buf
    del buf
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def far_out(dev):
    """The far-output buffer: three regions of REGION bytes (also the strided parse's, the ring
    scan's and the far build's buffer, which need more than the far buffer holds)."""
    import torch

    holder = [torch.empty(3 * REGION, dtype=torch.uint8, device=dev)]
    yield holder[0]
    holder.clear()
    torch.cuda.empty_cache()


def _t(dev, a, dtype=None):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dtype) if dtype is not None else a).to(dev)


def _placed(dev, far, frames, order):
    """`frames` written into the far buffer in `order`: (placement, offsets int32, lens int16)."""
    pl = F.place(frames, order)
    d = F.describe(pl)
    assert d["beyond_8g"] >= 16 and d["last_end"] == F.FAR_BYTES, d
    assert order == "first_far" or (d["straddle_4g"] == 1 and d["at_8g"] >= 1 and d["beyond_4g"] > d["beyond_8g"] + 64), d
    F.to_device(pl, frames, far)
    return (pl, *F.device_offsets(pl, dev))


def _filled(dev, shape, dtype=None):
    import torch

    return torch.full(shape, FILL, dtype=dtype or torch.uint8, device=dev)


def _np(x, dtype=None):
    a = x.cpu().numpy()
    return a if dtype is None else a.view(dtype)


A5_32 = int(np.array(0xA5A5A5A5, np.uint32).view(np.int32))


# ---- parse -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpora(oracle_lib):
    """name -> (frames, {flags: the oracle's records}, l3):
    "udp64": 1,024 plain 64 B UDP frames (every window takes the lane kernel's fast path);
    "imix": IMIX lengths, mixed protocols, one frame in 8 mutated (the general path; every status);
    "l3": the IMIX frames' IPv4 packets, parsed with HALO_RX_L3_START."""
    from halo_amd import synth
    from tests.helpers import strip_ethernet

    on = oracle_lib.NetIf.make()
    out = {}
    for name, kw in (("udp64", dict(length=64, first_index=9000)),
                     ("imix", dict(size_mode=synth.SIZE_IMIX, proto_mode=synth.PROTO_MIX, mutate_shift=3, first_index=77))):
        lay = synth.layout(N, **kw)
        data = oracle_lib.synth_batch(synth.SEED, kw["first_index"], lay["lens"], lay["kinds"], on, offsets_dw=lay["offsets_dw"])
        want = {fl: oracle_lib.rx_batch(data, lay["lens"], on, fl, offsets_dw=lay["offsets_dw"])[0] for fl in (0, 1)}
        out[name] = (F.frames_of(data, lay["offsets_dw"], lay["lens"]), want, False)
        if name == "imix":
            pdata, poffs, plens = strip_ethernet(data, lay["offsets_dw"], lay["lens"])
            want3 = {fl: oracle_lib.rx_batch(pdata, plens, on, fl | 0x10, offsets_dw=poffs)[0] for fl in (0, 1)}
            out["l3"] = (F.frames_of(pdata, poffs, plens), want3, True)
    assert (out["udp64"][1][1]["status"] == 0).all() and len(set(out["imix"][1][1]["status"].tolist())) >= 5
    return out


# (variant, max_len_hint) and the kernel each reaches for a ragged batch (rx_parse.hip pick_variant,
# rx_lane.hip launch_lane); n = 1,024 is 16 windows:
#   (0, 64)    auto, frames <= 64 B: the lane kernel. Without a histogram its grid covers the batch, so
#              it is the one-window form (rx_lane_lean1_kernel); with one it is rx_lane_kernel on a
#              halved grid, every wave looping over two windows. On "udp64" every window takes the
#              fast path (lane_window_fast), on the others the general one (frame_finish).
#   (1, h)     the lane kernel forced, the same forms, also for frames longer than 64 B.
#   (0, 1514), (0, 0)  auto, longer or unknown lengths: the stream kernel in one-wave blocks; windows
#              inside a band are dense and take its streaming branch, the interleaved and first_far
#              windows fail the d64 < 2^31 guard (frames 4 and 8 GiB above and below the first
#              readable one) and are summed frame by frame.
#   (-2, 0)    the stream kernel forced (four-wave blocks), the same two branches.
#   (4 | 8 | 16, 0)  the group kernel at each width; (-1, 0) the size-class mix kernel.
# The lane kernel's span form was removed and has no launch to reach.
LAUNCHES = {"udp64": ((0, 64), (1, 64), (0, 1514), (0, 0), (-2, 0), (4, 0), (8, 0), (16, 0), (-1, 0)),
            "imix": ((1, 1514), (0, 1514), (0, 0), (-2, 0), (4, 0), (8, 0), (16, 0), (-1, 0)),
            "l3": ((1, 0), (0, 1514), (-2, 0), (4, 0), (8, 0), (16, 0), (-1, 0))}


def _check_records(got, want, compact, what):
    from halo_amd._lib import RESULT_DTYPE, compact_of
    from tests.helpers import assert_records_equal

    raw = _np(got)
    assert np.all(raw[-1] == FILL), (what, "the record behind the last was written")
    if compact:
        wb = np.ascontiguousarray(compact_of(want)).view(np.uint8).reshape(-1, 16)
        bad = np.flatnonzero(np.any(raw[:-1] != wb, axis=1))
        assert bad.size == 0, (what, "compact records differ", bad[:8].tolist())
    else:
        assert_records_equal(np.ascontiguousarray(raw[:-1]).reshape(-1).view(RESULT_DTYPE), want, None, what)


@pytest.mark.parametrize("corpus", ["udp64", "imix", "l3"])
@pytest.mark.parametrize("order", F.ORDERS)
def test_parse(dev, far, corpora, order, corpus):
    """halo_rx_parse_batch_device: every variant and hint of LAUNCHES, full and compact records,
    checksum flag off and on, with and without a status histogram."""
    import torch

    from halo_amd import _lib
    from halo_amd._lib import NetIf

    frames, wants, l3 = corpora[corpus]
    pl, o, ln = _placed(dev, far, frames, order)
    st = torch.cuda.current_stream().cuda_stream
    for variant, hint in LAUNCHES[corpus]:
        for compact in (False, True):
            for fl in (0, 1):
                for with_hist in (False, True):
                    flags = (fl | _lib.variant_flags(variant) | (_lib.HALO_RX_RECORD_COMPACT if compact else 0)
                             | (_lib.HALO_RX_L3_START if l3 else 0))
                    out = _filled(dev, (N + 1, 16 if compact else 32))
                    hist = torch.full((15,), 3, dtype=torch.int32, device=dev)
                    _lib.check("parse", _lib.lib.halo_rx_parse_batch_device(
                        _lib.ptr(far), _lib.ptr(o), _lib.ptr(ln), N, flags, NetIf.make(), hint, _lib.ptr(out),
                        _lib.ptr(hist) if with_hist else None, st))
                    torch.cuda.synchronize()
                    what = f"{corpus} {order} variant {variant} hint {hint} compact {compact} flags {fl} hist {with_hist}"
                    _check_records(out, wants[fl], compact, what)
                    h = _np(hist).astype(np.int64) - 3
                    want_h = np.bincount(wants[fl]["status"], minlength=14) if with_hist else np.zeros(14, np.int64)
                    assert np.array_equal(h[:14], want_h) and h[14] == 0, (what, h)
    F.assert_bands(pl, far, frames, f"parse {corpus} {order}")  # a parse writes no frame byte


@pytest.mark.parametrize("order", F.ORDERS)
def test_parse_flow_and_route(dev, far, corpora, oracle_lib, order):
    """The fused parses: the plain parse's records, the oracle's flow hashes and buckets of those
    records, and the oracle's FindRoute of each record's destination."""
    import torch

    from halo_amd import _lib
    from halo_amd._lib import NetIf
    from tests.test_gpu_route import _replay_both

    ops = [("add", [0, 0, 1, 0]), ("add", [0xC0A86400, 0xFFFFFF00, 0, 1]), ("add", [0xC0A86464, 0xFFFFFFFF, 0, 2]),
           ("add", [0x0A000000, 0xFF000000, 5, 3]), ("add", [0x0A000000, 0xFF000000, 6, 3])]
    g, model = _replay_both(ops, oracle_lib)
    g.sync()
    st = torch.cuda.current_stream().cuda_stream
    try:
        for corpus in ("udp64", "imix"):
            frames, wants, _ = corpora[corpus]
            pl, o, ln = _placed(dev, far, frames, order)
            want = wants[1]
            want_ids = model.find_batch(want["dst_ip"])
            for variant, hint in LAUNCHES[corpus]:
                for compact in (False, True):
                    flags = 1 | _lib.variant_flags(variant) | (_lib.HALO_RX_RECORD_COMPACT if compact else 0)
                    what = f"{corpus} {order} variant {variant} hint {hint} compact {compact}"
                    for kind, nat, buckets in ((1, 0, 1 << 20), (0, 1, 0)):
                        out = _filled(dev, (N + 1, 16 if compact else 32))
                        h = torch.full((N + 1,), A5_32, dtype=torch.int64, device=dev)
                        b = torch.full((N + 1,), A5_32, dtype=torch.int32, device=dev)
                        _lib.check("flow", _lib.lib.halo_rx_parse_flow_batch_device(
                            _lib.ptr(far), _lib.ptr(o), _lib.ptr(ln), N, flags, NetIf.make(), hint, _lib.ptr(out), None, kind, nat,
                            _lib.ptr(h), buckets, _lib.ptr(b) if buckets else None, st))
                        torch.cuda.synchronize()
                        _check_records(out, want, compact, "flow " + what)
                        wh, wb = oracle_lib.flow_hash_batch(want, kind, nat, buckets)
                        assert np.array_equal(_np(h, np.uint64)[:N], wh) and int(h[N].item()) == A5_32, what
                        assert (np.array_equal(_np(b, np.uint32)[:N], wb) if buckets else True) and int(b[N].item()) == A5_32, what
                    out = _filled(dev, (N + 1, 16 if compact else 32))
                    rid = torch.full((N + 1,), A5_32, dtype=torch.int32, device=dev)
                    _lib.check("route", _lib.lib.halo_rx_parse_route_batch_device(
                        _lib.ptr(far), _lib.ptr(o), _lib.ptr(ln), N, flags, NetIf.make(), hint, _lib.ptr(out), None, g._t,
                        _lib.ptr(rid), st))
                    torch.cuda.synchronize()
                    _check_records(out, want, compact, "route " + what)
                    assert np.array_equal(_np(rid, np.uint32)[:N], want_ids) and int(rid[N].item()) == A5_32, what
    finally:
        g.close()


@pytest.mark.parametrize("corpus,hint", [("udp64", 64), ("imix", 1514)])
def test_parse_batches(dev, far, corpora, corpus, hint):
    """halo_rx_parse_batches_device with one batch in band N and one in band T (and a third made of
    the two straddling bands): "udp64" with hint 64 is one launch of rx_lane_multi_kernel, "imix" a
    launch per batch. With and without a histogram."""
    import torch

    from halo_amd import protocol
    from halo_amd._lib import NetIf

    frames, wants, _ = corpora[corpus]
    pl, o, ln = _placed(dev, far, frames, "banded")
    groups = [pl[2][0].members, pl[2][3].members, np.concatenate([pl[2][1].members, pl[2][2].members])]
    assert int(pl[0][groups[1]].min()) >= 1 << 31 and int(pl[0][groups[0]].max()) < 1 << 20
    for with_hist in (False, True):
        outs = [_filled(dev, (len(m) + 1, 32)) for m in groups]
        hist = torch.zeros(14, dtype=torch.int32, device=dev)
        idx = [torch.from_numpy(m).to(dev) for m in groups]
        protocol.parse_frames_batches([(far, o[i].contiguous(), ln[i].contiguous(), out) for i, out in zip(idx, outs)],
                                      netif=NetIf.make(), max_len_hint=hint, hist=hist if with_hist else None)
        torch.cuda.synchronize()
        for m, out in zip(groups, outs):
            _check_records(out, wants[1][m], False, f"batches {corpus} hist {with_hist}")
        want_h = np.bincount(wants[1]["status"], minlength=14) if with_hist else np.zeros(14, np.int64)
        assert np.array_equal(_np(hist), want_h)


def test_parse_strided(dev, far_out, corpora):
    """halo_rx_parse_strided_device: 1,100 frames with their own lengths at a stride of 8 MiB + 64,
    so frame 512 starts past 4 GiB and the frames from 1,024 on past 8 GiB."""
    import torch

    from halo_amd import protocol
    from halo_amd._lib import NetIf

    n, stride, width = 1100, (8 << 20) + 64, 1516
    frames, wants, _ = corpora["imix"]
    pick = np.arange(n) % N
    rows = np.full((n, width), F.GAP, np.uint8)
    for k, i in enumerate(pick):
        rows[k, :len(frames[i])] = np.frombuffer(frames[i], np.uint8)
    assert (n - 1) * stride + width <= far_out.numel() and 1024 * stride > F.MARK8
    slots = far_out.as_strided((n, width), (stride, 1))
    slots.copy_(_t(dev, rows))
    lens = _t(dev, np.array([len(frames[i]) for i in pick], np.uint16), np.int16)
    for with_hist in (False, True):
        out = _filled(dev, (n + 1, 32))
        hist = torch.zeros(14, dtype=torch.int32, device=dev)
        protocol.parse_frames_strided(far_out, stride, n, netif=NetIf.make(), lens=lens, out=out, hist=hist if with_hist else None)
        torch.cuda.synchronize()
        _check_records(out, wants[1][pick], False, f"strided hist {with_hist}")
        if with_hist:
            assert np.array_equal(_np(hist), np.bincount(wants[1][pick]["status"], minlength=14))
    assert np.array_equal(_np(slots.contiguous()), rows)


@pytest.mark.parametrize("order", F.ORDERS)
def test_synth_frames(dev, far, oracle_lib, order):
    """halo_synth_frames_device writes frame i at 4 * offsets_dw[i]: the oracle's frames, and no byte
    of a guard or gap."""
    import torch

    from halo_amd import _lib, synth
    from halo_amd._lib import NetIf

    lay = synth.layout(N, size_mode=synth.SIZE_IMIX, proto_mode=synth.PROTO_MIX, mutate_shift=4, first_index=31)
    data = oracle_lib.synth_batch(synth.SEED, 31, lay["lens"], lay["kinds"], oracle_lib.NetIf.make(), offsets_dw=lay["offsets_dw"])
    frames = F.frames_of(data, lay["offsets_dw"], lay["lens"])
    blank = [bytes([0x77]) * len(f) for f in frames]
    pl, o, ln = _placed(dev, far, blank, order)
    kinds = _t(dev, lay["kinds"])
    _lib.check("synth", _lib.lib.halo_synth_frames_device(synth.SEED, 31, N, _lib.ptr(ln), _lib.ptr(o), 0, _lib.ptr(kinds), NetIf.make(),
                                                        _lib.ptr(far), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    F.assert_bands(pl, far, frames, f"synth {order}")


def test_ring_scan_offsets_past_8g(dev, far, far_out):
    """halo_rx_ring_scan_device is the one entry that writes dword offsets: over a span of 9,020-byte
    records that reaches past 8 GiB, record k's frame is at dword (9020 k + 4) / 4, also where that
    is 2^31 and more. The span is made on the device by one broadcast copy of a 9,020-byte record."""
    import torch

    from halo_amd import _lib

    rec, length = 9020, 9014
    count = (F.MARK8 + (32 << 20)) // rec
    used = count * rec
    one = np.zeros(rec, np.uint8)
    one[:4] = np.frombuffer(np.uint32(length).tobytes(), np.uint8)
    one[4:4 + length] = 0x11
    far_out[:used].view(count, rec).copy_(_t(dev, one).expand(count, rec))
    wsb = int(_lib.lib.halo_rx_ring_scan_workspace(used, 9014))
    assert wsb > 0
    assert wsb <= far.numel()
    ws = far  # 4 GiB of scratch: the far buffer holds nothing a later test relies on
    offs = torch.full((count + 1,), A5_32, dtype=torch.int32, device=dev)
    lens = torch.full((count + 1,), -23131, dtype=torch.int16, device=dev)
    info = torch.zeros(8, dtype=torch.int64, device=dev)
    _lib.check("scan", _lib.lib.halo_rx_ring_scan_device(_lib.ptr(far_out), used, 1 << 34, 9014, 0, _lib.ptr(offs), _lib.ptr(lens),
                                                       _lib.ptr(info), _lib.ptr(ws), wsb, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = _np(info).view(np.uint8)[:_lib.RING_SCAN_DTYPE.itemsize].view(_lib.RING_SCAN_DTYPE)[0]
    assert int(got["n_frames"]) == count and int(got["end_bytes"]) == used and int(got["stop"]) == _lib.RING_STOP["EMPTY"]
    want = (np.arange(count, dtype=np.uint64) * rec + 4) // 4
    assert int(want[-1]) >= 1 << 31
    assert np.array_equal(_np(offs, np.uint32)[:count].astype(np.uint64), want) and int(offs[count].item()) == A5_32
    assert (_np(lens, np.uint16)[:count] == length).all() and int(lens[count].item()) == -23131


# ---- in place ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tx_corpus(oracle_lib):
    """1,024 cases spread evenly over tests/tx_cases.py's table (IHL 5..15, every relation of the
    total length to the frame, every step set), and the C oracle's frames and result bytes."""
    from tests import tx_cases as T

    c = T.ordered("mixed")
    pick = np.linspace(0, len(c.lens) - 1, N).astype(np.int64)
    sub = T._subset(c, pick)
    data, offs, lens = T.layout(sub, np.random.default_rng(0xFA7))
    ops = np.array(sub.ops)
    want, wres = oracle_lib.tx_batch(data, offs, lens, ops, flags=1)
    assert len(set(wres.tolist())) >= 4 and int((want != data).sum()) > 4 * N
    return F.frames_of(data, offs, lens), ops, F.frames_of(want, offs, lens), wres


@pytest.mark.parametrize("g", [1, 4, 8, 16])
@pytest.mark.parametrize("order", F.ORDERS)
def test_tx_fixup(dev, far, tx_corpus, order, g):
    """halo_tx_fixup_batch_device at the hint of each lanes-per-frame group tests/test_gpu_scale.py
    names (tests/tx_cases.HINTS)."""
    import torch

    from halo_amd import protocol
    from tests import tx_cases as T

    hint = T.HINTS[g]
    assert T.width_of(hint) == g
    frames, ops, after, wres = tx_corpus
    pl, o, ln = _placed(dev, far, frames, order)
    res = _filled(dev, (N + 1,))
    protocol.tx_fixup_batch(far, o, ln, _t(dev, ops.view(np.uint8)), max_len_hint=hint, result=res)
    torch.cuda.synchronize()
    got = _np(res)
    assert np.array_equal(got[:N], wres) and got[N] == FILL, np.flatnonzero(got[:N] != wres)[:8]
    F.assert_bands(pl, far, after, f"tx_fixup {order} G{g}")


@pytest.fixture(scope="module")
def deepnat_corpus(oracle_lib):
    """The first 1,024 rows of tests/deepnat_cases.py's hostile-quote corpus that fit a 1,514-byte
    frame, and the C oracle's quote records, rewritten frames and applied flags."""
    from tests import deepnat_cases as D

    c = D.corpus()
    pick = np.flatnonzero(c.lens <= 1514)[:N]
    assert len(pick) == N
    frames = [c.frames[i] for i in pick]
    nat = np.array(c.nat[pick])
    data, offs, lens = D.pack(frames, np.random.default_rng(5))
    want, quote, applied = D.expected(oracle_lib, data, offs, lens, nat, 1)
    assert int(applied.sum()) > N // 4
    return frames, nat, F.frames_of(want, offs, lens), quote, applied


@pytest.mark.parametrize("order", F.ORDERS)
def test_deep_nat(dev, far, deepnat_corpus, order):
    """halo_tx_icmp_deep_nat_batch_device, both passes: the checks alone (quote records, frames
    untouched), then the rewrite (frames, applied flags)."""
    import torch

    from halo_amd import protocol

    frames, nat, after, quote, applied = deepnat_corpus
    pl, o, ln = _placed(dev, far, frames, order)
    q, a = _filled(dev, (N + 1, 32)), _filled(dev, (N + 1,))
    protocol.icmp_ttl_deep_nat_batch(far, o, ln, nat=None, quote=q, applied=a)
    torch.cuda.synchronize()
    _check_records(q, quote, False, f"deep NAT quote {order}")
    assert not _np(a)[:N].any() and _np(a)[N] == FILL
    F.assert_bands(pl, far, frames, f"deep NAT checks {order}")
    q, a = _filled(dev, (N + 1, 32)), _filled(dev, (N + 1,))
    protocol.icmp_ttl_deep_nat_batch(far, o, ln, nat=_t(dev, nat.view(np.uint8)), quote=q, applied=a)
    torch.cuda.synchronize()
    _check_records(q, quote, False, f"deep NAT quote with results {order}")
    assert np.array_equal(_np(a)[:N], applied) and _np(a)[N] == FILL
    F.assert_bands(pl, far, after, f"deep NAT rewrite {order}")


@pytest.fixture(scope="module")
def arp_world(dev):
    """tests/arp_cases.py's forced 16-slot table, synced with the route table that has direct and
    next-hop routes, an emptied list and an ECMP list."""
    from tests import arp_cases as K

    pair, keys = K.forced_table(lambda **kw: K.Pair(**kw))
    rt = K.world_routes(keys)
    rt.sync()
    pair.t.sync(rt)
    yield pair, keys, rt
    pair.close()
    rt.close()


@pytest.mark.parametrize("entry", ["encap", "encap_tx", "encap_via"])
@pytest.mark.parametrize("order", F.ORDERS)
def test_arp_encap(dev, far, arp_world, order, entry):
    """The three L2 rewrites against their models: results, counters, and the frames afterwards
    (bytes 0-11 of the HIT frames and nothing else)."""
    import torch

    from halo_amd._lib import ARP_RESULT_DTYPE, PMFLOW_VIA_DTYPE
    from tests import arp_cases as K
    from tests import arp_model as AM
    from tests import pmflow_model as PM
    from tests import respond_model as RM

    pair, keys, rt = arp_world
    rng = np.random.default_rng(1500)
    if entry == "encap_tx":
        from tests.test_gpu_respond import _tx_batch

        frames, dsts, select, forced, names = _tx_batch(rng, keys, N)
    else:
        frames, dsts, select, forced, names = K.mixed_batch(rng, keys, N)
    rids = _np(rt.FindRoute(_t(dev, dsts, np.int32)), np.uint32).copy()
    for i, frc in enumerate(forced):
        if frc is not None:
            rids[i] = frc
    via = np.zeros(N, PMFLOW_VIA_DTYPE)
    if entry == "encap_via":
        from tests.test_gpu_pmflow import _via_for

        for i in range(N):
            via[i] = _via_for(rng, keys, i, names[i], int(dsts[i]))
    nif = 0
    want_res, after = np.zeros(N, ARP_RESULT_DTYPE), []
    for i, f in enumerate(frames):
        route, sel = K.route_of(rt, int(rids[i])), bool(select[i])
        if entry == "encap":
            v, out, tx, target, g = pair.m.encap(f, route, nif, sel)
        elif entry == "encap_tx":
            v, out, tx, target, g = RM.tx_ipv4(pair.m, f, route, nif, sel)
        else:
            v, out, tx, target, g = PM.encap_via(pair.m, f, route, tuple(int(x) for x in via[i]), nif, sel)
        want_res[i] = (v, out, tx, target)
        after.append(bytes(g))
    assert {AM.NONE, AM.MISS, AM.HIT} <= set(want_res["verdict"].tolist()) and sum(a != f for a, f in zip(after, frames)) > N // 8
    pl, o, ln = _placed(dev, far, frames, order)
    counts = torch.full((8,), 3, dtype=torch.int32, device=dev)
    miss = torch.full((2,), 5, dtype=torch.int32, device=dev)
    args = (far, o, ln, _t(dev, rids, np.int32), nif)
    kw = dict(select=_t(dev, select), counts=counts, miss_count=miss)
    if entry == "encap":
        res, _, _ = pair.t.encap(*args, **kw)
    elif entry == "encap_tx":
        res, _, _ = pair.t.encap_tx(*args, **kw)
    else:
        res, _, _ = pair.t.encap_via(*args, _t(dev, via.view(np.uint8).reshape(-1, 8)), **kw)
    torch.cuda.synchronize()
    got = _np(res).reshape(-1).view(ARP_RESULT_DTYPE)
    bad = np.flatnonzero(got != want_res)
    assert bad.size == 0, [(int(i), names[i], got[i], want_res[i]) for i in bad[:5]]
    assert list(_np(counts) - 3) == [int((want_res["verdict"] == v).sum()) for v in range(7)] + [0]
    assert list(_np(miss) - 5) == [int((want_res["verdict"] == AM.MISS).sum()), 0]
    F.assert_bands(pl, far, after, f"{entry} {order}")


# ---- read only ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", F.ORDERS)
def test_arp_gather(dev, far, order):
    """halo_arp_gather_device: the ARP messages of the frames for this NetIf, bytes 6-11 and 14-41 of
    each, in frame order."""
    import torch

    from halo_amd import protocol
    from halo_amd._lib import ARP_MSG_DTYPE
    from halo_amd.arp import ArpTable
    from tests import arp_cases as K
    from tests import arp_model as AM
    from tests.test_gpu_arp import _arp_frame

    rng = np.random.default_rng(21)
    nif, own = 0, K.NETIFS[0].mac
    frames = []
    for i in range(N):
        src = K.mac(int(rng.integers(0, 6)))
        if i % 64 in (0, 63) or i % 7 == 3:
            frames.append(_arp_frame(rng, own if i % 2 else AM.BCAST, src, nif, length=[42, 60, 77][i % 3]))
        elif i % 50 == 10:
            frames.append(_arp_frame(rng, K.mac(4242), src, nif))
        elif i % 50 == 11:
            frames.append(_arp_frame(rng, own, src, nif, length=41))
        else:
            frames.append(own + K.ipv4_frame(rng, int(rng.choice([60, 61, 64, 90])), 0x0A000005)[6:])
    want = [i for i, f in enumerate(frames) if AM.is_arp_for(f, own)]
    assert len(want) > N // 8
    data, offs, lens = K.pack(rng, frames)
    recs = protocol.parse_frames_batch(_t(dev, data), _t(dev, offs, np.int32), _t(dev, lens, np.int16), netif=K.lib_netifs()[nif])
    pl, o, ln = _placed(dev, far, frames, order)
    msgs, count = ArpTable.gather(far, o, ln, recs, nif)
    torch.cuda.synchronize()
    assert int(_np(count)[0]) == len(want)
    raw = _np(msgs)
    got = raw.reshape(-1).view(ARP_MSG_DTYPE)
    assert list(got["index"][:len(want)]) == want
    for j, i in enumerate(want):
        assert bytes(got[j]["eth_src"]) == frames[i][6:12] and bytes(got[j]["arp"]) == frames[i][14:42], (j, i)
        assert int(got[j]["netif"]) == nif and int(got[j]["pad"]) == 0
    assert not raw.reshape(-1)[len(want) * ARP_MSG_DTYPE.itemsize:].any()
    F.assert_bands(pl, far, frames, f"gather {order}")


def test_switch_forward(dev, far):
    """halo_switch_forward in device mode against the sequential model, one call per order and a
    second round that finds the first one's MACs learned."""
    import torch

    from halo_amd._lib import SW_RESULT_DTYPE
    from halo_amd.switch import Switch
    from tests import switch_cases as K
    from tests import switch_model as M

    vlans = [1, 1, 1, 2, 2, 2, 3, 3]
    sw, model = Switch(vlans, 128, max_batch=N, device=0), M.SwitchModel(vlans, 128)
    rng = np.random.default_rng(21)
    seen = np.zeros(6, np.uint64)
    counts = torch.zeros(6, dtype=torch.int32, device=dev)
    try:
        for call, order in enumerate(F.ORDERS * 2):
            frames, _ = K.numpy_random_frames(rng, 300, N)
            pl, o, ln = _placed(dev, far, frames, order)
            res = _filled(dev, (N + 1, 4))
            sw.forward(call % len(vlans), far, o, ln, 100 + call, results=res, counts=counts)
            torch.cuda.synchronize()
            v, p, t, c = model.forward(call % len(vlans), frames, 100 + call)
            seen += c
            got = _np(res).view(SW_RESULT_DTYPE)[:, 0]
            assert np.array_equal(got["verdict"][:N], v) and np.array_equal(got["out_port"][:N], p), (call, order)
            assert np.array_equal(got["tx_len"][:N], t) and np.all(_np(res)[N] == FILL), (call, order)
            assert np.array_equal(_np(counts).astype(np.uint64), seen)
            assert M.listed(sw.ListSwitchMacAddr()) == model.entries()
            F.assert_bands(pl, far, frames, f"switch {order}")
        assert seen[M.UNICAST] > N and (seen > 0).all(), seen
    finally:
        sw.close()


@pytest.mark.parametrize("order", F.ORDERS)
def test_forward_return_flows(dev, far, order):
    """The pmflow path (parse -> route -> pmflow lookup -> NAT lookup -> fixup -> encap_via, then
    egress) over a far batch of a LAN server's replies: the egress streams are the model's."""
    import torch

    from halo_amd import egress_arp, forward_return_flows
    from halo_amd._lib import TX_RECALC, TX_TTL
    from tests import pmflow_cases as C
    from tests.test_gpu_pmflow import _Router, _clients, _inbound, _replies, _want_items, _want_streams

    r = _Router(dev, pm_capacity=2 * N)
    try:
        clients = _clients(N)
        _, _, _, items = _inbound(r, clients, 500, dev)
        want_items = _want_items(r, clients)
        assert items.tobytes() == C.item_array(want_items).tobytes()
        dropped, added = r.pm.record(C.WAN2, items, 500)
        assert added == N and not dropped.any() and r.pm_m.record(C.WAN2, want_items, 500) == ([0] * N, N)
        r.pm.sync(r.rt)
        replies = _replies(r, clients)
        want = _want_streams(r, replies, 506)
        assert want[C.WAN1] == b"" and want[C.LAN] == b"" and len(want[C.WAN2]) >= 64 * N
        pl, o, ln = _placed(dev, far, replies, order)
        out = forward_return_flows(far, o, ln, netif=r.netifs[C.LAN], in_netif=C.LAN, now=506, pmflow=r.pm, routes=r.rt,
                                   arp=r.arp, nat=r.nat[C.WAN1], steps=TX_TTL | TX_RECALC)
        eg = egress_arp(far, o, ln, out.results, 3, 1 << 20, index_cap=N)
        torch.cuda.synchronize()
        streams = {q: eg.stream(q).tobytes() for q in range(3)}
        assert list(_np(out.pm_counts)) == [0, 0, 0, N]
        assert streams == want and eg.ports["frames"].tolist() == [0, 0, N]
        # in place: each band holds what the stream holds, in the band's frame order
        sent, at = [], 0
        for f in replies:  # record i is frame i: u32 tx_len, the frame, padding to tx_len and to a dword
            sent.append(want[C.WAN2][at + 4:at + 4 + len(f)])
            at += (4 + int.from_bytes(want[C.WAN2][at:at + 4], "little") + 3) & ~3
        assert at == len(want[C.WAN2]) and sum(a != f for a, f in zip(sent, replies)) == N
        F.assert_bands(pl, far, sent, f"return flows {order}")
    finally:
        r.close()


@pytest.mark.parametrize("order", F.ORDERS)
def test_respond_and_build(dev, far, order):
    """halo_tx_respond_device reads no frame byte: its descriptors' payload_off is 4 * offsets_dw[i]
    plus the payload's place in the frame, in Python integers. Those descriptors through
    halo_tx_build_batch_device with the far buffer as payload build the respond model's frames."""
    import torch

    from halo_amd import protocol
    from halo_amd._lib import BUILD_DESC_DTYPE
    from tests import respond_cases as C
    from tests import respond_model as RM
    from tests.test_gpu_respond import _device

    frames, nat, steps, result = C.columns(C.batch(905, N, "mixed"))
    data, offs, lens = C.pack(3, frames)
    pl, o, ln = _placed(dev, far, frames, order)
    for nat_enable in (False, True):
        recs = protocol.parse_frames_batch(_t(dev, data), _t(dev, offs, np.int32), _t(dev, lens, np.int16),
                                           netif=C.lib_netif(nat_enable))
        want = RM.respond(frames, pl[0], C.model_netif(nat_enable), nat=nat, fix=(steps, result), tcp_ports=C.SERVED)
        got = _device(dev, recs, _np(o, np.uint32), _np(ln, np.uint16), nat_enable, nat=nat, steps=steps, result=result,
                      ports=C.SERVED)  # the offsets the placement helper uploads, like every other row
        C.check_outputs(got, want, f"respond {order} nat_enable={nat_enable}")
        desc = got["desc"].reshape(-1).view(BUILD_DESC_DTYPE)[:want.count]
        assert want.count > N // 8
        for k, (i, rep) in enumerate(want.replies):
            at = 4 * int(pl[0][i])
            assert at <= int(desc["payload_off"][k]) == rep["payload_off"] <= at + len(frames[i]), (k, i)
        if order != "first_far":
            assert int((desc["payload_off"] >= F.MARK8).sum()) > 16 and int((desc["payload_off"] >= F.MARK4).sum()) > 64
        # the replies: the model builds them from the compact batch, the device from the far buffer
        near = RM.respond(frames, offs, C.model_netif(nat_enable), nat=nat, fix=(steps, result), tcp_ports=C.SERVED)
        built, ip_end = RM.build_frames(near.replies, data, C.MAC, 0xFFE0)
        b = protocol.TxBuilder(want.count, device=dev, ip_id=0xFFE0)
        slots = _filled(dev, (want.count + 1, 128))
        out_lens = torch.full((want.count + 1,), -23131, dtype=torch.int16, device=dev)
        out_res = _filled(dev, (want.count + 1,))
        b.build(_t(dev, desc.view(np.uint8)), far, netif=C.lib_netif(nat_enable), out_stride=128, frames=slots, lens=out_lens,
                result=out_res)
        torch.cuda.synchronize()
        g_slots, g_lens, g_res = _np(slots), _np(out_lens, np.uint16), _np(out_res)
        assert b.iph_id == ip_end and g_lens[want.count] == 0xA5A5 and g_res[want.count] == FILL and np.all(g_slots[want.count] == FILL)
        for k, (res, frame) in enumerate(built):
            assert res == 0 and int(g_res[k]) == 0 and int(g_lens[k]) == len(frame), (k, res, g_res[k], g_lens[k])
            assert g_slots[k, :len(frame)].tobytes() == frame, k
    F.assert_bands(pl, far, frames, f"respond {order}")


@pytest.mark.parametrize("order", F.ORDERS)
def test_deliver(dev, far, order):
    """halo_rx_deliver_device: the stream, summary and index of tests/deliver_model.py."""
    from tests import deliver_cases as C
    from tests import deliver_model as DM
    from tests.test_gpu_deliver import _device

    frames = C.batch(61, N, "all")[:N // 2] + C.batch(62, N // 2, "edges")
    nif = C.model_netif()
    want = DM.want_of(frames, nif, udp_ports=C.UDP_SERVED, tcp_ports=C.TCP_SERVED, dhcp=True)
    assert len(want.recs) > N // 2
    recs = _t(dev, C.records(frames, nif).view(np.uint8).reshape(-1, 32))
    pl, o, ln = _placed(dev, far, frames, order)
    got = _device(dev, far, o, ln, recs, False, (want.total_bytes + 15) & ~15, len(want.recs) + 2)
    C.check_outputs(got, want, order)
    F.assert_bands(pl, far, frames, f"deliver {order}")


def test_deliver_largest_region(dev, far, far_out):
    """The largest legal region, 2^32 - 16 bytes, with a handful of records from far frames; a region
    of 2^32 is HALO_E_INVAL."""
    import torch

    from halo_amd import _lib
    from halo_amd.deliver import deliver, port_map
    from tests import deliver_cases as C
    from tests import deliver_model as DM

    frames = C.batch(63, N, "sparse")
    nif = C.model_netif()
    want = DM.want_of(frames, nif, udp_ports=C.UDP_SERVED, tcp_ports=C.TCP_SERVED, dhcp=True)
    stream, summary, index = want.expect((1 << 32) - 16, N)
    assert 8 <= len(want.recs) < N // 8
    recs = _t(dev, C.records(frames, nif).view(np.uint8).reshape(-1, 32))
    pl, o, ln = _placed(dev, far, frames, "interleaved")
    far_out[:len(stream) + 4096] = FILL
    um, tm = _t(dev, port_map(C.UDP_SERVED), np.int32), _t(dev, port_map(C.TCP_SERVED), np.int32)
    r = deliver(far, o, ln, recs, netif=C.lib_netif(), region_bytes=(1 << 32) - 16, udp_ports=um, tcp_ports=tm, index_cap=N, dhcp=True,
                out=far_out)
    torch.cuda.synchronize()
    for k, v in summary.items():
        assert np.array_equal(r.summary[k], v), (k, r.summary[k], v)
    got = _np(far_out[:len(stream) + 4096])
    assert got[:len(stream)].tobytes() == stream and np.all(got[len(stream):] == FILL)
    assert [(int(e["frame"]), int(e["offset"])) for e in r.index] == index
    cfg = _lib.DeliverConfig()
    cfg.flags, cfg.index_cap, cfg.region_bytes = _lib.HALO_DELIVER_DHCP, 0, 1 << 32
    ws = torch.empty(max(int(_lib.lib.halo_rx_deliver_workspace(N)), 8), dtype=torch.uint8, device=dev)
    rc = _lib.lib.halo_rx_deliver_device(ctypes.byref(cfg), _lib.ptr(far), _lib.ptr(o), _lib.ptr(ln), _lib.ptr(recs), N, C.lib_netif(),
                                         _lib.ptr(um), _lib.ptr(tm), _lib.ptr(far_out), _lib.ptr(r.summary_raw), None, _lib.ptr(ws),
                                         ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.HALO_E_INVAL


def _check_egress(r, want, out_np, region, what):
    assert np.array_equal(r.ports, want.ports), (what, r.ports, want.ports)
    assert np.array_equal(out_np, want.out(FILL, size=len(out_np))), what
    assert all(np.array_equal(r.index(p), want.index[p]) for p in range(want.n_ports)), what


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["masks", "arp", "switch"])
@pytest.mark.parametrize("order", F.ORDERS)
def test_egress_far_source(dev, far, order, kind):
    """The three egress entries reading far frames into small regions: streams, summaries, index
    lists and the skip count of tests/egress_model.py."""
    import torch

    from halo_amd import egress as E
    from tests import egress_cases as C
    from tests import egress_model as EM
    from tests.test_egress_host import _selectors

    frames, _, _, _, masks = C.mixed(31, N, 3)
    sel, model_masks, flood = _selectors(kind, masks, 3, np.random.default_rng(5))
    free = EM.egress(frames, model_masks, 3, 1 << 40)
    region = C.region_for(int(free.ports["bytes"].max()))
    cap = int(free.ports["frames"].max()) + 3
    want = EM.egress(frames, model_masks, 3, region, cap)
    assert want.skipped > 0 and int(want.ports["frames_written"].min()) > 32
    pl, o, ln = _placed(dev, far, frames, order)
    out = _filled(dev, (3 * region + 32,))
    skipped = torch.full((1,), 7, dtype=torch.int32, device=dev)
    d_sel = _t(dev, sel, np.int64) if kind == 0 else _t(dev, sel.view(np.uint8).reshape(N, -1))
    args = (far, o, ln, d_sel) + ((flood,) if kind == 2 else ())
    fn = (E.egress_masks, E.egress_arp, E.egress_switch)[kind]
    r = fn(*args, 3, region, cap, out=out, skipped=skipped)
    torch.cuda.synchronize()
    _check_egress(r, want, _np(out), region, f"egress kind {kind} {order}")
    assert r.n_skipped - 7 == want.skipped
    F.assert_bands(pl, far, frames, f"egress {order}")


def _check_lo(r, want, n_netifs, what):
    assert np.array_equal(r.ports, want.ports), (what, r.ports, want.ports)
    for p in range(n_netifs):
        assert np.array_equal(r.pkt_off_dw(p), np.asarray(want.pkt_off[p], np.uint32)), (what, p)
        assert np.array_equal(r.pkt_len(p), np.asarray(want.pkt_len[p], np.uint16)), (what, p)
        assert np.array_equal(r.index(p), np.asarray(want.index[p], np.uint32)), (what, p)


@pytest.mark.parametrize("tx", [False, True], ids=["forward", "tx"])
@pytest.mark.parametrize("order", F.ORDERS)
def test_lo_gather_far_source(dev, far, order, tx):
    import torch

    from halo_amd import loopback as L
    from tests import lo_cases as C
    from tests import lo_model as LM

    frames, _, _, _, results = C.mixed(77 + tx, N, 4, tx)
    nifs = LM.netifs_of_results(results, 4)
    free = LM.gather(frames, nifs, 4, 1 << 34, 0, tx)
    region = C.region_for(int(free.ports["bytes"].max()))
    cap = int(free.ports["frames"].max()) + 3
    want = LM.gather(frames, nifs, 4, region, cap, tx)
    assert int(want.ports["frames_written"].sum()) > N // 8 and want.skipped > 0
    pl, o, ln = _placed(dev, far, frames, order)
    out = _filled(dev, (4 * region + 64,))
    skipped = torch.full((1,), 7, dtype=torch.int32, device=dev)
    r = L.gather(far, o, ln, _t(dev, results.view(np.uint8).reshape(N, 8)), 4, region, cap, tx=tx, out=out, skipped=skipped)
    torch.cuda.synchronize()
    _check_lo(r, want, 4, f"lo {order} tx={tx}")
    assert np.array_equal(_np(out), want.out(FILL, size=out.numel())) and r.n_skipped - 7 == want.skipped
    F.assert_bands(pl, far, frames, f"lo {order}")


# ---- far outputs, the source small and near ----------------------------------------------------------
MARGIN = 1 << 16  # bytes of 0xA5 prefill checked behind every port's stream


def _regions_prefill(far_out, lens_by_port):
    for p, n in enumerate(lens_by_port):
        far_out[p * REGION:p * REGION + n + MARGIN] = FILL
    for p in (1, 2):  # and the last bytes of the region before: a stream that starts early shows
        far_out[p * REGION - MARGIN:p * REGION] = FILL


def _regions_check(far_out, streams, what):
    for p, s in enumerate(streams):
        got = _np(far_out[p * REGION:p * REGION + len(s) + MARGIN])
        assert got[:len(s)].tobytes() == bytes(s), (what, p, "the stream differs")
        assert np.all(got[len(s):] == FILL), (what, p, "bytes behind the stream written")
    for p in (1, 2):
        assert np.all(_np(far_out[p * REGION - MARGIN:p * REGION]) == FILL), (what, p, "bytes before the region written")


def test_egress_far_output(dev, far_out):
    """Egress with n_ports = 3 and region_bytes = 2^32 - 4096: port 1's stream starts 4,096 bytes
    below 4 GiB and crosses it, port 2's starts 8,192 below 8 GiB and crosses it; every port gets
    several hundred records, many tiles' worth past its mark."""
    import torch

    from halo_amd import egress as E
    from tests import egress_cases as C
    from tests import egress_model as EM

    n = 2 * N
    frames, data, offs, lens, masks = C.mixed(32, n, 3)
    want = EM.egress(frames, masks, 3, REGION, n)
    # a tile of records (256) and more written past each mark: 4,096 bytes into port 1, 8,192 into port 2
    assert all(sum(at >= 4096 * p for at in want.offsets[p]) > 256 for p in range(3)) and want.skipped > 0
    _regions_prefill(far_out, [len(s) for s in want.streams])
    skipped = torch.full((1,), 7, dtype=torch.int32, device=dev)
    r = E.egress_masks(_t(dev, data), _t(dev, offs, np.int32), _t(dev, lens, np.int16), _t(dev, masks, np.int64), 3, REGION, n,
                       out=far_out, skipped=skipped)
    torch.cuda.synchronize()
    assert np.array_equal(r.ports, want.ports) and r.n_skipped - 7 == want.skipped
    assert all(np.array_equal(r.index(p), want.index[p]) for p in range(3))
    _regions_check(far_out, want.streams, "egress")


@pytest.mark.parametrize("tx", [False, True], ids=["forward", "tx"])
def test_lo_gather_far_output(dev, far_out, tx):
    """halo_lo_gather_device with the same geometry: three NetIfs' packet streams at 0, just below
    4 GiB and just below 8 GiB; pkt_off_dw stays relative to its region."""
    import torch

    from halo_amd import loopback as L
    from tests import lo_cases as C
    from tests import lo_model as LM

    n = (12 if tx else 4) * N  # tx-mode packets are cut to their total length: more of them for as many bytes
    frames, data, offs, lens, results = C.mixed(78 + tx, n, 3, tx, loopback_share=3)
    nifs = LM.netifs_of_results(results, 3)
    want = LM.gather(frames, nifs, 3, REGION, n, tx)
    # a tile of packets (256) and more written past each mark: 4,096 bytes into NetIf 1, 8,192 into NetIf 2
    assert all(sum(o != LM.NOT_WRITTEN and 4 * o >= 4096 * p for o in want.pkt_off[p]) > 256 for p in range(3))
    _regions_prefill(far_out, [len(s) for s in want.streams])
    skipped = torch.full((1,), 7, dtype=torch.int32, device=dev)
    r = L.gather(_t(dev, data), _t(dev, offs, np.int32), _t(dev, lens, np.int16), _t(dev, results.view(np.uint8).reshape(-1, 8)), 3,
                 REGION, n, tx=tx, out=far_out, skipped=skipped)
    torch.cuda.synchronize()
    _check_lo(r, want, 3, f"lo far output tx={tx}")
    assert r.n_skipped - 7 == want.skipped
    _regions_check(far_out, want.streams, "lo")


def test_tx_build_far_output(dev, far_out, oracle_lib):
    """halo_tx_build_batch_device with out_stride = 4 MiB and 2,100 descriptors: slot 1,024 starts at
    4 GiB and slot 2,048 at 8 GiB. The built frames (read back by one strided gather), every other
    byte of each slot's first 1,516 still the prefill, the lengths and results whole."""
    import torch

    from halo_amd import protocol
    from halo_amd._lib import NetIf
    from tests import build_cases as B

    n, stride, width = 2100, 4 << 20, 1516
    desc, payload = B.sweep("shuffled")
    desc = np.array(desc[:n])
    want = oracle_lib.tx_build_batch(desc, payload, B.MAC, 1, width, 0xFF00)
    assert int((want[2] == 0).sum()) > n // 2 and (n - 1) * stride + width <= far_out.numel()
    slots = far_out.as_strided((n, width), (stride, 1))
    slots.fill_(B.FILL)
    b = protocol.TxBuilder(n, device=dev, ip_id=0xFF00)
    lens = torch.full((n + 1,), -23131, dtype=torch.int16, device=dev)
    res = _filled(dev, (n + 1,))
    mac = B.MAC.hex()
    b.build(_t(dev, desc.view(np.uint8)), _t(dev, np.array(payload)), netif=NetIf.make(mac=":".join(mac[i:i + 2] for i in range(0, 12, 2)),
                                                                                   ip="192.168.100.1"),
            out_stride=stride, frames=far_out, lens=lens, result=res)
    torch.cuda.synchronize()
    got = (_np(slots.contiguous()), _np(lens, np.uint16)[:n], _np(res)[:n], b.iph_id)
    B.assert_slots(got, B.expected_slots(*want[:3]), want, "far build", desc)
    assert _np(lens, np.uint16)[n] == 0xA5A5 and _np(res)[n] == FILL
