"""GPU: the tx ring producer (halo_amd/csrc/tx_ring.hip through halo_amd.ring.RingProducer) against
a twin ring in the same state written by the host halo_ring_write_span (which tests/test_egress_host.py
pins to the oracle's ReadPacket): the whole ring memory with its 0xA5-filled data area, head, tail
and the result struct, and the device span left as it was between its sentinels. Record counts
around a wavefront and a walk tile, every pairing of span and ring alignment, the wraps, the room
set through tail, the malformed spans, spans longer than the ring, two chained writes, the copy
grid's second trip, the chain from the egress step into three rings and back through a device
consumer, and one bounded run against a live host consumer.

Every test detaches its producers (RingProducer.close, in `finally`) before its ring memory can be
freed: a kernel storing into memory that is no longer mapped is a fault, not a failure."""
from __future__ import annotations

import threading
import time

import numpy as np
import pytest

from tests import txring_cases as C

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 0x5C
PAD = 64  # sentinel bytes on each side of the device span
OK, SHORT, BAD = 0, 1, 2


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


def _ring(size, head, used):
    """A ring of `size` with the data area filled, head at `head` and `used` bytes unread."""
    from halo_amd.ring import RingBuffer

    r = RingBuffer(size)
    r.data[:] = FILL
    _set(r, head, head - used)
    return r


def _set(r, head=None, tail=None):
    if head is not None:
        r.mem[0:8].view(np.uint64)[0] = head
    if tail is not None:
        r.mem[64:72].view(np.uint64)[0] = tail


def _upload(dev, span, d_off=0):
    """The span in device memory at 16-byte offset class d_off, sentinels on both sides."""
    import torch

    host = np.full(PAD + d_off + span.nbytes + PAD, GUARD, np.uint8)
    host[PAD + d_off:PAD + d_off + span.nbytes] = span
    buf = torch.from_numpy(host).to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf, host, buf[PAD + d_off:PAD + d_off + span.nbytes]


def _host_write(twin, span):
    """halo_ring_write_span on the twin: (status, records, bytes, head after)."""
    import ctypes

    from halo_amd import _lib

    recs, taken = ctypes.c_uint32(), ctypes.c_uint64()
    span = np.ascontiguousarray(span)
    rc = _lib.lib.halo_ring_write_span(twin.mem.ctypes.data, _lib.ptr(span) if span.nbytes else None, span.nbytes,
                                       ctypes.byref(recs), ctypes.byref(taken))
    if rc == _lib.HALO_E_INVAL:
        return BAD, 0, 0, twin.head
    assert rc == 0, rc
    return (OK if taken.value == span.nbytes else SHORT), int(recs.value), int(taken.value), twin.head


def _result(res):
    from halo_amd.ring import RingProducer

    r = RingProducer.read_result(res)
    return int(r["status"]), int(r["records"]), int(r["bytes"]), int(r["head"])


def _same_ring(ring, twin, what=""):
    """Every byte of the two mappings but the header's buffer address (bytes 88-95: each ring's own,
    which must be the one halo_ring_create stored)."""
    assert int(ring.mem[88:96].view(np.uint64)[0]) == ring.mem.ctypes.data + 128
    diff = ring.mem != twin.mem
    diff[88:96] = False
    bad = np.flatnonzero(diff)
    assert bad.size == 0, f"{what}: {bad.size} ring bytes differ, first at {bad[:6]} (128 = data[0])"


def _case(dev, span, size, head, used, d_off=0, want=None, dwords=False, twin_span=None):
    """One device write beside one host write of the same span into rings in the same state. Where
    the device's answer is build-defined, `twin_span` is the span the host is given instead, or
    `want` replaces the twin's answer (the twin is then left alone)."""
    import torch

    from halo_amd import _lib
    from halo_amd.ring import RingProducer

    ring, twin = _ring(size, head, used), _ring(size, head, used)
    buf, host, d_span = _upload(dev, span, d_off)
    prod = RingProducer(ring)
    try:
        if dwords:
            _lib.check("copy_mode", _lib.lib.halo_tx_ring_debug_copy_mode(prod._h, 1))
        res = prod.write_span_async(d_span, span.nbytes)
        torch.cuda.synchronize()
        got = _result(res)
        exp = want if want is not None else _host_write(twin, span if twin_span is None else twin_span)
        assert got == exp, (got, exp)
        _same_ring(ring, twin, f"size {size} head {head:#x} used {used} d_off {d_off}")
        assert ring.head == exp[3] and ring.tail == head - used
        assert np.array_equal(buf.cpu().numpy(), host), "the device span or its sentinels were written"
    finally:
        prod.close()
    return got


def _pow2_at_least(n):
    return max(4096, 1 << (int(n) - 1).bit_length())


@pytest.mark.parametrize("n", C.SIZES)
def test_record_counts_and_lengths(dev, n):
    """n records of mixed lengths into an empty ring of 4 KiB ... 1 MiB, placed so that the span wraps
    around the data area's end; n = 65 carries a 9014-byte record as well."""
    pool = C.LENS + [9014] if n == 65 else C.LENS
    frames, span = C.mixed_span(n, n, pool)
    size = _pow2_at_least(2 * span.nbytes if n in (65, 1000) else span.nbytes)
    assert 4096 <= size <= 1 << 20
    if n == 1000:
        assert span.nbytes > 4 * 16384  # several walk tiles
    head = 7 * size + size - (span.nbytes // 2 & ~3)
    assert _case(dev, span, size, head, 0) == (OK, n, span.nbytes, head + span.nbytes)


@pytest.mark.parametrize("ring_mod", [0, 4, 8, 12])
@pytest.mark.parametrize("d_off", [0, 4, 8, 12])
def test_every_alignment_pair(dev, d_off, ring_mod):
    frames, span = C.mixed_span(40 + d_off + ring_mod // 4, 65)
    size = 1 << 16
    head = (1 << 32) + 4096 + ring_mod
    got = _case(dev, span, size, head, 128, d_off)
    assert got[0] == OK
    # and across the wrap, where the second segment starts at data[0] whatever the first's alignment
    _case(dev, span, size, 3 * size - 1024 + ring_mod, 0, d_off)


def test_plain_dword_copy_mode_leaves_the_same_bytes(dev):
    frames, span = C.mixed_span(9, 257)
    size = _pow2_at_least(span.nbytes)
    _case(dev, span, size, 5 * size - 4 * 1000 + 4, 64, d_off=8, dwords=True)


def _odd_split(ends):
    """8 bytes before a record's end (inside its data), and not a multiple of 16."""
    return int(next(e for e in ends[3:] if (int(e) - 8) % 16 == 4)) - 8


@pytest.mark.parametrize("wrap", ["ends_at_end", "ends_4_past", "inside_data", "header_in_last_4", "odd_split"])
def test_wraps(dev, wrap):
    """Where the span meets the data area's end; head above 2^32 throughout."""
    frames, span = C.mixed_span(21, 100)
    ends = C.ends_of(frames)
    size = 1 << 16
    assert span.nbytes < size
    first = {"ends_at_end": span.nbytes, "ends_4_past": span.nbytes - 4, "inside_data": int(ends[50]) - 8,
             "header_in_last_4": int(ends[50]) + 4, "odd_split": _odd_split(ends)}[wrap]  # bytes before the end
    head = (5 << 32) + size - first
    assert head > 1 << 32 and (head & (size - 1)) == size - first
    if wrap == "odd_split":
        assert first % 16 == 4
    assert _case(dev, span, size, head, 0)[0] == OK


@pytest.mark.parametrize("room", ["fits", "exact", "last_short_by_4", "mid_span", "below_first", "full"])
def test_room_through_tail(dev, room):
    """The free space is set through tail; the prefix taken is the host's. After a SHORT the host
    advances tail and the rest is resubmitted: the ring then holds the whole stream in order."""
    import torch

    from halo_amd.ring import RingProducer

    frames, span = C.mixed_span(33, 257)
    ends = C.ends_of(frames)
    size = _pow2_at_least(span.nbytes)
    free = {"fits": size, "exact": span.nbytes, "last_short_by_4": span.nbytes - 4, "mid_span": int(ends[100]) + 20,
            "below_first": int(ends[0]) - 4, "full": 0}[room]
    head, used = (1 << 33) + 12, size - free
    ring, twin = _ring(size, head, used), _ring(size, head, used)
    buf, host, d_span = _upload(dev, span, 4)
    prod = RingProducer(ring)
    try:
        res = prod.write_span_async(d_span, span.nbytes)
        torch.cuda.synchronize()
        got, exp = _result(res), _host_write(twin, span)
        assert got == exp
        want_records = {"fits": 257, "exact": 257, "last_short_by_4": 256, "mid_span": 101, "below_first": 0, "full": 0}
        assert got[:2] == (OK if want_records[room] == 257 else SHORT, want_records[room])
        _same_ring(ring, twin, room)
        if got[1] == 0:
            assert (ring.data == FILL).all() and ring.head == head  # no store to the ring at all
        if got[0] == SHORT:  # the consumer reads everything; the producer resubmits the tail
            for r in (ring, twin):
                _set(r, tail=r.head)
            status, records, taken = prod.write_span(d_span[got[2]:], span.nbytes - got[2])
            exp2 = _host_write(twin, span[got[2]:])
            assert (status, records, taken) == exp2[:3] == (OK, 257 - got[1], span.nbytes - got[2])
            _same_ring(ring, twin, room + " resubmitted")
            assert ring.head == head + span.nbytes
            # the ring holds the stream in order from the first write's position
            idx = ((head & (size - 1)) + np.arange(span.nbytes)) % size
            assert np.array_equal(ring.data[idx], span)
        assert np.array_equal(buf.cpu().numpy(), host)
    finally:
        prod.close()


@pytest.mark.parametrize("header", ["tail_off_grid", "used_above_size"])
def test_cursors_the_host_would_refuse_give_short_zero(dev, header):
    """The header is rewritten after the attach (attach itself refuses such a ring, as the host
    call does): room is 0, nothing is stored."""
    import torch

    from halo_amd.ring import RingProducer

    frames, span = C.mixed_span(2, 64)
    size, head = 1 << 16, (1 << 20) + 8
    ring = _ring(size, head, 0)
    buf, host, d_span = _upload(dev, span)
    prod = RingProducer(ring)
    try:
        _set(ring, tail=head - 6 if header == "tail_off_grid" else head - size - 4)
        before = ring.mem.copy()
        res = prod.write_span_async(d_span, span.nbytes)
        torch.cuda.synchronize()
        assert _result(res) == (SHORT, 0, 0, head)
        assert np.array_equal(ring.mem, before)
    finally:
        prod.close()


@pytest.mark.parametrize("kind", ["zero", "half_plus_4", "past_end", "walk_capacity"])
def test_bad_spans_write_nothing(dev, kind):
    size = 1 << 16
    span = C.bad_span(kind, size)
    head = 9 * size + 40
    if kind == "walk_capacity":
        # the host takes this span (a 16,380-byte record, size / 2 = 32,768): the device walk does not
        twin = _ring(size, head, 0)
        assert _host_write(twin, span) == (OK, 5, span.nbytes, head + span.nbytes)
        got = _case(dev, span, size, head, 0, want=(BAD, 0, 0, head))
    else:
        got = _case(dev, span, size, head, 0)  # the twin's HALO_E_INVAL is BAD_SPAN
    assert got == (BAD, 0, 0, head)


def test_span_longer_than_the_ring(dev):
    """Only the first `size` bytes are examined: a prefix is taken, a record cut by the window is not
    an error, and a malformed record beyond the window is not seen."""
    frames, good = C.mixed_span(8, 40, [60, 100, 570])
    size = 4096
    assert good.nbytes > size + 1000
    head = 3 * size + 2048
    ends = C.ends_of(frames)
    fit = int((ends <= size).sum())
    got = _case(dev, good, size, head, 0)  # all well-formed: the host's answer
    assert got == (SHORT, fit, int(ends[fit - 1]), head + int(ends[fit - 1]))
    bad = np.concatenate([good, C.raw_record(0, 60)])
    twin = _ring(size, head, 0)
    assert _host_write(twin, bad)[0] == BAD  # the host reads every header
    assert _case(dev, bad, size, head, 0, twin_span=good) == got
    # with less room than the window: still the host's prefix
    got = _case(dev, good, size, head, 1024)
    assert got[0] == SHORT and got[2] <= size - 1024


def test_empty_span_still_writes_the_result(dev):
    import torch

    from halo_amd.ring import RingProducer

    ring = _ring(4096, 4096 + 16, 16)
    before = ring.mem.copy()
    prod = RingProducer(ring)
    try:
        d = torch.full((64,), GUARD, dtype=torch.uint8, device=dev)
        res = torch.full((24,), 0x77, dtype=torch.uint8, device=dev)
        prod.write_span_async(d[1:1], 0, result=res)  # no bytes: the pointer needs no alignment
        torch.cuda.synchronize()
        assert _result(res) == (OK, 0, 0, 4096 + 16)
        assert np.array_equal(ring.mem, before) and (d.cpu().numpy() == GUARD).all()
    finally:
        prod.close()


def test_two_writes_back_to_back_on_one_stream(dev):
    """No synchronisation between them: the second reads the head the first published."""
    import torch

    from halo_amd.ring import RingProducer

    _, a = C.mixed_span(51, 300)
    _, b = C.mixed_span(52, 129)
    size = _pow2_at_least(a.nbytes + b.nbytes)
    head = 11 * size + size - a.nbytes - 200  # the second span wraps
    ring, twin = _ring(size, head, 0), _ring(size, head, 0)
    bufa, hosta, da = _upload(dev, a)
    bufb, hostb, db = _upload(dev, b, 12)
    prod = RingProducer(ring)
    try:
        st = torch.cuda.Stream(device=dev)
        prod._workspace(max(a.nbytes, b.nbytes), dev)  # one workspace for both, allocated up front
        torch.cuda.synchronize()
        ra = prod.write_span_async(da, a.nbytes, stream=st)
        rb = prod.write_span_async(db, b.nbytes, stream=st)
        st.synchronize()
        ea, eb = _host_write(twin, a), _host_write(twin, b)
        assert _result(ra) == ea and _result(rb) == eb
        assert eb == (OK, 129, b.nbytes, head + a.nbytes + b.nbytes)
        _same_ring(ring, twin, "two writes")
        assert np.array_equal(bufa.cpu().numpy(), hosta) and np.array_equal(bufb.cpu().numpy(), hostb)
    finally:
        prod.close()


@pytest.mark.parametrize("dwords", [False, True], ids=["aligned", "dwords"])
def test_past_the_copy_grid(dev, dwords):
    """One span past the bytes the capped copy grid moves in a pass (the only large case), in one
    piece — the copy kernel runs its loop per segment, so only an unwrapped span makes workgroups
    take a second trip — with each of the two copy kernels."""
    total = C.past("txring_copy_grid", 100)
    lens = [1514] * (total // 1520)
    rem = total - 1520 * len(lens)
    while rem < 64:
        lens.pop()
        rem += 1520
    lens.append(rem - 4)
    rng = np.random.default_rng(4)
    body = rng.integers(0, 256, total, dtype=np.uint8)
    pos = 0
    for n in lens:  # headers and zero alignment bytes over random payload
        body[pos:pos + 4] = np.frombuffer(np.uint32(n).tobytes(), np.uint8)
        body[pos + 4 + n:pos + C.record_size(n)] = 0
        pos += C.record_size(n)
    assert pos == total == body.nbytes
    size = 8 << 20
    head = (1 << 40) + (1 << 20) + 8
    c = C.read_constants()
    assert (head & (size - 1)) + total <= size and total > C.block_bytes(c) * c["copy_blocks"]  # one segment
    assert _case(dev, body, size, head, 4096, d_off=4, dwords=dwords) == (OK, len(lens), total, head + total)


def test_unregistered_attach_needs_a_mapped_ring(dev):
    """register=False: a ring nobody mapped for the device is refused (HALO_E_INVAL); a ring in
    memory the runtime pinned is taken through the runtime's own device view, and written like any."""
    import types

    import torch

    from halo_amd import _lib
    from halo_amd.ring import RingBuffer, RingProducer

    with pytest.raises(_lib.HaloError) as e:
        RingProducer(RingBuffer(4096), register=False)
    assert e.value.code == _lib.HALO_E_INVAL
    size, head = 1 << 16, 3 * (1 << 16) - 2048
    pinned = torch.empty(_lib.RING_HEADER + size + 64, dtype=torch.uint8, pin_memory=True)
    at = (-pinned.data_ptr()) % 64
    mem = pinned.numpy()[at:at + _lib.RING_HEADER + size]
    _lib.check("halo_ring_create", _lib.lib.halo_ring_create(mem.ctypes.data, mem.nbytes))
    mem[_lib.RING_HEADER:] = FILL
    ring = types.SimpleNamespace(mem=mem, size=size)
    _set(ring, head, head)
    twin = _ring(size, head, 0)
    frames, span = C.mixed_span(61, 65)
    buf, host, d_span = _upload(dev, span, 4)
    prod = RingProducer(ring, register=False)
    try:
        res = prod.write_span_async(d_span, span.nbytes)
        torch.cuda.synchronize()
        assert _result(res) == _host_write(twin, span) == (OK, 65, span.nbytes, head + span.nbytes)
        diff = mem != twin.mem
        diff[88:96] = False
        assert not diff.any(), np.flatnonzero(diff)[:6]
    finally:
        prod.close()
    del pinned  # after the detach


def _oracle_frames(O, ring_mem, capacity=1514):
    r = O.Ring(mem=ring_mem)
    out = []
    while True:
        ok, frame, _ = r.read(capacity)
        if not ok:
            return out
        out.append(frame)


def test_chain_from_egress_to_rings_and_back(dev, oracle_lib):
    """Frames go through egress_masks (3 ports), then publish_egress into three rings: each ring,
    read with the oracle's ReadPacket, yields its port's frames padded to 60 bytes, in order. Then
    the loop closed on the device: one ring carries a registered RingConsumer and an unregistered
    RingProducer; the device writes, the device polls, and the records are the parse of the frames."""
    import torch

    from halo_amd import egress as E
    from halo_amd._lib import NetIf
    from halo_amd.ring import RingBuffer, RingConsumer, RingProducer, publish_egress
    from oracle import oracle as O
    from tests import arp_cases as K

    rng = np.random.default_rng(77)
    n = 300
    lens_pool = [42, 59, 60, 61, 64, 100, 570, 1514]
    frames = [K.ipv4_frame(rng, lens_pool[i % len(lens_pool)], 0x0A000001 + i) for i in range(n)]
    masks = np.array([(1, 2, 4, 3, 7, 5)[i % 6] for i in range(n)], np.uint64)
    data, offs, lens = K.pack(rng, frames)
    padded = [f + b"\0" * max(0, 60 - len(f)) for f in frames]
    want = [[padded[i] for i in range(n) if masks[i] >> p & 1] for p in range(3)]
    region = (max(sum(C.record_size(len(f)) for f in w) for w in want) + 64 + 15) & ~15
    r = E.egress_masks(torch.from_numpy(data).to(dev), torch.from_numpy(offs.view(np.int32)).to(dev),
                       torch.from_numpy(lens.view(np.int16)).to(dev), torch.from_numpy(masks.view(np.int64)).to(dev),
                       3, region)
    rings = [RingBuffer(_pow2_at_least(region)) for _ in range(3)]
    prods = []
    try:
        for ring in rings:
            prods.append(RingProducer(ring))
        results = publish_egress(r, prods)
        for p in range(3):
            assert (int(results[p]["status"]), int(results[p]["records"])) == (OK, len(want[p])), results[p]
            assert int(results[p]["bytes"]) == int(r.ports[p]["bytes_written"]) == rings[p].head
    finally:
        for prod in prods:
            prod.close()
    for p in range(3):
        assert _oracle_frames(O, rings[p].mem) == want[p], p

    # the loop closed: device producer and device consumer under the consumer's registration
    ring = RingBuffer(_pow2_at_least(region))
    cons = RingConsumer(ring, capacity=1514, register=True)
    prod = None
    try:
        prod = RingProducer(ring, register=False)
        status, records, taken = prod.write_span(r.device_stream(2), int(r.ports[2]["bytes_written"]))
        assert (status, records) == (OK, len(want[2]))
        got, info, _ = cons.poll(NetIf.make())
        got = got.copy()
        assert info["n_frames"] == len(want[2]) and info["stop"] == "EMPTY" and info["end_bytes"] == taken
        cons.commit()
        assert ring.tail == ring.head == taken
    finally:
        if prod is not None:
            prod.close()
        cons.close()
    flat, foffs, pos = [], [], 0
    for f in want[2]:
        foffs.append(pos // 4)
        flat.append(f + b"\0" * (-len(f) % 4))
        pos += (len(f) + 3) & ~3
    blob = np.frombuffer(b"".join(flat) + b"\0" * 16, np.uint8)
    exp, _ = O.rx_batch(blob, np.array([len(f) for f in want[2]], np.uint16), O.NetIf.make(), 1,
                        offsets_dw=np.array(foffs, np.uint32))
    assert got.tobytes() == exp.tobytes()


def test_live_host_consumer(dev, oracle_lib):
    """The release / acquire pair: a host thread reads the ring with the oracle's ReadPacket while
    the device publishes ~200 spans of ~100 numbered frames into a 64 KiB ring, resubmitting SHORT
    tails. Every frame arrives once, in order, with its bytes. Bounded: past the deadline the test
    fails; nothing spins without it."""
    from halo_amd.ring import RingBuffer, RingProducer
    from oracle import oracle as O

    n_spans, per, deadline = 200, 100, time.monotonic() + 20.0
    rng = np.random.default_rng(31)
    lens = rng.choice([60, 61, 64, 100, 570], size=n_spans * per)
    payload = rng.integers(0, 256, 600, dtype=np.uint8).tobytes()

    def frame(i):
        return int(i).to_bytes(8, "little") + payload[(i % 19):(i % 19) + int(lens[i]) - 8]

    ring = RingBuffer(1 << 16)
    seen, stop = [], threading.Event()

    def consume():
        r = O.Ring(mem=ring.mem)
        while len(seen) < n_spans * per and not stop.is_set() and time.monotonic() < deadline:
            ok, f, _ = r.read(1514)
            if ok:
                seen.append(f)
            else:
                time.sleep(0)  # yield; the loop ends at the deadline

    th = threading.Thread(target=consume, daemon=True)
    prod = RingProducer(ring)
    try:
        th.start()
        import torch

        for s in range(n_spans):
            span = C.span_of(frame(i) for i in range(s * per, (s + 1) * per))
            d = torch.from_numpy(span).to(dev)
            done = 0
            while done < span.nbytes:
                assert time.monotonic() < deadline, f"deadline: span {s}, {len(seen)} frames seen"
                status, _, taken = prod.write_span(d[done:], span.nbytes - done)
                assert status in (OK, SHORT)
                done += taken
        th.join(max(0.0, deadline - time.monotonic()))
        assert not th.is_alive(), f"deadline: {len(seen)} of {n_spans * per} frames seen"
    finally:
        stop.set()
        th.join(5.0)
        prod.close()
    assert len(seen) == n_spans * per
    for i, f in enumerate(seen):
        assert f == frame(i), i
