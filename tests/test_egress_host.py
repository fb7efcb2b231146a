"""CPU: the egress step's host side (halo_amd/csrc/tx_egress_host.cc, halo_ring_write_span in
host_logic.cc) against tests/egress_model.py: hand-written known answers, the length / mask / port
mix of tests/egress_cases.py for all three kinds with every output prefilled and compared whole,
the region cut, results of the real host switch and of the ARP model's encap, the ring producer
against halo_ring_write_batch through the oracle's ReadPacket, and the device entry points'
argument checks, which are answered before any device is looked for."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import arp_cases as K
from tests import arp_model as AM
from tests import egress_cases as C
from tests import egress_model as EM
from tests import switch_model as SM

FILL = 0xA5


def _host(kind, data, offs, lens, selectors, n_ports, region, index_cap=0, jumbo=False, flood=0, skipped0=7):
    """halo_tx_egress_host into 0xA5-filled outputs: (result, the input bytes afterwards)."""
    from halo_amd import egress as E

    out = np.full(n_ports * region + 32, FILL, np.uint8)
    skipped = np.array([skipped0], np.uint32)  # incremented, not set
    before = data.copy()
    r = E.egress_host(kind, data, offs, lens, selectors, n_ports, region, index_cap, jumbo, flood, out=out, skipped=skipped)
    assert np.array_equal(data, before), "the input batch was written"
    r.skipped0 = skipped0
    return r


def _check(r, want: EM.Want):
    assert np.array_equal(r.ports, want.ports), (r.ports, want.ports)
    got = r.out
    exp = want.out(FILL, size=len(got))
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"{bad.size} output bytes differ, first at {bad[:6]}"
    for p in range(want.n_ports):
        assert np.array_equal(r.index(p), want.index[p]), p
    assert r.n_skipped - r.skipped0 == want.skipped


def _run_host_raw(kind, data, offs, lens, selectors, n_ports, region, index_cap, jumbo=False, flood=0):
    """Straight through ctypes with a 0xA5-filled index array, so that a stray index write shows."""
    from halo_amd import _lib

    cfg = _lib.EgressConfig()
    cfg.n_ports, cfg.flags, cfg.region_bytes, cfg.index_cap = n_ports, (2 if jumbo else 0), region, index_cap
    out = np.full(n_ports * region + 32, FILL, np.uint8)
    ports = np.full(n_ports, 0, _lib.EGRESS_PORT_DTYPE)
    ports.view(np.uint8)[:] = FILL
    index = np.full((n_ports, max(index_cap, 1)), 0xA5A5A5A5, np.uint32)
    skipped = np.array([3], np.uint32)
    rc = _lib.lib.halo_tx_egress_host(ctypes.byref(cfg), kind, _lib.ptr(data), _lib.ptr(offs), _lib.ptr(lens), len(lens),
                                      _lib.ptr(selectors), flood, _lib.ptr(out), _lib.ptr(ports), _lib.ptr(index),
                                      _lib.ptr(skipped))
    assert rc == 0
    return out, ports, index[:, :index_cap], int(skipped[0]) - 3


# ---- known answers -------------------------------------------------------------------------------
def _one_frame(frame: bytes):
    data = np.frombuffer(frame + bytes([0xEE] * (-len(frame) % 4 + 4)), np.uint8).copy()
    return data, np.array([0], np.uint32), np.array([len(frame)], np.uint16)


@pytest.mark.parametrize("length,size,header", [(42, 64, "3c000000"), (61, 68, "3d000000"), (64, 68, "40000000")])
def test_known_answers(length, size, header):
    frame = bytes((3 * k + 1) & 0xFF for k in range(length))
    expected = bytes.fromhex(header) + frame + bytes(size - 4 - length)
    if length == 42:  # written out in full: 3c 00 00 00, the 42 bytes, 18 zeros
        expected = bytes.fromhex(
            "3c000000" "0104070a0d101316191c1f2225282b2e3134373a3d404346494c4f5255585b5e6164676a6d707376797c" + "00" * 18)
    assert len(expected) == size
    data, offs, lens = _one_frame(frame)
    r = _host(0, data, offs, lens, np.array([1], np.uint64), 1, 80, index_cap=2)
    assert r.stream(0).tobytes() == expected
    assert tuple(r.ports[0]) == (1, 1, size, size) and list(r.index(0)) == [0]
    assert np.all(r.out[size:] == FILL)
    assert EM.record(frame) == expected  # the model says the same


# ---- host == model -------------------------------------------------------------------------------
def _selectors(kind, masks, n_ports, rng):
    """Selectors of `kind` that decode to something related to `masks`, and the model's masks for
    them: the masks themselves; ARP results over every verdict and out NetIfs below, at and above
    n_ports and 0xFF; switch results over every verdict with a flood mask that has bits at or above
    n_ports."""
    from halo_amd import _lib

    n = len(masks)
    if kind == 0:
        return masks, masks, 0
    if kind == 1:
        res = np.zeros(n, _lib.ARP_RESULT_DTYPE)
        res["verdict"] = np.where(rng.random(n) < 0.6, AM.HIT, np.arange(n) % 7)
        res["out_netif"] = rng.choice(np.array([0, n_ports - 1, n_ports // 2, min(n_ports, 255), 64, 200, 0xFF], np.uint8), n)
        res["tx_len"] = rng.integers(0, 1 << 16, n)  # not read: lens decides
        res["target_ip"] = rng.integers(0, 1 << 32, n)
        return res, EM.masks_of_arp(res), 0
    res = np.zeros(n, _lib.SW_RESULT_DTYPE)
    res["verdict"] = np.where(rng.random(n) < 0.6, np.where(rng.random(n) < 0.5, SM.UNICAST, SM.FLOOD), np.arange(n) % 6)
    res["out_port"] = rng.choice(np.array([0, n_ports - 1, n_ports // 2, min(n_ports, 255), 64, 0xFF], np.uint8), n)
    res["tx_len"] = rng.integers(0, 1 << 16, n)
    flood = (0x8000000000000005 | 1 << (n_ports - 1) | 1 << min(n_ports, 63)) & C.ALL
    return res, EM.masks_of_switch(res, flood), flood


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("n_ports", [1, 3, 64])
@pytest.mark.parametrize("jumbo", [False, True])
def test_host_matches_model(kind, n_ports, jumbo):
    n = 260
    frames, data, offs, lens, masks = C.mixed(11 * n_ports + kind, n, n_ports, jumbo)
    assert set((offs * 4) % 16) == {0, 4, 8, 12}
    assert set(lens.tolist()) == set(C.JUMBO_LENS if jumbo else C.LENS)
    rng = np.random.default_rng(5)
    sel, model_masks, flood = _selectors(kind, masks, n_ports, rng)
    free = EM.egress(frames, model_masks, n_ports, 1 << 40, 0, jumbo)
    region = C.region_for(int(free.ports["bytes"].max()))
    index_cap = int(free.ports["frames"].max()) + 3
    want = EM.egress(frames, model_masks, n_ports, region, index_cap, jumbo)
    assert want.skipped > 0 and int(want.ports["frames"].sum()) > 0
    if kind == 0:
        assert int(want.ports["frames"].min()) > 0  # every port got something, the last one too
    r = _host(kind, data, offs, lens, sel, n_ports, region, index_cap, jumbo, flood)
    _check(r, want)
    out, ports, index, skipped = _run_host_raw(kind, data, offs, lens, sel, n_ports, region, index_cap, jumbo, flood)
    assert np.array_equal(ports, want.ports) and skipped == want.skipped
    assert np.array_equal(index, want.index_array()), "index entries beyond min(frames, index_cap) were written"
    # a short index list: only the first index_cap entries, and `frames` still the total
    short = EM.egress(frames, model_masks, n_ports, region, 2, jumbo)
    _, ports, index, _ = _run_host_raw(kind, data, offs, lens, sel, n_ports, region, 2, jumbo, flood)
    assert np.array_equal(ports, short.ports) and np.array_equal(index, short.index_array())


def test_no_byte_past_a_frames_last_word_reaches_the_output():
    """A 61-byte frame's last word holds three bytes of its neighbour: they stay out."""
    f0, f1 = bytes([0x11] * 61), bytes([0x22] * 60)
    data, offs, lens = SM.pack([f0, f1])
    data[61:64] = 0x77
    r = _host(0, data, offs, lens, np.array([1, 1], np.uint64), 1, 256)
    assert r.stream(0).tobytes() == EM.record(f0) + EM.record(f1)


# ---- region cut ----------------------------------------------------------------------------------
def test_region_cut():
    """Five 60-byte frames (64-byte records) and one 100-byte frame on two ports. The cut exactly on
    a record boundary, one byte short of it, in the middle of the batch, and no region at all."""
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in (60, 60, 100, 60, 60, 60)]
    data, offs, lens = K.pack(rng, frames)
    masks = np.array([3, 1, 3, 3, 2, 3], np.uint64)
    boundary = 64 + 64 + 104  # port 0 after its third record
    for region, written0 in ((boundary, 3), (boundary - 1, 2), (boundary + 1, 3), (130, 2), (64, 1), (63, 0), (0, 0),
                             (1 << 20, 5)):
        want = EM.egress(frames, masks, 2, region, 8)
        assert int(want.ports[0]["frames_written"]) == written0 and int(want.ports[0]["frames"]) == 5
        r = _host(0, data, offs, lens, masks, 2, region, 8)
        _check(r, want)
        assert list(r.index(0)) == [0, 1, 2, 3, 5]  # also for records beyond the region
    # the first record that does not fit ends the prefix: a later, shorter one is not taken
    want = EM.egress(frames, masks, 2, 64 + 64 + 64, 8)
    assert int(want.ports[0]["frames_written"]) == 2 and int(want.ports[1]["frames_written"]) == 2
    _check(_host(0, data, offs, lens, masks, 2, 192, 8), want)


# ---- the switch kind over the real host switch ------------------------------------------------------
def test_switch_kind_over_host_switch():
    from halo_amd._lib import SW_RESULT_DTYPE
    from halo_amd.switch import Switch

    warm, frames = C.switch_batch()
    sw = Switch([10, 10, 10, 20], 4)
    for port, fr, now in warm:
        sw.forward(port, *SM.pack(fr), now)
    rng = np.random.default_rng(8)
    data, offs, lens = K.pack(rng, frames)
    res, _ = sw.forward(0, data, offs, lens, 2)
    res = np.ascontiguousarray(res).view(SW_RESULT_DTYPE).reshape(-1)
    assert sorted(set(res["verdict"].tolist())) == list(range(6))
    assert int(res["out_port"][0]) == 0 and int(res["verdict"][0]) == SM.UNICAST
    flood = sw.flood_mask(0)
    assert flood == 0b0110
    masks = EM.masks_of_switch(res, flood)
    want = EM.egress(frames, masks, 4, 4096, 16)
    assert [int(x) for x in want.ports["frames"]] == [1, 1 + 2, 2 + 2, 0] and want.skipped == 0
    _check(_host(2, data, offs, lens, res, 4, 4096, 16, flood=flood), want)
    sw.close()


# ---- the ARP kind over the model's encap -------------------------------------------------------------
def test_arp_kind_over_model_encap():
    from halo_amd._lib import ARP_RESULT_DTYPE

    model = AM.Model(K.NETIFS, 64)
    keys = []
    for k in range(15):
        nif = k % 3
        ip = (K.NETIFS[nif].ip & 0xFFFFFF00) | (10 + k)
        model.set(nif, ip, K.mac(100 + k), 50)
        keys.append((nif, ip))
    rng = np.random.default_rng(21)
    frames, dsts, select, forced, names = K.mixed_batch(rng, keys, 200)

    def route(i):  # a direct route to the NetIf that owns the /24, else none; the cases' special routes by name
        if forced[i] is not None:
            return None
        d = int(dsts[i])
        if (d & 0xFFFF0000) == K.NH_HIT:
            return keys[0][1], keys[0][0]
        if (d & 0xFFFF0000) == K.NH_MISS:
            return K.absent(keys, 2, 0), 2
        if (d & 0xFFFF0000) == K.NH_OWN:
            return K.NETIFS[1].ip, 1
        if (d & 0xFFFF0000) == K.PANIC:
            return AM.ROUTE_PANIC_ID
        if (d & 0xFFFF0000) == K.BAD_NETIF:
            return 0, 9
        for nif, m in enumerate(K.NETIFS):
            if (d & 0xFFFFFF00) == (m.ip & 0xFFFFFF00):
                return 0, nif
        return AM.ROUTE_NONE

    res = np.zeros(len(frames), ARP_RESULT_DTYPE)
    after = []
    for i, f in enumerate(frames):
        v, out, tx, target, g = model.encap(f, route(i), 0, bool(select[i]))
        res[i] = (v, out, tx, target)
        after.append(g)
    assert set(res["verdict"].tolist()) == set(range(7))
    data, offs, lens = K.pack(rng, after)
    masks = EM.masks_of_arp(res)
    assert np.array_equal(masks != 0, res["verdict"] == AM.HIT)  # every non-HIT verdict emits nothing
    want = EM.egress(after, masks, 3, 1 << 16, 64)
    assert int(want.ports["frames"].sum()) == int((res["verdict"] == AM.HIT).sum()) and want.skipped == 0
    assert all(int(x) > 0 for x in want.ports["frames"])
    _check(_host(1, data, offs, lens, res, 3, 1 << 16, 64), want)


# ---- halo_ring_write_span ----------------------------------------------------------------------------
def _ring_pair(size, pos):
    from halo_amd.ring import RingBuffer
    from oracle import oracle as O

    rings = []
    for _ in range(2):
        rb = RingBuffer(size)
        ora = O.Ring(mem=rb.mem)
        ora.set_cursors(pos)
        rings.append((rb, ora))
    return rings


def _drain(ora):
    got = []
    while True:
        ok, f, _ = ora.read()
        if not ok:
            return got
        got.append(f)


def _padded(frames):
    return [f + bytes(max(0, 60 - len(f))) for f in frames]


def _stream_of(frames, region=1 << 20):
    rng = np.random.default_rng(1)
    data, offs, lens = K.pack(rng, frames)
    r = _host(0, data, offs, lens, np.ones(len(frames), np.uint64), 1, region)
    return r


@pytest.mark.parametrize("where", ["fresh", "wrap"])
def test_write_span_equals_write_batch(oracle_lib, where):
    """The frames ReadPacket returns after write_span(egress stream) are those it returns after
    halo_ring_write_batch of the host-padded frames, and head is equal: from a fresh ring, and from
    a head placed so that one record's data wraps and a later record's header sits in the last four
    bytes of the data area."""
    rng = np.random.default_rng(4)
    size = 1024
    frames = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in (60, 42, 61, 100, 64, 14, 63)]
    sizes = [EM.record_size(len(f)) for f in frames]
    # the fourth record's header in the last four bytes: head + 64 + 64 + 68 = size - 4 (mod size)
    pos = 0 if where == "fresh" else 5 * size + (size - 4 - sum(sizes[:3]))
    (rb_a, ora_a), (rb_b, ora_b) = _ring_pair(size, pos)
    r = _stream_of(frames)
    stream = r.stream(0)
    assert len(stream) == sum(sizes)
    assert rb_a.write_span(stream) == (len(frames), len(stream))
    assert rb_b.write(_padded(frames)) == len(frames)
    assert rb_a.head == rb_b.head == pos + sum(sizes)
    if where == "wrap":
        assert (pos + sum(sizes[:3])) % size == size - 4  # a header alone before the end; its data wraps
    got_a, got_b = _drain(ora_a), _drain(ora_b)
    assert got_a == got_b == _padded(frames)
    # the ring bytes are WritePacket's, plus zero alignment bytes where WritePacket wrote nothing
    differ = np.flatnonzero(rb_a.data != rb_b.data)
    align = set()
    at = pos
    for f, s in zip(frames, sizes):
        align.update((at + 4 + max(len(f), 60) + k) % size for k in range(s - 4 - max(len(f), 60)))
        at += s
    assert set(differ.tolist()) <= align
    assert np.all(rb_a.data[sorted(align)] == 0) if align else True


def test_write_span_takes_the_longest_prefix(oracle_lib):
    frames = [bytes([k + 1] * 60) for k in range(6)]  # 64-byte records
    (rb, ora), _ = _ring_pair(256, 0)
    stream = _stream_of(frames).stream(0)
    assert rb.write_span(stream) == (4, 256)  # a full ring: four of six
    assert rb.write_span(stream[256:]) == (0, 0) and rb.head == 256
    assert [ora.read()[1] for _ in range(3)] == frames[:3]  # the consumer advances by three records
    rb.mem[64:72].view(np.uint64)[0] = ora._ct.value
    assert rb.tail == 192
    assert rb.write_span(stream[256:]) == (2, 128)
    assert _drain(ora) == frames[3:]
    # room for one record and a bit: one is taken
    (rb, ora), _ = _ring_pair(256, 64)
    rb.mem[0:8].view(np.uint64)[0] = 64 + 156  # 100 bytes free
    before = rb.mem.copy()
    assert rb.write_span(stream) == (1, 64) and rb.head == 64 + 156 + 64
    assert np.array_equal(rb.data[220:256], stream[:36]) and np.array_equal(rb.data[:28], stream[36:64])  # wrapped
    assert np.array_equal(np.delete(rb.mem, np.r_[0:8, 128 + 220:128 + 256, 128:128 + 28]),
                          np.delete(before, np.r_[0:8, 128 + 220:128 + 256, 128:128 + 28]))


@pytest.mark.parametrize("bad", ["zero", "overlong", "past_span", "short_header"])
def test_write_span_rejects_a_malformed_span(bad):
    from halo_amd import _lib
    from halo_amd.ring import RingBuffer

    rb = RingBuffer(256)
    good = EM.record(bytes([9] * 60))
    if bad == "zero":
        span = good + (0).to_bytes(4, "little") + bytes(60)
    elif bad == "overlong":  # above size / 2
        span = good + (129).to_bytes(4, "little") + bytes(132)
    elif bad == "past_span":
        span = good + EM.record(bytes([8] * 61))[:-4]
    else:
        span = good + b"\x3c\x00"
    before = rb.mem.copy()
    arr = np.frombuffer(span, np.uint8)
    recs, taken = ctypes.c_uint32(77), ctypes.c_uint64(77)
    rc = _lib.lib.halo_ring_write_span(rb.mem.ctypes.data, _lib.ptr(arr), len(span), ctypes.byref(recs), ctypes.byref(taken))
    assert rc == _lib.HALO_E_INVAL
    assert np.array_equal(rb.mem, before) and rb.head == 0
    with pytest.raises(_lib.HaloError):
        rb.write_span(arr)
    # length 128 = size / 2 is the longest a ring takes
    ok = (128).to_bytes(4, "little") + bytes(128)
    assert rb.write_span(np.frombuffer(ok, np.uint8)) == (1, 132)


def test_ring_scan_over_a_stream_finds_frames_written(oracle_lib):
    O = oracle_lib
    frames, data, offs, lens, masks = C.mixed(2, 120, 3)
    free = EM.egress(frames, masks, 3, 1 << 40)
    region = (int(free.ports["bytes"].max()) // 2) & ~15  # a cut, so that written < frames
    want = EM.egress(frames, masks, 3, region)
    r = _host(0, data, offs, lens, masks, 3, region)
    for p in range(3):
        s = r.stream(p)
        assert int(want.ports[p]["frames_written"]) < int(want.ports[p]["frames"])
        off_dw, ln, stop, end, _ = O.ring_scan(s, len(s), 1 << 30, capacity=1514)
        assert len(off_dw) == int(r.ports[p]["frames_written"]) == len(want.offsets[p]) and end == len(s)
        assert stop == O.RING_STOP["EMPTY"]
        assert [4 * int(o) - 4 for o in off_dw] == want.offsets[p]


# ---- argument errors ---------------------------------------------------------------------------------
def test_device_entry_points_check_arguments_before_any_device():
    """Every malformed call is HALO_E_INVAL whether or not the machine has a device: the checks
    come first. (A well-formed call on a machine without one is HALO_E_NODEV.)"""
    import torch

    from halo_amd import _lib

    L = _lib.lib
    INVAL = _lib.HALO_E_INVAL
    buf = np.zeros(4096, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 64
    ws = int(L.halo_tx_egress_workspace(300, 3))
    assert ws == 16 * 2 * 3 and int(L.halo_tx_egress_workspace(0, 64)) == 16 * 64
    assert int(L.halo_tx_egress_workspace(1, 0)) == 0 and int(L.halo_tx_egress_workspace(1, 65)) == 0

    def call(fn="masks", n_ports=3, flags=0, region=1024, index_cap=4, cfg_null=False, n=300, d_bytes=base,
             d_offs=base + 64, d_lens=base + 128, d_sel=base + 192, d_out=base + 256, d_ports=base + 512, d_index=base + 768,
             d_skipped=base + 896, d_ws=base + 1024, ws_bytes=ws):
        cfg = _lib.EgressConfig()
        cfg.n_ports, cfg.flags, cfg.region_bytes, cfg.index_cap = n_ports, flags, region, index_cap
        c = None if cfg_null else ctypes.byref(cfg)
        if fn == "switch":
            return L.halo_tx_egress_switch_device(c, d_bytes, d_offs, d_lens, n, d_sel, 6, d_out, d_ports, d_index, d_skipped,
                                                  d_ws, ws_bytes, None)
        return getattr(L, f"halo_tx_egress_{fn}_device")(c, d_bytes, d_offs, d_lens, n, d_sel, d_out, d_ports, d_index,
                                                         d_skipped, d_ws, ws_bytes, None)

    for fn in ("masks", "arp", "switch"):
        bad = [dict(cfg_null=True), dict(n_ports=0), dict(n_ports=65), dict(flags=1), dict(region=1032), dict(region=8),
               dict(d_out=base + 264), dict(d_out=None), dict(d_ports=None), dict(d_index=None), dict(d_bytes=None),
               dict(d_offs=None), dict(d_lens=None), dict(d_sel=None), dict(d_ws=None), dict(ws_bytes=ws - 1),
               dict(d_offs=base + 66), dict(d_lens=base + 129), dict(d_sel=base + 193), dict(d_ports=base + 516),
               dict(d_index=base + 770), dict(d_skipped=base + 898), dict(d_ws=base + 1028)]
        for kw in bad:
            assert call(fn, **kw) == INVAL, (fn, kw)
    assert call("masks", d_sel=base + 196) == INVAL and call("arp", d_sel=base + 196) == INVAL
    # the host entry: the same checks, a bad kind, and no alignment asked of `out` or the region
    cfg = _lib.EgressConfig()
    cfg.n_ports, cfg.region_bytes = 1, 0
    ports = np.zeros(1, _lib.EGRESS_PORT_DTYPE)
    assert L.halo_tx_egress_host(ctypes.byref(cfg), 3, None, None, None, 0, None, 0, None, _lib.ptr(ports), None, None) == INVAL
    assert L.halo_tx_egress_host(ctypes.byref(cfg), 0, None, None, None, 0, None, 0, None, None, None, None) == INVAL
    assert L.halo_tx_egress_host(ctypes.byref(cfg), 0, None, None, None, 1, None, 0, None, _lib.ptr(ports), None, None) == INVAL
    ports.view(np.uint8)[:] = FILL
    assert L.halo_tx_egress_host(ctypes.byref(cfg), 0, None, None, None, 0, None, 0, None, _lib.ptr(ports), None, None) == 0
    assert tuple(ports[0]) == (0, 0, 0, 0)  # n == 0 zeroes the summaries
    if not torch.cuda.is_available():  # the checks passed and only then was a device looked for
        assert call("masks") == _lib.HALO_E_NODEV


def test_derived_edges_equal_the_table():
    got = C.derived(C.read_constants())
    assert got == {k: v["first_past"] for k, v in C.BOUNDARIES.items()}, got


def test_uniform_model_path_equals_the_loop():
    frames2d, data, offs, lens = C.uniform_batch(6, 700)
    masks = np.array([(1, 2, 7, 0, 5)[i % 5] for i in range(700)], np.uint64)
    for region in (1 << 20, 68 * 100, 68 * 100 + 16, 0):
        a = EM.egress([f.tobytes() for f in frames2d], masks, 3, region, 150)
        b = EM.egress_uniform(frames2d, masks, 3, region, 150)
        assert np.array_equal(a.ports, b.ports) and np.array_equal(a.out(), b.out())
        assert all(np.array_equal(x, y) for x, y in zip(a.index, b.index))
