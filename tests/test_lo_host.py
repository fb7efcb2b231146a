"""CPU: the loopback gather's host loop (halo_lo_gather_host, halo_amd/csrc/lo_gather_host.cc through
halo_amd.loopback.gather_host) against tests/lo_model.py, bit for bit: the whole output buffer with a
0xA5 sentinel beyond each NetIf's written bytes, the summaries, the three per-packet arrays, the
skip count. Both modes, the region cut, index_cap below the count, out NetIfs at and above
n_netifs, every argument error, what the corpus reaches, and one known answer written by hand."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import arp_model as AM
from tests import lo_cases as C
from tests import lo_model as LM

FILL = C.FILL


def _run(frames, data, offs, lens, results, n_netifs, region, index_cap, tx=False, jumbo=False, skipped0=7):
    from halo_amd import loopback as L

    want = LM.gather(frames, LM.netifs_of_results(results, n_netifs), n_netifs, region, index_cap, tx, jumbo)
    out = np.full(n_netifs * region + 64, FILL, np.uint8)
    before = data.copy()
    r = L.gather_host(data, offs, lens, results, n_netifs, region, index_cap, tx=tx, jumbo=jumbo, out=out,
                      skipped=np.full(1, skipped0, np.uint32))
    # the arrays are allocated by the wrapper: fill what no entry covers the way the model does
    assert np.array_equal(data, before), "the input batch was written"
    assert np.array_equal(r.ports, want.ports), (r.ports, want.ports)
    exp = want.out(FILL, size=len(out))
    bad = np.flatnonzero(r.out != exp)
    assert bad.size == 0, f"{bad.size} output bytes differ, first at {bad[:6]}"
    for p in range(n_netifs):
        assert np.array_equal(r.pkt_off_dw(p), np.asarray(want.pkt_off[p], np.uint32)), p
        assert np.array_equal(r.pkt_len(p), np.asarray(want.pkt_len[p], np.uint16)), p
        assert np.array_equal(r.index(p), np.asarray(want.index[p], np.uint32)), p
    assert r.n_skipped - skipped0 == want.skipped
    return r, want


def _raw_call(cfg, data, offs, lens, n, results, out, ports, pkt_off, pkt_len, index, skipped):
    from halo_amd import _lib

    return _lib.lib.halo_lo_gather_host(None if cfg is None else ctypes.byref(cfg), _lib.ptr(data), _lib.ptr(offs),
                                        _lib.ptr(lens), n, _lib.ptr(results), _lib.ptr(out), _lib.ptr(ports),
                                        _lib.ptr(pkt_off), _lib.ptr(pkt_len), _lib.ptr(index), _lib.ptr(skipped))


@pytest.mark.parametrize("tx", [False, True], ids=["forward", "tx"])
@pytest.mark.parametrize("n_netifs", [1, 4, 64])
@pytest.mark.parametrize("n", C.SIZES)
def test_host_matches_model(n, n_netifs, tx):
    jumbo = n == 257  # one size carries the jumbo lengths as well
    frames, data, offs, lens, results = C.mixed(1000 * n_netifs + n + (7 if tx else 0), n, n_netifs, tx, jumbo)
    free = LM.gather(frames, LM.netifs_of_results(results, n_netifs), n_netifs, 1 << 34, 0, tx, jumbo)
    region = C.region_for(int(free.ports["bytes"].max()))
    index_cap = int(free.ports["frames"].max()) + 3
    r, want = _run(frames, data, offs, lens, results, n_netifs, region, index_cap, tx, jumbo)
    assert np.array_equal(want.ports["frames"], want.ports["frames_written"])
    if n >= 255:
        assert want.skipped > 0 and int(want.ports["frames"][0]) > 0
    # the arrays beyond the written entries and the bytes between regions were left alone (the
    # wrapper zero-fills its own arrays): the raw entries past min(frames, index_cap) are zero
    for p in range(n_netifs):
        k = min(int(want.ports[p]["frames"]), index_cap)
        assert not r.index_raw[p, k:].any() and not r.pkt_len_raw[p, k:].any() and not r.pkt_off_dw_raw[p, k:].any()
    # a short list: only the first two entries per NetIf, `frames` still the total
    _run(frames, data, offs, lens, results, n_netifs, region, 2, tx, jumbo)
    _run(frames, data, offs, lens, results, n_netifs, region, 0, tx, jumbo)


@pytest.mark.parametrize("tx", [False, True], ids=["forward", "tx"])
@pytest.mark.parametrize("cut", ["half", "one_packet", "nothing_fits", "exact"])
def test_region_cut(cut, tx):
    frames, data, offs, lens, results = C.mixed(55, 400, 4, tx)
    free = LM.gather(frames, LM.netifs_of_results(results, 4), 4, 1 << 34, 0, tx)
    most = int(free.ports["bytes"].max())
    region = {"half": most // 2, "one_packet": int(free.ports["bytes"].min()) // 3, "nothing_fits": 16, "exact": most}[cut]
    r, want = _run(frames, data, offs, lens, results, 4, region, 400, tx)
    cut_ports = [p for p in range(4) if int(want.ports[p]["frames_written"]) < int(want.ports[p]["frames"])]
    if cut == "exact":
        assert not cut_ports and int(want.ports["bytes_written"].max()) == region
    else:
        assert cut_ports
        for p in cut_ports:  # the entries beyond the prefix say so, and keep their length and index
            k = int(want.ports[p]["frames_written"])
            assert (r.pkt_off_dw(p)[k:] == LM.NOT_WRITTEN).all() and (r.pkt_off_dw(p)[:k] != LM.NOT_WRITTEN).all()
    if cut == "nothing_fits":
        assert not want.ports["frames_written"].any()


def test_out_netif_at_and_above_n_netifs_goes_nowhere():
    n = 60
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, 64, dtype=np.uint8).tobytes() for _ in range(n)]
    from tests import arp_cases as K

    data, offs, lens = K.pack(rng, frames)
    results = np.zeros(n, C.ARP_RESULT_DTYPE)
    results["verdict"] = AM.LOOPBACK
    results["out_netif"] = [[0, 2, 3, 4, 63, 64, 255][i % 7] for i in range(n)]
    r, want = _run(frames, data, offs, lens, results, 3, 4096, n)
    assert [int(x) for x in want.ports["frames"]] == [9, 0, 9] and want.skipped == 0


def test_what_the_corpus_reaches():
    seen_mod, seen_len, seen_verdicts, seen_tx = set(), set(), set(), set()
    for n_netifs in (1, 4, 64):
        for tx in (False, True):
            for jumbo in (False, True):
                frames, _data, _offs, lens, results = C.mixed(9 + n_netifs, 600, n_netifs, tx, jumbo)
                netifs = LM.netifs_of_results(results, n_netifs)
                seen_verdicts |= set(results["verdict"].tolist())
                assert any(int(r["verdict"]) == AM.LOOPBACK and int(r["out_netif"]) >= n_netifs for r in results)
                sent = set()
                for f, p in zip(frames, netifs):
                    if p is None:
                        continue
                    sent.add(p)
                    pkt = LM.packet_of(f, tx, jumbo)
                    if tx and len(f) >= 34:
                        total = f[16] << 8 | f[17]
                        seen_tx.add("below" if total < len(f) - 14 else "equal" if total == len(f) - 14 else "above")
                    if pkt is not None and not tx:
                        seen_mod.add(len(pkt) % 4)
                        seen_len.add((len(f), jumbo))
                assert sent == {0, n_netifs // 2, n_netifs - 1}  # the first, one in the middle, the last
    assert seen_mod == {0, 1, 2, 3}
    assert {(x, False) for x in (34, 35, 36, 37, 60, 64, 1514)} <= seen_len and (9014, True) in seen_len
    assert (1515, False) not in seen_len and (9014, False) not in seen_len and (9015, True) not in seen_len
    assert seen_tx == {"below", "equal", "above"} and seen_verdicts == set(range(7))


def test_known_answer_canonical_udp_frame():
    """SURVEY.md §8's canonical 64-byte UDP frame (192.168.100.1:12345 -> 192.168.100.100:22222, TTL
    0x80, id 1, payload 00..15), re-addressed to a second NetIf's address 10.9.8.1 (IP checksum
    f103 -> 0407, UDP checksum c07a -> d37d, both re-derived by hand from the address words), after
    the TTL step of :134 (TTL 7f, IP checksum 0507): the LoChan packet of NetIf 1 is the frame's
    bytes 14-63, 50 bytes, followed by two zero bytes."""
    from oracle import ref_py as R

    received = bytes.fromhex("aaaaaaaaaaaa020000000001080045000032000100008011" "0407" "c0a86401" "0a090801"
                             "303956ce001e" "d37d" "000102030405060708090a0b0c0d0e0f101112131415")
    at_encap = bytes.fromhex("aaaaaaaaaaaa02000000000108004500003200010000" "7f11" "0507" "c0a86401" "0a090801"
                             "303956ce001e" "d37d" "000102030405060708090a0b0c0d0e0f101112131415")
    want_pkt = bytes.fromhex("4500003200010000" "7f11" "0507" "c0a86401" "0a090801" "303956ce001e" "d37d"
                             "000102030405060708090a0b0c0d0e0f101112131415")
    assert len(received) == len(at_encap) == 64 and len(want_pkt) == 50 and want_pkt == at_encap[14:64]
    # the frame verifies as received and the packet verifies as drained: the hand sums are right
    rec = R.rx_frame(received, bytes([0xAA] * 6), 0xC0A86464)
    assert rec["status"] == "OK" and rec["dst_ip"] == 0x0A090801
    assert R.engine_lo(want_pkt, 0x0A090801) == "LOCAL_UDP"
    results = np.zeros(1, C.ARP_RESULT_DTYPE)
    results[0] = (AM.LOOPBACK, 1, 0, 0)
    from halo_amd import loopback as L

    data = np.frombuffer(at_encap, np.uint8).copy()
    out = np.full(2 * 64, FILL, np.uint8)
    r = L.gather_host(data, np.zeros(1, np.uint32), np.full(1, 64, np.uint16), results, 2, 64, 4, out=out)
    assert r.ports.tolist() == [(0, 0, 0, 0), (1, 1, 52, 52)]
    assert bytes(r.out[64:64 + 50]) == want_pkt and bytes(r.out[64 + 50:64 + 52]) == b"\0\0"
    assert (r.out[:64] == FILL).all() and (r.out[64 + 52:] == FILL).all()
    assert r.pkt_off_dw(1).tolist() == [0] and r.pkt_len(1).tolist() == [50] and r.index(1).tolist() == [0]


def test_argument_errors():
    from halo_amd import _lib

    E, OK = _lib.HALO_E_INVAL, 0
    frames, data, offs, lens, results = C.mixed(1, 16, 2)
    n = 16
    out = np.zeros(2 * 4096, np.uint8)
    ports = np.zeros(2, _lib.EGRESS_PORT_DTYPE)
    off_a, len_a, idx_a = np.zeros((2, 8), np.uint32), np.zeros((2, 8), np.uint16), np.zeros((2, 8), np.uint32)
    skipped = np.zeros(1, np.uint32)

    def cfg(n_netifs=2, flags=0, region=4096, cap=8):
        c = _lib.LoConfig()
        c.n_netifs, c.flags, c.region_bytes, c.index_cap = n_netifs, flags, region, cap
        return c

    def call(c, **kw):
        a = dict(data=data, offs=offs, lens=lens, n=n, results=results, out=out, ports=ports, pkt_off=off_a, pkt_len=len_a,
                 index=idx_a, skipped=skipped)
        a.update(kw)
        return _raw_call(c, **a)

    assert call(cfg()) == OK
    assert call(None) == E and call(cfg(), ports=None) == E
    assert call(cfg(n_netifs=0)) == E and call(cfg(n_netifs=65)) == E
    for bad in (0x1, 0x4, 0x10, 0x200, 0x80000000):
        assert call(cfg(flags=bad)) == E, hex(bad)
    assert call(cfg(flags=_lib.HALO_LO_TX | _lib.HALO_RX_JUMBO_EXT)) == OK
    assert call(cfg(region=(1 << 34) + 16)) == E
    assert call(cfg(region=4095)) == OK  # the host loop takes any region
    assert call(cfg(), out=None) == E and call(cfg(region=0), out=None) == OK
    for name in ("data", "offs", "lens", "results"):
        assert call(cfg(), **{name: None}) == E, name
        assert call(cfg(), n=0, **{name: None}) == OK, name
    for name in ("pkt_off", "pkt_len", "index"):
        assert call(cfg(), **{name: None}) == E, name
        assert call(cfg(cap=0), **{name: None}) == OK, name
    assert call(cfg(), skipped=None) == OK

    class _Off:  # an address inside an array
        def __init__(self, a, by):
            self.ctypes = type("c", (), {"data": a.ctypes.data + by})

    big = np.zeros(1 << 15, np.uint8)
    assert call(cfg(), data=_Off(big, 2)) == E and call(cfg(), offs=_Off(big, 2)) == E and call(cfg(), lens=_Off(big, 1)) == E
    assert call(cfg(), results=_Off(big, 4)) == E and call(cfg(), ports=_Off(big, 4)) == E
    assert call(cfg(), pkt_off=_Off(big, 2)) == E and call(cfg(), pkt_len=_Off(big, 1)) == E
    assert call(cfg(), index=_Off(big, 2)) == E and call(cfg(), skipped=_Off(big, 2)) == E
    # n == 0 zeroes the summaries
    ports["frames"] = 9
    assert call(cfg(), n=0) == OK and not ports.view(np.uint8).any()
    # the device call: the same checks before a device is looked for, plus its own
    ws = np.zeros(64, np.uint64)
    L = _lib.lib

    def dcall(c, region_out=out, ws_=ws, wsb=None, **kw):
        a = dict(data=data, offs=offs, lens=lens, n=n, results=results, out=region_out, ports=ports, pkt_off=off_a,
                 pkt_len=len_a, index=idx_a, skipped=skipped)
        a.update(kw)
        need = int(L.halo_lo_gather_workspace(a["n"], c.n_netifs)) if c is not None else 0
        return L.halo_lo_gather_device(None if c is None else ctypes.byref(c), _lib.ptr(a["data"]), _lib.ptr(a["offs"]),
                                       _lib.ptr(a["lens"]), a["n"], _lib.ptr(a["results"]), _lib.ptr(a["out"]),
                                       _lib.ptr(a["ports"]), _lib.ptr(a["pkt_off"]), _lib.ptr(a["pkt_len"]), _lib.ptr(a["index"]),
                                       _lib.ptr(a["skipped"]), _lib.ptr(ws_), need if wsb is None else wsb, None)

    assert L.halo_lo_gather_workspace(1, 0) == 0 and L.halo_lo_gather_workspace(1, 65) == 0
    assert L.halo_lo_gather_workspace(0, 1) == 16 and L.halo_lo_gather_workspace(257, 3) == 16 * 2 * 3
    assert dcall(None) == E and dcall(cfg(region=4104)) == E and dcall(cfg(flags=0x1)) == E
    assert dcall(cfg(), ws_=None) == E and dcall(cfg(), wsb=8) == E and dcall(cfg(), ws_=_Off(big, 4)) == E
    assert dcall(cfg(), region_out=_Off(big, 8)) == E
    import torch

    if not torch.cuda.is_available():
        assert dcall(cfg()) == _lib.HALO_E_NODEV  # no CPU fallback behind the device call
        assert L.halo_arp_loopback_mark_device(None, None, 0, None, 0, None, None, None) == E
