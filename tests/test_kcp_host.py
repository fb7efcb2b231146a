"""CPU: KCP ingest's host loop (halo_kcp_ingest_host, halo_amd/csrc/rx_kcp_host.cc, through
halo_amd.kcp) against tests/kcp_model.py bit for bit, into 0xA5-prefilled outputs with a sentinel
element behind each: every crafted datagram of tests/kcp_cases.py in all four byte-check modes,
selection among other kinds and ports and unwritten records, capacity cuts, every HALO_E_INVAL
answer, the host byte checks against zlib and the XXH3 oracle, and ``feed`` against the model's
list."""
from __future__ import annotations

import ctypes
import zlib

import numpy as np
import pytest

from tests import kcp_cases as C
from tests import kcp_model as M


def _host(delivery, mode, dgram_cap, seg_cap, *, port=C.PORT, index_cap=None):
    from halo_amd import _lib

    cfg = _lib.KcpConfig()
    cfg.byte_check_mode, cfg.port, cfg.dgram_cap, cfg.seg_cap = mode, port, dgram_cap, seg_cap
    dg = np.full((dgram_cap + 1, 40), C.FILL, np.uint8)
    sg = np.full((seg_cap + 1, 32), C.FILL, np.uint8)
    sm = np.full(96 + 8, C.FILL, np.uint8)
    cap = delivery.index_cap if index_cap is None else index_cap
    rc = _lib.lib.halo_kcp_ingest_host(ctypes.byref(cfg), _lib.ptr(delivery.out), _lib.ptr(delivery.summary_raw),
                                       _lib.ptr(delivery.index_raw), cap, _lib.ptr(dg), _lib.ptr(sg), _lib.ptr(sm))
    assert rc == 0, rc
    return dict(dgrams=dg, segs=sg, summary=sm)


def _check(delivery, mode, dgram_cap, seg_cap, what="", **kw):
    want = M.want_of(delivery, port=kw.get("port", C.PORT), mode=mode, dgram_cap=dgram_cap, seg_cap=seg_cap, index_cap=kw.get("index_cap"))
    C.check_outputs(_host(delivery, mode, dgram_cap, seg_cap, **kw), want, dgram_cap, seg_cap, (what, mode))
    return want


@pytest.mark.parametrize("mode", M.MODES)
def test_crafted_set_matches_model(mode):
    cases = C.crafted(mode)
    d = C.Delivery(C.udp([p for _, p in cases]))
    want = _check(d, mode, len(cases), 8192, "all")
    s = want.summary
    assert s["ignored"] >= 8 and list(s["enet_counts"]) == [1, 1, 1, 1]
    assert all(int(c) > 0 for c in s["ret_counts"][:4]) and (int(s["ret_counts"][4]) > 0) == (mode != M.DISABLED)
    assert (int(s["bytes_hashed"]) > 65507 - 32) == (mode in (M.CRC32, M.XXH3))  # more than the big segment
    assert (int(s["bytes_hashed"]) == 0) == (mode in (M.DISABLED, M.ZERO))
    by = {name: i for i, (name, _) in enumerate(cases)}
    rec = {int(x["index"]): x for x in want.dgrams}
    assert int(rec[by["conv_changes"]]["ret"]) == -1 and int(rec[by["conv_changes"]]["n_segs"]) == 1
    assert int(rec[by["length_past"]]["ret"]) == -2 and int(rec[by["cmd80"]]["ret"]) == -3 and int(rec[by["short_tail"]]["ret"]) == 0
    assert int(rec[by["ack_garbage_field"]]["ret"]) == 0 and int(rec[by["ack_garbage_field"]]["n_segs"]) == 3
    assert int(rec[by["many_empty_segments"]]["n_segs"]) == 2040 and int(rec[by["one_big_segment"]]["n_segs"]) == 1
    if mode != M.DISABLED:
        assert (int(rec[by["bad_hash_1st"]]["ret"]), int(rec[by["bad_hash_1st"]]["n_segs"]), int(rec[by["bad_hash_1st"]]["n_walked"])) == (-4, 0, 2)
        assert (int(rec[by["bad_hash_2nd"]]["ret"]), int(rec[by["bad_hash_2nd"]]["n_segs"]), int(rec[by["bad_hash_2nd"]]["n_walked"])) == (-4, 1, 4)
        assert int(rec[by["zero_mode_nonzero_field"]]["ret"]) == -4 and int(rec[by["empty_push_bad_field"]]["ret"]) == -4
        assert int(rec[by["empty_push"]]["ret"]) == 0 and int(rec[by["mtu"]]["ret"]) == 0
    # each case alone, so that none hides behind another
    for name, p in cases:
        _check(C.Delivery(C.udp([p])), mode, 1, 2100, name)


@pytest.mark.parametrize("mode", (M.DISABLED, M.CRC32))
def test_selection_other_kinds_ports_unwritten_and_index_cap(mode):
    ps = [p for _, p in C.crafted(mode)][:40]
    items = []
    for i, p in enumerate(ps):
        items.append((C.UDP, C.PORT, p))
        items.append(((C.TCP, C.PORT, p), (C.DHCP, 67, p), (C.UDP, C.PORT + 1, p), (C.UDP, 0, p))[i % 4])
    d = C.Delivery(items, unwritten=9)
    want = _check(d, mode, len(items), 4096, "interleaved")
    assert [int(x) for x in want.dgrams["index"]] == sorted(set(int(x) for x in want.dgrams["index"])) and all(
        int(x) % 2 == 0 for x in want.dgrams["index"])
    _check(d, mode, len(items), 4096, "other port", port=C.PORT + 1)
    assert len(_check(d, mode, len(items), 4096, "no such port", port=9).dgrams) == 0
    for cap in (0, 1, 7, len(items), len(items) + 3):
        _check(d, mode, len(items), 4096, ("index_cap", cap), index_cap=cap)
    empty = C.Delivery([], unwritten=0)
    assert int(_check(empty, mode, 4, 4, "empty").summary["dgrams"]) == 0


@pytest.mark.parametrize("mode", (M.ZERO, M.XXH3))
def test_capacity_cuts(mode):
    ps = [C.seg(mode, C.ACK) * 3, C.enet(0), C.seg(mode, C.PUSH, b"x" * 9) * 5, C.seg(mode, C.PUSH, b"bad", field=3) + C.seg(mode, C.ACK),
          C.enet(2), C.seg(mode, C.ACK) * 2]
    d = C.Delivery(C.udp(ps))
    # walked segments per datagram: 3, 0, 5, 2, 0, 2
    for dgram_cap, seg_cap, n in ((6, 12, 6), (6, 11, 5), (6, 10, 5), (6, 9, 3), (6, 8, 3), (6, 7, 2), (6, 3, 2), (6, 2, 0), (0, 12, 0),
                                  (1, 12, 1), (3, 12, 3), (5, 100, 5), (6, 0, 0)):
        want = _check(d, mode, dgram_cap, seg_cap, (dgram_cap, seg_cap))
        assert len(want.dgrams) == n and int(want.summary["dgrams"]) == 6 and int(want.summary["segs"]) == 12


def test_invalid_arguments():
    from halo_amd import _lib

    d = C.Delivery(C.udp([C.enet(0)]))
    dg, sg, sm = np.zeros((2, 40), np.uint8), np.zeros((2, 32), np.uint8), np.zeros(96, np.uint8)

    def call(mode=1, port=C.PORT, dgram_cap=1, seg_cap=1, out=d.out, dsum=d.summary_raw, index=d.index_raw, cap=1, dgrams=dg, segs=sg,
             summary=sm, cfg_null=False):
        cfg = _lib.KcpConfig()
        cfg.byte_check_mode, cfg.port, cfg.dgram_cap, cfg.seg_cap = mode, port, dgram_cap, seg_cap
        return _lib.lib.halo_kcp_ingest_host(None if cfg_null else ctypes.byref(cfg), _lib.ptr(out), _lib.ptr(dsum), _lib.ptr(index), cap,
                                             _lib.ptr(dgrams), _lib.ptr(segs), _lib.ptr(summary))

    assert call() == 0
    for bad in (dict(cfg_null=True), dict(summary=None), dict(dsum=None), dict(mode=-2), dict(mode=3), dict(port=65536), dict(out=None),
                dict(index=None), dict(dgrams=None), dict(segs=None)):
        assert call(**bad) == _lib.HALO_E_INVAL, bad
    # what a zero capacity excuses
    assert call(out=None, index=None, cap=0) == 0 and call(dgrams=None, dgram_cap=0) == 0 and call(segs=None, seg_cap=0) == 0
    assert int(_lib.lib.halo_kcp_ingest_workspace(1, 1)) == 32 and int(_lib.lib.halo_kcp_ingest_workspace(257, 10)) == 16 + 240


def test_device_entry_checks_every_argument_before_any_device_call():
    """Every HALO_E_INVAL answer of halo_kcp_ingest_device — nulls, mode, port, the workspace size
    and one misaligned address per documented alignment — over 64-byte-aligned host addresses: the
    checks come before any device is looked for. A well-formed call is not INVAL: without a device
    it is HALO_E_NODEV (with one, tests/test_gpu_kcp.py sends the same calls over device memory,
    where the well-formed one runs)."""
    import torch

    from halo_amd import _lib

    buf = np.zeros(4096 + 64, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 64
    # with a device, a well-formed call would launch kernels over host memory: only the rejected ones are sent
    ok, answers = C.device_entry_answers(base, send_well_formed=not torch.cuda.is_available())
    assert ok in (None, _lib.HALO_E_NODEV), ok
    assert len(answers) >= 22
    for what, rc in answers:
        assert rc == _lib.HALO_E_INVAL, (what, rc)


def test_host_byte_checks_match_zlib_and_the_xxh3_oracle():
    """The hash field the host loop accepts is zlib.crc32's / the oracle's, for lengths of every XXH3
    class: a PUSH segment encoded with the model's hash passes, and fails with one bit flipped."""
    for mode in (M.CRC32, M.XXH3):
        lens = [0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 96, 97, 128, 129, 240, 241, 1023, 1024, 1025, 2048, 2049, 4000]
        good = [C.seg(mode, C.PUSH, C.rnd(n, n)) for n in lens]
        bad = [C.seg(mode, C.PUSH, C.rnd(n, n), field=M.byte_check_hash(mode, C.rnd(n, n)) ^ 1 << (n % 32)) for n in lens]
        want = _check(C.Delivery(C.udp(good + bad)), mode, 2 * len(lens), 2 * len(lens))
        assert list(want.dgrams["ret"]) == [0] * len(lens) + [-4] * len(lens)
    assert M.byte_check_hash(M.CRC32, b"123456789") == 0xCBF43926 == zlib.crc32(b"123456789")


@pytest.mark.parametrize("mode", M.MODES)
def test_feed_matches_the_models_list(mode):
    from halo_amd import kcp

    cases = C.crafted(mode)
    d = C.Delivery(C.udp([p for _, p in cases]))
    want = M.want_of(d, port=C.PORT, mode=mode, dgram_cap=len(cases), seg_cap=8192)
    r = kcp.ingest_host(d, port=C.PORT, byte_check_mode=mode, seg_cap=8192, dgram_cap=len(cases))
    assert C.feed_log(r) == want.feed and len(want.feed) == int(r.summary["dgrams_written"]) > 20
    j = [int(x["index"]) for x in r.dgrams].index([n for n, _ in cases].index("mixed"))
    assert [int(s["cmd"]) for s in r.segments_of(j)] == [82, 81, 83, 81, 84]
    by_name = kcp.ingest_host(d, port=C.PORT, byte_check_mode={-1: "disabled", 0: "zero", 1: "crc32", 2: "xxh3"}[mode], seg_cap=8192,
                              dgram_cap=len(cases))
    assert by_name.summary == r.summary
    d.index_raw = None  # a delivery made without an index cannot be ingested
    with pytest.raises(ValueError):
        kcp.ingest_host(d, port=C.PORT, byte_check_mode=mode, seg_cap=8, dgram_cap=8)
