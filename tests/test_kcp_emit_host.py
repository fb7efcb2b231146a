"""CPU: KCP emit's host side (halo_amd/csrc/tx_kcp_host.cc through halo_kcp_emit_host) against
tests/kcp_emit_model.py, bit for bit into 0xA5-prefilled outputs with a sentinel behind each: the
crafted batches of tests/kcp_emit_cases.py in all four byte-check modes, all in one call and each
alone; random batches; capacity cuts by dgram_cap and by stream_cap inside an entry and exactly on
its boundary; every HALO_E_INVAL answer of both entry points; the round trip through KCP ingest's
host loop and tests/kcp_model.py; and the descriptors through the CPU transmit-build oracle."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import kcp_cases as KC
from tests import kcp_emit_cases as C
from tests import kcp_emit_model as M
from tests import kcp_model as KM


def _check(b, mode, dgram_cap, stream_cap, what=""):
    arrays = b.arrays() if isinstance(b, C.Batch) else b
    want = C.want(arrays, mode, dgram_cap, stream_cap)
    got = C.host_call(arrays, mode, dgram_cap, stream_cap)
    C.check_outputs(got, want, len(arrays[0]), dgram_cap, stream_cap, (what, mode))
    return want


@pytest.mark.parametrize("mode", M.MODES)
def test_crafted_set_in_one_call(mode):
    cases = C.crafted(mode)
    want = _check(C.batch_of(cases), mode, 4096, 1 << 20, "crafted")
    s = want.summary
    assert all(int(c) > 3 for c in s["status_counts"]) and int(s["sessions_written"]) == int(s["sessions"]) > 40
    assert int(s["dgrams"]) > 60 and (int(s["bytes_hashed"]) > 0) == (mode in (M.CRC32, M.XXH3))
    assert int(s["out_pkts"]) == int(s["dgrams_written"]) and int(s["out_segs"]) == int(s["segs_written"])
    # capacities that just fit, and the same batch with every segment's data one byte further on
    _check(C.batch_of(cases), mode, int(s["dgrams"]), int(s["bytes"]), "exact capacities")
    shifted = C.Batch()
    shifted.payload += b"\x00"
    for _, fn in cases:
        fn(shifted)
    _check(shifted, mode, 4096, 1 << 20, "shifted")


@pytest.mark.parametrize("mode", M.MODES)
def test_every_crafted_case_alone(mode):
    seen = set()
    for name, fn in C.crafted(mode):
        b = C.Batch()
        fn(b)
        want = _check(b, mode, 256, 1 << 16, name)
        seen |= {int(x) for x in want.status}
    assert seen == {0, 1, 2, 3}


def test_crafted_packing_is_what_the_issue_says():
    """The model's own answers on the packing edges, so that model and host cannot agree on a wrong rule."""
    for mode in M.MODES:
        H = M.overhead(mode)
        by = dict(C.crafted(mode))

        def dgrams(name):
            b = C.Batch()
            by[name](b)
            return C.want(b.arrays(), mode, 256, 1 << 16).dgrams

        assert [int(x) for x in dgrams("exact_fit")["len"]] == [200] and [int(x) for x in dgrams("one_over")["len"]] == [H + 50, 150 - H]
        assert [int(x) for x in dgrams("fifty_acks")["n_segs"]] == ([50] if H == 28 else [43, 7])
        assert len(dgrams("zero_segments")) == 0 and [int(x) for x in dgrams("empty_push")["len"]] == [H]
        assert [int(x) for x in dgrams("enet_types")["len"]] == [20] * 4


@pytest.mark.parametrize("seed,n,bad", [(1, 40, 0.0), (2, 300, 0.1), (3, 300, 0.5), (4, 700, 0.02)])
def test_random_batches(seed, n, bad):
    b = C.random_batch(seed, n, bad)
    for mode in M.MODES:
        want = _check(b, mode, 4 * n, 1 << 20, ("random", seed))
    if bad >= 0.1:
        assert all(int(c) for c in want.summary["status_counts"])


@pytest.mark.parametrize("mode", (M.DISABLED, M.CRC32))
def test_capacity_cuts(mode):
    b = C.Batch()
    for k in range(30):
        b.kcp([(KC.PUSH, KC.rnd(k, 60 + k % 3), k % 4)] * 3, mtu=200)  # two datagrams per entry
        if k % 5 == 0:
            b.kcp([(KC.ACK,)], mtu=20)  # non-OK: does not end the prefix
        if k % 7 == 0:
            b.enet(k % 4)
    arrays = b.arrays()
    full = C.want(arrays, mode, 1000, 1 << 20)
    nd, nb = int(full.summary["dgrams"]), int(full.summary["bytes"])
    assert nd == 60 + 5 and int(full.summary["sessions"]) == 35
    ends = np.cumsum([(int(d["len"]) + 3) & ~3 for d in full.dgrams])
    for dgram_cap in (0, 1, 2, 3, 4, 5, 31, 32, nd - 1, nd, nd + 1):  # inside an entry and on its boundary
        w = _check(arrays, mode, dgram_cap, 1 << 20, ("dgram_cap", dgram_cap))
        assert int(w.summary["dgrams"]) == nd and int(w.summary["dgrams_written"]) <= dgram_cap
    for stream_cap in (0, 3, 19, 20, int(ends[0]), int(ends[1]) - 1, int(ends[1]), int(ends[1]) + 1, int(ends[2]), int(ends[20]) + 2,
                       nb - 1, nb, nb + 1):
        w = _check(arrays, mode, 1000, stream_cap, ("stream_cap", stream_cap))
        assert int(w.summary["bytes"]) == nb and int(w.summary["bytes_written"]) <= stream_cap
    w = _check(arrays, mode, 7, int(ends[3]), "both")
    assert 0 < int(w.summary["sessions_written"]) < 35
    # an empty OK entry behind the cut is not written either; status counts stay totals
    assert int(w.summary["status_counts"][M.BAD_MTU]) == 6


def test_no_sessions_zeroes_the_summary():
    got = C.host_call(C.Batch().arrays(), M.CRC32, 4, 64)
    assert got["summary"][:88].tobytes() == bytes(88) and (got["stream"] == C.FILL).all() and (got["dgrams"] == C.FILL).all()


def entry_answers(fn_name, base, device):
    """The argument checks of halo_kcp_emit_device / _host over addresses from ``base`` (64-byte
    aligned, 4 KiB): [(what, answer)] of calls that each differ from a well-formed one in one
    argument. Nothing is dereferenced before the checks."""
    from halo_amd import _lib

    L = _lib.lib
    wsb = int(L.halo_kcp_emit_workspace(2, 3))
    assert wsb == ((12 * 1 + 12 * 2 + 7) & ~7) + ((36 * 3 + 7) & ~7)
    at = dict(sessions=base, segs=base + 128, payload=base + 256, stream=base + 512, dgrams=base + 1024, descs=base + 1280,
              status=base + 1792, summary=base + 1856, ws=base + 2048)

    def call(mode=1, src_port=C.SRC_PORT, dgram_cap=4, stream_cap=256, cfg_null=False, n_sessions=2, n_segs=3, ws_bytes=wsb, **ptr):
        a = {**at, **ptr}
        cfg = _lib.KcpEmitConfig()
        cfg.byte_check_mode, cfg.src_ip, cfg.src_port, cfg.dgram_cap, cfg.stream_cap = mode, 1, src_port, dgram_cap, stream_cap
        args = [None if cfg_null else ctypes.byref(cfg), a["sessions"], n_sessions, a["segs"], n_segs, a["payload"], 64, a["stream"],
                a["dgrams"], a["descs"], a["status"], a["summary"]]
        if device:
            args += [a["ws"], ws_bytes, None]
        return getattr(L, fn_name)(*args)

    bad = [dict(cfg_null=True), dict(summary=None), dict(mode=-2), dict(mode=3), dict(src_port=65536), dict(sessions=None),
           dict(status=None), dict(segs=None), dict(payload=None), dict(dgrams=None), dict(descs=None), dict(stream=None),
           dict(n_sessions=_lib.KCP_EMIT_MAX + 1), dict(n_segs=_lib.KCP_EMIT_MAX + 1)]
    if device:  # segs, dgrams 16; sessions, descs, summary, workspace 8; payload, stream 4
        bad += [dict(ws=None), dict(ws_bytes=wsb - 1), dict(segs=at["segs"] + 8), dict(dgrams=at["dgrams"] + 8),
                dict(sessions=at["sessions"] + 4), dict(descs=at["descs"] + 4), dict(summary=at["summary"] + 4), dict(ws=at["ws"] + 4),
                dict(payload=at["payload"] + 2), dict(stream=at["stream"] + 1)]
    return [(kw, call(**kw)) for kw in bad]


@pytest.mark.parametrize("fn,device", [("halo_kcp_emit_host", False), ("halo_kcp_emit_device", True)])
def test_every_inval_answer(fn, device):
    from halo_amd import _lib

    buf = np.zeros(4096 + 64, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 64
    answers = entry_answers(fn, base, device)
    assert len(answers) >= (24 if device else 14)
    for what, rc in answers:
        assert rc == _lib.HALO_E_INVAL, (what, rc)
    assert not buf.any()


@pytest.mark.parametrize("mode", M.MODES)
def test_round_trip_through_ingest_host(mode):
    """The emitted datagrams, wrapped as UDP deliveries, through halo_kcp_ingest_host and
    tests/kcp_model.py: every datagram returns 0, every PUSH is PASSED (NA when disabled), and the
    descriptors' cmd..len and data equal the input, per session in order."""
    from halo_amd import _lib

    cases = [(n, fn) for n, fn in C.crafted(mode) if n not in ("any_cmd",)]  # ingest's walk refuses a cmd outside 81..84
    sessions, segs, pay, nbytes = arrays = C.batch_of(cases).arrays()
    want = C.want(arrays, mode, 4096, 1 << 20)
    got = C.host_call(arrays, mode, 4096, 1 << 20)
    nd = int(want.summary["dgrams_written"])
    recs = got["dgrams"][:nd].reshape(-1).view(M.DGRAM)
    stream = got["stream"].tobytes()
    payloads = [stream[int(r["offset"]):int(r["offset"]) + int(r["len"])] for r in recs]
    d = KC.Delivery(KC.udp(payloads))
    cfg = _lib.KcpConfig()
    cfg.byte_check_mode, cfg.port, cfg.dgram_cap, cfg.seg_cap = mode, KC.PORT, nd, len(segs)
    dg = np.zeros((nd + 1, 40), np.uint8)
    sg = np.zeros((len(segs) + 1, 32), np.uint8)
    sm = np.zeros(96, np.uint8)
    assert _lib.lib.halo_kcp_ingest_host(ctypes.byref(cfg), _lib.ptr(d.out), _lib.ptr(d.summary_raw), _lib.ptr(d.index_raw), d.index_cap,
                                         _lib.ptr(dg), _lib.ptr(sg), _lib.ptr(sm)) == 0
    model = KM.want_of(d, port=KC.PORT, mode=mode, dgram_cap=nd, seg_cap=len(segs))
    isum = sm.view(KM.SUMMARY)[0]
    assert sm.tobytes() == model.summary.tobytes() and int(isum["dgrams_written"]) == nd
    assert int(isum["ret_counts"][0]) + int(isum["enet_counts"].sum()) == nd and int(isum["in_errs"]) == 0 and int(isum["ignored"]) == 0
    idg = dg[:nd].reshape(-1).view(KM.DGRAM)
    isg = sg[:int(isum["segs_written"])].reshape(-1).view(KM.SEG)
    assert dg[:nd].tobytes() == model.dgrams.tobytes() and isg.tobytes() == model.segs.tobytes()
    back = d.stream().tobytes()
    for j, r in enumerate(recs):
        e = sessions[int(r["session"])]
        if e["kind"] == M.ENET:
            assert int(idg[j]["kind"]) == 1 and int(idg[j]["conn_type"]) == int(e["conn_type"])
            assert (int(idg[j]["session_id"]), int(idg[j]["conv"]), int(idg[j]["enet_type"])) == \
                (int(e["session_id"]), int(e["enet_conv"]), int(e["enet_type"]))
            continue
        assert int(idg[j]["ret"]) == 0 and int(idg[j]["conv0"]) == int(e["conv"]) and int(idg[j]["n_segs"]) == int(r["n_segs"])
        for i in range(int(r["n_segs"])):
            a, x = segs[int(r["first_seg"]) + i], isg[int(idg[j]["first_seg"]) + i]
            for f in ("cmd", "frg", "wnd", "ts", "sn", "una", "len"):
                assert int(a[f]) == int(x[f]), (j, i, f)
            assert int(x["check"]) == (1 if a["cmd"] == KC.PUSH and mode != M.DISABLED else 0), (j, i)
            assert back[int(x["data_off"]):int(x["data_off"]) + int(x["len"])] == \
                pay.tobytes()[int(a["data_off"]):int(a["data_off"]) + int(a["len"])], (j, i)
    assert int(isum["segs_written"]) == int(want.summary["segs_written"])


def test_descs_through_the_build_oracle():
    """The descriptors and the stream handed to the CPU transmit build (the tx oracle): every frame's
    UDP payload is the datagram, its ports and addresses the entry's."""
    from oracle import oracle

    mode = M.CRC32
    arrays = C.batch_of(C.crafted(mode)).arrays()
    got = C.host_call(arrays, mode, 4096, 1 << 20)
    s = got["summary"][:88].view(M.SUMMARY)[0]
    nd = int(s["dgrams_written"])
    desc = got["descs"][:nd].reshape(-1).view(M.DESC)
    stream = got["stream"][:int(s["bytes_written"])]
    frames, lens, res, _ = oracle.tx_build_batch(desc, stream, bytes.fromhex("020000000001"), 1, 1516, 7)
    assert not res.any() and nd > 60
    recs = got["dgrams"][:nd].reshape(-1).view(M.DGRAM)
    for j in range(nd):
        n = int(recs[j]["len"])
        f = frames[j].tobytes()
        assert int(lens[j]) == max(42 + n, 60)
        assert f[42:42 + n] == stream.tobytes()[int(recs[j]["offset"]):int(recs[j]["offset"]) + n], j
        e = arrays[0][int(recs[j]["session"])]
        assert f[23] == 17 and int.from_bytes(f[26:30], "big") == C.SRC_IP and int.from_bytes(f[30:34], "big") == int(e["dst_ip"])
        assert int.from_bytes(f[34:36], "big") == C.SRC_PORT and int.from_bytes(f[36:38], "big") == int(e["dst_port"])
        assert int.from_bytes(f[38:40], "big") == 8 + n


def test_python_wrapper_and_relay_helper():
    from halo_amd import _lib, kcp

    mode = M.XXH3
    sessions, segs, pay, nbytes = arrays = C.batch_of(C.crafted(mode)[:12]).arrays()
    r = kcp.emit_host(sessions, segs, pay[:nbytes], byte_check_mode="xxh3", src_ip=C.SRC_IP, src_port=C.SRC_PORT, dgram_cap=512,
                      stream_cap=1 << 16)
    want = C.want(arrays, mode, 512, 1 << 16)
    assert r.summary.tobytes() == want.summary.tobytes() and np.array_equal(r.status, want.status)
    assert r.dgrams().tobytes() == want.dgrams.tobytes() and r.descs().tobytes() == want.descs.tobytes()
    assert r.datagrams() == [want.stream[int(d["offset"]):int(d["offset"]) + int(d["len"])] for d in want.dgrams]
    assert _lib.KCP_OUT_SESSION_DTYPE == M.SESSION and _lib.KCP_OUT_DGRAM_DTYPE == M.DGRAM and _lib.KCP_EMIT_SUMMARY_DTYPE == M.SUMMARY
    with pytest.raises(ValueError):
        r.build(None, netif=None)
    # sessions_of, and an ingest result relayed: the emitted datagrams ingested, their segments emitted again
    d = KC.Delivery(KC.udp(r.datagrams()))
    ing = kcp.ingest_host(d, port=KC.PORT, byte_check_mode=mode, seg_cap=len(segs), dgram_cap=len(want.dgrams))
    rsegs, ranges = kcp.relay_segments(ing)
    ents = kcp.sessions_of([dict(conv=int(ing.dgrams[j]["conv0"]), n_segs=n, mtu=1472, dst_ip=9, dst_port=10) for j, _, n in ranges]
                           + [dict(conn_type="ConnEnetFin", session_id=1, enet_conv=2, enet_type=3, dst_ip=9, dst_port=10)])
    again = kcp.emit_host(ents, rsegs, d.stream(), byte_check_mode=mode, src_ip=1, src_port=2, dgram_cap=512, stream_cap=1 << 16)
    assert not again.status.any() and int(again.summary["segs_written"]) == len(rsegs)
    kcp_dgrams = [p for p, g in zip(r.datagrams(), ing.dgrams) if int(g["kind"]) == 0 and int(g["ret"]) == 0]
    assert len(kcp_dgrams) > 10 and len(kcp_dgrams) < len(ing.dgrams)  # any_cmd's datagram is refused by Input (ret -3) and not relayed
    assert again.datagrams()[:-1] == kcp_dgrams and again.datagrams()[-1] == KC.enet(2, 1, 2, 3)
