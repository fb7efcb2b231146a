"""TEST INFRASTRUCTURE ONLY: KCP emit's crafted flush batches and the helpers its CPU and GPU tests
share — a builder of (entries, segment descriptors, payload) with the data placed at a chosen source
alignment, the crafted cases (tests run each alone and all in one batch), random batches, and the
bit-for-bit comparison of a call's prefilled outputs with tests/kcp_emit_model.py."""
from __future__ import annotations

import numpy as np

from tests import kcp_emit_model as M
from tests.kcp_cases import ACK, CONV, FILL, PUSH, WASK, WINS, rnd  # noqa: F401

SRC_IP, SRC_PORT = 0x0A000001, 22102


class Batch:
    """Entries, descriptors and payload of one emit call. A segment is (cmd, data) or (cmd, data,
    source alignment 0..3)."""

    def __init__(self):
        self.entries, self.segs, self.payload = [], [], bytearray(b"\xC3")  # offset 0 is never a segment's

    def _place(self, data: bytes, align=None) -> int:
        if align is not None:
            self.payload += b"\xC3" * ((align - len(self.payload)) % 4)
        at = len(self.payload)
        self.payload += data
        return at

    def seg(self, cmd, data=b"", align=None, **kw):
        x = np.zeros(1, M.SEG)[0]
        n = len(self.segs)
        x["dgram"], x["check"] = 0xDEAD0000 + n, 2  # ignored on input
        x["cmd"], x["frg"], x["wnd"], x["ts"], x["sn"], x["una"] = cmd, n % 7, 256 + n, 1000 + 3 * n, n, n // 2
        x["len"], x["data_off"] = len(data), self._place(data, align)
        for k, v in kw.items():
            x[k] = v
        self.segs.append(x)

    def gap(self, n=1):
        """descriptors no entry owns"""
        for _ in range(n):
            self.seg(PUSH, b"not sent")

    def kcp(self, segments, mtu=1400, conv=None, **kw):
        e = np.zeros(1, M.SESSION)[0]
        k = len(self.entries)
        e["conv"], e["first_seg"], e["n_segs"], e["mtu"] = CONV + k if conv is None else conv, len(self.segs), len(segments), mtu
        e["dst_ip"], e["dst_port"] = 0x0A000100 + k, 4000 + k
        for s in segments:
            self.seg(*s)
        for f, v in kw.items():
            e[f] = v
        self.entries.append(e)

    def enet(self, conn_type, session_id=0x01020304, conv=0x0A0B0C0D, enet_type=1234567890, **kw):
        e = np.zeros(1, M.SESSION)[0]
        k = len(self.entries)
        e["kind"], e["conn_type"], e["session_id"], e["enet_conv"], e["enet_type"] = M.ENET, conn_type, session_id, conv, enet_type
        e["first_seg"], e["dst_ip"], e["dst_port"] = len(self.segs), 0x0A000100 + k, 4000 + k
        for f, v in kw.items():
            e[f] = v
        self.entries.append(e)

    def arrays(self):
        """(sessions, segs, payload uint8 padded to whole dwords, payload_bytes)"""
        pay = np.frombuffer(bytes(self.payload) + bytes(-len(self.payload) % 4), np.uint8).copy()
        return (np.array(self.entries, M.SESSION) if self.entries else np.zeros(0, M.SESSION),
                np.array(self.segs, M.SEG) if self.segs else np.zeros(0, M.SEG), pay, len(self.payload))


def _ok(b):
    b.kcp([(PUSH, b"ok-data"), (ACK,)])


def crafted(mode):
    """[(name, fn(batch))] — each fn appends its entries."""
    H = M.overhead(mode)
    out = []
    out.append(("zero_segments", lambda b: b.kcp([])))
    # size + need == mtu stays in the datagram; == mtu + 1 splits
    out.append(("exact_fit", lambda b: b.kcp([(PUSH, rnd(1, 50)), (PUSH, rnd(2, 200 - 2 * H - 50))], mtu=200)))
    out.append(("one_over", lambda b: b.kcp([(PUSH, rnd(1, 50)), (PUSH, rnd(2, 200 - 2 * H - 50))], mtu=199)))
    out.append(("fifty_acks", lambda b: b.kcp([(ACK,)] * 50, mtu=1400)))  # H 28: one datagram of exactly 1400; H 32: 43 + 7
    out.append(("empty_push", lambda b: b.kcp([(PUSH, b"")])))
    out.append(("push_lengths", lambda b: b.kcp([(PUSH, rnd(10 + n, n)) for n in (1, 3, 4, 5, 31, 32, 33, 511, 512, 513, 1400 - H)])))
    out.append(("mtu_1472", lambda b: b.kcp([(PUSH, rnd(3, 1472 - H)), (ACK,)], mtu=1472)))
    out.append(("smallest_mtu", lambda b: b.kcp([(PUSH, b"z"), (ACK,), (PUSH, b"")], mtu=H + 1)))

    def alignments(b):  # the second segment's data: source alignment sa, destination alignment da (H % 4 == 0)
        for sa in range(4):
            for da in range(4):
                b.kcp([(ACK, rnd(da, da)), (PUSH, rnd(100 + 4 * sa + da, 37 + sa), sa), (PUSH, rnd(sa, 9 + da), (sa + 1) % 4), (WINS,)])
    out.append(("alignments", alignments))
    out.append(("non_push_with_data", lambda b: b.kcp([(ACK, rnd(5, 9)), (WASK, rnd(6, 2)), (WINS, rnd(7, 64)), (PUSH, rnd(8, 11))])))
    out.append(("any_cmd", lambda b: b.kcp([(0, b"abc"), (255, b""), (80, b"q")])))  # encode does not validate cmd
    out.append(("enet_types", lambda b: [b.enet(t, 100 + t, 200 + t, 300 + t) for t in range(4)]))

    def gaps(b):
        b.gap(2)
        b.kcp([(PUSH, rnd(20, 40))] * 3, mtu=150)
        b.gap(1)
        b.enet(1)
        b.gap(3)
        b.kcp([(ACK,), (PUSH, rnd(21, 5))])
    out.append(("gaps", gaps))
    out.append(("many_datagrams", lambda b: b.kcp([(PUSH, rnd(30 + i, 90 + i % 5), i % 4) for i in range(40)], mtu=256)))

    # each non-OK status alone (the tests run every case alone) and between OK entries
    def between(bad):
        def fn(b):
            _ok(b)
            bad(b)
            _ok(b)
            _ok(b)  # the entry behind one whose range ends past the list is held against that end: BAD_RANGE too
        return fn
    bads = {
        "seg_too_long": lambda b: b.kcp([(ACK,), (PUSH, rnd(40, 200 - H + 1))], mtu=200),
        "seg_too_long_first": lambda b: b.kcp([(PUSH, rnd(41, 1473 - H))], mtu=1472),
        "mtu_is_H": lambda b: b.kcp([(ACK,)], mtu=H),
        "mtu_below_H": lambda b: b.kcp([], mtu=3),
        "mtu_1473": lambda b: b.kcp([(PUSH, b"x")], mtu=1473),
        "mtu_65535": lambda b: b.kcp([(PUSH, b"x")], mtu=65535),
        "range_past_list": lambda b: b.kcp([(ACK,)], n_segs=0x7FFFFFFF),
        "range_wraps_u32": lambda b: b.kcp([(ACK,)], first_seg=0xFFFFFFFF, n_segs=2),
        "range_overlaps_previous": lambda b: (b.kcp([(ACK,), (ACK,), (ACK,)]), b.kcp([], first_seg=len(b.segs) - 1, n_segs=1)),
        "data_past_payload": lambda b: b.kcp([(ACK,), (PUSH, b"abcd")]) or b.segs[-1].__setitem__("data_off", 0xFFFFFFF0),
        "data_end_past_payload": lambda b: b.kcp([(PUSH, b"")]) or b.segs[-1].__setitem__("len", 0x7FFFFFFF),
        "enet_conn_type_4": lambda b: b.enet(4),
        "enet_with_segments": lambda b: (b.gap(1), b.enet(2, first_seg=len(b.segs) - 1, n_segs=1)),
        "kind_2": lambda b: b.kcp([(ACK,)], kind=2),
    }
    for name, bad in bads.items():
        out.append((name, bad))
        out.append((name + "_between", between(bad)))
    return out


def batch_of(cases) -> Batch:
    b = Batch()
    for _, fn in cases:
        fn(b)
    return b


def random_batch(seed, n_sessions, bad=0.0, max_segs=3) -> Batch:
    """n_sessions entries of 0..max_segs segments; a share `bad` of them non-OK, of every status."""
    rng = np.random.default_rng(seed)
    b = Batch()
    for k in range(n_sessions):
        r = rng.random()
        segs = [((PUSH, ACK, PUSH, WINS)[int(rng.integers(4))], rnd(seed + 31 * k + i, int(rng.integers(0, 90))), int(rng.integers(4)))
                for i in range(int(rng.integers(0, max_segs + 1)))]
        if r < bad:
            which = int(rng.integers(5))
            if which == 0:
                b.kcp(segs + [(PUSH, rnd(k, 200))], mtu=100)
            elif which == 1:
                b.kcp(segs, mtu=int(rng.choice([0, 28, 1473, 40000])))
            elif which == 2:
                b.enet(int(rng.integers(4, 256)))
            elif which == 3:
                b.kcp(segs + [(PUSH, b"abc")])
                b.segs[-1]["data_off"] = 0xFFFFFFFE
            else:
                b.kcp(segs, first_seg=max(len(b.segs) - 1, 0) if b.entries and b.entries[-1]["n_segs"] else 0xFFFFFF00)
        elif r < bad + 0.1:
            b.enet(k % 4, k, 2 * k, 3 * k)
        else:
            b.kcp(segs, mtu=int(rng.choice([122, 300, 1400])))  # 122 >= 32 + 89: every segment fits
        if rng.random() < 0.1:
            b.gap(1)
    return b


def want(arrays, mode, dgram_cap, stream_cap) -> M.Want:
    sessions, segs, pay, nbytes = arrays
    return M.want_of(sessions, segs, pay.tobytes()[:nbytes], mode=mode, src_ip=SRC_IP, src_port=SRC_PORT, dgram_cap=dgram_cap,
                     stream_cap=stream_cap)


def check_outputs(got, want: M.Want, n_sessions, dgram_cap, stream_cap, what=""):
    """got: dict(stream=[stream_cap + 8] u8, dgrams=[dgram_cap + 1, 16] u8, descs=[dgram_cap + 1, 40] u8,
    status=[n_sessions + 8] u8, summary=[88 + 8] u8), each 0xA5-prefilled with a sentinel behind it."""
    s = got["summary"][:88].view(M.SUMMARY)[0]
    for f in M.SUMMARY.names:
        assert np.array_equal(s[f], want.summary[f]), (what, f, s[f], want.summary[f])
    assert (got["summary"][88:] == FILL).all(), (what, "summary sentinel")
    assert np.array_equal(got["status"][:n_sessions], want.status), (what, "status", np.flatnonzero(got["status"][:n_sessions] != want.status)[:8])
    assert (got["status"][n_sessions:] == FILL).all(), (what, "status sentinel")
    nd, nb = int(s["dgrams_written"]), int(s["bytes_written"])
    assert nd == len(want.dgrams) <= dgram_cap and nb == len(want.stream) <= stream_cap, what
    d = got["dgrams"][:nd].reshape(-1).view(M.DGRAM)
    for f in M.DGRAM.names:
        assert np.array_equal(d[f], want.dgrams[f]), (what, "dgram", f, np.flatnonzero(d[f] != want.dgrams[f])[:5])
    x = got["descs"][:nd].reshape(-1).view(M.DESC)
    for f in M.DESC.names:
        assert np.array_equal(x[f], want.descs[f]), (what, "desc", f)
    assert got["dgrams"][:nd].tobytes() == want.dgrams.tobytes() and got["descs"][:nd].tobytes() == want.descs.tobytes(), what
    stream = got["stream"][:nb].tobytes()
    if stream != want.stream:
        bad = np.flatnonzero(np.frombuffer(stream, np.uint8) != np.frombuffer(want.stream, np.uint8))
        raise AssertionError((what, "stream", bad[:8], stream[bad[0] - 4:bad[0] + 8].hex(), want.stream[bad[0] - 4:bad[0] + 8].hex()))
    assert (got["dgrams"][nd:] == FILL).all() and (got["descs"][nd:] == FILL).all() and (got["stream"][nb:] == FILL).all(), \
        (what, "written beyond the prefixes")


def host_call(arrays, mode, dgram_cap, stream_cap, *, src_ip=SRC_IP, src_port=SRC_PORT):
    """halo_kcp_emit_host into 0xA5-filled outputs, straight through ctypes."""
    import ctypes

    from halo_amd import _lib

    sessions, segs, pay, nbytes = arrays
    cfg = _lib.KcpEmitConfig()
    cfg.byte_check_mode, cfg.src_ip, cfg.src_port, cfg.dgram_cap, cfg.stream_cap = mode, src_ip, src_port, dgram_cap, stream_cap
    got = dict(stream=np.full(stream_cap + 8, FILL, np.uint8), dgrams=np.full((dgram_cap + 1, 16), FILL, np.uint8),
               descs=np.full((dgram_cap + 1, 40), FILL, np.uint8), status=np.full(len(sessions) + 8, FILL, np.uint8),
               summary=np.full(88 + 8, FILL, np.uint8))
    rc = _lib.lib.halo_kcp_emit_host(ctypes.byref(cfg), _lib.ptr(sessions.view(np.uint8)) if len(sessions) else None, len(sessions),
                                     _lib.ptr(segs.view(np.uint8)) if len(segs) else None, len(segs), _lib.ptr(pay), nbytes,
                                     _lib.ptr(got["stream"]), _lib.ptr(got["dgrams"]), _lib.ptr(got["descs"]), _lib.ptr(got["status"]),
                                     _lib.ptr(got["summary"]))
    assert rc == 0, rc
    return got
