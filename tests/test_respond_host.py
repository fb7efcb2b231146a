"""CPU: the local responders' host side (halo_amd/csrc/tx_respond_host.cc over tx_respond.h and
rx_dispatch.h) against tests/respond_model.py, which works from frame bytes: hand-written known
answers; every golden frame under the four flag words with and without nat_enable, the golden
LoChan packets, the structured fuzz corpus and the crafted frames of tests/respond_cases.py, with
synthetic nat / ops / result inputs in every "input absent" combination and every output prefilled
and compared whole; `cap` below, at and above the count; the reply frames built from the host's
descriptors parsed as the peer sees them; and the device entry points' argument checks, which are
answered before any device is looked for."""
from __future__ import annotations

import itertools
import os

import numpy as np
import pytest

from oracle import ref_py as R
from oracle import ref_tx_py as T
from tests import respond_cases as C
from tests import respond_model as RM
from tests.helpers import expected_records, golden_arrays, lo_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = C.FILL


def _records(frames, nif, flags=1, l3=False):
    """The records of `frames`, from the Python restatement of the rx path."""
    from halo_amd._lib import RESULT_DTYPE
    from halo_amd.protocol import STATUS_NAMES

    out = np.zeros(len(frames), RESULT_DTYPE)
    for i, f in enumerate(frames):
        r = (R.rx_lo_packet(f, nif.ip, bool(flags & 1), bool(flags & 2)) if l3
             else R.rx_frame(f, nif.mac, nif.ip, bool(flags & 1), bool(flags & 2)))
        for k, v in r.items():
            out[i][k] = STATUS_NAMES.index(v) if k == "status" else v
    return out


def _host(offs, lens, recs, nat_enable, *, nat=None, steps=None, result=None, ports=None, cap=None, l3=False, kc0=9):
    """halo_tx_respond_host into 0xA5-filled outputs, straight through ctypes: a dict of the raw
    output arrays (each with slack behind it) and the count."""
    from halo_amd import _lib
    from halo_amd.respond import tcp_port_map

    n = len(lens)
    cap = n if cap is None else cap
    o = dict(desc=np.full((cap + 2, 40), FILL, np.uint8), src=np.full((cap + 2, 8), FILL, np.uint8),
             dst_ip=np.full(cap + 2, 0xA5A5A5A5, np.uint32), count=np.full(2, 0xA5A5A5A5, np.uint32),
             kinds=np.full(5, kc0, np.uint32), actions=np.full(n + 2, FILL, np.uint8))
    ops = None if steps is None else C.ops_array(steps)
    pm = None if ports is None else tcp_port_map(ports)
    rc = _lib.lib.halo_tx_respond_host(
        _lib.ptr(offs), _lib.ptr(lens), _lib.ptr(recs), n, _lib.HALO_RX_L3_START if l3 else 0, C.lib_netif(nat_enable),
        _lib.ptr(nat), _lib.ptr(ops), _lib.ptr(result), _lib.ptr(pm), _lib.ptr(o["desc"]), _lib.ptr(o["src"]),
        _lib.ptr(o["dst_ip"]), cap, _lib.ptr(o["count"]), _lib.ptr(o["kinds"]), _lib.ptr(o["actions"]))
    assert rc == 0, rc
    o.update(cap=cap, n=n, kc0=kc0)
    return o


check_outputs = C.check_outputs


# ---- known answers, literal bytes ------------------------------------------------------------------
ECHO_REQ = bytes.fromhex(
    "aaaaaaaaaaaa02112233445508004500" "005400070000400130e6c0a86407c0a8" "64640800eeb712340001" + bytes(range(56)).hex())
ECHO_REPLY = bytes.fromhex(
    "021122334455aaaaaaaaaaaa08004500" "0054000100008001f0ebc0a86464c0a8" "64070000f6b712340001" + bytes(range(56)).hex())
UDP_TTL1 = bytes.fromhex(
    "aaaaaaaaaaaa02112233445508004500" "002c00070000011184fbc0a864070808" "080813880035001895d9747261636572"
    "6f7574652d70726f62650000")
TTL_EXCEEDED = bytes.fromhex(
    "021122334455aaaaaaaaaaaa08004500" "0038000100008001f107c0a86464c0a8" "64070b004b5100000000"
    "4500002c00070000011184fbc0a864070808080813880035001895d9")
TCP_SYN = bytes.fromhex(
    "aaaaaaaaaaaa02112233445508004500" "0028000700004006310dc0a86407c0a8" "64649c400050000003e8000000635002"
    "0100c44a0000000000000000")
TCP_SYNACK = bytes.fromhex(
    "021122334455aaaaaaaaaaaa08004500" "0028000100008006f112c0a86464c0a8" "640700509c40499602d2000003e95012"
    "010078340000000000000000")


def _ones_add(a, b):
    s = a + b
    return (s & 0xFFFF) + (s >> 16)


@pytest.mark.parametrize("name, frame, kw, kind, payload, want", [
    ("echo", ECHO_REQ, {}, RM.ECHO, (42, 56), ECHO_REPLY),
    ("ttl", UDP_TTL1, dict(steps=[0x0A], result=[0]), RM.TTL, (14, 28), TTL_EXCEEDED),
    ("syn", TCP_SYN, dict(ports=[80]), RM.TCP_SYN, (0, 0), TCP_SYNACK),
])
def test_known_answers(name, frame, kw, kind, payload, want):
    from halo_amd._lib import BUILD_DESC_DTYPE, RESPOND_SRC_DTYPE

    assert len(ECHO_REQ) == 98 and len(TTL_EXCEEDED) == 70
    nif = C.model_netif()
    lead = 8  # the frame does not start the buffer: payload_off is absolute
    data = np.frombuffer(bytes(lead) + frame, np.uint8)
    offs, lens = np.array([lead // 4], np.uint32), np.array([len(frame)], np.uint16)
    kw = {k: np.array(v, np.uint8) if k != "ports" else v for k, v in kw.items()}
    o = _host(offs, lens, _records([frame], nif), False, **kw)
    assert int(o["count"][0]) == 1
    d = o["desc"].reshape(-1).view(BUILD_DESC_DTYPE)[0]
    s = o["src"].reshape(-1).view(RESPOND_SRC_DTYPE)[0]
    assert (int(s["index"]), int(s["kind"])) == (0, kind) and bytes(s["pad"]) == bytes(3)
    assert (int(d["payload_off"]), int(d["payload_len"])) == (lead + payload[0], payload[1])
    assert bytes(d["dst_mac"]) == bytes(6) and int(d["mode"]) == 0 and int(d["pad"]) == 0
    assert int(d["src_ip"]) == C.OWN_IP and int(d["dst_ip"]) == C.PEER == int(o["dst_ip"][0])
    desc = {f: int(d[f]) for f in RM.DESC_FIELDS}
    desc.update(dst_mac=C.PEER_MAC, mode=0)  # what TxIpv4's ARP step would find
    po = int(d["payload_off"])
    res, built = T.tx_build(desc, data[po:po + payload[1]].tobytes(), C.MAC, T.IphId(0))
    assert res == 0 and built == want, (built.hex(), want.hex())
    if name == "echo":  # type 8 -> 0 and nothing else: the checksum moves by 0x0800
        assert R.be16(want[36:38]) == _ones_add(R.be16(frame[36:38]), 0x0800)
    if name == "syn":
        assert int(d["seq"]) == 1234567890 and int(d["ack"]) == 1001 and int(d["aux"]) == 0x12


# ---- host == model -----------------------------------------------------------------------------------
def _synthetic(n, seed):
    rng = np.random.default_rng(seed)
    nat = rng.choice(np.array([0, 1, 2, 2, 3, 4, 5], np.uint8), n)
    steps = rng.integers(0, 32, n, dtype=np.uint8)
    result = rng.integers(0, 8, n, dtype=np.uint8)
    return nat, steps, result


def _compare(frames, offs, lens, recs, nat_enable, nat, steps, result, ports, flags=1, l3=False, cap=None, what=""):
    nif = C.model_netif(nat_enable)
    want = RM.respond(frames, offs, nif, nat=nat, fix=None if steps is None else (steps, result),
                      tcp_ports=() if ports is None else ports, check_sum_enable=bool(flags & 1), jumbo=bool(flags & 2), l3=l3)
    o = _host(offs, lens, recs, nat_enable, nat=nat, steps=steps, result=result, ports=ports, cap=cap, l3=l3)
    check_outputs(o, want, what)
    return want


@pytest.mark.parametrize("nat_enable", [False, True])
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_golden_frames(golden, flags, nat_enable):
    from halo_amd._lib import RESULT_DTYPE
    from halo_amd.engine import dispatch

    meta, blob = golden
    data, offs, lens, names = golden_arrays(meta, blob)
    frames = [bytes(data[4 * int(o):4 * int(o) + int(ln)]) for o, ln in zip(offs, lens)]
    recs = expected_records(meta, flags, RESULT_DTYPE)
    ports = sorted({int(p) for p in recs["dport"][recs["ip_proto"] == 6] if p % 2 == 0})
    assert ports
    nat, steps, result = _synthetic(len(frames), 100 + flags)
    want = _compare(frames, offs, lens, recs, nat_enable, nat, steps, result, ports, flags, what=f"golden {flags}")
    assert np.array_equal(want.actions, dispatch(recs, C.lib_netif(nat_enable)))
    assert want.count > 0


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_golden_lochan_packets(flags):
    from halo_amd._lib import RESULT_DTYPE
    from halo_amd.engine import dispatch_loopback

    meta, blob = lo_golden(ROOT)
    data, offs, lens, names = golden_arrays(meta, blob, key="packets")
    pkts = [bytes(data[4 * int(o):4 * int(o) + int(ln)]) for o, ln in zip(offs, lens)]
    recs = expected_records(meta, flags, RESULT_DTYPE, key="packets")
    ports = sorted({int(p) for p in recs["dport"][recs["ip_proto"] == 6] if p % 2 == 0})
    nat, steps, result = _synthetic(len(pkts), 200 + flags)  # given, and never consulted: only LOCAL_* rows apply
    for nat_enable in (False, True):
        want = _compare(pkts, offs, lens, recs, nat_enable, nat, steps, result, ports, flags, l3=True, what=f"lo {flags}")
        assert np.array_equal(want.actions, dispatch_loopback(recs, C.lib_netif(nat_enable)))
        assert want.kind_counts[RM.TTL] == 0 and want.kind_counts[RM.ECHO] > 0


ABSENT = list(itertools.product([False, True], repeat=3))  # nat, ops / result, ports: given or not


@pytest.fixture(scope="module")
def fuzz(oracle_lib):
    """A few thousand frames of the structured fuzz corpus followed by the crafted frames, with
    records from the C restatement of the rx path."""
    nif = oracle_lib.NetIf.make()
    data, offs, lens = oracle_lib.fuzz_batch(0xF00D, 3000, nif)
    frames = [bytes(data[4 * int(o):4 * int(o) + int(ln)]) for o, ln in zip(offs, lens)]
    cases = C.crafted() * 3
    cf, cnat, csteps, cresult = C.columns(cases)
    cdata, coffs, clens = C.pack(5, cf)
    base = (len(data) + 3) // 4
    data = np.concatenate([data, np.zeros(4 * base - len(data), np.uint8), cdata])
    offs = np.concatenate([offs, (coffs + base).astype(np.uint32)])
    lens = np.concatenate([lens, clens])
    nat, steps, result = _synthetic(3000, 77)
    recs = {en: oracle_lib.rx_batch(data, lens, oracle_lib.NetIf.make(nat_enable=en), 1, offsets_dw=offs)[0] for en in (False, True)}
    assert np.array_equal(recs[False].view(np.uint8), recs[True].view(np.uint8))  # records do not read nat_enable
    return dict(frames=frames + cf, data=data, offs=offs, lens=lens, recs=recs[False], nat=np.concatenate([nat, cnat]),
                steps=np.concatenate([steps, csteps]), result=np.concatenate([result, cresult]),
                names=["fuzz"] * 3000 + [c[0] for c in cases])


@pytest.mark.parametrize("nat_enable", [False, True])
@pytest.mark.parametrize("given", ABSENT)
def test_fuzz_corpus_every_input_combination(fuzz, given, nat_enable):
    from halo_amd.engine import dispatch

    g_nat, g_fix, g_ports = given
    f = fuzz
    want = _compare(f["frames"], f["offs"], f["lens"], f["recs"], nat_enable, f["nat"] if g_nat else None,
                    f["steps"] if g_fix else None, f["result"] if g_fix else None, C.SERVED if g_ports else None,
                    what=f"fuzz {given} {nat_enable}")
    assert np.array_equal(want.actions, dispatch(f["recs"], C.lib_netif(nat_enable)))
    kc = want.kind_counts
    if not g_fix:
        assert kc[RM.TTL] == 0
    if not g_ports:
        assert kc[RM.TCP_SYN] == 0 and kc[RM.TCP_SYNACK] == 0
    if g_nat and g_fix and g_ports:  # every kind occurs; a NATing NetIf forwards what is addressed to it
        assert np.all(kc > 0) if not nat_enable else (kc[RM.ECHO] > 0 and kc[RM.TTL] > 0), kc


def test_corpus_holds_what_it_must(fuzz):
    """Checked with the model alone: every kind, the NAT-miss ICMP fallback, a WAN miss that is not
    ICMP, an unserved port, a SYN|ACK and the ack wrap are in the corpus and behave as named."""
    by_name = {c[0]: c for c in C.crafted()}
    assert set(C.MUST) <= set(fuzz["names"])
    for name, (nat_enable, kind) in C.MUST.items():
        _, frame, nat, fix = by_name[name]
        act, r = RM.reply_of(frame, C.model_netif(nat_enable), nat=nat, fix=fix, tcp_ports=C.SERVED)
        assert (None if r is None else r["kind"]) == kind, (name, act, r)
    _, frame, nat, fix = by_name["echo_nat_miss"]
    assert RM.reply_of(frame, C.model_netif(True), nat=nat, fix=fix)[0] == "FORWARD"       # not a local echo
    assert RM.reply_of(frame, C.model_netif(True), nat=C.NAT_V_FLOW, fix=fix)[1] is None   # and only on a miss
    _, frame, nat, fix = by_name["udp_nat_miss"]
    assert nat == C.NAT_V_MISS and frame[23] == 17
    _, frame, nat, fix = by_name["tcp_syn_wrap"]
    r = RM.reply_of(frame, C.model_netif(), tcp_ports=C.SERVED)[1]
    assert frame[38:42] == b"\xff" * 4 and r["ack"] == 0


def test_cap_below_at_and_above(fuzz):
    f = fuzz
    sl = slice(3000, None)  # the crafted frames
    args = ([f["frames"][i] for i in range(3000, len(f["frames"]))], f["offs"][sl], f["lens"][sl], f["recs"][sl], False,
            f["nat"][sl], f["steps"][sl], f["result"][sl], C.SERVED)
    count = _compare(*args).count
    assert count >= 8
    for cap in (0, 1, count - 1, count, count + 1, count + 40):
        _compare(*args, cap=cap, what=f"cap {cap}")


def test_empty_batch_and_null_outputs():
    from halo_amd import _lib

    o = _host(np.zeros(0, np.uint32), np.zeros(0, np.uint16), np.zeros(0, _lib.RESULT_DTYPE), False)
    check_outputs(o, RM.Want([], []))
    # cap 0 with null outputs, no kind counts, no actions
    frames = [C.echo_request(C.PEER)] * 3
    data, offs, lens = C.pack(1, frames)
    recs = _records(frames, C.model_netif())
    count = np.zeros(1, np.uint32)
    rc = _lib.lib.halo_tx_respond_host(_lib.ptr(offs), _lib.ptr(lens), _lib.ptr(recs), 3, 0, C.lib_netif(), None, None, None,
                                       None, None, None, None, 0, _lib.ptr(count), None, None)
    assert rc == 0 and int(count[0]) == 3


def test_reply_frames_parse_clean_at_the_peer(fuzz):
    """Every reply built from the host's descriptors by the tx restatement, with the peer's MAC as
    TxIpv4 would find it, passes the rx restatement as the peer: OK, for it, and the right type."""
    from halo_amd._lib import BUILD_DESC_DTYPE, RESPOND_SRC_DTYPE

    f = fuzz
    o = _host(f["offs"], f["lens"], f["recs"], False, nat=f["nat"], steps=f["steps"], result=f["result"], ports=C.SERVED)
    w = int(o["count"][0])
    desc = o["desc"].reshape(-1).view(BUILD_DESC_DTYPE)[:w]
    src = o["src"].reshape(-1).view(RESPOND_SRC_DTYPE)[:w]
    iph = T.IphId(0xFFF0)  # wraps on the way
    built = 0
    for d, s in zip(desc, src):
        dd = {k: int(d[k]) for k in RM.DESC_FIELDS}
        dd.update(dst_mac=C.PEER_MAC, mode=0)
        po, pl = dd["payload_off"], dd["payload_len"]
        res, frame = T.tx_build(dd, f["data"][po:po + pl].tobytes(), C.MAC, iph)
        if res != 0:  # a jumbo echo: emitted here, rejected by the build
            assert res == T.B_PAYLOAD_LEN and pl > 1472
            continue
        built += 1
        r = R.rx_frame(frame, C.PEER_MAC, dd["dst_ip"])
        assert r["status"] == "OK" and r["flags"] & 1 and r["flags"] & 4 and r["src_ip"] == C.OWN_IP, (s, r)
        kind = int(s["kind"])
        want_aux = {RM.ECHO: 0, RM.TTL: 11, RM.TCP_SYN: 0x12, RM.TCP_SYNACK: 0x10}[kind]
        assert r["l4_aux"] == want_aux and r["ip_proto"] == (6 if kind >= RM.TCP_SYN else 1)
    assert built > 50 and iph.value == (0xFFF0 + built) & 0xFFFF


# ---- argument checks, before any device is looked for -----------------------------------------------
def test_device_argument_errors_need_no_device():
    from halo_amd import _lib

    E = _lib.HALO_E_INVAL
    n = 4
    a8 = np.zeros(4096, np.uint64)  # 8-byte aligned host memory standing in for device pointers: never dereferenced
    base = a8.ctypes.data
    offs, lens, recs, desc, src, dst, cnt, ws = (base + 256 * k for k in range(8))
    nif = C.lib_netif()
    wsb = int(_lib.lib.halo_tx_respond_workspace(n))
    assert wsb == 4 and _lib.lib.halo_tx_respond_workspace(257) == 8 and _lib.lib.halo_tx_respond_workspace(0) == 4

    def call(offs=offs, lens=lens, recs=recs, n=n, flags=0, netif=nif, nat=None, ops=None, res=None, ports=None, desc=desc,
             src=src, dst=dst, cap=n, cnt=cnt, kinds=None, acts=None, ws=ws, wsb=wsb):
        return _lib.lib.halo_tx_respond_device(offs, lens, recs, n, flags, netif, nat, ops, res, ports, desc, src, dst, cap,
                                               cnt, kinds, acts, ws, wsb, None)

    assert call(netif=None) == E and call(cnt=None) == E
    assert call(offs=None) == E and call(lens=None) == E and call(recs=None) == E and call(ws=None) == E
    assert call(desc=None) == E and call(src=None) == E
    assert call(ops=base + 2048) == E and call(res=base + 2048) == E  # only one of the pair
    assert call(flags=1) == E and call(flags=0x20) == E
    assert call(wsb=wsb - 1) == E
    assert call(offs=offs + 2) == E and call(lens=lens + 1) == E and call(recs=recs + 8) == E
    assert call(desc=desc + 4) == E and call(src=src + 4) == E and call(dst=dst + 2) == E and call(cnt=cnt + 2) == E
    assert call(kinds=base + 2050) == E and call(ports=base + 2050) == E and call(ws=ws + 2) == E
    # and the encap's sibling: a null table, a NetIf the table does not have
    from tests import arp_cases as K

    assert _lib.lib.halo_arp_encap_tx_device(None, offs, offs, lens, n, offs, 0, None, desc, None, cnt, None) == E
    t = K.Pair(capacity=4).t
    assert _lib.lib.halo_arp_encap_tx_device(t._t, offs, offs, lens, n, offs, 3, None, desc, None, cnt, None) == _lib.HALO_E_RANGE
    t.close()


def test_derived_edges_are_pinned():
    c = C.read_constants()
    assert C.derived(c) == {k: v["first_past"] for k, v in C.BOUNDARIES.items()}, (c, C.derived(c))
    from tests import scale_cases as S

    assert c["kTile"] == S.read_constants()["kGatherTile"]  # the gather's tile
