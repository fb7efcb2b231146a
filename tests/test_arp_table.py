"""CPU: the host control plane of the ARP neighbour cache (halo_amd/csrc/arp_table.cc through
halo_amd.arp.ArpTable) against known-answer frames written out byte by byte and the dict model
(tests/arp_model.py): every HandleArp branch, the reference's quirks, the u32 wraps of the expiry
and refresh ticks, and a random differential trace compared after every call."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import arp_cases as K
from tests import arp_model as M

H = bytes.fromhex
OWN0, IP0 = K.NETIFS[0].mac, K.NETIFS[0].ip  # 02:00:00:00:00:01, 10.0.0.1
PEER, PEER_IP = H("02aabbccddee"), 0x0A000009  # 10.0.0.9

# BuildEthFrm(dst = ff.., src = own, 0x0806) around BuildArpPkt(REQUEST, own mac, 10.0.0.1,
# ff:ff:ff:ff:ff:ff, 10.0.0.7): the body's target MAC is the broadcast MAC; 42 bytes + 18 zeros
REQ_FRAME = H("ffffffffffff" "020000000001" "0806"
              "0001" "0800" "06" "04" "0001"
              "020000000001" "0a000001"
              "ffffffffffff" "0a000007") + bytes(18)
# SendFreeArp: the same with the own address as the target
FREE_FRAME = H("ffffffffffff" "020000000001" "0806"
               "0001" "0800" "06" "04" "0001"
               "020000000001" "0a000001"
               "ffffffffffff" "0a000001") + bytes(18)
# the reply to 02:aa:bb:cc:dd:ee / 10.0.0.9 asking for 10.0.0.1
REPLY_FRAME = H("02aabbccddee" "020000000001" "0806"
                "0001" "0800" "06" "04" "0002"
                "020000000001" "0a000001"
                "02aabbccddee" "0a000009") + bytes(18)


@pytest.fixture
def pair():
    made = []

    def make(**kw):
        made.append(K.Pair(**kw))
        return made[-1]

    yield make
    for p in made:
        p.close()


def test_known_answer_frames(pair):
    p = pair(capacity=4)
    assert len(REQ_FRAME) == len(FREE_FRAME) == len(REPLY_FRAME) == 60
    assert bytes(p.t.SendArpReq(0, 0x0A000007)) == REQ_FRAME == p.m.request(0, 0x0A000007)
    assert bytes(p.t.SendFreeArp(0)) == FREE_FRAME == p.m.request(0, IP0)
    arr = K.msg_array([(0, M.arp_pkt(1, PEER, PEER_IP, bytes(6), IP0), PEER)])
    v, replies, changed = p.t.HandleArp(arr, 100)
    assert list(v) == [M.ACCEPTED | M.F_REPLY] and changed == 1
    assert [bytes(r) for r in replies] == [REPLY_FRAME]


def test_every_handle_branch(pair):
    p = pair(capacity=2)
    other = K.mac(5)
    msgs = [
        (0, M.arp_pkt(3, PEER, PEER_IP, bytes(6), IP0), PEER),            # BAD_OP
        (0, M.arp_pkt(0, PEER, PEER_IP, bytes(6), IP0), PEER),            # BAD_OP
        (0, M.arp_pkt(1, PEER, PEER_IP, bytes(6), IP0), other),           # SRC_MISMATCH
        (0, M.arp_pkt(2, PEER, IP0, OWN0, 0x0A000003), PEER),             # CONFLICT
        (0, M.arp_pkt(1, PEER, PEER_IP, bytes(6), IP0), PEER),            # learn + reply
        (0, M.arp_pkt(1, PEER, PEER_IP, bytes(6), 0x0A000003), PEER),     # request for someone else: learn, no reply
        (0, M.arp_pkt(2, other, 0x0A000004, K.mac(9), 0x0A000077), other),  # a reply not for us still learns
        # garbage hardware type, protocol type and address lengths: ParseArpPkt never looks
        (1, M.arp_pkt(2, PEER, 0x0A010009, bytes(6), 0, head=H("dead beef 99 77".replace(" ", ""))), PEER),
    ]
    v = p.handle(msgs[:7], 10)
    assert list(v) == [M.BAD_OP, M.BAD_OP, M.SRC_MISMATCH, M.CONFLICT, M.ACCEPTED | M.F_REPLY, M.ACCEPTED, M.ACCEPTED]
    p.check()
    assert len(p.m.cache) == 2
    # the table is full: the garbage-header message is accepted but not learned ...
    assert list(p.handle(msgs[7:], 11)) == [M.ACCEPTED | M.F_NOT_LEARNED]
    # ... a request for us from a stranger is answered although it cannot be learned ...
    stranger = K.mac(77)
    v = p.handle([(0, M.arp_pkt(1, stranger, 0x0A000042, bytes(6), IP0), stranger)], 12)
    assert list(v) == [M.ACCEPTED | M.F_NOT_LEARNED | M.F_REPLY]
    assert p.t.GetArpCache(0, 0x0A000042)[0] == M.GET_ABSENT
    # ... and an existing key is refreshed (new MAC, new ExpTime) although the table is full
    newmac = K.mac(1234)
    assert list(p.handle([(0, M.arp_pkt(2, newmac, PEER_IP, OWN0, IP0), newmac)], 500)) == [M.ACCEPTED]
    f, e = p.t.GetArpCache(0, PEER_IP)
    assert f == M.GET_FOUND and bytes(e["mac"]) == newmac and int(e["exp_time"]) == 800
    p.check()
    # with room again the garbage-header message learns
    assert p.expire(400) == 1
    assert list(p.handle(msgs[7:], 401)) == [M.ACCEPTED]
    assert p.t.GetArpCache(1, 0x0A010009)[0] == M.GET_FOUND
    p.check()


def test_set_and_get(pair):
    p = pair(capacity=3)
    assert p.t.dirty  # no device copy yet
    p.set(0, PEER_IP, PEER, 7)
    p.set(2, PEER_IP, K.mac(2), 8)  # the same address on another NetIf, another MAC
    p.set(0, 0x0A0000FE, H("01005e000001"), 9)  # a group MAC is stored unchecked
    p.set(1, 0x0A010002, K.mac(3), 9)  # full: silently nothing
    p.check()
    assert len(p.t.ListArp()) == 3
    f, e = p.t.GetArpCache(0, PEER_IP)
    assert f == M.GET_FOUND and bytes(e["mac"]) == PEER and int(e["exp_time"]) == 307 and int(e["netif"]) == 0
    f, e = p.t.GetArpCache(2, PEER_IP)
    assert f == M.GET_FOUND and bytes(e["mac"]) == K.mac(2) and int(e["netif"]) == 2
    assert p.t.GetArpCache(1, PEER_IP) == (M.GET_ABSENT, None)
    assert p.t.GetArpCache(1, 0x0A010002) == (M.GET_ABSENT, None)
    assert bytes(p.t.GetArpCache(0, 0x0A0000FE)[1]["mac"]) == H("01005e000001")
    # the own address is nil without a request
    assert p.t.GetArpCache(0, IP0) == (M.GET_OWN_IP, None)
    assert p.t.GetArpCache(1, IP0) == (M.GET_ABSENT, None)  # NetIf 1's own address is another
    p.set(0, PEER_IP, K.mac(4), 1000)  # refresh when full
    f, e = p.t.GetArpCache(0, PEER_IP)
    assert bytes(e["mac"]) == K.mac(4) and int(e["exp_time"]) == 1300
    # age is not checked by GetArpCache: an entry long past its ExpTime is still returned
    assert p.t.GetArpCache(2, PEER_IP)[0] == M.GET_FOUND
    p.check()


def test_expiry_and_refresh_edges(pair):
    p = pair(capacity=8)
    p.set(0, 0x0A000002, K.mac(1), 1000)  # ExpTime 1300
    for now, due in ((1290, False), (1291, True), (1300, True)):
        assert (len(p.t.ArpTableRefresh(now)[0]) == 1) == due
        p.check(now)
    assert p.expire(1300) == 0  # now == ExpTime stays
    assert p.expire(1301) == 1  # now == ExpTime + 1 goes
    # set at 0xFFFFFF00: ExpTime wraps to 0x2C, so any later `now` before the wrap removes it at once
    p.set(0, 0x0A000003, K.mac(2), 0xFFFFFF00)
    assert int(p.t.GetArpCache(0, 0x0A000003)[1]["exp_time"]) == 0x2C
    p.check(0x2C)
    # ExpTime - 10 = 0x22: due from 0x23
    assert len(p.t.ArpTableRefresh(0x22)[0]) == 0 and len(p.t.ArpTableRefresh(0x23)[0]) == 1
    assert p.expire(0x2C) == 0
    assert p.expire(0xFFFFFF01) == 1
    # ExpTime < 10: ExpTime - 10 wraps to a huge value and the entry is never refreshed
    p.set(1, 0x0A010005, K.mac(3), (5 - 300) & M.U32)
    assert int(p.t.GetArpCache(1, 0x0A010005)[1]["exp_time"]) == 5
    for now in (0, 5, 6, 1000, 0xFFFFFFF0):
        assert len(p.t.ArpTableRefresh(now)[0]) == 0
        p.check(now)
    assert p.expire(5) == 0 and p.expire(6) == 1
    p.check()


def test_random_differential_trace(pair):
    rng = np.random.default_rng(11)
    p = pair(capacity=12)
    now = 0xFFFFFC00  # crosses the u32 wrap
    ips = [[(nif.ip & 0xFFFFFF00) | k for k in range(1, 12)] for nif in K.NETIFS]  # host 1 is the own address
    seen = set()
    for _ in range(600):
        op = int(rng.integers(0, 10))
        now = (now + int(rng.integers(0, 40))) & M.U32
        if op < 2:
            nif = int(rng.integers(0, 3))
            p.set(nif, ips[nif][int(rng.integers(0, 11))], K.mac(int(rng.integers(0, 6))), now)
        elif op < 7:
            msgs = []
            for _ in range(int(rng.integers(0, 6))):
                nif = int(rng.integers(0, 3))
                sha = K.mac(int(rng.integers(0, 6)))
                src = sha if rng.integers(0, 6) else K.mac(50)
                o = int(rng.choice([1, 1, 2, 2, 0, 7]))
                spa, tpa = ips[nif][int(rng.integers(0, 11))], ips[nif][int(rng.integers(0, 3))]
                msgs.append((nif, M.arp_pkt(o, sha, spa, K.mac(0), tpa), src))
            seen |= set(int(x) for x in p.handle(msgs, now))
        elif op < 8:
            p.expire(now)
        else:
            nif = int(rng.integers(0, 3))
            ip = ips[nif][int(rng.integers(0, 11))]
            f, e = p.t.GetArpCache(nif, ip)
            wf, we = p.m.get(nif, ip)
            assert f == wf and (e is None or (bytes(e["mac"]), int(e["exp_time"])) == tuple(we))
        p.check(now)
    base = {v & 0x0F for v in seen}
    assert base == {M.BAD_OP, M.SRC_MISMATCH, M.CONFLICT, M.ACCEPTED}
    assert any(v & M.F_NOT_LEARNED for v in seen) and any(v & M.F_REPLY for v in seen)
    assert any(v & M.F_NOT_LEARNED and v & M.F_REPLY for v in seen)


def test_argument_errors_leave_the_table(pair):
    from halo_amd import _lib
    from halo_amd._lib import HALO_E_INVAL, HALO_E_NODEV, HALO_E_RANGE

    L = _lib.lib
    p = pair(capacity=4)
    p.set(0, PEER_IP, PEER, 1)
    t = p.t._t
    m6 = np.frombuffer(PEER, np.uint8).copy()
    f = ctypes.c_uint32()
    assert L.halo_arp_set(t, 3, 1, _lib.ptr(m6), 1) == HALO_E_RANGE
    assert L.halo_arp_set(t, 0, 1, None, 1) == HALO_E_INVAL
    assert L.halo_arp_set(None, 0, 1, _lib.ptr(m6), 1) == HALO_E_INVAL
    assert L.halo_arp_get(t, 3, 1, None, ctypes.byref(f)) == HALO_E_RANGE
    assert L.halo_arp_get(t, 0, 1, None, None) == HALO_E_INVAL
    out = np.zeros(60, np.uint8)
    assert L.halo_arp_build_request(t, 3, 1, _lib.ptr(out)) == HALO_E_RANGE
    assert L.halo_arp_build_request(t, 0, 1, None) == HALO_E_INVAL
    # one message with a NetIf the table does not have: nothing of the batch is applied
    msgs = K.msg_array([(0, M.arp_pkt(2, K.mac(1), 0x0A000005, OWN0, IP0), K.mac(1)),
                        (3, M.arp_pkt(2, K.mac(2), 0x0A000006, OWN0, IP0), K.mac(2))])
    v = np.zeros(2, np.uint8)
    assert L.halo_arp_handle_msgs(t, _lib.ptr(msgs), 2, 5, _lib.ptr(v), None, None, None) == HALO_E_RANGE
    assert L.halo_arp_handle_msgs(t, None, 2, 5, _lib.ptr(v), None, None, None) == HALO_E_INVAL
    assert L.halo_arp_handle_msgs(t, _lib.ptr(msgs), 2, 5, None, None, None, None) == HALO_E_INVAL
    assert L.halo_arp_handle_msgs(t, None, 0, 5, None, None, None, None) == 0
    n = ctypes.c_uint32()
    assert L.halo_arp_list(t, None, 1, ctypes.byref(n)) == HALO_E_INVAL
    assert L.halo_arp_refresh_list(t, 0, None, None, 1, ctypes.byref(n)) == HALO_E_INVAL
    assert L.halo_arp_expire(None, 0, None) == HALO_E_INVAL
    assert L.halo_arp_layout_stats(t, None) == HALO_E_INVAL
    assert L.halo_arp_sync_device(t, None, -1) == HALO_E_INVAL
    assert L.halo_arp_gather_device(None, None, None, None, 0, 64, None, 0, None, None, 0, None) == HALO_E_INVAL
    p.check()
    assert len(p.t.ListArp()) == 1
    # configurations
    cfg = _lib.ArpConfig()
    h = ctypes.c_void_p()
    for n_netifs, cap, log2 in ((0, 4, 0), (65, 4, 0), (1, 0, 0), (1, 16, 4), (1, 4, 29)):
        cfg.n_netifs, cfg.capacity, cfg.slots_log2 = n_netifs, cap, log2
        assert L.halo_arp_table_create(ctypes.byref(cfg), ctypes.byref(h)) == HALO_E_INVAL and not h.value
    assert L.halo_arp_table_destroy(None) == HALO_E_INVAL
    assert int(L.halo_arp_gather_workspace(0)) == 4 and int(L.halo_arp_gather_workspace(257)) == 8
    import torch

    if not torch.cuda.is_available():  # no quiet fallback: the device calls need a device
        assert L.halo_arp_sync_device(t, None, 0) == HALO_E_NODEV
        assert L.halo_arp_lookup_device(t, None, None, 0, 0, None, None, None, None) == HALO_E_INVAL  # never synced


def test_forced_layout(pair):
    p, keys = K.forced_table(pair)
    st = p.t.layout_stats()
    assert int(st["slots"]) == 16 and int(st["entries"]) == 15
    assert int(st["longest_chain"]) >= 3 and int(st["wrapped"]) >= 1
    for k, (nif, ip) in enumerate(keys):  # the host table is a map: the layout changes no answer
        f, e = p.t.GetArpCache(nif, ip)
        assert f == M.GET_FOUND and bytes(e["mac"]) == K.mac(100 + k)
    auto = pair(capacity=15)
    assert int(auto.t.layout_stats()["slots"]) == 32  # the next power of two >= 2 * capacity
