"""Not a test: a from-scratch statement of the local responders (include/halo_rx.h, "local
responders") that works from frame BYTES, not records. A frame is parsed with the Python
restatement of the rx path (oracle/ref_py.py), the engine branch is taken with the engine
restatement there (engine_rx / engine_lo), frames are walked in order and the reply the reference
would send — RxIcmp's echo reply (engine/icmp_engine.go:12-23), Ipv4RouteForward's time-exceeded
message (engine/ipv4_engine.go:133-142), RxTcp's handshake answers (engine/tcp_engine.go:16-24) —
is appended. Expected reply frames come from oracle/ref_tx_py.py's tx_build, and TxIpv4's route /
ARP step (engine/ipv4_engine.go:50-99) is restated over tests/arp_model.py and a route function.

What the model is told per frame beside the bytes is what the reference's state would say: whether
the WAN NAT lookup missed (`nat`, a HALO_NAT_V_* verdict or None), whether the TTL step ran and the
packet died (`fix` = (steps, result) or None) and which TCP ports are served.
"""
from __future__ import annotations

import numpy as np

from oracle import ref_py as R
from oracle import ref_tx_py as T
from tests import arp_model as AM

ECHO, TTL, TCP_SYN, TCP_SYNACK = range(4)
KINDS = 4
NAT_V_MISS = 2
TX_TTL, R_TTL_ALIVE = 0x02, 0x01
DESC_FIELDS = ("payload_off", "payload_len", "proto", "aux", "src_port", "dst_port", "src_ip", "dst_ip", "seq", "ack")


class NetIf:
    def __init__(self, mac: bytes, ip: int, nat_enable: bool = False):
        self.mac, self.ip, self.nat_enable = bytes(mac), int(ip), bool(nat_enable)


def _rx_icmp(ipv4_payload: bytes, c: R.Cfg, at: int):
    """RxIcmp: (icmp payload offset relative to the buffer, its length, id, seq) of the echo reply
    it sends, or None. `at` is where ipv4_payload starts in the buffer."""
    pay, typ, icmp_id, seq, err = R.parse_icmp_pkt(ipv4_payload, c)
    if err or typ != 0x08:
        return None
    return at + 8, len(pay), R.be16(icmp_id), seq


def reply_of(buf: bytes, nif: NetIf, *, check_sum_enable=True, jumbo=False, l3=False, nat=None, fix=None, tcp_ports=()):
    """(action name, reply or None) for one received frame (or LoChan packet with l3). The reply
    is a dict: kind and the halo_tx_build_desc_t fields, payload_off relative to the buffer."""
    c = R.Cfg(check_sum_enable, jumbo)
    if l3:
        act = R.engine_lo(buf, nif.ip, check_sum_enable, jumbo)
        pkt, at = buf, 0
    else:
        act = R.engine_rx(buf, nif.mac, nif.ip, nif.nat_enable, check_sum_enable, jumbo)
        pkt, at = buf[14:], 14
    if act not in ("FORWARD", "LOCAL_ICMP", "LOCAL_TCP"):
        return act, None
    ip_payload, proto, src, _dst, _tl, err = R.parse_ipv4_pkt(pkt, c)
    assert not err
    base = dict(src_ip=nif.ip, dst_ip=R.ip_addr_to_u(src), seq=0, ack=0, src_port=0, dst_port=0, payload_len=0)

    def echo():
        e = _rx_icmp(ip_payload, c, at + 20)
        if e is None:
            return None
        return dict(base, kind=ECHO, proto=1, aux=0, payload_off=e[0], payload_len=e[1], src_port=e[2], dst_port=e[3])

    if act == "LOCAL_ICMP":
        return act, echo()
    if act == "FORWARD":
        if nat == NAT_V_MISS:  # Ipv4RouteForward returned false (:120-124); RxIpv4 :33-35
            return act, (echo() if proto == 0x01 else None)
        if fix is not None and (fix[0] & TX_TTL) and not (fix[1] & R_TTL_ALIVE):
            return act, dict(base, kind=TTL, proto=1, aux=11, payload_off=at, payload_len=min(28, len(pkt)))
        return act, None
    # RxTcp
    _pay, sport, dport, seq, _ack, flags, err = R.parse_tcp_pkt(ip_payload, src, nif.ip.to_bytes(4, "big"), c)
    assert not err
    if dport not in tcp_ports or not flags & 0x02:
        return act, None
    if flags & 0x10:
        return act, dict(base, kind=TCP_SYNACK, proto=6, aux=0x10, payload_off=0, src_port=dport, dst_port=sport,
                         seq=1234567891, ack=(seq + 1) & 0xFFFFFFFF)
    return act, dict(base, kind=TCP_SYN, proto=6, aux=0x12, payload_off=0, src_port=dport, dst_port=sport,
                     seq=1234567890, ack=(seq + 1) & 0xFFFFFFFF)


class Want:
    """The outputs of one responder call, whole: `desc` (BUILD_DESC_DTYPE-shaped dict arrays),
    `index`, `kind`, `dst_ip` of every reply in frame order, `kind_counts`, `actions`."""

    def __init__(self, replies, actions):
        self.replies = replies  # [(frame index, reply dict with absolute payload_off)]
        self.actions = np.array([R.ACTIONS.index(a) for a in actions], np.uint8)
        self.count = len(replies)
        self.kind_counts = np.bincount([r["kind"] for _, r in replies], minlength=KINDS).astype(np.uint32)

    def arrays(self, desc_dtype, src_dtype):
        desc = np.zeros(self.count, desc_dtype)
        src = np.zeros(self.count, src_dtype)
        for k, (i, r) in enumerate(self.replies):
            for f in DESC_FIELDS:
                desc[k][f] = r[f]
            src[k]["index"], src[k]["kind"] = i, r["kind"]
        return desc, src, desc["dst_ip"].astype(np.uint32)


def respond(frames, offsets_dw, nif: NetIf, *, nat=None, fix=None, **kw) -> Want:
    """Walk `frames` (bytes each) in order. `nat`: verdict per frame or None; `fix`: (steps,
    results) arrays or None."""
    replies, actions = [], []
    for i, f in enumerate(frames):
        act, r = reply_of(f, nif, nat=None if nat is None else int(nat[i]),
                          fix=None if fix is None else (int(fix[0][i]), int(fix[1][i])), **kw)
        actions.append(act)
        if r is not None:
            # a reply without payload keeps the frame's start, as the descriptor does
            r["payload_off"] = 4 * int(offsets_dw[i]) + r["payload_off"]
            replies.append((i, r))
    return Want(replies, actions)


def respond_uniform(templates, tid, offsets_dw, nif: NetIf, *, nat_t=None, fix_t=None, **kw):
    """The vectorised path for batches that repeat a few template frames: template t's decision is
    taken once (with its own nat / fix inputs nat_t[t], fix_t[t]) and frame i gets that of
    tid[i]. Returns (desc fields dict of arrays, index, kind, kind_counts, actions) in frame order."""
    per = [reply_of(f, nif, nat=None if nat_t is None else nat_t[t], fix=None if fix_t is None else fix_t[t], **kw)
           for t, f in enumerate(templates)]
    tid = np.asarray(tid)
    actions = np.array([R.ACTIONS.index(a) for a, _ in per], np.uint8)[tid]
    has = np.array([r is not None for _, r in per])[tid]
    index = np.flatnonzero(has).astype(np.uint32)
    t_of = tid[index]
    out = {}
    for f in DESC_FIELDS:
        col = np.array([0 if r is None else r[f] for _, r in per], np.uint64)[t_of]
        out[f] = col + 4 * offsets_dw[index].astype(np.uint64) if f == "payload_off" else col
    kind = np.array([0 if r is None else r["kind"] for _, r in per], np.uint8)[t_of]
    return out, index, kind, np.bincount(kind, minlength=KINDS).astype(np.uint32), actions


# ---- the reply frames ---------------------------------------------------------------------------
def build_frames(replies, data: np.ndarray, src_mac: bytes, ip_id: int, check_sum_enable=True):
    """TxIcmp / TxTcp -> TxIpv4's BuildIpv4Pkt -> BuildEthFrm for every reply in order, with the
    payload bytes taken from `data` (the rx batch as the fixup left it) and a zero destination MAC
    (TxIpv4's L2 step fills it): ([(result, frame bytes)], the final iphId)."""
    iph = T.IphId(ip_id)
    out = []
    for _i, r in replies:
        d = dict(r, dst_mac=bytes(6), mode=0)
        po, pl = int(r["payload_off"]), int(r["payload_len"])
        out.append(T.tx_build(d, bytes(data[po:po + pl]), src_mac, iph, check_sum_enable))
    return out, iph.value


# ---- TxIpv4's L3 / L2 step (engine/ipv4_engine.go:50-99) -------------------------------------------
def tx_ipv4(arp: AM.Model, frame: bytes, route, self_netif: int, selected: bool = True):
    """For one built frame: (verdict, out_netif, tx_len, target_ip, the frame afterwards). `route`
    is what FindRoute(dst) gave: AM.ROUTE_NONE, AM.ROUTE_PANIC_ID, None (an id the device copy does
    not know) or (next_hop, netif)."""
    n = len(frame)
    if not selected or n < 34 or frame[12:14] != b"\x08\x00":
        return AM.NONE, 0xFF, 0, 0, frame
    if frame[33] == 255:  # :60-61, :85-86, :92-93
        nif = arp.netifs[self_netif]
        return AM.HIT, self_netif, max(n, 60), 0, AM.BCAST + nif.mac + frame[12:]
    if route is None:
        return AM.NONE, 0xFF, 0, 0, frame
    if route == AM.ROUTE_NONE:
        return AM.NO_ROUTE, 0xFF, 0, 0, frame
    if route == AM.ROUTE_PANIC_ID:
        return AM.ROUTE_PANIC, 0xFF, 0, 0, frame
    next_hop, out = route
    if out >= len(arp.netifs):
        return AM.NONE, 0xFF, 0, 0, frame
    nif = arp.netifs[out]
    dst = AM.ip_of(frame[30:34])
    if dst == nif.ip:  # :71-80, whatever NatEnable says
        return AM.LOOPBACK, out, 0, 0, frame
    target = next_hop or dst
    found, e = arp.get(out, target)
    if found == AM.GET_OWN_IP:
        return AM.OWN_IP, out, 0, target, frame
    if found == AM.GET_ABSENT:
        return AM.MISS, out, 0, target, frame
    return AM.HIT, out, max(n, 60), target, e[0] + nif.mac + frame[12:]
