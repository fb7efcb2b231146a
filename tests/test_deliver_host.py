"""CPU: local delivery's host side (halo_amd/csrc/rx_deliver_host.cc over rx_deliver.h and
rx_dispatch.h) against tests/deliver_model.py, which works from frame bytes: the crafted frames of
tests/deliver_cases.py as frames and as LoChan packets, with and without NatEnable and the DHCP
flag, every output prefilled with 0xA5 behind a sentinel and compared whole; the region cut at 0,
one byte short of a record, at a record end and above the total; `index_cap` below, at and above
the count; each map absent; a record whose payload overruns its frame; the device entry point's
argument checks, which are answered before any device is looked for; and DeliverResult.dispatch
against NetIf._deliver with recording handlers."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import deliver_cases as C
from tests import deliver_model as DM

FILL = C.FILL


def _host(data, offs, lens, recs, nat_enable, region, index_cap, *, udp=C.UDP_SERVED, tcp=C.TCP_SERVED, l3=False, dhcp=True):
    """halo_rx_deliver_host into 0xA5-filled outputs, straight through ctypes."""
    from halo_amd import _lib
    from halo_amd.deliver import port_map

    o = C.new_outputs(region, index_cap)
    cfg = _lib.DeliverConfig()
    cfg.flags = (_lib.HALO_RX_L3_START if l3 else 0) | (_lib.HALO_DELIVER_DHCP if dhcp else 0)
    cfg.index_cap, cfg.region_bytes = index_cap, region
    um = None if udp is None else port_map(udp)
    tm = None if tcp is None else port_map(tcp)
    rc = _lib.lib.halo_rx_deliver_host(ctypes.byref(cfg), _lib.ptr(data), _lib.ptr(offs), _lib.ptr(lens), _lib.ptr(recs),
                                       len(lens), C.lib_netif(nat_enable), _lib.ptr(um), _lib.ptr(tm), _lib.ptr(o["out"]),
                                       _lib.ptr(o["summary"]), _lib.ptr(o["index"]) if index_cap else None)
    assert rc == 0, rc
    return o


def _crafted(l3: bool, jumbo: bool):
    cases = C.crafted(jumbo)
    return [f for _, f in (C.as_lo_packets(cases) if l3 else cases)]


def test_crafted_set_covers_what_it_must():
    nif = C.model_netif()
    kw = dict(udp_ports=C.UDP_SERVED, tcp_ports=C.TCP_SERVED, dhcp=True)
    by_name = {name: DM.delivery_of(f, nif, **kw) for name, f in C.crafted(jumbo=False)}
    for name in ("udp_served", "udp_port0", "udp_port65535", "bcast_67", "bcast_68", "tcp_syn_empty", "tcp_synack", "tcp_port0"):
        assert by_name[name] is not None, name
    for name in ("udp_unserved", "udp_bad_checksum", "udp_other_address", "bcast_53", "bcast_67_bad_checksum", "tcp_unserved",
                 "tcp_bad_checksum", "icmp_echo", "arp", "wrong_mac", "short"):
        assert by_name[name] is None, name
    assert [len(by_name[f"udp_len_{n}"]["payload"]) for n in C.PAYLOAD_LENS] == list(C.PAYLOAD_LENS)
    assert by_name["tcp_syn_empty"]["tcp_flags"] == 0x02 and by_name["tcp_synack"]["seq"] == 0xFFFFFFFF
    # every data-offset nibble is delivered, and the payloads start at all four byte alignments
    assert all(by_name[f"tcp_nibble_{k}"] is not None for k in range(16))
    nibbles = [f for name, f in C.crafted() if name.startswith("tcp_nibble_")]
    assert C.source_alignments(nibbles, nif, **kw) == {0, 1, 2, 3}
    assert C.source_alignments([f[14:] for f in nibbles], nif, l3=True, **kw) == {0, 1, 2, 3}
    # NatEnable forwards what was local; the broadcast row stays
    nat = DM.want_of([f for _, f in C.crafted()], C.model_netif(True), **kw)
    assert [d["kind"] for _, d in nat.items] == [DM.DHCP, DM.DHCP]
    jumbo = dict(C.crafted(jumbo=True))[f"udp_len_{C.JUMBO_PAYLOAD}"]
    assert len(DM.delivery_of(jumbo, nif, jumbo=True, **kw)["payload"]) == C.JUMBO_PAYLOAD
    assert DM.delivery_of(jumbo, nif, **kw) is None


@pytest.mark.parametrize("l3", [False, True], ids=["frames", "lo_packets"])
@pytest.mark.parametrize("nat_enable", [False, True], ids=["local", "nat"])
@pytest.mark.parametrize("dhcp", [True, False], ids=["dhcp", "no_dhcp"])
@pytest.mark.parametrize("jumbo", [False, True], ids=["std", "jumbo"])
def test_host_equals_model_on_the_crafted_set(l3, nat_enable, dhcp, jumbo):
    frames = _crafted(l3, jumbo)
    nif = C.model_netif(nat_enable)
    want = DM.want_of(frames, nif, jumbo=jumbo, l3=l3, udp_ports=C.UDP_SERVED, tcp_ports=C.TCP_SERVED, dhcp=dhcp)
    if not nat_enable or l3:  # the LoChan drain has no NAT branch
        assert want.kind_counts[DM.UDP] and want.kind_counts[DM.TCP]
    assert bool(want.kind_counts[DM.DHCP]) == (dhcp and not l3)
    data, offs, lens = C.pack(11, frames)
    recs = C.records(frames, nif, jumbo=jumbo, l3=l3)
    for region in C.cuts(want) if want.recs else [0, 64]:
        for cap in sorted({0, max(len(want.recs) - 1, 0), len(want.recs), len(want.recs) + 3}):
            o = _host(data, offs, lens, recs, nat_enable, region, cap, l3=l3, dhcp=dhcp)
            C.check_outputs(o, want, (region, cap))


def test_region_cut_at_every_interesting_byte():
    frames = _crafted(False, False)
    nif = C.model_netif()
    want = DM.want_of(frames, nif, udp_ports=C.UDP_SERVED, tcp_ports=C.TCP_SERVED, dhcp=True)
    data, offs, lens = C.pack(12, frames)
    recs = C.records(frames, nif)
    ends = np.cumsum([len(r) for r in want.recs])
    seen = set()
    for end in (int(ends[0]), int(ends[len(ends) // 2]), int(ends[-1])):
        for region in (end - 1, end, end + 1):  # the host call takes any region
            o = _host(data, offs, lens, recs, False, region, len(want.recs))
            C.check_outputs(o, want, region)
            seen.add(int(o["summary"][:40].view(np.uint32)[1]))
    assert len(seen) >= 5  # the cuts moved the written prefix
    o = _host(data, offs, lens, recs, False, 0, 2)
    C.check_outputs(o, want, "region 0")
    assert o["index"][:2].reshape(-1).view(np.uint32)[1::2].tolist() == [DM.NOT_WRITTEN] * 2


@pytest.mark.parametrize("udp,tcp", [(None, C.TCP_SERVED), (C.UDP_SERVED, None), (None, None), ((), ())],
                         ids=["no_udp_map", "no_tcp_map", "no_maps", "empty_maps"])
def test_each_map_absent(udp, tcp):
    frames = _crafted(False, False)
    nif = C.model_netif()
    want = DM.want_of(frames, nif, udp_ports=udp or (), tcp_ports=tcp or (), dhcp=True)
    assert bool(want.kind_counts[DM.UDP]) == bool(udp) and bool(want.kind_counts[DM.TCP]) == bool(tcp)
    data, offs, lens = C.pack(13, frames)
    o = _host(data, offs, lens, C.records(frames, nif), False, 8192, 64, udp=udp, tcp=tcp)
    C.check_outputs(o, want)


def test_record_that_overruns_its_frame_is_skipped():
    """A record that is not the frame's: payload_off + payload_len > lens[i]. Nothing is
    delivered for it and nothing of the buffer behind the frame is copied."""
    nif = C.model_netif()
    long_f, short_f = C.udp(53, bytes(range(200))), C.udp(53, b"tiny")
    frames = [short_f, short_f, long_f]
    data, offs, lens = C.pack(14, frames)
    data = data[:int(offs[2]) * 4 + len(long_f)].copy()  # the batch ends with its last frame
    recs = C.records(frames, nif)
    recs[1] = recs[2]  # frame 1 is 60 bytes; its record now says 42 + 200
    good = DM.want_of(frames, nif, udp_ports=C.UDP_SERVED)
    want = DM.Want([good.items[0], good.items[2]], skipped=1)
    o = _host(data, offs, lens, recs, False, 1024, 4)
    C.check_outputs(o, want)
    recs[2]["payload_len"] += 1  # one byte past the last frame of the batch
    o = _host(data, offs, lens, recs, False, 1024, 4)
    C.check_outputs(o, DM.Want([good.items[0]], skipped=2))


def test_device_entry_point_checks_arguments_before_any_device():
    """Every malformed call is HALO_E_INVAL whether or not the machine has a device: the checks
    come first. (A well-formed call on a machine without one is HALO_E_NODEV.)"""
    import torch

    from halo_amd import _lib

    L = _lib.lib
    INVAL = _lib.HALO_E_INVAL
    buf = np.zeros(16384, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 64
    ws = int(L.halo_rx_deliver_workspace(300))
    assert ws == 20 * 2 and int(L.halo_rx_deliver_workspace(0)) == 24 and int(L.halo_rx_deliver_workspace(257)) == 40  # 20 B per tile, to 8
    nif = C.lib_netif()

    def call(flags=0, region=1024, index_cap=4, cfg_null=False, netif=nif, n=300, d_bytes=base, d_offs=base + 64,
             d_lens=base + 128, d_recs=base + 192, d_udp=base + 256, d_tcp=base + 320, d_out=base + 384, d_sum=base + 448,
             d_index=base + 512, d_ws=base + 576, ws_bytes=ws):
        cfg = _lib.DeliverConfig()
        cfg.flags, cfg.region_bytes, cfg.index_cap = flags, region, index_cap
        return L.halo_rx_deliver_device(None if cfg_null else ctypes.byref(cfg), d_bytes, d_offs, d_lens, d_recs, n, netif,
                                        d_udp, d_tcp, d_out, d_sum, d_index, d_ws, ws_bytes, None)

    bad = [dict(cfg_null=True), dict(netif=None), dict(d_sum=None), dict(flags=1), dict(flags=0x20), dict(region=1032),
           dict(region=8), dict(region=1 << 32), dict(region=(1 << 32) + 16), dict(d_out=None), dict(d_index=None),
           dict(d_bytes=None), dict(d_offs=None), dict(d_lens=None), dict(d_recs=None), dict(d_ws=None), dict(ws_bytes=ws - 1),
           dict(d_out=base + 392), dict(d_recs=base + 200), dict(d_sum=base + 452), dict(d_index=base + 516),
           dict(d_ws=base + 580), dict(d_bytes=base + 2), dict(d_udp=base + 258), dict(d_tcp=base + 322),
           dict(d_offs=base + 66), dict(d_lens=base + 129)]
    for kw in bad:
        assert call(**kw) == INVAL, kw
    # the host entry: the same null checks and flags, no alignment and any region
    cfg = _lib.DeliverConfig()
    cfg.region_bytes = 7
    summary = np.full(41, FILL, np.uint8)
    host = lambda c, n, out, s, idx: L.halo_rx_deliver_host(c, None, None, None, None, n, nif, None, None, out, s, idx)  # noqa: E731
    assert host(None, 0, base, summary.ctypes.data + 1, None) == INVAL
    assert host(ctypes.byref(cfg), 0, base, None, None) == INVAL
    assert host(ctypes.byref(cfg), 0, None, summary.ctypes.data + 1, None) == INVAL  # a region without an output
    assert host(ctypes.byref(cfg), 1, base, summary.ctypes.data + 1, None) == INVAL  # frames without arrays
    assert host(ctypes.byref(cfg), 0, base, summary.ctypes.data + 1, None) == 0
    assert summary[0] == FILL and not summary[1:].any()  # n == 0 zeroes the summary, at any alignment
    cfg.index_cap = 1
    assert host(ctypes.byref(cfg), 0, base, summary.ctypes.data + 1, None) == INVAL
    cfg.index_cap, cfg.flags = 0, _lib.HALO_RX_JUMBO_EXT | 1
    assert host(ctypes.byref(cfg), 0, base, summary.ctypes.data + 1, None) == INVAL
    if not torch.cuda.is_available():  # the checks passed and only then was a device looked for
        assert call() == _lib.HALO_E_NODEV
        assert call(region=(1 << 32) - 16, flags=_lib.HALO_RX_L3_START | _lib.HALO_DELIVER_DHCP, d_udp=None, d_tcp=None,
                    d_index=None, index_cap=0) == _lib.HALO_E_NODEV


def _recording_netif(log):
    from halo_amd.engine import NetIf

    nif = NetIf("eth0", "AA:AA:AA:AA:AA:AA", "192.168.100.100", lambda: None)
    for p in C.UDP_SERVED:
        nif.RecvUdp(p, lambda s, payload, p=p: log.append(("udp", p, s.RemoteIp, s.RemotePort, bytes(payload))))
    for p in C.TCP_SERVED:
        nif.RecvTcp(p, lambda s, payload, seq, ack, fl, p=p: log.append(("tcp", p, s.RemoteIp, s.RemotePort, bytes(payload),
                                                                        seq, ack, fl)))
    return nif


@pytest.mark.parametrize("l3", [False, True], ids=["frames", "lo_packets"])
def test_dispatch_calls_the_handlers_as_netif_deliver_does(l3):
    """DeliverResult.dispatch over halo_rx_deliver_host's stream == NetIf._deliver over the same
    frames, records from the CPU entry point: the same handler calls in the same order."""
    from halo_amd import cpu, deliver_host, port_map
    from halo_amd.engine import dispatch, dispatch_loopback

    frames = _crafted(l3, False) + ([] if l3 else C.batch(5, 150, "all"))
    data, offs, lens = C.pack(15, frames)
    abi = C.lib_netif()
    recs = cpu.parse_frames_cpu(data, offs.astype(np.uint64) * 4, lens, netif=abi, l3_start=l3)
    want_log, got_log, dhcp_log = [], [], []
    ref = _recording_netif(want_log)
    ref._deliver(frames, recs, (dispatch_loopback if l3 else dispatch)(recs, abi))
    r = deliver_host(data, offs, lens, recs, netif=abi, region_bytes=1 << 20, udp_ports=port_map(ref.UdpServiceMap),
                     tcp_ports=port_map(ref.TcpServiceMap), l3_start=l3, dhcp=True, index_cap=8)
    calls = r.dispatch(_recording_netif(got_log), dhcp=lambda *a: dhcp_log.append(a))
    assert got_log == want_log and len(want_log) > 20
    assert calls == len(got_log) + len(dhcp_log)
    model = DM.want_of(frames, C.model_netif(), l3=l3, udp_ports=C.UDP_SERVED, tcp_ports=C.TCP_SERVED, dhcp=True)
    assert [e for e in model.handler_log() if e[0] != "dhcp"] == got_log
    assert [("dhcp", *a) for a in dhcp_log] == [e for e in model.handler_log() if e[0] == "dhcp"]
    assert len(dhcp_log) == (0 if l3 else 2)
    # records() yields what the stream holds, and the index points at the records
    recs_out = list(r.records())
    assert len(recs_out) == int(r.summary["records_written"]) == len(model.items)
    s = r.stream()
    for e, (h, _) in zip(r.index, recs_out):
        assert int.from_bytes(s[int(e["offset"]):int(e["offset"]) + 4].tobytes(), "little") == int(e["frame"]) == int(h["frame"])
