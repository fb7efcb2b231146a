"""ctypes binding of libhalo_rx.so — the C ABI declared in include/halo_rx.h.

The shared library is built in-tree (``__graft_entry__.build()`` or
``python -m halo_amd.build``) and loaded from ``halo_amd/lib/``. There is no CPU
fallback: if the library is missing, importing this module raises.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")
# HALO_RX_LIB overrides the library path (A/B experiments with alternative builds only)
LIB_PATH = os.environ.get("HALO_RX_LIB") or os.path.join(LIB_DIR, "libhalo_rx.so")

# ---- constants mirrored from include/halo_rx.h ---------------------------------------
HALO_OK = 0
HALO_E_INVAL = -1
HALO_E_NODEV = -2
HALO_E_ARCH = -3
HALO_E_HIP = -4
HALO_E_NOMEM = -5
HALO_E_RANGE = -6

HALO_RX_CSUM_ENABLE = 0x1
HALO_RX_JUMBO_EXT = 0x2
HALO_RX_RECORD_COMPACT = 0x4
HALO_RX_UNIFORM_LEN = 0x8
HALO_RX_L3_START = 0x10  # LoChan packets: every buffer starts at its IPv4 header
HALO_RX_VARIANT_SHIFT = 8
# lanes per frame -> HALO_RX_VARIANT_* (0 = automatic, -1 = the size-class mix kernel,
# -2 = the byte-stream kernel)
_VARIANT_CODE = {0: 0, 1: 1, 4: 2, 8: 3, 16: 4, -1: 5, -2: 6}


def variant_flags(lanes_per_frame: int) -> int:
    """The flags bits that force a kernel variant for one call (HALO_RX_VARIANT_*)."""
    return _VARIANT_CODE[lanes_per_frame] << HALO_RX_VARIANT_SHIFT

STATUS_NAMES = (
    "OK", "ETH_LEN", "ETH_TYPE", "IP_LEN", "IP_VER", "IP_FRAG", "IP_PROTO", "IP_HDR_CKSUM",
    "IP_TOTLEN_UNDERFLOW", "IP_TOTLEN_OVERRUN", "L4_LEN", "ICMP_TYPE", "ICMP_CODE", "L4_CKSUM",
)
STATUS = {name: code for code, name in enumerate(STATUS_NAMES)}
HALO_RX_STATUS_COUNT = len(STATUS_NAMES)

F_MAC_MATCH = 0x01
F_IP_BCAST = 0x02
F_DST_IS_OWN = 0x04

ACTION_NAMES = (
    "DROP_ETH", "IGNORE_MAC", "ARP", "IGNORE_TYPE", "DROP_IP", "BCAST_UDP", "DROP_BCAST_UDP",
    "IGNORE_BCAST", "FORWARD", "LOCAL_ICMP", "LOCAL_UDP", "LOCAL_TCP", "DROP_L4", "LO_NOT_OWN",
)
ACTION = {name: code for code, name in enumerate(ACTION_NAMES)}
HALO_RX_ACT_COUNT = len(ACTION_NAMES)

# halo_rx_result_t (32 bytes, little-endian)
RESULT_DTYPE = np.dtype([
    ("status", "u1"), ("flags", "u1"), ("ethertype", "<u2"),
    ("ip_proto", "u1"), ("l4_aux", "u1"), ("ip_total_len", "<u2"),
    ("src_ip", "<u4"), ("dst_ip", "<u4"),
    ("sport", "<u2"), ("dport", "<u2"),
    ("payload_off", "<u2"), ("payload_len", "<u2"),
    ("l4_seq", "<u4"), ("l4_ack", "<u4"),
])
assert RESULT_DTYPE.itemsize == 32

# halo_rx_record16_t (16 bytes): flags bits 4-5 hold the EtherType class
RECORD16_DTYPE = np.dtype([
    ("status", "u1"), ("flags", "u1"), ("ip_proto", "u1"), ("l4_aux", "u1"),
    ("src_ip", "<u4"), ("dst_ip", "<u4"), ("sport", "<u2"), ("dport", "<u2"),
])
assert RECORD16_DTYPE.itemsize == 16
ET_CLASS = {0x0800: 0x00, 0x0806: 0x10, 0x86DD: 0x20, 0x05DC: 0x30}


def compact_of(full: np.ndarray) -> np.ndarray:
    """The halo_rx_record16_t a full record maps to (host-side reference of the packing)."""
    out = np.zeros(full.shape[0], dtype=RECORD16_DTYPE)
    for f in ("status", "ip_proto", "l4_aux", "src_ip", "dst_ip", "sport", "dport"):
        out[f] = full[f]
    cls = np.zeros(full.shape[0], dtype=np.uint8)
    for et, c in ET_CLASS.items():
        cls[full["ethertype"] == et] = c
    out["flags"] = full["flags"] | cls
    return out

# halo_tx_op_t (16 bytes): per-frame steps of halo_tx_fixup_batch_device
TX_OP_DTYPE = np.dtype([("steps", "u1"), ("pad", "u1"), ("dst_port", "<u2"), ("dst_ip", "<u4"),
                        ("src_port", "<u2"), ("pad2", "<u2"), ("src_ip", "<u4")])
assert TX_OP_DTYPE.itemsize == 16
TX_NAT_DST, TX_TTL, TX_NAT_SRC, TX_RECALC, TX_DPDK_FILL = 0x01, 0x02, 0x04, 0x08, 0x10
TX_R_TTL_ALIVE, TX_R_SKIPPED, TX_R_OVERRUN = 0x01, 0x02, 0x04
# halo_tx_build_desc_t (40 bytes): one locally originated packet for halo_tx_build_batch_device
BUILD_DESC_DTYPE = np.dtype([("payload_off", "<u8"), ("payload_len", "<u2"), ("proto", "u1"), ("aux", "u1"),
                             ("src_port", "<u2"), ("dst_port", "<u2"), ("src_ip", "<u4"), ("dst_ip", "<u4"),
                             ("seq", "<u4"), ("ack", "<u4"), ("dst_mac", "u1", (6,)), ("mode", "u1"),
                             ("pad", "u1")])
assert BUILD_DESC_DTYPE.itemsize == 40
TX_BUILD_ETH, TX_BUILD_LOOPBACK = 0, 1   # HALO_TX_BUILD_*
DEEP_NAT_DTYPE = np.dtype([("lan_ip", "<u4"), ("lan_port", "<u2"), ("found", "u1"), ("pad", "u1")])  # halo_tx_deep_nat_t
TX_B_OK, TX_B_PAYLOAD_LEN, TX_B_PROTO, TX_B_SLOT = 0, 1, 2, 3
FLOW_NAT_LAN, FLOW_NAT_WAN = 0, 1        # HALO_FLOW_*
NAT_SYMMETRIC, NAT_FULL_CONE = 0, 1      # HALO_NAT_* (engine.NatTypeSymmetric / NatTypeFullCone)
ROUTE_DTYPE = np.dtype([("dst_ip", "<u4"), ("network_mask", "<u4"), ("next_hop", "<u4"), ("netif", "<u4")])
ROUTE_NONE, ROUTE_PANIC = 0xFFFFFFFF, 0xFFFFFFFE  # HALO_ROUTE_*
# halo_nat_flow_t (28 bytes), halo_nat_layout_stats_t and the HALO_NAT_V_* verdicts of the NAT lookups
NAT_FLOW_DTYPE = np.dtype([("remote_ip", "<u4"), ("wan_ip", "<u4"), ("lan_ip", "<u4"), ("last_alive", "<u4"),
                           ("remote_port", "<u2"), ("wan_port", "<u2"), ("lan_port", "<u2"), ("proto", "u1"),
                           ("pad", "u1"), ("id", "<u4")])
assert NAT_FLOW_DTYPE.itemsize == 28
NAT_LAYOUT_DTYPE = np.dtype([("slots", "<u4"), ("port_mappings", "<u4"), ("entries", "<u4", (2,)),
                             ("longest_chain", "<u4", (2,)), ("wrapped", "<u4", (2,))])
NAT_NO_FLOW = 0xFFFFFFFF
NAT_MAX_PORT_MAPPINGS = 256
NAT_V_NONE, NAT_V_SKIP, NAT_V_MISS, NAT_V_FLOW, NAT_V_MAPPING, NAT_V_DROP = range(6)
# the miss path: halo_nat_miss_item_t (20 bytes) and halo_nat_answer_t (16 bytes)
NAT_MISS_ITEM_DTYPE = np.dtype([("index", "<u4"), ("src_ip", "<u4"), ("dst_ip", "<u4"), ("sport", "<u2"), ("dport", "<u2"),
                                ("proto", "u1"), ("pad", "u1", (3,))])
NAT_ANSWER_DTYPE = np.dtype([("ip", "<u4"), ("ref", "<u4"), ("port", "<u2"), ("verdict", "u1"), ("pad", "u1", (5,))])
assert NAT_MISS_ITEM_DTYPE.itemsize == 20 and NAT_ANSWER_DTYPE.itemsize == 16
# the L2 switch: halo_sw_result_t (4 bytes), halo_switch_entry_t (12 bytes), halo_switch_layout_stats_t, HALO_SW_V_*
SW_RESULT_DTYPE = np.dtype([("verdict", "u1"), ("out_port", "u1"), ("tx_len", "<u2")])
SW_ENTRY_DTYPE = np.dtype([("mac", "u1", (6,)), ("port", "u1"), ("pad", "u1"), ("create_time", "<u4")])
assert SW_RESULT_DTYPE.itemsize == 4 and SW_ENTRY_DTYPE.itemsize == 12
SW_LAYOUT_DTYPE = np.dtype([("slots", "<u4"), ("entries", "<u4"), ("longest_chain", "<u4"), ("wrapped", "<u4")])
SW_VERDICT_NAMES = ("ETH_LEN", "ETH_TYPE", "SRC_MCAST", "TABLE_FULL", "UNICAST", "FLOOD")
SW_V = {name: code for code, name in enumerate(SW_VERDICT_NAMES)}
SW_V_COUNT = len(SW_VERDICT_NAMES)
SW_MAX_PORTS = 64
# the ARP neighbour cache: halo_arp_entry_t (16 bytes), halo_arp_msg_t (40), halo_arp_result_t (8),
# halo_arp_layout_stats_t, HALO_ARP_H_* / HALO_ARP_GET_* / HALO_ARP_V_*
ARP_ENTRY_DTYPE = np.dtype([("ip", "<u4"), ("mac", "u1", (6,)), ("netif", "u1"), ("pad", "u1"), ("exp_time", "<u4")])
ARP_MSG_DTYPE = np.dtype([("index", "<u4"), ("netif", "u1"), ("pad", "u1"), ("eth_src", "u1", (6,)), ("arp", "u1", (28,))])
ARP_RESULT_DTYPE = np.dtype([("verdict", "u1"), ("out_netif", "u1"), ("tx_len", "<u2"), ("target_ip", "<u4")])
assert ARP_ENTRY_DTYPE.itemsize == 16 and ARP_MSG_DTYPE.itemsize == 40 and ARP_RESULT_DTYPE.itemsize == 8
ARP_LAYOUT_DTYPE = np.dtype([("slots", "<u4"), ("entries", "<u4"), ("longest_chain", "<u4"), ("wrapped", "<u4")])
ARP_H_NAMES = ("BAD_OP", "SRC_MISMATCH", "CONFLICT", "ACCEPTED")
ARP_H = {name: code for code, name in enumerate(ARP_H_NAMES)}
ARP_H_MASK, ARP_H_F_NOT_LEARNED, ARP_H_F_REPLY = 0x0F, 0x40, 0x80
ARP_GET_ABSENT, ARP_GET_FOUND, ARP_GET_OWN_IP = 0, 1, 2
ARP_VERDICT_NAMES = ("NONE", "NO_ROUTE", "ROUTE_PANIC", "LOOPBACK", "OWN_IP", "MISS", "HIT")
ARP_V = {name: code for code, name in enumerate(ARP_VERDICT_NAMES)}
ARP_V_COUNT = len(ARP_VERDICT_NAMES)
ARP_MAX_NETIFS = 64
ARP_AGE, ARP_REFRESH_AHEAD = 300, 10
# port-mapping return flows: halo_pmflow_item_t (20 bytes), halo_pmflow_entry_t (24), halo_pmflow_via_t (8),
# halo_pmflow_layout_stats_t, HALO_PMFLOW_V_*
PMFLOW_ITEM_DTYPE = np.dtype([("index", "<u4"), ("remote_ip", "<u4"), ("lan_ip", "<u4"), ("remote_port", "<u2"),
                              ("lan_port", "<u2"), ("wan_port", "<u2"), ("proto", "u1"), ("pad", "u1")])
PMFLOW_ENTRY_DTYPE = np.dtype([("remote_ip", "<u4"), ("lan_ip", "<u4"), ("last_alive", "<u4"), ("id", "<u4"),
                               ("remote_port", "<u2"), ("lan_port", "<u2"), ("wan_port", "<u2"), ("proto", "u1"),
                               ("wan_netif", "u1")])
PMFLOW_VIA_DTYPE = np.dtype([("verdict", "u1"), ("wan_netif", "u1"), ("wan_port", "<u2"), ("next_hop", "<u4")])
assert PMFLOW_ITEM_DTYPE.itemsize == 20 and PMFLOW_ENTRY_DTYPE.itemsize == 24 and PMFLOW_VIA_DTYPE.itemsize == 8
PMFLOW_LAYOUT_DTYPE = np.dtype([("slots", "<u4"), ("entries", "<u4"), ("longest_chain", "<u4"), ("wrapped", "<u4")])
PMFLOW_VERDICT_NAMES = ("NONE", "MISS", "HIT", "OVERRIDE")
PMFLOW_V = {name: code for code, name in enumerate(PMFLOW_VERDICT_NAMES)}
PMFLOW_V_COUNT = len(PMFLOW_VERDICT_NAMES)
# the egress step: halo_egress_port_t (24 bytes), HALO_EGRESS_KIND_*
EGRESS_PORT_DTYPE = np.dtype([("frames", "<u4"), ("frames_written", "<u4"), ("bytes", "<u8"), ("bytes_written", "<u8")])
assert EGRESS_PORT_DTYPE.itemsize == 24
EGRESS_MAX_PORTS = 64
HALO_LO_TX = 0x100  # halo_lo_config_t.flags: tx mode
LO_NOT_WRITTEN = 0xFFFFFFFF  # d_pkt_off_dw of a packet beyond the written prefix
EGRESS_KIND_MASKS, EGRESS_KIND_ARP, EGRESS_KIND_SWITCH = 0, 1, 2
# the local responders: halo_respond_src_t (8 bytes), HALO_RESPOND_*
RESPOND_SRC_DTYPE = np.dtype([("index", "<u4"), ("kind", "u1"), ("pad", "u1", (3,))])
assert RESPOND_SRC_DTYPE.itemsize == 8
RESPOND_KIND_NAMES = ("ECHO", "TTL", "TCP_SYN", "TCP_SYNACK")
RESPOND_KIND = {name: code for code, name in enumerate(RESPOND_KIND_NAMES)}
RESPOND_KIND_COUNT = len(RESPOND_KIND_NAMES)
# local delivery: halo_deliver_hdr_t (24 bytes), halo_deliver_summary_t (40), halo_deliver_index_t (8), HALO_DELIVER_*
DELIVER_HDR_DTYPE = np.dtype([("frame", "<u4"), ("kind", "u1"), ("tcp_flags", "u1"), ("payload_len", "<u2"),
                              ("remote_ip", "<u4"), ("remote_port", "<u2"), ("local_port", "<u2"), ("seq", "<u4"),
                              ("ack", "<u4")])
DELIVER_SUMMARY_DTYPE = np.dtype([("records", "<u4"), ("records_written", "<u4"), ("bytes", "<u8"),
                                  ("bytes_written", "<u8"), ("kind_counts", "<u4", (3,)), ("skipped", "<u4")])
DELIVER_INDEX_DTYPE = np.dtype([("frame", "<u4"), ("offset", "<u4")])
assert (DELIVER_HDR_DTYPE.itemsize, DELIVER_SUMMARY_DTYPE.itemsize, DELIVER_INDEX_DTYPE.itemsize) == (24, 40, 8)
DELIVER_KIND_NAMES = ("UDP", "TCP", "DHCP")
DELIVER_KIND = {name: code for code, name in enumerate(DELIVER_KIND_NAMES)}
DELIVER_KIND_COUNT = len(DELIVER_KIND_NAMES)
HALO_DELIVER_DHCP = 0x2  # also the bit of halo_deliver_config_t.flags that enables the kind
DELIVER_NOT_WRITTEN = 0xFFFFFFFF  # an index entry's offset beyond the written prefix
# KCP ingest: halo_kcp_dgram_t (40 bytes), halo_kcp_seg_t (32), halo_kcp_summary_t (96), HALO_KCP_*
KCP_DGRAM_DTYPE = np.dtype([("index", "<u4"), ("kind", "u1"), ("conn_type", "u1"), ("ret", "i1"), ("reserved", "u1"),
                            ("conv0", "<u8"), ("n_segs", "<u2"), ("n_walked", "<u2"), ("first_seg", "<u4"),
                            ("payload_len", "<u4"), ("session_id", "<u4"), ("conv", "<u4"), ("enet_type", "<u4")])
KCP_SEG_DTYPE = np.dtype([("dgram", "<u4"), ("cmd", "u1"), ("frg", "u1"), ("wnd", "<u2"), ("ts", "<u4"), ("sn", "<u4"),
                          ("una", "<u4"), ("len", "<u4"), ("data_off", "<u4"), ("check", "u1"), ("reserved", "u1", (3,))])
KCP_SUMMARY_DTYPE = np.dtype([("dgrams", "<u4"), ("dgrams_written", "<u4"), ("segs", "<u4"), ("segs_written", "<u4"),
                              ("ret_counts", "<u4", (5,)), ("enet_counts", "<u4", (4,)), ("ignored", "<u4"),
                              ("bytes_hashed", "<u8"), ("in_pkts", "<u8"), ("in_bytes", "<u8"), ("in_errs", "<u8"),
                              ("in_segs", "<u8")])
assert (KCP_DGRAM_DTYPE.itemsize, KCP_SEG_DTYPE.itemsize, KCP_SUMMARY_DTYPE.itemsize) == (40, 32, 96)
KCP_CHECK_MODES = {"disabled": -1, "zero": 0, "crc32": 1, "xxh3": 2}  # byte_check_mode (kcp.go:34-41)
KCP_DGRAM_KCP, KCP_DGRAM_ENET = 0, 1
KCP_ENET_NAMES = ("ConnEnetSyn", "ConnEnetEst", "ConnEnetFin", "ConnEnetPing")  # conn_type
KCP_SEG_CHECK_NA, KCP_SEG_CHECK_PASSED, KCP_SEG_CHECK_FAILED = 0, 1, 2
# KCP emit: halo_kcp_out_session_t (40 bytes), halo_kcp_out_dgram_t (16), halo_kcp_emit_summary_t (88), HALO_KCP_EMIT_*
KCP_OUT_SESSION_DTYPE = np.dtype([("conv", "<u8"), ("first_seg", "<u4"), ("n_segs", "<u4"), ("dst_ip", "<u4"), ("dst_port", "<u2"),
                                  ("mtu", "<u2"), ("kind", "u1"), ("conn_type", "u1"), ("reserved", "<u2"), ("session_id", "<u4"),
                                  ("enet_conv", "<u4"), ("enet_type", "<u4")])
KCP_OUT_DGRAM_DTYPE = np.dtype([("offset", "<u4"), ("len", "<u2"), ("n_segs", "<u2"), ("session", "<u4"), ("first_seg", "<u4")])
KCP_EMIT_SUMMARY_DTYPE = np.dtype([("sessions", "<u4"), ("sessions_written", "<u4"), ("dgrams", "<u4"), ("dgrams_written", "<u4"),
                                   ("segs", "<u4"), ("segs_written", "<u4"), ("status_counts", "<u4", (4,)), ("bytes", "<u8"),
                                   ("bytes_written", "<u8"), ("bytes_hashed", "<u8"), ("out_segs", "<u8"), ("out_pkts", "<u8"),
                                   ("out_bytes", "<u8")])
assert (KCP_OUT_SESSION_DTYPE.itemsize, KCP_OUT_DGRAM_DTYPE.itemsize, KCP_EMIT_SUMMARY_DTYPE.itemsize) == (40, 16, 88)
KCP_EMIT_STATUS_NAMES = ("OK", "SEG_TOO_LONG", "BAD_MTU", "BAD_RANGE")
KCP_EMIT_STATUS = {name: code for code, name in enumerate(KCP_EMIT_STATUS_NAMES)}
KCP_EMIT_MAX = 1 << 23
# DHCP: halo_dhcp_msg_t (128 bytes), halo_dhcp_summary_t (64), halo_dhcp_lease_t (80), halo_dhcp_reply_t (32),
# halo_dhcp_client_event_t (24), HALO_DHCP_*
DHCP_MSG_DTYPE = np.dtype([("index", "<u4"), ("status", "u1"), ("dir", "u1"), ("msg_type", "u1"), ("reserved0", "u1"),
                           ("options", "<u4"), ("xid", "u1", (4,)), ("yiaddr", "<u4"), ("chaddr", "u1", (6,)),
                           ("payload_len", "<u2"), ("remote_ip", "<u4"), ("req_ip", "<u4"), ("mask", "u1", (4,)),
                           ("gateway", "u1", (4,)), ("dns", "u1", (4,)), ("mask_n", "u1"), ("gateway_n", "u1"),
                           ("reserved1", "u1", (2,)), ("reserved2", "<u4", (3,)), ("hostname", "u1", (64,))])
DHCP_SUMMARY_DTYPE = np.dtype([("msgs", "<u4"), ("msgs_written", "<u4"), ("status_counts", "<u4", (5,)),
                               ("type_counts", "<u4", (9,))])
DHCP_LEASE_DTYPE = np.dtype([("ip", "<u4"), ("mac", "u1", (6,)), ("reserved", "<u2"), ("exp_time", "<u4"),
                             ("hostname", "u1", (64,))])
DHCP_REPLY_DTYPE = np.dtype([("kind", "u1"), ("reserved0", "u1", (3,)), ("xid", "u1", (4,)), ("yiaddr", "<u4"),
                             ("chaddr", "u1", (6,)), ("reserved1", "<u2"), ("req_ip", "<u4"), ("server_id", "<u4"),
                             ("reserved2", "<u4")])
DHCP_EVENT_DTYPE = np.dtype([("msg", "<u4"), ("ip", "<u4"), ("mask", "u1", (4,)), ("gateway", "u1", (4,)), ("dns", "u1", (4,)),
                             ("mask_n", "u1"), ("gateway_n", "u1"), ("options", "u1"), ("reserved", "u1")])
assert (DHCP_MSG_DTYPE.itemsize, DHCP_SUMMARY_DTYPE.itemsize, DHCP_LEASE_DTYPE.itemsize, DHCP_REPLY_DTYPE.itemsize,
        DHCP_EVENT_DTYPE.itemsize) == (128, 64, 80, 32, 24)
DHCP_STATUS_NAMES = ("OK", "PORTS", "SHORT", "COOKIE", "REF_PANIC")
DHCP_STATUS = {name: code for code, name in enumerate(DHCP_STATUS_NAMES)}
DHCP_TO_SERVER, DHCP_TO_CLIENT, DHCP_DIR_NONE = 0, 1, 2
DHCP_OPT_MASK, DHCP_OPT_ROUTER, DHCP_OPT_DNS, DHCP_OPT_HOSTNAME = 0x01, 0x02, 0x04, 0x08
DHCP_OPT_REQ_IP, DHCP_OPT_MSG_TYPE, DHCP_OPT_DNS_SHORT = 0x10, 0x20, 0x40
DHCP_DISCOVER, DHCP_OFFER, DHCP_REQUEST, DHCP_ACK, DHCP_NAK, DHCP_RELEASE = 1, 2, 3, 5, 6, 7
DHCP_H_NAMES = ("NONE", "OFFER", "NO_ADDR", "NO_REQ_IP", "NAK_ZERO", "NAK_SUBNET", "NAK_OTHER_MAC", "NAK_FULL", "ACK_NAK",
                "REF_PANIC", "RELEASED", "RELEASE_ABSENT", "CLIENT_REQUEST", "CLIENT_ACK")
DHCP_H = {name: code for code, name in enumerate(DHCP_H_NAMES)}
DHCP_H_MASK, DHCP_H_F_REUSED, DHCP_H_F_REPLY = 0x0F, 0x40, 0x80
DHCP_SLOT_BYTES = 288
DHCP_BUILD_MAX = 1 << 23
# halo_rx_ring_scan_t (24 bytes) and HALO_RING_STOP_* / HALO_RING_REGISTER
RING_SCAN_DTYPE = np.dtype([("n_frames", "<u4"), ("stop", "<u4"), ("end_bytes", "<u8"), ("max_len", "<u4"),
                            ("pad", "<u4")])
assert RING_SCAN_DTYPE.itemsize == 24
# halo_rx_ring_stats_t (8 x u64)
RING_STATS_DTYPE = np.dtype([(k, "<u8") for k in ("polls", "frames", "small_polls", "service_requests",
                                                  "service_launches", "walk_ns", "wait_ns", "service_gpu_ns")])
# halo_rx_host_stats_t (8 x u64)
HOST_STATS_DTYPE = np.dtype([(k, "<u8") for k in ("calls", "frames", "resident_calls", "resident_parked",
                                                  "service_launches", "pack_ns", "wait_ns", "service_gpu_ns")])
RING_STOP_NAMES = ("EMPTY", "BAD_LEN", "PARTIAL", "CAPACITY", "MAX", "BAD_CURSOR")
RING_STOP = {name: code for code, name in enumerate(RING_STOP_NAMES)}
RING_REGISTER = 0x1
RING_PERSISTENT = 0x2  # HALO_RING_PERSISTENT: small polls served by a resident consumer kernel
# the tx ring producer: halo_tx_ring_result_t (24 bytes), HALO_TXRING_*
TXRING_RESULT_DTYPE = np.dtype([("status", "<u4"), ("records", "<u4"), ("bytes", "<u8"), ("head", "<u8")])
assert TXRING_RESULT_DTYPE.itemsize == 24
TXRING_STATUS_NAMES = ("OK", "SHORT", "BAD_SPAN")
TXRING_OK, TXRING_SHORT, TXRING_BAD_SPAN = 0, 1, 2
TXRING_MAX_RECORD = 16376

def host_array(shape, dtype=np.uint8) -> np.ndarray:
    """A zeroed host array on pages of its own: an anonymous mmap, page-aligned, its size rounded
    up to whole pages, unmapped when the array is freed. For every buffer handed to
    ``halo_rx_host_register`` or attached with ``RING_REGISTER``: hipHostRegister pins whole pages,
    so a heap array (np.zeros) can share its first or last page with an unrelated allocation that
    outlives the registration, and a later transfer that pins that neighbour in place then meets a
    stale mapping. Pages that only this array uses go back to the OS with it."""
    import mmap

    dt = np.dtype(dtype)
    shape = (shape,) if isinstance(shape, (int, np.integer)) else tuple(shape)
    nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
    size = max(mmap.PAGESIZE, -(-nbytes // mmap.PAGESIZE) * mmap.PAGESIZE)
    buf = mmap.mmap(-1, size, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS)
    return np.frombuffer(buf, dtype=np.uint8, count=nbytes).view(dt).reshape(shape)

def host_pages(nbytes: int) -> int:
    """The whole-page size host_array maps for `nbytes` (what a registration of it covers)."""
    import mmap

    return max(mmap.PAGESIZE, -(-int(nbytes) // mmap.PAGESIZE) * mmap.PAGESIZE)


_leaked: list = []  # host arrays whose registration could not be removed: never freed


class registered:
    """``with registered(arr):`` — halo_rx_host_register over the whole pages of a host_array for
    the block, unregistered on exit even when the block raises. If the unregistration fails the
    array is kept alive for the rest of the process (its pages may still be mapped for the
    device) and HaloError is raised."""

    def __init__(self, arr: np.ndarray):
        self.arr = arr

    def __enter__(self):
        check("halo_rx_host_register", lib.halo_rx_host_register(self.arr.ctypes.data, host_pages(self.arr.nbytes)))
        return self.arr

    def __exit__(self, *exc):
        rc = lib.halo_rx_host_unregister(self.arr.ctypes.data)
        if rc != HALO_OK:
            _leaked.append(self.arr)
            if exc[0] is None:
                check("halo_rx_host_unregister", rc)
        return False


def registered_count() -> int:
    """Live host registrations made through the library (halo_rx_host_registered_count)."""
    return int(lib.halo_rx_host_registered_count())


def registrations() -> list:
    """(base, bytes) of every live registration, in address order."""
    n = int(lib.halo_rx_host_registrations(None, None, 0))
    bases = (ctypes.c_void_p * max(n, 1))()
    sizes = (ctypes.c_uint64 * max(n, 1))()
    n = int(lib.halo_rx_host_registrations(bases, sizes, n))
    return [(int(bases[i] or 0), int(sizes[i])) for i in range(n)]


RING_HEADER = 128  # sizeof(RingBuffer), mem/ring_buffer.go:18-26


class NetIf(ctypes.Structure):
    """halo_rx_netif_t — engine.NetIfConfig's MacAddr / IpAddr / NatEnable."""

    _fields_ = [
        ("mac", ctypes.c_uint8 * 6),
        ("pad", ctypes.c_uint8 * 2),
        ("ip", ctypes.c_uint32),
        ("nat_enable", ctypes.c_uint32),
    ]

    @classmethod
    def make(cls, mac: str = "AA:AA:AA:AA:AA:AA", ip: str = "192.168.100.100", nat_enable: bool = False):
        """Parse addresses like protocol.ParseMacAddr / ParseIpAddr (protocol/utils.go:57-82)."""
        n = cls()
        for i, part in enumerate(mac.split(":")[:6]):
            n.mac[i] = int(part, 16)
        a = [int(x) for x in ip.split(".")[:4]]
        n.ip = (a[0] << 24) | (a[1] << 16) | (a[2] << 8) | a[3]  # IpAddrToU (utils.go:34-44)
        n.nat_enable = 1 if nat_enable else 0
        return n


class NatConfig(ctypes.Structure):
    """halo_nat_config_t."""

    _fields_ = [("wan_ip", ctypes.c_uint32), ("nat_type", ctypes.c_uint32), ("capacity_log2", ctypes.c_uint32),
                ("pad", ctypes.c_uint32)]


class SwitchConfig(ctypes.Structure):
    """halo_switch_config_t."""

    _fields_ = [("n_ports", ctypes.c_uint32), ("vlan_id", ctypes.c_uint16 * 64), ("capacity", ctypes.c_uint32),
                ("slots_log2", ctypes.c_uint32), ("max_batch", ctypes.c_uint32), ("device", ctypes.c_int)]


class ArpConfig(ctypes.Structure):
    """halo_arp_config_t."""

    _fields_ = [("n_netifs", ctypes.c_uint32), ("netif", NetIf * 64), ("capacity", ctypes.c_uint32),
                ("slots_log2", ctypes.c_uint32)]


class PmflowConfig(ctypes.Structure):
    """halo_pmflow_config_t."""

    _fields_ = [("n_netifs", ctypes.c_uint32), ("netif", NetIf * 64), ("gateway", ctypes.c_uint32 * 64),
                ("capacity", ctypes.c_uint32), ("capacity_log2", ctypes.c_uint32)]


class LoConfig(ctypes.Structure):
    """halo_lo_config_t."""

    _fields_ = [("n_netifs", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("region_bytes", ctypes.c_uint64),
                ("index_cap", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class EgressConfig(ctypes.Structure):
    """halo_egress_config_t."""

    _fields_ = [("n_ports", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("region_bytes", ctypes.c_uint64),
                ("index_cap", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


assert ctypes.sizeof(EgressConfig) == 24


class DeliverConfig(ctypes.Structure):
    """halo_deliver_config_t."""

    _fields_ = [("flags", ctypes.c_uint32), ("index_cap", ctypes.c_uint32), ("region_bytes", ctypes.c_uint64)]


assert ctypes.sizeof(DeliverConfig) == 16


class KcpConfig(ctypes.Structure):
    """halo_kcp_config_t."""

    _fields_ = [("byte_check_mode", ctypes.c_int32), ("port", ctypes.c_uint32), ("dgram_cap", ctypes.c_uint32),
                ("seg_cap", ctypes.c_uint32)]


assert ctypes.sizeof(KcpConfig) == 16


class KcpEmitConfig(ctypes.Structure):
    """halo_kcp_emit_config_t."""

    _fields_ = [("byte_check_mode", ctypes.c_int32), ("src_ip", ctypes.c_uint32), ("src_port", ctypes.c_uint32),
                ("dgram_cap", ctypes.c_uint32), ("stream_cap", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


assert ctypes.sizeof(KcpEmitConfig) == 24


class DhcpConfig(ctypes.Structure):
    """halo_dhcp_config_t."""

    _fields_ = [("ip", ctypes.c_uint32), ("network_mask", ctypes.c_uint32), ("dns", ctypes.c_uint32),
                ("mac", ctypes.c_uint8 * 6), ("server_enable", ctypes.c_uint8), ("client_enable", ctypes.c_uint8),
                ("capacity", ctypes.c_uint32)]


assert ctypes.sizeof(DhcpConfig) == 24


class BatchDesc(ctypes.Structure):
    """halo_rx_batch_desc_t — one batch of halo_rx_parse_batches_device."""

    _fields_ = [("d_bytes", ctypes.c_void_p), ("d_offsets_dw", ctypes.c_void_p), ("d_lens", ctypes.c_void_p),
                ("d_out", ctypes.c_void_p), ("n", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


assert ctypes.sizeof(BatchDesc) == 40

_u8p = ctypes.c_void_p
_PROTOS = {
    "halo_rx_version": (ctypes.c_char_p, []),
    "halo_rx_init": (ctypes.c_int, [ctypes.c_int]),
    "halo_rx_debug_hist_keys": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_uint32]),
    "halo_rx_device_synchronize": (ctypes.c_int, [ctypes.c_int]),
    "halo_rx_release": (ctypes.c_int, [ctypes.c_int]),
    "halo_rx_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "halo_rx_status_name": (ctypes.c_char_p, [ctypes.c_int]),
    "halo_rx_parse_batch_device": (ctypes.c_int, [
        _u8p, _u8p, _u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(NetIf), ctypes.c_uint32,
        _u8p, _u8p, ctypes.c_void_p]),
    "halo_rx_parse_strided_device": (ctypes.c_int, [
        _u8p, ctypes.c_uint64, _u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
        ctypes.POINTER(NetIf), _u8p, _u8p, ctypes.c_void_p]),
    "halo_rx_parse_batches_device": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(NetIf), ctypes.c_uint32, _u8p,
        ctypes.c_void_p]),
    "halo_rx_host_ctx_create": (ctypes.c_int, [
        ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)]),
    "halo_rx_host_ctx_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "halo_rx_host_ctx_set_zero_copy": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "halo_rx_host_ctx_set_resident": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64]),
    "halo_rx_host_ctx_set_service_timeout": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "halo_rx_host_ctx_get_stats": (ctypes.c_int, [ctypes.c_void_p, _u8p]),
    "halo_rx_parse_batch_host": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, _u8p, _u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(NetIf),
        _u8p, _u8p]),
    "halo_rx_host_register": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "halo_rx_host_unregister": (ctypes.c_int, [ctypes.c_void_p]),
    "halo_rx_host_registered_count": (ctypes.c_uint32, []),
    "halo_rx_host_registrations": (ctypes.c_uint32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]),
    "halo_rx_dispatch": (ctypes.c_int, [_u8p, ctypes.c_uint32, ctypes.POINTER(NetIf), _u8p, _u8p]),
    "halo_rx_dispatch_compact": (ctypes.c_int, [_u8p, ctypes.c_uint32, ctypes.POINTER(NetIf), _u8p, _u8p]),
    "halo_rx_dispatch_loopback": (ctypes.c_int, [_u8p, ctypes.c_uint32, ctypes.POINTER(NetIf), _u8p, _u8p]),
    "halo_tx_icmp_deep_nat_batch_device": (ctypes.c_int, [
        _u8p, _u8p, _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint32, _u8p, _u8p, ctypes.c_void_p]),
    "halo_tx_fixup_batch_device": (ctypes.c_int, [
        _u8p, _u8p, _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u8p, ctypes.c_void_p]),
    "halo_tx_build_workspace": (ctypes.c_uint64, [ctypes.c_uint32]),
    "halo_tx_build_batch_device": (ctypes.c_int, [
        _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint32, ctypes.POINTER(NetIf), ctypes.c_uint32, _u8p, ctypes.c_uint32,
        _u8p, _u8p, _u8p, _u8p, ctypes.c_uint64, ctypes.c_void_p]),
    "halo_xxh3_64_batch_device": (ctypes.c_int, [_u8p, _u8p, _u8p, ctypes.c_uint32, _u8p, ctypes.c_void_p]),
    "halo_rx_parse_flow_batch_device": (ctypes.c_int, [
        _u8p, _u8p, _u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(NetIf), ctypes.c_uint32, _u8p, _u8p,
        ctypes.c_uint32, ctypes.c_uint32, _u8p, ctypes.c_uint32, _u8p, ctypes.c_void_p]),
    "halo_rx_parse_route_batch_device": (ctypes.c_int, [
        _u8p, _u8p, _u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(NetIf), ctypes.c_uint32, _u8p, _u8p,
        ctypes.c_void_p, _u8p, ctypes.c_void_p]),
    "halo_flow_hash_device": (ctypes.c_int, [
        _u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _u8p, ctypes.c_uint32, _u8p, ctypes.c_void_p]),
    "halo_flow_hash_compact_device": (ctypes.c_int, [
        _u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _u8p, ctypes.c_uint32, _u8p, ctypes.c_void_p]),
    "halo_route_table_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p)]),
    "halo_route_table_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "halo_route_update": (ctypes.c_int, [ctypes.c_void_p, _u8p, _u8p, ctypes.POINTER(ctypes.c_uint32)]),
    "halo_route_get": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, _u8p]),
    "halo_route_sync_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "halo_route_lookup_device": (ctypes.c_int, [ctypes.c_void_p, _u8p, ctypes.c_uint32, _u8p, ctypes.c_void_p]),
    "halo_route_lookup_records_device": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, ctypes.c_uint32, _u8p, ctypes.c_void_p]),
    "halo_nat_table_create": (ctypes.c_int, [ctypes.POINTER(NatConfig), ctypes.POINTER(ctypes.c_void_p)]),
    "halo_nat_table_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "halo_nat_port_mapping_add": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint16, ctypes.c_uint8]),
    "halo_nat_add_flow": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint16, ctypes.c_uint16, ctypes.c_uint8,
        ctypes.c_uint32, _u8p, ctypes.POINTER(ctypes.c_uint32)]),
    "halo_nat_get_flow_lan": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint16, ctypes.c_uint8, _u8p,
        ctypes.POINTER(ctypes.c_uint32)]),
    "halo_nat_get_flow_wan": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint16, ctypes.c_uint8, _u8p,
        ctypes.POINTER(ctypes.c_uint32)]),
    "halo_nat_resolve_misses": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_uint32, _u8p, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u8p, _u8p,
        ctypes.POINTER(ctypes.c_uint32)]),
    "halo_nat_expire": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
    "halo_nat_list": (ctypes.c_int, [ctypes.c_void_p, _u8p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
    "halo_nat_layout_stats": (ctypes.c_int, [ctypes.c_void_p, _u8p]),
    "halo_nat_sync_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    **{f"halo_nat_lookup_{d}{c}_device": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u8p, _u8p, _u8p, _u8p, _u8p, ctypes.c_void_p])
       for d in ("wan", "lan") for c in ("", "_compact")},
    "halo_nat_lookup_quote_device": (ctypes.c_int, [ctypes.c_void_p, _u8p, ctypes.c_uint32, _u8p, ctypes.c_void_p]),
    "halo_nat_miss_workspace": (ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint32]),
    **{f"halo_nat_collect_misses{c}_device": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_uint32, _u8p, _u8p, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u8p, ctypes.c_uint32,
        _u8p, _u8p, _u8p, ctypes.c_uint64, ctypes.c_void_p]) for c in ("", "_compact")},
    "halo_nat_collect_misses_host": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_uint32, _u8p, _u8p, _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint32, _u8p, _u8p]),
    "halo_nat_resolve_items": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_uint32, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u8p, ctypes.POINTER(ctypes.c_uint32)]),
    "halo_nat_apply_answers_device": (ctypes.c_int, [
        ctypes.c_uint32, _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint32, _u8p, _u8p, _u8p, _u8p, ctypes.c_void_p]),
    "halo_switch_create": (ctypes.c_int, [ctypes.POINTER(SwitchConfig), ctypes.POINTER(ctypes.c_void_p)]),
    "halo_switch_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "halo_switch_flood_mask": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]),
    "halo_switch_forward": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_uint32, _u8p, _u8p, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u8p, _u8p,
        ctypes.c_void_p]),
    "halo_switch_expire": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
    "halo_switch_list": (ctypes.c_int, [ctypes.c_void_p, _u8p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
    "halo_switch_layout_stats": (ctypes.c_int, [ctypes.c_void_p, _u8p]),
    "halo_switch_debug_set_epoch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]),
    "halo_arp_table_create": (ctypes.c_int, [ctypes.POINTER(ArpConfig), ctypes.POINTER(ctypes.c_void_p)]),
    "halo_arp_table_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "halo_arp_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, _u8p, ctypes.c_uint32]),
    "halo_arp_get": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, _u8p, ctypes.POINTER(ctypes.c_uint32)]),
    "halo_arp_handle_msgs": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u8p, _u8p, ctypes.POINTER(ctypes.c_uint32),
        ctypes.POINTER(ctypes.c_uint32)]),
    "halo_arp_build_request": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, _u8p]),
    "halo_arp_expire": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
    "halo_arp_refresh_list": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_uint32, _u8p, _u8p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
    "halo_arp_list": (ctypes.c_int, [ctypes.c_void_p, _u8p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
    "halo_arp_layout_stats": (ctypes.c_int, [ctypes.c_void_p, _u8p]),
    "halo_arp_dirty": (ctypes.c_int, [ctypes.c_void_p]),
    "halo_arp_sync_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "halo_arp_lookup_device": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u8p, _u8p, _u8p, ctypes.c_void_p]),
    "halo_arp_encap_device": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, _u8p, _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint32, _u8p, _u8p, _u8p, _u8p,
        ctypes.c_void_p]),
    "halo_arp_gather_workspace": (ctypes.c_uint64, [ctypes.c_uint32]),
    "halo_arp_gather_device": (ctypes.c_int, [
        _u8p, _u8p, _u8p, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u8p, ctypes.c_uint32, _u8p, _u8p, ctypes.c_uint64,
        ctypes.c_void_p]),
    "halo_rx_shard_multi": (ctypes.c_int, [
        _u8p, ctypes.c_uint32, _u8p, _u8p, _u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(NetIf), _u8p,
        _u8p, _u8p]),
    "halo_rx_ring_attach": (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32,
        ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]),
    "halo_rx_ring_detach": (ctypes.c_int, [ctypes.c_void_p]),
    "halo_rx_ring_poll": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(NetIf), _u8p, _u8p, _u8p, _u8p]),
    "halo_rx_ring_commit": (ctypes.c_int, [ctypes.c_void_p]),
    "halo_rx_ring_get_stats": (ctypes.c_int, [ctypes.c_void_p, _u8p]),
    "halo_rx_ring_set_small_poll": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "halo_rx_ring_set_service_timeout": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "halo_rx_ring_scan_workspace": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint32]),
    "halo_rx_ring_scan_device": (ctypes.c_int, [
        _u8p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _u8p, _u8p, _u8p, _u8p,
        ctypes.c_uint64, ctypes.c_void_p]),
    "halo_ring_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "halo_ring_write_batch": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, _u8p, _u8p, ctypes.c_uint32, _u8p, ctypes.POINTER(ctypes.c_uint32)]),
    "halo_ring_write_span": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)]),
    "halo_tx_ring_attach": (ctypes.c_int, [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]),
    "halo_tx_ring_detach": (ctypes.c_int, [ctypes.c_void_p]),
    "halo_tx_ring_workspace": (ctypes.c_uint64, [ctypes.c_uint64]),
    "halo_tx_ring_write_span_device": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, ctypes.c_uint64, _u8p, _u8p, ctypes.c_uint64, ctypes.c_void_p]),
    "halo_tx_ring_debug_copy_mode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]),
    "halo_tx_egress_workspace": (ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint32]),
    "halo_tx_egress_masks_device": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, _u8p, _u8p, ctypes.c_uint32, _u8p, _u8p, _u8p, _u8p, _u8p, _u8p, ctypes.c_uint64,
        ctypes.c_void_p]),
    "halo_tx_egress_arp_device": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, _u8p, _u8p, ctypes.c_uint32, _u8p, _u8p, _u8p, _u8p, _u8p, _u8p, ctypes.c_uint64,
        ctypes.c_void_p]),
    "halo_tx_egress_switch_device": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, _u8p, _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint64, _u8p, _u8p, _u8p, _u8p, _u8p,
        ctypes.c_uint64, ctypes.c_void_p]),
    "halo_tx_egress_host": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_uint32, _u8p, _u8p, _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint64, _u8p, _u8p, _u8p,
        _u8p]),
    "halo_arp_encap_tx_device": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, _u8p, _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint32, _u8p, _u8p, _u8p, _u8p,
        ctypes.c_void_p]),
    "halo_pmflow_table_create": (ctypes.c_int, [ctypes.POINTER(PmflowConfig), ctypes.POINTER(ctypes.c_void_p)]),
    "halo_pmflow_table_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "halo_pmflow_record": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_uint32, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u8p, ctypes.POINTER(ctypes.c_uint32)]),
    "halo_pmflow_get": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint16, ctypes.c_uint8,
        ctypes.POINTER(ctypes.c_uint32), _u8p, ctypes.POINTER(ctypes.c_uint32)]),
    "halo_pmflow_expire": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
    "halo_pmflow_list": (ctypes.c_int, [ctypes.c_void_p, _u8p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
    "halo_pmflow_layout_stats": (ctypes.c_int, [ctypes.c_void_p, _u8p]),
    "halo_pmflow_dirty": (ctypes.c_int, [ctypes.c_void_p]),
    "halo_pmflow_sync_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "halo_pmflow_lookup_device": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u8p, _u8p, _u8p, _u8p, _u8p, _u8p, ctypes.c_void_p]),
    "halo_pmflow_record_workspace": (ctypes.c_uint64, [ctypes.c_uint32]),
    "halo_pmflow_record_device": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_uint32, _u8p, _u8p, _u8p, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u8p,
        ctypes.c_uint32, _u8p, _u8p, ctypes.c_uint64, ctypes.c_void_p]),
    "halo_arp_drop_device": (ctypes.c_int, [_u8p, _u8p, ctypes.c_uint32, ctypes.c_void_p]),
    "halo_arp_encap_via_device": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, _u8p, _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint32, _u8p, _u8p, _u8p, _u8p, _u8p,
        ctypes.c_void_p]),
    "halo_tx_respond_workspace": (ctypes.c_uint64, [ctypes.c_uint32]),
    "halo_tx_respond_device": (ctypes.c_int, [
        _u8p, _u8p, _u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(NetIf), _u8p, _u8p, _u8p, _u8p, _u8p, _u8p,
        _u8p, ctypes.c_uint32, _u8p, _u8p, _u8p, _u8p, ctypes.c_uint64, ctypes.c_void_p]),
    "halo_tx_respond_host": (ctypes.c_int, [
        _u8p, _u8p, _u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(NetIf), _u8p, _u8p, _u8p, _u8p, _u8p, _u8p,
        _u8p, ctypes.c_uint32, _u8p, _u8p, _u8p]),
    "halo_rx_deliver_workspace": (ctypes.c_uint64, [ctypes.c_uint32]),
    "halo_rx_deliver_device": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, _u8p, _u8p, _u8p, ctypes.c_uint32, ctypes.POINTER(NetIf), _u8p, _u8p, _u8p, _u8p, _u8p,
        _u8p, ctypes.c_uint64, ctypes.c_void_p]),
    "halo_rx_deliver_host": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, _u8p, _u8p, _u8p, ctypes.c_uint32, ctypes.POINTER(NetIf), _u8p, _u8p, _u8p, _u8p, _u8p]),
    "halo_kcp_ingest_workspace": (ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint32]),
    "halo_kcp_ingest_device": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, _u8p, _u8p, ctypes.c_uint32, _u8p, _u8p, _u8p, _u8p, ctypes.c_uint64, ctypes.c_void_p]),
    "halo_kcp_ingest_host": (ctypes.c_int, [ctypes.c_void_p, _u8p, _u8p, _u8p, ctypes.c_uint32, _u8p, _u8p, _u8p]),
    "halo_kcp_emit_workspace": (ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint32]),
    "halo_kcp_emit_device": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint64, _u8p, _u8p, _u8p, _u8p, _u8p,
        _u8p, ctypes.c_uint64, ctypes.c_void_p]),
    "halo_kcp_emit_host": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint64, _u8p, _u8p, _u8p, _u8p, _u8p]),
    "halo_dhcp_decode_workspace": (ctypes.c_uint64, [ctypes.c_uint32]),
    "halo_dhcp_decode_device": (ctypes.c_int, [
        _u8p, _u8p, _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint32, _u8p, _u8p, ctypes.c_uint64, ctypes.c_void_p]),
    "halo_dhcp_decode_host": (ctypes.c_int, [_u8p, _u8p, _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint32, _u8p]),
    "halo_dhcp_server_create": (ctypes.c_int, [ctypes.POINTER(DhcpConfig), ctypes.POINTER(ctypes.c_void_p)]),
    "halo_dhcp_server_destroy": (None, [ctypes.c_void_p]),
    "halo_dhcp_handle_msgs": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, ctypes.c_uint32, ctypes.c_uint64, _u8p, ctypes.c_uint32, _u8p, ctypes.POINTER(ctypes.c_uint32),
        _u8p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
    "halo_dhcp_list": (ctypes.c_uint32, [ctypes.c_void_p, _u8p, ctypes.c_uint32]),
    "halo_dhcp_clear": (ctypes.c_uint32, [ctypes.c_void_p, ctypes.c_uint64]),
    "halo_dhcp_set_dns": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]),
    "halo_dhcp_set_client_xid": (ctypes.c_int, [ctypes.c_void_p, _u8p]),
    "halo_dhcp_discover": (ctypes.c_int, [ctypes.c_void_p, _u8p, _u8p]),
    "halo_dhcp_server_config": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(DhcpConfig)]),
    "halo_dhcp_reply_build_device": (ctypes.c_int, [
        ctypes.POINTER(DhcpConfig), _u8p, ctypes.c_uint32, _u8p, _u8p, ctypes.c_void_p]),
    "halo_dhcp_reply_build_host": (ctypes.c_int, [ctypes.POINTER(DhcpConfig), _u8p, ctypes.c_uint32, _u8p, _u8p]),
    "halo_arp_loopback_mark_device": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint32, _u8p, _u8p, ctypes.c_void_p]),
    "halo_lo_gather_workspace": (ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint32]),
    "halo_lo_gather_device": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, _u8p, _u8p, ctypes.c_uint32, _u8p, _u8p, _u8p, _u8p, _u8p, _u8p, _u8p, _u8p, ctypes.c_uint64,
        ctypes.c_void_p]),
    "halo_lo_gather_host": (ctypes.c_int, [
        ctypes.c_void_p, _u8p, _u8p, _u8p, ctypes.c_uint32, _u8p, _u8p, _u8p, _u8p, _u8p, _u8p, _u8p]),
    "halo_synth_layout": (ctypes.c_int, [
        ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
        ctypes.c_uint32, ctypes.c_uint32, _u8p, _u8p, _u8p, ctypes.POINTER(ctypes.c_uint64)]),
    "halo_synth_frames_device": (ctypes.c_int, [
        ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, _u8p, _u8p, ctypes.c_uint64, _u8p,
        ctypes.POINTER(NetIf), _u8p, ctypes.c_void_p]),
}


class HaloError(RuntimeError):
    def __init__(self, fn: str, code: int):
        super().__init__(f"{fn} failed: {code} ({strerror(code)})")
        self.code = code


def _same_hip_runtime_as_torch() -> None:
    """One HIP runtime per process. libhalo_rx.so needs libamdhip64.so.7; PyTorch-ROCm ships its own
    copy (same soname) and links it by the name libamdhip64.so. Whichever loads first decides: if
    torch comes first, our library binds to torch's copy; if we came first with /opt/rocm's, torch
    would later load its copy as a SECOND runtime, and the two fight over the device (every call
    here then fails with HALO_E_NODEV). So when torch is installed, load its runtime first (without
    importing torch). Processes without torch (a cgo host) use the system runtime."""
    import importlib.util

    if "torch" in __import__("sys").modules:
        return
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    rt = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(rt):
        ctypes.CDLL(rt, mode=ctypes.RTLD_GLOBAL)


def _load() -> ctypes.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP library first "
            "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    _same_hip_runtime_as_torch()
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def strerror(code: int) -> str:
    return lib.halo_rx_strerror(code).decode()


def check(fn: str, code: int) -> None:
    if code != HALO_OK:
        raise HaloError(fn, code)


def device_synchronize(device: int = 0) -> None:
    """hipDeviceSynchronize for `device` after parking this library's resident consumers there
    (halo_rx_device_synchronize): use it instead of torch.cuda.synchronize() while a persistent ring
    or a resident host context is live, which a plain device sync would wait on."""
    check("halo_rx_device_synchronize", lib.halo_rx_device_synchronize(device))


def ptr(x) -> int | None:
    """Device/host address of a torch tensor or numpy array (None for None)."""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return x.ctypes.data
