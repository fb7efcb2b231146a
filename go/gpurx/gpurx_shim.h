/*
 * gpurx_shim.h — the C side of package gpurx's cgo preamble (included by gpurx.go and parse.go;
 * static inline, so each cgo file gets its own copy). Compiled and run against include/halo_rx.h
 * and libhalo_rx.so by tests/test_go_binding.py, since this image has no Go toolchain.
 */
#ifndef GPURX_SHIM_H
#define GPURX_SHIM_H
#include <stddef.h>
#include <string.h>

#include "halo_rx.h"

// The Go mirrors below must keep these layouts.
_Static_assert(sizeof(halo_rx_result_t) == 32, "halo_rx_result_t is 32 bytes");
_Static_assert(offsetof(halo_rx_result_t, src_ip) == 8, "halo_rx_result_t.src_ip");
_Static_assert(offsetof(halo_rx_result_t, payload_off) == 20, "halo_rx_result_t.payload_off");
_Static_assert(offsetof(halo_rx_result_t, l4_ack) == 28, "halo_rx_result_t.l4_ack");
_Static_assert(sizeof(halo_rx_netif_t) == 16, "halo_rx_netif_t is 16 bytes");
// deliver.go's DeliverHdr, DeliverSummary and DeliverIndex
_Static_assert(sizeof(halo_deliver_hdr_t) == 24, "halo_deliver_hdr_t is 24 bytes");
_Static_assert(offsetof(halo_deliver_hdr_t, remote_ip) == 8, "halo_deliver_hdr_t.remote_ip");
_Static_assert(offsetof(halo_deliver_hdr_t, seq) == 16, "halo_deliver_hdr_t.seq");
_Static_assert(sizeof(halo_deliver_summary_t) == 40, "halo_deliver_summary_t is 40 bytes");
_Static_assert(offsetof(halo_deliver_summary_t, kind_counts) == 24, "halo_deliver_summary_t.kind_counts");
_Static_assert(sizeof(halo_deliver_index_t) == 8, "halo_deliver_index_t is 8 bytes");
_Static_assert(sizeof(halo_deliver_config_t) == 16, "halo_deliver_config_t is 16 bytes");
// kcp.go's KcpDgram, KcpSeg and KcpSummary
_Static_assert(sizeof(halo_kcp_dgram_t) == 40, "halo_kcp_dgram_t is 40 bytes");
_Static_assert(offsetof(halo_kcp_dgram_t, conv0) == 8, "halo_kcp_dgram_t.conv0");
_Static_assert(offsetof(halo_kcp_dgram_t, first_seg) == 20, "halo_kcp_dgram_t.first_seg");
_Static_assert(offsetof(halo_kcp_dgram_t, enet_type) == 36, "halo_kcp_dgram_t.enet_type");
_Static_assert(sizeof(halo_kcp_seg_t) == 32, "halo_kcp_seg_t is 32 bytes");
_Static_assert(offsetof(halo_kcp_seg_t, data_off) == 24, "halo_kcp_seg_t.data_off");
_Static_assert(offsetof(halo_kcp_seg_t, check) == 28, "halo_kcp_seg_t.check");
_Static_assert(sizeof(halo_kcp_summary_t) == 96, "halo_kcp_summary_t is 96 bytes");
_Static_assert(offsetof(halo_kcp_summary_t, ret_counts) == 16, "halo_kcp_summary_t.ret_counts");
_Static_assert(offsetof(halo_kcp_summary_t, bytes_hashed) == 56, "halo_kcp_summary_t.bytes_hashed");
_Static_assert(sizeof(halo_kcp_config_t) == 16, "halo_kcp_config_t is 16 bytes");
// dhcp.go's DhcpMsg, DhcpSummary, DhcpLease, DhcpReply and DhcpClientEvent
_Static_assert(sizeof(halo_dhcp_msg_t) == 128, "halo_dhcp_msg_t is 128 bytes");
_Static_assert(offsetof(halo_dhcp_msg_t, yiaddr) == 16, "halo_dhcp_msg_t.yiaddr");
_Static_assert(offsetof(halo_dhcp_msg_t, req_ip) == 32, "halo_dhcp_msg_t.req_ip");
_Static_assert(offsetof(halo_dhcp_msg_t, mask_n) == 48, "halo_dhcp_msg_t.mask_n");
_Static_assert(offsetof(halo_dhcp_msg_t, hostname) == 64, "halo_dhcp_msg_t.hostname");
_Static_assert(sizeof(halo_dhcp_summary_t) == 64, "halo_dhcp_summary_t is 64 bytes");
_Static_assert(sizeof(halo_dhcp_lease_t) == 80, "halo_dhcp_lease_t is 80 bytes");
_Static_assert(sizeof(halo_dhcp_reply_t) == 32, "halo_dhcp_reply_t is 32 bytes");
_Static_assert(offsetof(halo_dhcp_reply_t, req_ip) == 20, "halo_dhcp_reply_t.req_ip");
_Static_assert(sizeof(halo_dhcp_client_event_t) == 24, "halo_dhcp_client_event_t is 24 bytes");
_Static_assert(sizeof(halo_dhcp_config_t) == 24, "halo_dhcp_config_t is 24 bytes");

// gpurx_netif: a halo_rx_netif_t from NetIf.MacAddr, IpAddrToU(NetIf.IpAddr), NatEnable.
static inline halo_rx_netif_t gpurx_netif(const uint8_t* mac, uint32_t ip, int nat_enable) {
    halo_rx_netif_t n;
    memset(&n, 0, sizeof n);
    memcpy(n.mac, mac, 6);
    n.ip = ip;
    n.nat_enable = nat_enable ? 1u : 0u;
    return n;
}

// gpurx_kcp_config: a halo_kcp_config_t (byte_check_mode is HALO_KCP_CHECK_*, -1..2).
static inline halo_kcp_config_t gpurx_kcp_config(int byte_check_mode, uint32_t port, uint32_t dgram_cap, uint32_t seg_cap) {
    halo_kcp_config_t c;
    c.byte_check_mode = byte_check_mode;
    c.port = port;
    c.dgram_cap = dgram_cap;
    c.seg_cap = seg_cap;
    return c;
}

// gpurx_kcp_emit_config: a halo_kcp_emit_config_t (byte_check_mode is HALO_KCP_CHECK_*, -1..2).
static inline halo_kcp_emit_config_t gpurx_kcp_emit_config(int byte_check_mode, uint32_t src_ip, uint32_t src_port,
                                                           uint32_t dgram_cap, uint32_t stream_cap) {
    halo_kcp_emit_config_t c;
    c.byte_check_mode = byte_check_mode;
    c.src_ip = src_ip;
    c.src_port = src_port;
    c.dgram_cap = dgram_cap;
    c.stream_cap = stream_cap;
    c.reserved = 0;
    return c;
}

// gpurx_dhcp_config: a halo_dhcp_config_t from the NetIf's addresses (IpAddrToU form), MAC and switches.
static inline halo_dhcp_config_t gpurx_dhcp_config(uint32_t ip, uint32_t network_mask, uint32_t dns, const uint8_t* mac,
                                                   int server_enable, int client_enable, uint32_t capacity) {
    halo_dhcp_config_t c;
    memset(&c, 0, sizeof c);
    c.ip = ip;
    c.network_mask = network_mask;
    c.dns = dns;
    memcpy(c.mac, mac, 6);
    c.server_enable = server_enable != 0;
    c.client_enable = client_enable != 0;
    c.capacity = capacity;
    return c;
}

// gpurx_lo_config: a halo_lo_config_t for the loopback gather (tx: HALO_LO_TX, jumbo: HALO_RX_JUMBO_EXT).
static inline halo_lo_config_t gpurx_lo_config(uint32_t n_netifs, int tx, int jumbo, uint64_t region_bytes,
                                               uint32_t index_cap) {
    halo_lo_config_t c;
    memset(&c, 0, sizeof c);
    c.n_netifs = n_netifs;
    c.flags = (tx ? HALO_LO_TX : 0u) | (jumbo ? HALO_RX_JUMBO_EXT : 0u);
    c.region_bytes = region_bytes;
    c.index_cap = index_cap;
    return c;
}

// gpurx_parse_one: one frame (l3 = 0) or one bare IPv4 packet (l3 = 1) through the host entry
// point, as a batch of one. The netif only sets the dispatch flags, which the Parse* wrappers
// do not read.
static inline int gpurx_parse_one(halo_rx_host_ctx_t* ctx, const uint8_t* buf, uint16_t len, int csum, int l3,
                                  halo_rx_result_t* out) {
    const uint64_t off = 0;
    const uint8_t mac[6] = {0, 0, 0, 0, 0, 0};
    const halo_rx_netif_t n = gpurx_netif(mac, 0, 0);
    const uint32_t flags = (csum ? HALO_RX_CSUM_ENABLE : 0u) | (l3 ? HALO_RX_L3_START : 0u);
    return halo_rx_parse_batch_host(ctx, buf, &off, &len, 1, flags, &n, out, NULL);
}

#endif /* GPURX_SHIM_H */
