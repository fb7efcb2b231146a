// tx_respond.h — the local responders (include/halo_rx.h, "local responders"): the per-frame
// decision the host loop (tx_respond_host.cc) and the kernels (tx_respond.hip) share — which of
// RxIcmp's echo reply, Ipv4RouteForward's time-exceeded message and RxTcp's handshake answers a
// received frame gets, and the halo_tx_build_desc_t of it — from the frame's record, length and
// offset alone. Plain C++17, no HIP: tx_respond_host.cc compiles alone with g++
// (tools/fuzz_respond.cc drives it under ASan/UBSan) and into libhalo_rx.so.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HALO_RESPOND_FN __host__ __device__ __forceinline__
#else
#define HALO_RESPOND_FN inline
#endif
#include <stdint.h>

#include "../../include/halo_rx.h"
#include "host_layout.h"
#include "rx_dispatch.h"

namespace halo {
namespace respond {

constexpr uint32_t kTile = 256;  // frames per tile = lanes per workgroup (arp::kGatherTile, checked in tx_respond.hip)
constexpr uint32_t kNone = 0xFFu;  // no reply
constexpr uint32_t kFlagsMask = HALO_RX_L3_START;

// The record fields the decision reads, as the dwords a kernel loads: w0 = status | flags << 8 |
// ethertype << 16, w1 = ip_proto | l4_aux << 8 | ip_total_len << 16, w4 = sport | dport << 16,
// w5 = payload_off | payload_len << 16.
struct Rec {
    uint32_t w0, w1, src_ip, w4, w5, l4_seq;
};

// A frame's decision: the reply's kind and descriptor, and the frame's action.
struct Reply {
    uint32_t kind;    // HALO_RESPOND_*, or kNone
    uint32_t action;  // halo_rx_dispatch's
    // halo_tx_build_desc_t as five 8-byte words (little-endian): payload_off; payload_len | proto
    // << 16 | aux << 24, src_port | dst_port << 16; src_ip, dst_ip; seq, ack; dst_mac, mode, pad = 0
    uint64_t payload_off;
    uint32_t w2, w3, src_ip, dst_ip, seq, ack;
};

HALO_RESPOND_FN bool tcp_served(const uint32_t* tcp_ports, uint32_t port) {
    return tcp_ports && (tcp_ports[port >> 5] >> (port & 31u) & 1u);
}

// The table of include/halo_rx.h, in the reference's order. What the call was given beside the
// records comes per frame as nat = d_nat_verdict[i], or kNone when absent, and fix = ops[i].steps |
// result[i] << 8, or 0 when the pair is absent (no TTL step: the row never fires). Reads tcp_ports
// only for a LOCAL_TCP frame with SYN set.
HALO_RESPOND_FN Reply decide(const Rec& r, uint32_t len, uint32_t off_dw, uint32_t nat, uint32_t fix,
                             const uint32_t* tcp_ports, uint32_t own_ip, bool nat_enable, uint32_t flags) {
    const uint32_t status = r.w0 & 0xFFu, rflags = (r.w0 >> 8) & 0xFFu, ethertype = r.w0 >> 16;
    const uint32_t ip_proto = r.w1 & 0xFFu, l4_aux = (r.w1 >> 8) & 0xFFu;
    const bool l3 = (flags & HALO_RX_L3_START) != 0;
    Reply o;
    o.action = l3 ? action_of_loopback(status, rflags, ip_proto) : action_of(status, rflags, ethertype, ip_proto, nat_enable);
    o.kind = kNone;
    o.payload_off = 4ull * off_dw;
    o.w2 = o.w3 = o.seq = o.ack = 0;
    o.src_ip = own_ip;
    o.dst_ip = r.src_ip;
    const bool fwd = !l3 && o.action == HALO_RX_ACT_FORWARD;
    const bool echo_req = ip_proto == 0x01u && status == HALO_RX_OK && l4_aux == 8u;
    if ((o.action == HALO_RX_ACT_LOCAL_ICMP && l4_aux == 8u) || (fwd && nat == HALO_NAT_V_MISS && echo_req)) {
        // RxIcmp: TxIcmp(icmpPayload, ICMP_REPLY, icmpId, icmpSeq, src)   icmp_engine.go:12-23
        o.kind = HALO_RESPOND_ECHO;
        o.payload_off += r.w5 & 0xFFFFu;
        o.w2 = (r.w5 >> 16) | 0x01u << 16;  // payload_len, proto 1, aux 0
        o.w3 = (r.l4_seq >> 16) | (r.l4_seq & 0xFFFFu) << 16;
    } else if (fwd && nat == HALO_NAT_V_MISS) {
        // Ipv4RouteForward returned false before the TTL step and the packet is not an echo request
    } else if (fwd && (fix & HALO_TX_TTL) && !(fix >> 8 & HALO_TX_R_TTL_ALIVE)) {
        // TxIcmp(ethPayload[:28], ICMP_TTL, {0,0}, 0, src)   ipv4_engine.go:133-142
        o.kind = HALO_RESPOND_TTL;
        const uint32_t rest = len > 14u ? len - 14u : 0u;
        o.payload_off += 14u;
        o.w2 = (rest < 28u ? rest : 28u) | 0x01u << 16 | 11u << 24;
    } else if (o.action == HALO_RX_ACT_LOCAL_TCP && (l4_aux & 0x02u) && tcp_served(tcp_ports, r.w4 >> 16)) {
        // RxTcp: SYN -> SYN|ACK, SYN|ACK -> ACK   tcp_engine.go:16-24
        const bool ack = (l4_aux & 0x10u) != 0;
        o.kind = ack ? HALO_RESPOND_TCP_SYNACK : HALO_RESPOND_TCP_SYN;
        o.w2 = 0x06u << 16 | (ack ? 0x10u : 0x12u) << 24;  // no payload
        o.w3 = (r.w4 >> 16) | (r.w4 & 0xFFFFu) << 16;      // src_port = dport, dst_port = sport
        o.seq = ack ? 1234567891u : 1234567890u;
        o.ack = r.l4_seq + 1u;
    }
    return o;
}

// The device side (tx_respond.hip); tx_respond_host.cc reaches it only through this, after it
// has checked every argument.
struct DeviceOps {
    int (*run)(const uint32_t* d_offsets_dw, const uint16_t* d_lens, const halo_rx_result_t* d_records, uint32_t n,
               uint32_t flags, const halo_rx_netif_t* netif, const uint8_t* d_nat_verdict, const halo_tx_op_t* d_ops,
               const uint8_t* d_fixup_result, const uint32_t* d_tcp_ports, halo_tx_build_desc_t* d_desc,
               halo_respond_src_t* d_src, uint32_t* d_dst_ip, uint32_t cap, uint32_t* d_count, uint32_t* d_kind_counts,
               uint8_t* d_actions, void* d_workspace, halo_stream_t stream);
};
// Defined by tx_respond.hip; absent (null) in a host-only build, where the device call is HALO_E_NODEV.
const DeviceOps* device_ops() __attribute__((weak));

}  // namespace respond
}  // namespace halo
