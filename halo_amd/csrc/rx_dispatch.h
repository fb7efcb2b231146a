// rx_dispatch.h — the reference engine's per-frame decision over the fields of a record
// (engine/ethernet_engine.go:13-31, engine/ipv4_engine.go:18-47, the LoChan drain of
// engine/engine.go:353-381): what halo_rx_dispatch / halo_rx_dispatch_loopback (host_logic.cc)
// return, as a function the responder kernels (tx_respond.hip) evaluate too. Plain C++17 that
// compiles with and without HIP.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HALO_DISPATCH_FN __host__ __device__ __forceinline__
#else
#define HALO_DISPATCH_FN inline
#endif
#include <stdint.h>

#include "../../include/halo_rx.h"

namespace halo {

HALO_DISPATCH_FN uint8_t local_action(uint32_t ip_proto) {
    return ip_proto == 0x01u ? HALO_RX_ACT_LOCAL_ICMP : ip_proto == 0x11u ? HALO_RX_ACT_LOCAL_UDP : HALO_RX_ACT_LOCAL_TCP;
}

// RxEthernet -> RxIpv4 -> Rx* for a frame a NetIf received
HALO_DISPATCH_FN uint8_t action_of(uint32_t status, uint32_t flags, uint32_t ethertype, uint32_t ip_proto,
                                   bool nat_enable) {
    if (status == HALO_RX_ETH_LEN || status == HALO_RX_ETH_TYPE) return HALO_RX_ACT_DROP_ETH;  // ethernet_engine.go:18-21
    if (!(flags & HALO_RX_F_MAC_MATCH)) return HALO_RX_ACT_IGNORE_MAC;                           // ethernet_engine.go:22
    if (ethertype == 0x0806u) return HALO_RX_ACT_ARP;                                            // ethernet_engine.go:24-25
    if (ethertype != 0x0800u) return HALO_RX_ACT_IGNORE_TYPE;                                    // ethernet_engine.go:28
    if (status >= HALO_RX_IP_LEN && status <= HALO_RX_IP_TOTLEN_OVERRUN) return HALO_RX_ACT_DROP_IP;  // ipv4_engine.go:19-23
    if (flags & HALO_RX_F_IP_BCAST) {                                                            // ipv4_engine.go:24-30
        if (ip_proto == 0x11u) return status == HALO_RX_OK ? HALO_RX_ACT_BCAST_UDP : HALO_RX_ACT_DROP_BCAST_UDP;
        return HALO_RX_ACT_IGNORE_BCAST;
    }
    if (!(flags & HALO_RX_F_DST_IS_OWN) || nat_enable) return HALO_RX_ACT_FORWARD;               // ipv4_engine.go:31-37
    if (status != HALO_RX_OK) return HALO_RX_ACT_DROP_L4;                                        // {udp,tcp,icmp}_engine.go Rx*
    return local_action(ip_proto);                                                               // ipv4_engine.go:38-46
}

// PacketHandle's LoChan drain for a packet parsed with HALO_RX_L3_START
HALO_DISPATCH_FN uint8_t action_of_loopback(uint32_t status, uint32_t flags, uint32_t ip_proto) {
    if (status >= HALO_RX_ETH_LEN && status <= HALO_RX_IP_TOTLEN_OVERRUN) return HALO_RX_ACT_DROP_IP;  // engine.go:362-365
    if (!(flags & HALO_RX_F_DST_IS_OWN)) return HALO_RX_ACT_LO_NOT_OWN;                                // engine.go:366-368
    if (status != HALO_RX_OK) return HALO_RX_ACT_DROP_L4;                                              // Rx{Icmp,Udp,Tcp} log and drop
    return local_action(ip_proto);                                                                     // engine.go:369-376
}

}  // namespace halo
