// lo_gather.h — the loopback step (include/halo_rx.h, "loopback"): the selection and layout
// arithmetic the host loop (lo_gather_host.cc) and the kernels (lo_gather.hip) must agree on — which
// ARP result selects a frame, a packet's length in either mode, which packets are sendable, a
// packet's size in its NetIf's region; the workspace layout and the argument checks it has in common
// with the egress step are host_layout.h's. Plain C++17, no HIP:
// lo_gather_host.cc compiles alone with g++ (tools/fuzz_lo.cc drives it under ASan/UBSan) and into
// libhalo_rx.so.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HALO_LO_FN __host__ __device__ __forceinline__
#else
#define HALO_LO_FN inline
#endif
#include <stdint.h>

#include "../../include/halo_rx.h"
#include "host_layout.h"

namespace halo {
namespace lo {

constexpr uint32_t kTile = 256;       // frames per tile = lanes per workgroup of the count and scatter kernels
constexpr uint32_t kEthHeader = 14;   // a packet starts here in its frame: 2 bytes into frame dword 3
constexpr uint32_t kNotWritten = 0xFFFFFFFFu;  // d_pkt_off_dw of a packet beyond the written prefix

// The out NetIf an ARP result's first u32 (verdict | out_netif << 8 | tx_len << 16) sends a LoChan
// copy to, or n_netifs and above (0xFFFFFFFF) for none.
HALO_LO_FN uint32_t netif_of(uint32_t w, uint32_t n_netifs) {
    const uint32_t out = (w >> 8) & 0xFFu;
    return (w & 0xFFu) == HALO_ARP_V_LOOPBACK && out < n_netifs ? out : 0xFFFFFFFFu;
}
HALO_LO_FN uint32_t max_len(uint32_t flags) { return (flags & HALO_RX_JUMBO_EXT) ? 9014u : 1514u; }
// Forward mode (:193-201): the whole ethPayload. Sendable: an IPv4 header's worth, and what
// BuildEthFrm takes.
HALO_LO_FN bool fwd_sendable(uint32_t len, uint32_t flags) { return len >= 34u && len <= max_len(flags); }
// Tx mode (:71-80): whether a frame of len bytes holds the dword with bytes 16-19, and, given
// that dword as loaded (little-endian), totalLen and whether the packet is sendable.
HALO_LO_FN bool tx_has_total_len(uint32_t len) { return len >= 34u; }
HALO_LO_FN uint32_t tx_total_len(uint32_t w4) { return (w4 & 0xFFu) << 8 | ((w4 >> 8) & 0xFFu); }
HALO_LO_FN bool tx_sendable(uint32_t total_len, uint32_t len) { return total_len >= 20u && total_len <= len - kEthHeader; }
// A packet's bytes in its region: the packet, then zeros up to the next 4-byte boundary
HALO_LO_FN uint32_t packet_size(uint32_t pkt_len) { return (pkt_len + 3u) & ~3u; }

// The device side (lo_gather.hip); lo_gather_host.cc reaches it only through this, after it has
// checked every argument.
struct DeviceOps {
    int (*run)(const halo_lo_config_t* cfg, const uint8_t* d_bytes, const uint32_t* d_offsets_dw, const uint16_t* d_lens,
               uint32_t n, const halo_arp_result_t* d_results, uint8_t* d_out, halo_egress_port_t* d_ports,
               uint32_t* d_pkt_off_dw, uint16_t* d_pkt_len, uint32_t* d_index, uint32_t* d_skipped, void* d_workspace,
               halo_stream_t stream);
};
// Defined by lo_gather.hip; absent (null) in a host-only build, where the device call is HALO_E_NODEV.
const DeviceOps* device_ops() __attribute__((weak));

}  // namespace lo
}  // namespace halo
