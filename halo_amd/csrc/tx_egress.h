// tx_egress.h — the egress step (include/halo_rx.h, "egress"): the layout arithmetic the host loop
// (tx_egress_host.cc) and the kernels (tx_egress.hip) must agree on — tx_len, record size, which
// frames are sendable, how each kind's selector becomes a port mask; the workspace layout and the
// argument checks it has in common with the loopback step are host_layout.h's. Plain C++17, no HIP: tx_egress_host.cc compiles alone with g++ (tools/fuzz_egress.cc drives it
// under ASan/UBSan) and into libhalo_rx.so.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HALO_EGRESS_FN __host__ __device__ __forceinline__
#else
#define HALO_EGRESS_FN inline
#endif
#include <stdint.h>

#include "../../include/halo_rx.h"
#include "host_layout.h"

namespace halo {
namespace egress {

constexpr uint32_t kTile = 256;  // frames per tile = lanes per workgroup of the count and scatter kernels

// BuildEthFrm's length and ringBufferRecordSize of it
HALO_EGRESS_FN uint32_t tx_len(uint32_t len) { return len < 60u ? 60u : len; }
HALO_EGRESS_FN uint32_t record_size(uint32_t len) { return (4u + tx_len(len) + 3u) & ~3u; }
HALO_EGRESS_FN uint32_t max_len(uint32_t flags) { return (flags & HALO_RX_JUMBO_EXT) ? 9014u : 1514u; }
HALO_EGRESS_FN bool sendable(uint32_t len, uint32_t flags) { return len >= 14u && len <= max_len(flags); }
HALO_EGRESS_FN uint64_t port_bits(uint32_t n_ports) { return n_ports >= 64u ? ~0ull : (1ull << n_ports) - 1ull; }

// A frame's port mask per kind, before port_bits cuts it. The selector words are read as the
// kernels read them: one u64 per mask, the first u32 of an ARP result (verdict | out_netif << 8 |
// tx_len << 16), the u32 of a switch result (verdict | out_port << 8 | tx_len << 16).
HALO_EGRESS_FN uint64_t mask_of_masks(uint64_t m) { return m; }
HALO_EGRESS_FN uint64_t mask_of_arp(uint32_t w) {
    const uint32_t out = (w >> 8) & 0xFFu;
    return (w & 0xFFu) == HALO_ARP_V_HIT && out < 64u ? 1ull << out : 0ull;
}
HALO_EGRESS_FN uint64_t mask_of_switch(uint32_t w, uint64_t flood_mask) {
    const uint32_t v = w & 0xFFu, out = (w >> 8) & 0xFFu;
    if (v == HALO_SW_V_FLOOD) return flood_mask;
    return v == HALO_SW_V_UNICAST && out < 64u ? 1ull << out : 0ull;
}

// The device side (tx_egress.hip); tx_egress_host.cc reaches it only through this, after it has
// checked every argument. kind = HALO_EGRESS_KIND_*.
struct DeviceOps {
    int (*run)(const halo_egress_config_t* cfg, uint32_t kind, const uint8_t* d_bytes, const uint32_t* d_offsets_dw,
               const uint16_t* d_lens, uint32_t n, const void* d_selectors, uint64_t flood_mask, uint8_t* d_out,
               halo_egress_port_t* d_ports, uint32_t* d_index, uint32_t* d_skipped, void* d_workspace,
               halo_stream_t stream);
};
// Defined by tx_egress.hip; absent (null) in a host-only build, where the device calls are HALO_E_NODEV.
const DeviceOps* device_ops() __attribute__((weak));

}  // namespace egress
}  // namespace halo
