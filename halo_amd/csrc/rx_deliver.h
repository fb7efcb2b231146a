// rx_deliver.h — local delivery (include/halo_rx.h, "local delivery"): what the host loop
// (rx_deliver_host.cc) and the kernels (rx_deliver.hip) must agree on — which frames RxUdp, RxTcp
// and RxUdpBroadcast hand to a service, from the frame's record, length and the two served-port
// maps alone; the record's size and header words; how one destination dword is made of two source
// dwords — and the workspace layout. Plain C++17, no HIP: rx_deliver_host.cc compiles alone with
// g++ (tools/fuzz_deliver.cc drives it under ASan/UBSan) and into libhalo_rx.so.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HALO_DELIVER_FN __host__ __device__ __forceinline__
#else
#define HALO_DELIVER_FN inline
#endif
#include <stdint.h>

#include "../../include/halo_rx.h"
#include "host_layout.h"
#include "rx_dispatch.h"

namespace halo {
namespace deliver {

constexpr uint32_t kTile = 256;  // frames per tile = lanes per workgroup of the count and scatter kernels
constexpr uint32_t kNone = 0xFFu;  // not delivered
constexpr uint32_t kFlagsMask = HALO_RX_L3_START | HALO_DELIVER_DHCP;
constexpr uint32_t kHdrBytes = 24;
constexpr uint64_t kMaxDeviceRegion = (1ull << 32) - 16;  // a record's offset fits the index's u32

// The record as the dwords a kernel loads (two 16-byte loads): w0 = status | flags << 8 |
// ethertype << 16, w1 = ip_proto | l4_aux << 8 | ip_total_len << 16, w4 = sport | dport << 16,
// w5 = payload_off | payload_len << 16.
struct Rec {
    uint32_t w0, w1, src_ip, w4, w5, l4_seq, l4_ack;
};

HALO_DELIVER_FN bool served(const uint32_t* ports, uint32_t port) {
    return ports && (ports[port >> 5] >> (port & 31u) & 1u);
}

// HALO_DELIVER_* of the frame, or kNone. Reads a map word only for a LOCAL_UDP / LOCAL_TCP frame.
HALO_DELIVER_FN uint32_t kind_of(const Rec& r, const uint32_t* udp_ports, const uint32_t* tcp_ports, bool nat_enable,
                                 uint32_t flags) {
    const uint32_t status = r.w0 & 0xFFu, rflags = (r.w0 >> 8) & 0xFFu, ethertype = r.w0 >> 16;
    const uint32_t ip_proto = r.w1 & 0xFFu, dport = r.w4 >> 16;
    const bool l3 = (flags & HALO_RX_L3_START) != 0;
    const uint32_t a = l3 ? action_of_loopback(status, rflags, ip_proto) : action_of(status, rflags, ethertype, ip_proto, nat_enable);
    if (a == HALO_RX_ACT_LOCAL_UDP) return served(udp_ports, dport) ? HALO_DELIVER_UDP : kNone;  // udp_engine.go:16-20
    if (a == HALO_RX_ACT_LOCAL_TCP) return served(tcp_ports, dport) ? HALO_DELIVER_TCP : kNone;  // tcp_engine.go:16-25
    if (a == HALO_RX_ACT_BCAST_UDP && (flags & HALO_DELIVER_DHCP) && (dport == 67u || dport == 68u))
        return HALO_DELIVER_DHCP;                                                                 // udp_engine.go:41-43
    return kNone;
}

HALO_DELIVER_FN uint32_t payload_off(const Rec& r) { return r.w5 & 0xFFFFu; }
HALO_DELIVER_FN uint32_t payload_len(const Rec& r) { return r.w5 >> 16; }
// the record's payload lies inside a frame of len bytes
HALO_DELIVER_FN bool inside(const Rec& r, uint32_t len) { return payload_off(r) + payload_len(r) <= len; }
HALO_DELIVER_FN uint32_t payload_dwords(uint32_t plen) { return (plen + 3u) >> 2; }
HALO_DELIVER_FN uint32_t record_size(uint32_t plen) { return kHdrBytes + 4u * payload_dwords(plen); }

// halo_deliver_hdr_t as six little-endian dwords
HALO_DELIVER_FN void header_words(const Rec& r, uint32_t frame, uint32_t kind, uint32_t w[6]) {
    w[0] = frame;
    w[1] = kind | (r.w1 & 0xFF00u) | (r.w5 & 0xFFFF0000u);  // kind, tcp_flags = l4_aux, payload_len
    w[2] = r.src_ip;
    w[3] = r.w4;  // remote_port = sport, local_port = dport
    w[4] = r.l4_seq;
    w[5] = r.l4_ack;
}

// Payload dword j (j < payload_dwords(plen)) of a payload that starts poff bytes into a frame whose
// first byte is 4-byte aligned. It comes of the frame's dwords s + j and s + j + 1, s = poff >> 2:
// needs_upper says whether the second holds a byte of the dword (never for poff & 3 == 0, and not
// when the payload ends in the first), so that no word beyond the payload's last is loaded;
// funnel shifts the pair (v_alignbyte_b32 on the device) and the last dword is masked to plen.
HALO_DELIVER_FN bool needs_upper(uint32_t poff, uint32_t plen, uint32_t j) {
    const uint32_t last = 4u * j + 3u < plen ? 4u * j + 3u : plen - 1u;  // the dword's last payload byte
    return ((poff & 3u) + last) >> 2 > j;
}
HALO_DELIVER_FN uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t shift) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, shift);
#else
    return shift ? lo >> 8u * shift | hi << (32u - 8u * shift) : lo;
#endif
}
HALO_DELIVER_FN uint32_t tail_mask(uint32_t plen, uint32_t j) {
    return (j + 1u == payload_dwords(plen) && (plen & 3u)) ? (1u << 8u * (plen & 3u)) - 1u : 0xFFFFFFFFu;
}

// Workspace of a device call, per tile: a u64 byte base (scan), then a u32 record count that the
// scan turns into the rank base, then a u32 byte count (a tile's record bytes fit: 256 * 65,560),
// then the tile's UDP, TCP and skipped counts in one u32 (each at most kTile = 256: nine bits); the
// DHCP count is the rest of the records. 20 bytes per tile, rounded up to the 8-byte alignment.
HALO_DELIVER_FN uint64_t workspace_bytes(uint32_t n) { return (20ull * tiles_of(n, kTile) + 7) & ~7ull; }
static_assert(kTile <= 0x1FFu, "a tile's count fits nine bits");
HALO_DELIVER_FN uint32_t pack_kinds(uint32_t udp, uint32_t tcp, uint32_t skipped) { return udp | tcp << 9 | skipped << 18; }
HALO_DELIVER_FN uint32_t packed_udp(uint32_t w) { return w & 0x1FFu; }
HALO_DELIVER_FN uint32_t packed_tcp(uint32_t w) { return (w >> 9) & 0x1FFu; }
HALO_DELIVER_FN uint32_t packed_skipped(uint32_t w) { return w >> 18; }

// The device side (rx_deliver.hip); rx_deliver_host.cc reaches it only through this, after it has
// checked every argument.
struct DeviceOps {
    int (*run)(const halo_deliver_config_t* cfg, const uint8_t* d_bytes, const uint32_t* d_offsets_dw,
               const uint16_t* d_lens, const halo_rx_result_t* d_records, uint32_t n, const halo_rx_netif_t* netif,
               const uint32_t* d_udp_ports, const uint32_t* d_tcp_ports, uint8_t* d_out, halo_deliver_summary_t* d_summary,
               halo_deliver_index_t* d_index, void* d_workspace, halo_stream_t stream);
};
// Defined by rx_deliver.hip; absent (null) in a host-only build, where the device call is HALO_E_NODEV.
const DeviceOps* device_ops() __attribute__((weak));

}  // namespace deliver
}  // namespace halo
