// tx_dhcp_host.cc — the DHCP reply build's C entry points (include/halo_rx.h, "DHCP"): the
// argument checks of halo_dhcp_reply_build_device, answered before any device is looked for, and
// halo_dhcp_reply_build_host, the sequential loop with the same outputs. No HIP: the kernel lives
// in tx_dhcp.hip behind dhcp::build_ops(), and this file compiles alone with g++
// (tools/fuzz_dhcp.cc drives it under ASan/UBSan).
#include <string.h>

#include "rx_dhcp.h"

using namespace halo;  // host_layout.h
using namespace halo::dhcp;

namespace {

int check(const halo_dhcp_config_t* cfg, const halo_dhcp_reply_t* replies, uint32_t n, const uint8_t* payload,
          const halo_tx_build_desc_t* descs) {
    if (!cfg || n > HALO_DHCP_BUILD_MAX) return HALO_E_INVAL;
    if (n && (!replies || !payload || !descs)) return HALO_E_INVAL;
    return HALO_OK;
}

}  // namespace

extern "C" HALO_API int halo_dhcp_reply_build_device(const halo_dhcp_config_t* cfg, const halo_dhcp_reply_t* d_replies,
                                                     uint32_t n, uint8_t* d_payload, halo_tx_build_desc_t* d_descs,
                                                     halo_stream_t stream) {
    int rc;
    if ((rc = check(cfg, d_replies, n, d_payload, d_descs))) return rc;
    if (misaligned(d_replies, 16) || misaligned(d_descs, 8) || misaligned(d_payload, 4)) return HALO_E_INVAL;
    const dhcp::BuildOps* ops = dhcp::build_ops ? dhcp::build_ops() : nullptr;
    return ops ? ops->build(cfg, d_replies, n, d_payload, d_descs, stream) : HALO_E_NODEV;
}

extern "C" HALO_API int halo_dhcp_reply_build_host(const halo_dhcp_config_t* cfg, const halo_dhcp_reply_t* replies, uint32_t n,
                                                   uint8_t* payload, halo_tx_build_desc_t* descs) {
    int rc;
    if ((rc = check(cfg, replies, n, payload, descs))) return rc;
    Addrs a;
    memcpy(&a, cfg, sizeof a);  // ip, network_mask, dns: the config's first three words
    for (uint32_t i = 0; i < n; ++i) {
        Reply r;
        memcpy(r.w, reinterpret_cast<const uint8_t*>(replies) + 32ull * i, 32);
        uint8_t* slot = payload + (uint64_t)i * kSlot;
        for (uint32_t pos = 0; pos < kSlot; ++pos) slot[pos] = (uint8_t)reply_byte(r, a, pos);
        uint32_t w[kDescWords];
        desc_words(r, a, i, w);
        memcpy(reinterpret_cast<uint8_t*>(descs) + 40ull * i, w, sizeof w);
    }
    return HALO_OK;
}
