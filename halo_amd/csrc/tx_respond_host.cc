// tx_respond_host.cc — the local responders' C entry points (include/halo_rx.h, "local
// responders"): the argument checks of halo_tx_respond_device, answered before any device is
// looked for, and halo_tx_respond_host, the sequential loop with the same outputs. No HIP: the
// kernels live in tx_respond.hip behind respond::device_ops(), and this file compiles alone with
// g++ (tools/fuzz_respond.cc drives it under ASan/UBSan).
#include <string.h>

#include "tx_respond.h"

namespace halo {
namespace respond {
namespace {

// What both entry points ask; `dev` adds the alignment the kernels' vector accesses need.
int check(const uint32_t* offsets_dw, const uint16_t* lens, const halo_rx_result_t* records, uint32_t n, uint32_t flags,
          const halo_rx_netif_t* netif, const halo_tx_op_t* ops, const uint8_t* fixup_result,
          const halo_tx_build_desc_t* desc, const halo_respond_src_t* src, uint32_t cap, const uint32_t* count, bool dev) {
    if (!netif || !count || (flags & ~kFlagsMask)) return HALO_E_INVAL;
    if ((ops == nullptr) != (fixup_result == nullptr)) return HALO_E_INVAL;
    if (cap && (!desc || !src)) return HALO_E_INVAL;
    if (n && (!offsets_dw || !lens || !records)) return HALO_E_INVAL;
    if (dev && (misaligned(offsets_dw, 4) || misaligned(lens, 2) || misaligned(records, 16) || misaligned(ops, 4) ||
                misaligned(desc, 8) || misaligned(src, 8) || misaligned(count, 4)))
        return HALO_E_INVAL;
    return HALO_OK;
}

}  // namespace
}  // namespace respond
}  // namespace halo

using namespace halo;  // host_layout.h
using namespace halo::respond;

extern "C" HALO_API uint64_t halo_tx_respond_workspace(uint32_t n) { return 4 * tiles_of(n, kTile); }  // one u32 per tile

extern "C" HALO_API int halo_tx_respond_device(const uint32_t* d_offsets_dw, const uint16_t* d_lens,
                                               const halo_rx_result_t* d_records, uint32_t n, uint32_t flags,
                                               const halo_rx_netif_t* netif, const uint8_t* d_nat_verdict,
                                               const halo_tx_op_t* d_ops, const uint8_t* d_fixup_result,
                                               const uint32_t* d_tcp_ports, halo_tx_build_desc_t* d_desc,
                                               halo_respond_src_t* d_src, uint32_t* d_dst_ip, uint32_t cap,
                                               uint32_t* d_count, uint32_t* d_kind_counts, uint8_t* d_actions,
                                               void* d_workspace, uint64_t workspace_bytes, halo_stream_t stream) {
    int rc;
    if ((rc = check(d_offsets_dw, d_lens, d_records, n, flags, netif, d_ops, d_fixup_result, d_desc, d_src, cap, d_count,
                    true)))
        return rc;
    if (misaligned(d_tcp_ports, 4) || misaligned(d_dst_ip, 4) || misaligned(d_kind_counts, 4) || misaligned(d_workspace, 4))
        return HALO_E_INVAL;
    if (n && (!d_workspace || workspace_bytes < halo_tx_respond_workspace(n))) return HALO_E_INVAL;
    const DeviceOps* ops = device_ops ? device_ops() : nullptr;
    return ops ? ops->run(d_offsets_dw, d_lens, d_records, n, flags, netif, d_nat_verdict, d_ops, d_fixup_result,
                          d_tcp_ports, d_desc, d_src, d_dst_ip, cap, d_count, d_kind_counts, d_actions, d_workspace, stream)
               : HALO_E_NODEV;
}

extern "C" HALO_API int halo_tx_respond_host(const uint32_t* offsets_dw, const uint16_t* lens,
                                             const halo_rx_result_t* records, uint32_t n, uint32_t flags,
                                             const halo_rx_netif_t* netif, const uint8_t* nat_verdict,
                                             const halo_tx_op_t* ops, const uint8_t* fixup_result,
                                             const uint32_t* tcp_ports, halo_tx_build_desc_t* desc,
                                             halo_respond_src_t* src, uint32_t* dst_ip, uint32_t cap, uint32_t* count,
                                             uint32_t* kind_counts, uint8_t* actions) {
    int rc;
    if ((rc = check(offsets_dw, lens, records, n, flags, netif, ops, fixup_result, desc, src, cap, count, false))) return rc;
    uint32_t k = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t* rb = reinterpret_cast<const uint8_t*>(records + i);  // no alignment asked of host memory
        const Rec r{load_u32(rb), load_u32(rb + 4), load_u32(rb + 8), load_u32(rb + 16), load_u32(rb + 20), load_u32(rb + 24)};
        uint16_t len;
        memcpy(&len, reinterpret_cast<const uint8_t*>(lens) + 2ull * i, 2);
        const uint32_t nat = nat_verdict ? nat_verdict[i] : kNone;
        const uint32_t fix = ops ? (uint32_t)ops[i].steps | (uint32_t)fixup_result[i] << 8 : 0u;
        const Reply o = decide(r, len, load_u32(reinterpret_cast<const uint8_t*>(offsets_dw) + 4ull * i), nat, fix, tcp_ports,
                               netif->ip, netif->nat_enable != 0, flags);
        if (actions) actions[i] = (uint8_t)o.action;
        if (o.kind == kNone) continue;
        if (k < cap) {
            const uint32_t w[10] = {(uint32_t)o.payload_off, (uint32_t)(o.payload_off >> 32), o.w2, o.w3, o.src_ip, o.dst_ip,
                                    o.seq, o.ack, 0u, 0u};
            memcpy(reinterpret_cast<uint8_t*>(desc) + 40ull * k, w, 40);
            const uint32_t s[2] = {i, o.kind};
            memcpy(reinterpret_cast<uint8_t*>(src) + 8ull * k, s, 8);
            if (dst_ip) memcpy(reinterpret_cast<uint8_t*>(dst_ip) + 4ull * k, &o.dst_ip, 4);
        }
        if (kind_counts) ++kind_counts[o.kind];
        ++k;
    }
    *count = k;
    return HALO_OK;
}
