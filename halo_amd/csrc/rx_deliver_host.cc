// rx_deliver_host.cc — local delivery's C entry points (include/halo_rx.h, "local delivery"): the
// argument checks of halo_rx_deliver_device, answered before any device is looked for, and
// halo_rx_deliver_host, the sequential loop with the same outputs. No HIP: the kernels live in
// rx_deliver.hip behind deliver::device_ops(), and this file compiles alone with g++
// (tools/fuzz_deliver.cc drives it under ASan/UBSan).
#include <string.h>

#include "rx_deliver.h"

namespace halo {
namespace deliver {
namespace {

// What both entry points ask
int check(const halo_deliver_config_t* cfg, const uint8_t* bytes, const uint32_t* offsets_dw, const uint16_t* lens,
          const halo_rx_result_t* records, uint32_t n, const halo_rx_netif_t* netif, const uint8_t* out,
          const halo_deliver_summary_t* summary, const halo_deliver_index_t* index) {
    if (!cfg || !netif || !summary) return HALO_E_INVAL;
    if (cfg->flags & ~kFlagsMask) return HALO_E_INVAL;
    if (n && (!bytes || !offsets_dw || !lens || !records)) return HALO_E_INVAL;
    if (cfg->region_bytes && !out) return HALO_E_INVAL;
    if (cfg->index_cap && !index) return HALO_E_INVAL;
    return HALO_OK;
}

}  // namespace
}  // namespace deliver
}  // namespace halo

using namespace halo;  // host_layout.h
using namespace halo::deliver;

extern "C" HALO_API uint64_t halo_rx_deliver_workspace(uint32_t n) { return workspace_bytes(n); }

extern "C" HALO_API int halo_rx_deliver_device(const halo_deliver_config_t* cfg, const uint8_t* d_bytes,
                                               const uint32_t* d_offsets_dw, const uint16_t* d_lens,
                                               const halo_rx_result_t* d_records, uint32_t n,
                                               const halo_rx_netif_t* netif, const uint32_t* d_udp_ports,
                                               const uint32_t* d_tcp_ports, uint8_t* d_out,
                                               halo_deliver_summary_t* d_summary, halo_deliver_index_t* d_index,
                                               void* d_workspace, uint64_t workspace_bytes, halo_stream_t stream) {
    int rc;
    if ((rc = check(cfg, d_bytes, d_offsets_dw, d_lens, d_records, n, netif, d_out, d_summary, d_index))) return rc;
    if ((cfg->region_bytes & 15u) || cfg->region_bytes > kMaxDeviceRegion) return HALO_E_INVAL;
    if (misaligned(d_out, 16) || misaligned(d_records, 16) || misaligned(d_summary, 8) || misaligned(d_index, 8) ||
        misaligned(d_workspace, 8) || misaligned(d_bytes, 4) || misaligned(d_udp_ports, 4) || misaligned(d_tcp_ports, 4) ||
        misaligned(d_offsets_dw, 4) || misaligned(d_lens, 2))
        return HALO_E_INVAL;
    if (n && (!d_workspace || workspace_bytes < halo_rx_deliver_workspace(n))) return HALO_E_INVAL;
    const DeviceOps* ops = device_ops ? device_ops() : nullptr;
    return ops ? ops->run(cfg, d_bytes, d_offsets_dw, d_lens, d_records, n, netif, d_udp_ports, d_tcp_ports, d_out, d_summary,
                          d_index, d_workspace, stream)
               : HALO_E_NODEV;
}

extern "C" HALO_API int halo_rx_deliver_host(const halo_deliver_config_t* cfg, const uint8_t* bytes,
                                             const uint32_t* offsets_dw, const uint16_t* lens,
                                             const halo_rx_result_t* records, uint32_t n, const halo_rx_netif_t* netif,
                                             const uint32_t* udp_ports, const uint32_t* tcp_ports, uint8_t* out,
                                             halo_deliver_summary_t* summary, halo_deliver_index_t* index) {
    int rc;
    if ((rc = check(cfg, bytes, offsets_dw, lens, records, n, netif, out, summary, index))) return rc;
    const uint64_t region = cfg->region_bytes;
    halo_deliver_summary_t s;  // no alignment asked of host memory: built here, copied out
    memset(&s, 0, sizeof s);
    bool cut = false;  // a record did not fit
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t* rb = reinterpret_cast<const uint8_t*>(records) + 32ull * i;
        const Rec r{load_u32(rb), load_u32(rb + 4), load_u32(rb + 8), load_u32(rb + 16), load_u32(rb + 20), load_u32(rb + 24),
                    load_u32(rb + 28)};
        const uint32_t kind = kind_of(r, udp_ports, tcp_ports, netif->nat_enable != 0, cfg->flags);
        if (kind == kNone) continue;
        uint16_t len;
        memcpy(&len, reinterpret_cast<const uint8_t*>(lens) + 2ull * i, 2);
        if (!inside(r, len)) {
            ++s.skipped;
            continue;
        }
        const uint32_t plen = payload_len(r), rec = record_size(plen);
        uint32_t where = 0xFFFFFFFFu;
        if (!cut && s.bytes + rec <= region) {
            uint8_t* o = out + s.bytes;
            uint32_t w[6];
            header_words(r, i, kind, w);
            memcpy(o, w, kHdrBytes);
            memcpy(o + kHdrBytes, bytes + 4ull * load_u32(reinterpret_cast<const uint8_t*>(offsets_dw) + 4ull * i) + payload_off(r),
                   plen);
            memset(o + kHdrBytes + plen, 0, rec - kHdrBytes - plen);
            if (s.bytes < 0xFFFFFFFFull) where = (uint32_t)s.bytes;
            ++s.records_written;
            s.bytes_written += rec;
        } else {
            cut = true;
        }
        if (s.records < cfg->index_cap) {
            const uint32_t e[2] = {i, where};
            memcpy(reinterpret_cast<uint8_t*>(index) + 8ull * s.records, e, 8);
        }
        ++s.records;
        s.bytes += rec;
        ++s.kind_counts[kind];
    }
    memcpy(summary, &s, sizeof s);
    return HALO_OK;
}
