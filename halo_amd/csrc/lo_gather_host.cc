// lo_gather_host.cc — the loopback gather's C entry points (include/halo_rx.h, "loopback"): the
// argument checks of the device call, which are answered before any device is looked for, and
// halo_lo_gather_host, the sequential loop with the same outputs. No HIP: the kernels live in
// lo_gather.hip behind lo::device_ops(), and this file compiles alone with g++ (tools/fuzz_lo.cc
// drives it under ASan/UBSan).
#include <string.h>

#include "lo_gather.h"

namespace halo {
namespace lo {
namespace {

// What both entry points ask of cfg, the batch and the outputs: host_layout.h's checks of a
// per-port stream call and the three per-packet arrays
int check_args(const halo_lo_config_t* cfg, uintptr_t out_align, const uint8_t* bytes, const uint32_t* offsets_dw,
               const uint16_t* lens, uint32_t n, const halo_arp_result_t* results, const uint8_t* out,
               const halo_egress_port_t* ports, const uint32_t* pkt_off_dw, const uint16_t* pkt_len, const uint32_t* index,
               const uint32_t* skipped) {
    if (!cfg || (cfg->index_cap && (!pkt_off_dw || !pkt_len || !index))) return HALO_E_INVAL;
    if (misaligned(pkt_off_dw, 4) || misaligned(pkt_len, 2) || misaligned(results, 8)) return HALO_E_INVAL;
    // a region's bound: a packet's offset is a u32 of dwords from its region's start
    return check_port_stream_args(cfg->n_netifs, HALO_ARP_MAX_NETIFS, cfg->flags, HALO_RX_JUMBO_EXT | HALO_LO_TX, cfg->region_bytes,
                                  1ull << 34, out, out_align, ports, index, skipped, bytes, offsets_dw, lens, n, results);
}

}  // namespace
}  // namespace lo
}  // namespace halo

using namespace halo;  // host_layout.h
using namespace halo::lo;

// Workspace of a device call: host_layout.h's, for tiles of kTile frames
extern "C" HALO_API uint64_t halo_lo_gather_workspace(uint32_t n, uint32_t n_netifs) {
    if (n_netifs < 1 || n_netifs > HALO_ARP_MAX_NETIFS) return 0;
    return port_stream_workspace(n, kTile, n_netifs);
}

extern "C" HALO_API int halo_lo_gather_device(const halo_lo_config_t* cfg, const uint8_t* d_bytes,
                                              const uint32_t* d_offsets_dw, const uint16_t* d_lens, uint32_t n,
                                              const halo_arp_result_t* d_results, uint8_t* d_out,
                                              halo_egress_port_t* d_ports, uint32_t* d_pkt_off_dw, uint16_t* d_pkt_len,
                                              uint32_t* d_index, uint32_t* d_skipped, void* d_workspace,
                                              uint64_t workspace_bytes, halo_stream_t stream) {
    const int rc = check_args(cfg, 16, d_bytes, d_offsets_dw, d_lens, n, d_results, d_out, d_ports, d_pkt_off_dw, d_pkt_len,
                              d_index, d_skipped);
    if (rc) return rc;
    if (n && (!d_workspace || workspace_bytes < halo_lo_gather_workspace(n, cfg->n_netifs))) return HALO_E_INVAL;
    if (misaligned(d_workspace, 8)) return HALO_E_INVAL;
    const DeviceOps* ops = device_ops ? device_ops() : nullptr;
    return ops ? ops->run(cfg, d_bytes, d_offsets_dw, d_lens, n, d_results, d_out, d_ports, d_pkt_off_dw, d_pkt_len, d_index,
                          d_skipped, d_workspace, stream)
               : HALO_E_NODEV;
}

extern "C" HALO_API int halo_lo_gather_host(const halo_lo_config_t* cfg, const uint8_t* bytes, const uint32_t* offsets_dw,
                                            const uint16_t* lens, uint32_t n, const halo_arp_result_t* results,
                                            uint8_t* out, halo_egress_port_t* ports, uint32_t* pkt_off_dw,
                                            uint16_t* pkt_len, uint32_t* index, uint32_t* skipped) {
    const int rc = check_args(cfg, 1, bytes, offsets_dw, lens, n, results, out, ports, pkt_off_dw, pkt_len, index, skipped);
    if (rc) return rc;
    const uint32_t n_netifs = cfg->n_netifs, cap = cfg->index_cap;
    const uint64_t region = cfg->region_bytes;
    memset(ports, 0, n_netifs * sizeof *ports);
    bool cut[HALO_ARP_MAX_NETIFS] = {};  // the NetIf met a packet that did not fit
    uint32_t skips = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t p = netif_of(load_u32(reinterpret_cast<const uint8_t*>(results) + 8ull * i), n_netifs);
        if (p >= n_netifs) continue;
        const uint32_t len = lens[i];
        const uint8_t* f = bytes + 4ull * offsets_dw[i];
        uint32_t plen = len - kEthHeader;
        bool ok;
        if (cfg->flags & HALO_LO_TX) {
            ok = tx_has_total_len(len);
            if (ok) plen = tx_total_len(load_u32(f + 16)), ok = tx_sendable(plen, len);
        } else {
            ok = fwd_sendable(len, cfg->flags);
        }
        if (!ok) {
            ++skips;
            continue;
        }
        const uint32_t size = packet_size(plen);
        halo_egress_port_t& s = ports[p];
        const bool fits = !cut[p] && s.bytes + size <= region;
        if (s.frames < cap) {
            const uint64_t at = (uint64_t)p * cap + s.frames;
            pkt_off_dw[at] = fits ? (uint32_t)(s.bytes / 4) : kNotWritten;
            pkt_len[at] = (uint16_t)plen;
            index[at] = i;
        }
        if (fits) {
            uint8_t* o = out + p * region + s.bytes;
            memcpy(o, f + kEthHeader, plen);
            memset(o + plen, 0, size - plen);
            ++s.frames_written;
            s.bytes_written += size;
        } else {
            cut[p] = true;
        }
        ++s.frames;
        s.bytes += size;
    }
    if (skipped) *skipped += skips;
    return HALO_OK;
}
