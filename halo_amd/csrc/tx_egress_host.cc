// tx_egress_host.cc — the egress step's C entry points (include/halo_rx.h, "egress"): argument
// checks of the three device calls, which are answered before any device is looked for, and
// halo_tx_egress_host, the sequential loop with the same outputs. No HIP: the kernels live in
// tx_egress.hip behind egress::device_ops(), and this file compiles alone with g++
// (tools/fuzz_egress.cc drives it under ASan/UBSan).
#include <string.h>

#include "tx_egress.h"

namespace halo {
namespace egress {
namespace {

// What all four entry points ask of cfg, the batch and the outputs: host_layout.h's checks of a
// per-port stream call, the index list and the selectors' alignment by kind
int check_args(const halo_egress_config_t* cfg, const void* out, uintptr_t out_align, const halo_egress_port_t* ports,
               const uint32_t* index, const uint32_t* skipped, const uint8_t* bytes, const uint32_t* offsets_dw,
               const uint16_t* lens, uint32_t n, const void* selectors, uintptr_t selector_align) {
    if (!cfg || (cfg->index_cap && !index) || misaligned(selectors, selector_align)) return HALO_E_INVAL;
    return check_port_stream_args(cfg->n_ports, HALO_EGRESS_MAX_PORTS, cfg->flags, HALO_RX_JUMBO_EXT, cfg->region_bytes,
                                  1ull << 56, out, out_align, ports, index, skipped, bytes, offsets_dw, lens, n, selectors);
}

int device_call(const halo_egress_config_t* cfg, uint32_t kind, uintptr_t selector_align, const uint8_t* d_bytes,
                const uint32_t* d_offsets_dw, const uint16_t* d_lens, uint32_t n, const void* d_selectors,
                uint64_t flood_mask, uint8_t* d_out, halo_egress_port_t* d_ports, uint32_t* d_index, uint32_t* d_skipped,
                void* d_workspace, uint64_t workspace_bytes, halo_stream_t stream) {
    const int rc = check_args(cfg, d_out, 16, d_ports, d_index, d_skipped, d_bytes, d_offsets_dw, d_lens, n, d_selectors,
                              selector_align);
    if (rc) return rc;
    if (n && (!d_workspace || workspace_bytes < halo_tx_egress_workspace(n, cfg->n_ports))) return HALO_E_INVAL;
    if (misaligned(d_workspace, 8)) return HALO_E_INVAL;
    const DeviceOps* ops = device_ops ? device_ops() : nullptr;
    return ops ? ops->run(cfg, kind, d_bytes, d_offsets_dw, d_lens, n, d_selectors, flood_mask, d_out, d_ports, d_index,
                          d_skipped, d_workspace, stream)
               : HALO_E_NODEV;
}

}  // namespace
}  // namespace egress
}  // namespace halo

using namespace halo;  // host_layout.h
using namespace halo::egress;

// Workspace of a device call: host_layout.h's, for tiles of kTile frames
extern "C" HALO_API uint64_t halo_tx_egress_workspace(uint32_t n, uint32_t n_ports) {
    if (n_ports < 1 || n_ports > HALO_EGRESS_MAX_PORTS) return 0;
    return port_stream_workspace(n, kTile, n_ports);
}

extern "C" HALO_API int halo_tx_egress_masks_device(const halo_egress_config_t* cfg, const uint8_t* d_bytes,
                                                    const uint32_t* d_offsets_dw, const uint16_t* d_lens, uint32_t n,
                                                    const uint64_t* d_masks, uint8_t* d_out, halo_egress_port_t* d_ports,
                                                    uint32_t* d_index, uint32_t* d_skipped, void* d_workspace,
                                                    uint64_t workspace_bytes, halo_stream_t stream) {
    return device_call(cfg, HALO_EGRESS_KIND_MASKS, 8, d_bytes, d_offsets_dw, d_lens, n, d_masks, 0, d_out, d_ports,
                       d_index, d_skipped, d_workspace, workspace_bytes, stream);
}

extern "C" HALO_API int halo_tx_egress_arp_device(const halo_egress_config_t* cfg, const uint8_t* d_bytes,
                                                  const uint32_t* d_offsets_dw, const uint16_t* d_lens, uint32_t n,
                                                  const halo_arp_result_t* d_results, uint8_t* d_out,
                                                  halo_egress_port_t* d_ports, uint32_t* d_index, uint32_t* d_skipped,
                                                  void* d_workspace, uint64_t workspace_bytes, halo_stream_t stream) {
    return device_call(cfg, HALO_EGRESS_KIND_ARP, 8, d_bytes, d_offsets_dw, d_lens, n, d_results, 0, d_out, d_ports,
                       d_index, d_skipped, d_workspace, workspace_bytes, stream);
}

extern "C" HALO_API int halo_tx_egress_switch_device(const halo_egress_config_t* cfg, const uint8_t* d_bytes,
                                                     const uint32_t* d_offsets_dw, const uint16_t* d_lens, uint32_t n,
                                                     const halo_sw_result_t* d_results, uint64_t flood_mask,
                                                     uint8_t* d_out, halo_egress_port_t* d_ports, uint32_t* d_index,
                                                     uint32_t* d_skipped, void* d_workspace, uint64_t workspace_bytes,
                                                     halo_stream_t stream) {
    return device_call(cfg, HALO_EGRESS_KIND_SWITCH, 4, d_bytes, d_offsets_dw, d_lens, n, d_results, flood_mask, d_out,
                       d_ports, d_index, d_skipped, d_workspace, workspace_bytes, stream);
}

extern "C" HALO_API int halo_tx_egress_host(const halo_egress_config_t* cfg, uint32_t kind, const uint8_t* bytes,
                                            const uint32_t* offsets_dw, const uint16_t* lens, uint32_t n,
                                            const void* selectors, uint64_t flood_mask, uint8_t* out,
                                            halo_egress_port_t* ports, uint32_t* index, uint32_t* skipped) {
    if (kind > HALO_EGRESS_KIND_SWITCH) return HALO_E_INVAL;
    const int rc = check_args(cfg, out, 1, ports, index, skipped, bytes, offsets_dw, lens, n, selectors,
                              kind == HALO_EGRESS_KIND_SWITCH ? 4 : 8);
    if (rc) return rc;
    const uint32_t n_ports = cfg->n_ports;
    const uint64_t valid = port_bits(n_ports), region = cfg->region_bytes;
    memset(ports, 0, n_ports * sizeof *ports);
    bool cut[HALO_EGRESS_MAX_PORTS] = {};  // the port met a record that did not fit
    uint32_t skips = 0;
    const uint8_t* sel = static_cast<const uint8_t*>(selectors);
    for (uint32_t i = 0; i < n; ++i) {
        uint64_t m;
        if (kind == HALO_EGRESS_KIND_MASKS) {
            memcpy(&m, sel + 8ull * i, 8);
            m = mask_of_masks(m);
        } else if (kind == HALO_EGRESS_KIND_ARP) {
            m = mask_of_arp(load_u32(sel + 8ull * i));
        } else {
            m = mask_of_switch(load_u32(sel + 4ull * i), flood_mask);
        }
        m &= valid;
        if (!m) continue;
        const uint32_t len = lens[i];
        if (!sendable(len, cfg->flags)) {
            ++skips;
            continue;
        }
        const uint32_t tx = tx_len(len), rec = record_size(len);
        const uint8_t* src = bytes + 4ull * offsets_dw[i];
        for (uint32_t p = 0; p < n_ports; ++p) {
            if (!(m >> p & 1)) continue;
            halo_egress_port_t& s = ports[p];
            if (s.frames < cfg->index_cap) index[(uint64_t)p * cfg->index_cap + s.frames] = i;
            if (!cut[p] && s.bytes + rec <= region) {
                uint8_t* o = out + p * region + s.bytes;
                memcpy(o, &tx, 4);
                memcpy(o + 4, src, len);
                memset(o + 4 + len, 0, rec - 4 - len);
                ++s.frames_written;
                s.bytes_written += rec;
            } else {
                cut[p] = true;
            }
            ++s.frames;
            s.bytes += rec;
        }
    }
    if (skipped) *skipped += skips;
    return HALO_OK;
}
