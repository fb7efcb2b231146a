// host_layout.h — what the host sides of the tile-based stages (tx_egress, tx_respond, tx_ring,
// rx_deliver, lo_gather) each had a copy of. Plain C++17, no HIP: the *_host.cc files and the
// layout headers that include it compile alone with g++. Host code only.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/halo_rx.h"

namespace halo {

// tiles of `tile` frames that cover n frames; one for an empty batch, so that no workspace is empty
inline uint64_t tiles_of(uint32_t n, uint32_t tile) {
    const uint64_t t = ((uint64_t)n + tile - 1) / tile;
    return t ? t : 1;
}
inline bool misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) & (a - 1); }  // a: a power of two
inline uint32_t load_u32(const void* p) {  // p needs no alignment
    uint32_t w;
    memcpy(&w, p, 4);
    return w;
}

// A per-port stream call (tx_egress, lo_gather; the kernels are port_streams.h). Its workspace: per
// port and tile a u64 byte base, then a u32 record count that the scan turns into the rank base,
// then a u32 byte count. Column-major: port p's tiles are contiguous.
constexpr uint64_t kPortStreamCellBytes = 16;
inline uint64_t port_stream_workspace(uint32_t n, uint32_t tile, uint32_t n_ports) {
    return kPortStreamCellBytes * tiles_of(n, tile) * n_ports;
}
// What its entry points all ask of the configuration, the batch and the outputs: HALO_E_INVAL or
// HALO_OK. out_align: 16 for a device region (the output's alignment), 1 for a host loop.
inline int check_port_stream_args(uint32_t n_ports, uint32_t max_ports, uint32_t flags, uint32_t allowed_flags,
                                  uint64_t region_bytes, uint64_t max_region, const void* out, uintptr_t out_align,
                                  const void* ports, const uint32_t* index, const uint32_t* skipped, const uint8_t* bytes,
                                  const uint32_t* offsets_dw, const uint16_t* lens, uint32_t n, const void* selectors) {
    if (!ports || n_ports < 1 || n_ports > max_ports || (flags & ~allowed_flags)) return HALO_E_INVAL;
    if ((region_bytes & (out_align - 1)) || region_bytes > max_region) return HALO_E_INVAL;
    if ((region_bytes && !out) || misaligned(out, out_align)) return HALO_E_INVAL;
    if (misaligned(ports, 8) || misaligned(index, 4) || misaligned(skipped, 4)) return HALO_E_INVAL;
    if (n && (!bytes || !offsets_dw || !lens || !selectors)) return HALO_E_INVAL;
    return misaligned(bytes, 4) || misaligned(offsets_dw, 4) || misaligned(lens, 2) ? HALO_E_INVAL : HALO_OK;
}

}  // namespace halo
