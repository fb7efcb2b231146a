// host_layout.h — what the host sides of the tile-based stages (tx_egress, tx_respond, tx_ring,
// rx_deliver) each had a copy of. Plain C++17, no HIP: the *_host.cc files and the layout headers
// that include it compile alone with g++. Host code only.
#pragma once
#include <stdint.h>
#include <string.h>

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

}  // namespace halo
