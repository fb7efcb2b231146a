// kcp_crc_device.h — the CRC-32 of a byte string in HBM by a group of kCrcLanes lanes, which KCP
// ingest (rx_kcp.hip, to compare) and KCP emit (tx_kcp.hip, to fill the header's field) share:
// rx_kcp.h's arithmetic over whole aligned dwords. gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include "rx_kcp.h"

namespace halo {
namespace {

// `n` (1..4) data bytes at stream byte address a, in the low bytes
__device__ __forceinline__ uint32_t data_bytes(const uint32_t* dw, uint32_t a, uint32_t n) {
    const uint32_t s = a & 3u, lo = dw[a >> 2], hi = s + n > 4u ? dw[(a >> 2) + 1] : 0u;
    return deliver::funnel(lo, hi, s) & (n == 4u ? 0xFFFFFFFFu : (1u << 8u * n) - 1u);
}

// The CRC register after data bytes [b0, b1) at stream address a + b0.., from register c.
__device__ __forceinline__ uint32_t crc_chunk(const uint32_t* dw, uint32_t a, uint32_t b0, uint32_t b1, uint32_t c) {
    const uint32_t head = (b1 - b0) & 3u;  // a partial dword first: the rest ends on the chunk's end
    if (head) {
        c = kcp::crc_steps(c ^ data_bytes(dw, a + b0, head), 8u * head);
        b0 += head;
    }
    const uint32_t n = (b1 - b0) >> 2;
    if (n == 0) return c;
    const uint32_t at = a + b0, s = at & 3u;
    const uint32_t* p = dw + (at >> 2);
    uint32_t cur = p[0];
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t w = cur;
        if (s) {  // the dword's last s bytes lie in the next word
            cur = p[i + 1];
            w = deliver::funnel(w, cur, s);
        } else if (i + 1 < n) {
            cur = p[i + 1];
        }
        c = kcp::crc_steps(c ^ w, 32);
    }
    return c;
}

// crc32.ChecksumIEEE of `len` bytes at byte address a behind dw, by the kCrcLanes lanes of a group
// (g = the lane's number in it; every lane of the group calls, with the same a and len). The value
// is lane 0's.
__device__ __forceinline__ uint32_t crc_group(const uint32_t* dw, uint32_t a, uint32_t len, uint32_t g) {
    const uint32_t P = kcp::crc_passes(len);
    uint32_t v = 0;
    for (uint32_t p = 0; p < P; ++p) {
        uint32_t b0, b1;
        bool first;
        kcp::crc_lane_range(len, P, p, g, &b0, &b1, &first);
        if (p) v = kcp::crc_mulmod(v, kcp::kCrcXStride);  // pass 0 starts from zero
        if (b1 > b0) v ^= crc_chunk(dw, a, b0, b1, first ? 0xFFFFFFFFu : 0u);
    }
    // level l: lane g of every 2^(l+1) takes in lane g + 2^l. A one-pass segment occupies only its
    // last `occ` lanes: while occ <= 2^l the receiving lanes still hold zero, and zero times a
    // power of x is zero, so the multiplication is skipped (group-uniform).
    constexpr uint32_t x0 = kcp::crc_xlevel(0), x1 = kcp::crc_xlevel(1), x2 = kcp::crc_xlevel(2), x3 = kcp::crc_xlevel(3);
    static_assert(kcp::kCrcLevels == 4, "four levels written out");
    const uint32_t occ = P > 1 ? kcp::kCrcLanes : (len + kcp::kCrcChunk - 1) / kcp::kCrcChunk;
    v = (occ > 1 ? kcp::crc_mulmod(v, x0) : v) ^ __shfl_down(v, 1, kcp::kCrcLanes);
    v = (occ > 2 ? kcp::crc_mulmod(v, x1) : v) ^ __shfl_down(v, 2, kcp::kCrcLanes);
    v = (occ > 4 ? kcp::crc_mulmod(v, x2) : v) ^ __shfl_down(v, 4, kcp::kCrcLanes);
    v = (occ > 8 ? kcp::crc_mulmod(v, x3) : v) ^ __shfl_down(v, 8, kcp::kCrcLanes);
    return len ? ~v : 0u;
}

}  // namespace
}  // namespace halo
