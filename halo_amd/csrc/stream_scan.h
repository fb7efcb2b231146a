// stream_scan.h — what the stream stages share on the device (port_streams.h: a stream per port,
// of ring records for tx_egress.hip and of L3 packets for lo_gather.hip; rx_deliver.hip: one of
// delivery records; a stream's region takes the longest prefix of whole records that fits): the
// one-workgroup scan of the tiles' record counts and bytes together, which finds the tile the
// region's cut falls in, and the count kernels' wave sum. On top of tile_scan.h. gfx950 only.
// (The scatter's fit bookkeeping and copy loop stay in port_streams.h and rx_deliver.hip:
// DESIGN.md §22.1, §22.4.)
#pragma once
#include <stddef.h>

#include "../../include/halo_rx.h"
#include "tile_scan.h"

namespace halo {
namespace {

// What a stream's summary starts with: halo_egress_port_t whole, halo_deliver_summary_t's first 24 bytes.
struct StreamSummary {
    uint32_t total, written;  // records selected, also beyond the region; the prefix of them that fits wholly
    unsigned long long bytes, bytes_written;
};
#define HALO_STARTS_AS_STREAM(T, total_m, written_m)                                                     \
    (offsetof(T, total_m) == offsetof(StreamSummary, total) && offsetof(T, written_m) == offsetof(StreamSummary, written) && \
     offsetof(T, bytes) == offsetof(StreamSummary, bytes) && offsetof(T, bytes_written) == offsetof(StreamSummary, bytes_written))
static_assert(HALO_STARTS_AS_STREAM(halo_egress_port_t, frames, frames_written) &&
                  HALO_STARTS_AS_STREAM(halo_deliver_summary_t, records, records_written),
              "both summaries start as StreamSummary");
#undef HALO_STARTS_AS_STREAM
// A scan kernel touches its summary through StreamSummary* only (the scatter kernels, through the C
// type only), so no kernel reads through one type what it wrote through the other.

// x summed over the wave, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
    for (uint32_t d = 32; d; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

struct StreamTotals {  // records and record bytes
    uint32_t c;
    unsigned long long b;
};
struct StreamScanLds {  // the wave totals of a pass, double-buffered
    uint32_t c[2][4];
    unsigned long long b[2][4];
};

// One workgroup of 256 lanes, one stream of n_tiles tiles: cnt[t] (a tile's records) becomes the
// records of the tiles before t, byte_base[t] the sum of tile_bytes before t; returns the sums of
// all, in every lane. One barrier per pass: the wave totals are double-buffered in `s` (the
// caller's: it may use the slots again behind a __syncthreads) and the carry lives in registers.
// The written prefix needs no reduction: the tile the cut falls in is the one with base <= region
// < base + bytes, and its lane writes the prefix of whole tiles before it to o (the scatter adds
// that tile's own part). per_tile(t, in) is called for each of the lane's four tiles of a pass,
// in = t < n_tiles: a callable that loads selects on `in`, as the scan's own loads do, so that a
// pass's loads all issue before the one wait (a load under a branch on `in` waited per tile).
template <typename PerTile>
__device__ __forceinline__ StreamTotals scan_stream_tiles(StreamScanLds& s, uint32_t* cnt, const uint32_t* tile_bytes,
                                                          uint64_t* byte_base, uint32_t n_tiles, uint64_t region,
                                                          StreamSummary* o, PerTile per_tile) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t base_c = 0, par = 0;
    unsigned long long base_b = 0;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += kScanPass, par ^= 1) {
        const uint32_t t = t0 + 4 * threadIdx.x;
        uint32_t c[4], b[4], csum = 0;
        unsigned long long bsum = 0;
        for (uint32_t k = 0; k < 4; ++k) {
            c[k] = t + k < n_tiles ? cnt[t + k] : 0u;
            b[k] = t + k < n_tiles ? tile_bytes[t + k] : 0u;
            per_tile(t + k, t + k < n_tiles);
            csum += c[k];
            bsum += b[k];
        }
        const uint32_t cinc = wave_inclusive(csum, lane);
        const unsigned long long binc = wave_inclusive(bsum, lane);
        if (lane == 63) s.c[par][wave] = cinc, s.b[par][wave] = binc;
        __syncthreads();
        uint32_t run_c = base_c + cinc - csum;
        unsigned long long run_b = base_b + binc - bsum;
        for (uint32_t w = 0; w < 4; ++w) {
            if (w < wave) run_c += s.c[par][w], run_b += s.b[par][w];
            base_c += s.c[par][w];
            base_b += s.b[par][w];
        }
        for (uint32_t k = 0; k < 4; ++k) {
            if (t + k < n_tiles) {
                cnt[t + k] = run_c;
                byte_base[t + k] = run_b;
                if (run_b <= region && run_b + b[k] > region) o->written = run_c, o->bytes_written = run_b;  // the cut is here
            }
            run_c += c[k];
            run_b += b[k];
        }
    }
    return StreamTotals{base_c, base_b};
}

// The scan's last writes, by one lane: the totals, which are the written prefix too without a cut.
__device__ __forceinline__ void write_stream_totals(StreamSummary* o, StreamTotals all, uint64_t region) {
    o->total = all.c, o->bytes = all.b;
    if (all.b <= region) o->written = all.c, o->bytes_written = all.b;
}

}  // namespace
}  // namespace halo
