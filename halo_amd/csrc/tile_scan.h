// tile_scan.h — the workgroup-level steps of the count / scan / scatter kernels (arp_fwd.hip's
// gather, pmflow_fwd.hip's listing, tx_respond.hip, switch_fwd.hip's probe / scan / admit): a
// tile's count of selected lanes, the one-workgroup exclusive scan over the tile counts, and a
// lane's rank among the selected lanes of its tile; and the wave's inclusive prefix sum. The stream
// stages scan counts and bytes together: stream_scan.h, on top of this. gfx950 (CDNA4, wave64) only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace halo {
namespace {

// the number of set ballot bits below the calling lane
__device__ __forceinline__ uint32_t lanes_below(uint64_t ballot) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// x (u32 or u64) summed over the caller's lane (threadIdx.x & 63) and the lanes below it in the wave
template <typename T>
__device__ __forceinline__ T wave_inclusive(T x, uint32_t lane) {
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

constexpr uint32_t kScanPass = 1024;  // tiles per pass of a scan: four consecutive tiles per lane
static_assert(kScanPass == 4 * 256, "scan pass == four tiles per lane of a 256-lane workgroup");

// tiles[blockIdx.x] = the number of lanes of this workgroup for which sel() is true. sel is a
// callable, so that the counter is cleared, and that barrier passed, ahead of the lane's loads, as
// in the kernels this block came from. Holds two __syncthreads: every lane of the workgroup calls
// it, before any early return.
template <typename Sel>
__device__ __forceinline__ void tile_count(uint32_t* tiles, Sel sel) {
    __shared__ uint32_t s_sel;
    if (threadIdx.x == 0) s_sel = 0;
    __syncthreads();
    const uint32_t c = (uint32_t)__popcll(__ballot(sel()));
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(&s_sel, c);
    __syncthreads();
    if (threadIdx.x == 0) tiles[blockIdx.x] = s_sel;
}

// One workgroup of 256 lanes: tiles[t] becomes the sum of the tiles before t; returns the sum of
// all, in every lane.
__device__ __forceinline__ uint32_t scan_tiles(uint32_t* tiles, uint32_t n_tiles) {
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_base;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += kScanPass) {  // four consecutive tiles per lane and pass
        const uint32_t t = t0 + 4 * threadIdx.x;
        uint32_t x[4], sum = 0;
        for (uint32_t k = 0; k < 4; ++k) {
            x[k] = t + k < n_tiles ? tiles[t + k] : 0u;
            sum += x[k];
        }
        const uint32_t inc = wave_inclusive(sum, lane);
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        uint32_t before = s_base;
        for (uint32_t w = 0; w < wave; ++w) before += s_wave[w];
        uint32_t run = before + inc - sum;
        for (uint32_t k = 0; k < 4; ++k) {
            if (t + k < n_tiles) tiles[t + k] = run;
            run += x[k];
        }
        __syncthreads();
        if (threadIdx.x == 255) s_base = before + inc;
        __syncthreads();
    }
    return s_base;
}

// A lane's rank among the lanes of its kTile-lane workgroup with `sel`, in two steps, so that a
// kernel leaves between them with the lanes that need no rank, as each kernel did when it had this
// block to itself. tile_votes holds the __syncthreads: every lane of the workgroup calls it,
// before any early return.
template <uint32_t kTile>
__device__ __forceinline__ uint32_t* tile_wave_counts() {
    __shared__ uint32_t s_wave[kTile / 64];
    return s_wave;
}
// the ballot of `sel` over the caller's wave; every wave's count is in LDS when it returns
template <uint32_t kTile>
__device__ __forceinline__ uint64_t tile_votes(bool sel) {
    const uint64_t b = __ballot(sel);
    if ((threadIdx.x & 63u) == 0) tile_wave_counts<kTile>()[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    return b;
}
// base + the number of selected lanes of the workgroup before the caller, from its wave's votes
template <uint32_t kTile>
__device__ __forceinline__ uint32_t tile_rank(uint64_t votes, uint32_t base) {
    uint32_t rank = base + lanes_below(votes);
    for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) rank += tile_wave_counts<kTile>()[w];
    return rank;
}

}  // namespace
}  // namespace halo
