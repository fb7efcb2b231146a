// rx_launch.h — how rx_parse.hip reaches the rx kernels: one launcher per kernel family, defined in
// the family's file next to its kernels, its grid and its LDS bytes. `layout` is RxParams' LAYOUT
// (0 ragged, 1 strided with lengths, 2 strided uniform, 3 ragged LoChan packets) and `fuse` the
// fused pass (0 none, 1 flow hash, 2 route). Every launcher instantiates the same six pairs
// (each_layout_fuse) and returns HALO_OK, HALO_E_HIP, or HALO_E_INVAL for any other pair.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "halo_common.h"

namespace halo {

int launch_lane(const RxParams& p, int layout, int fuse, hipStream_t s);                   // rx_lane.hip
int launch_group(const RxParams& p, int layout, int fuse, int lanes, hipStream_t s);       // rx_group.hip: lanes 4, 8, 16
int launch_mix(const RxParams& p, int layout, int fuse, hipStream_t s);                    // rx_stream.hip
int launch_stream(const RxParams& p, int layout, int fuse, bool mixed, hipStream_t s);     // rx_stream.hip: mixed = one-wave blocks

// halo_rx_parse_batches_device's launch: up to kMultiMax batches whose 64-frame windows form one grid
// (rx_lane_multi_kernel, rx_lane.hip). layout 0 or 3; `windows` = win_end[k - 1].
constexpr uint32_t kMultiMax = 32;
struct MultiBatches {
    RxParams p;  // the shared fields (flags, netif, histogram); per-batch arrays below
    uint32_t k;
    uint32_t win_end[kMultiMax];  // windows of batches 0..b
    uint32_t n[kMultiMax];
    const uint8_t* bytes[kMultiMax];
    const uint32_t* offsets_dw[kMultiMax];
    const uint16_t* lens[kMultiMax];
    halo_rx_result_t* out[kMultiMax];
};
int launch_lane_multi(const MultiBatches& mb, int layout, uint64_t windows, hipStream_t s);

// Grid cap, in 4-wave blocks (the lane kernel scales it to its block size). Effectively no cap:
// a launch takes one wave per 64 frames (per frame group) and lets the dispatcher refill CUs as
// waves finish. The round-1 cap of 16384 blocks made waves loop over several groups in big batches,
// and a looping wave serialises its round trips: lifting it took 16M x 64 B 314 -> 294 us,
// 128M x 64 B 2.74 -> 2.32 ms, IMIX 1.32 -> 1.28 ms, jumbo 6.20 -> 6.14 ms, 1500 B within noise
// (profiles/r02/ab_grid_cap_raised.log).
constexpr uint64_t kMaxBlocks = 4194304ull;
inline uint32_t grid_for(uint64_t n, uint32_t frames_per_wave, uint64_t max_blocks = kMaxBlocks,
                         uint32_t waves_per_block = 4) {
    const uint64_t waves = (n + frames_per_wave - 1) / frames_per_wave;
    uint64_t blocks = (waves + waves_per_block - 1) / waves_per_block;
    return (uint32_t)(blocks > max_blocks ? max_blocks : blocks);
}

// f(LAYOUT, FUSE) as compile-time constants for the (layout, fuse) pairs the library instantiates:
// every layout plain, and the two fused passes on the ragged layout alone.
template <typename F>
int each_layout_fuse(int layout, int fuse, F&& f) {
    using std::integral_constant;
    switch (layout * 4 + fuse) {
        case 0: return f(integral_constant<int, 0>{}, integral_constant<int, 0>{});
        case 1: return f(integral_constant<int, 0>{}, integral_constant<int, 1>{});
        case 2: return f(integral_constant<int, 0>{}, integral_constant<int, 2>{});
        case 4: return f(integral_constant<int, 1>{}, integral_constant<int, 0>{});
        case 8: return f(integral_constant<int, 2>{}, integral_constant<int, 0>{});
        case 12: return f(integral_constant<int, 3>{}, integral_constant<int, 0>{});
        default: return HALO_E_INVAL;
    }
}

}  // namespace halo
