// rx_group.hip — the rx kernel that puts G lanes of a wave on every frame of a uniform batch (G = 4,
// 8 or 16), and its launch. The mix kernel, which runs the same group passes per size class, lives
// in rx_stream.hip (DESIGN.md §22.3 says why). The per-frame code is rx_frame.h, the histogram rx_hist.h.
#include <hip/hip_runtime.h>

#include "rx_frame.h"
#include "rx_launch.h"

namespace halo {
namespace {

// Uniform batches: G lanes per frame for every frame (G in {1,4,8,16}); 64/G frames per wave.
template <int G, int LAYOUT, int FUSE, int R0 = kRound0, int U = kLaterChunks>
__device__ __forceinline__ void group_kernel_body(const RxParams& p) {
    constexpr uint32_t FPW = 64 / G;  // frames per wave
    __shared__ uint32_t s_hist[HALO_RX_STATUS_COUNT];
    if (threadIdx.x < HALO_RX_STATUS_COUNT) s_hist[threadIdx.x] = 0;
    __syncthreads();
    Hist hist = hist_open(p, s_hist);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gl = lane & (G - 1);
    const uint32_t grp_base = lane & ~(uint32_t)(G - 1);
    // frame indices fit in 32 bits (n is a u32): 32-bit loop state keeps the SGPR budget low
    // Blocks are dealt round-robin over the 8 XCDs, so neighbouring waves sit on different XCDs and
    // the 128-byte line two neighbouring frames share is fetched into two L2s: 1500 B frames read
    // 1.033x their bytes. Runs of R consecutive blocks per XCD, the XCDs taking runs in turn, keep
    // all but one wave boundary in 4R inside one L2 and still sweep the batch in order: R = 8 reads
    // 1.013x at the same time (r5p/r5q: R = 4 / 8 / 16 / 64 read 1.017 / 1.013 / 1.012 / 1.011x; one
    // contiguous range per XCD read 1.011x but ran 4 % slower). Not for 16 lanes per frame: jumbo
    // frames share a line in 9000 B and ran 0.5 % slower with it.
    uint32_t lblock = blockIdx.x;
    if constexpr (G <= 8) {
        constexpr uint32_t R = kGroupXcd;
        const uint32_t b = blockIdx.x, grp = b / (8 * R);
        if ((grp + 1) * 8 * R <= gridDim.x) lblock = grp * 8 * R + (b & 7u) * R + (b >> 3) % R;
    }
    const uint32_t wave = (lblock * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t base = wave * FPW; base < p.n; base += nwaves * FPW) {
        const uint32_t i = base + lane / G;
        process_frame<G, LAYOUT, FUSE, R0, U>(p, i, i < p.n, gl, grp_base, hist);
    }
    flush_hist(p, hist);
}

// G lanes per frame (G in {4, 8, 16}); VGPR-limited occupancy, so no SGPR cap.
// (Tried: other block sizes and dynamic LDS padding to cap the resident blocks per CU; in git
// history up to 9ac2a89.)
constexpr uint32_t kGroupBlock = 256, kGroupWaves = 5;
template <int G, int LAYOUT, int FUSE>
__global__ void __launch_bounds__(kGroupBlock) __attribute__((amdgpu_waves_per_eu(kGroupWaves)))
rx_group_kernel(const RxParams p) {
    static_assert(G == 4 || G == 8 || G == 16, "G must be 4, 8 or 16");
    group_kernel_body<G, LAYOUT, FUSE>(p);
}

}  // namespace

int launch_group(const RxParams& p, int layout, int fuse, int lanes, hipStream_t s) {
    if (lanes != 4 && lanes != 8 && lanes != 16) return HALO_E_INVAL;
    return each_layout_fuse(layout, fuse, [&](auto layout_c, auto fuse_c) {
        constexpr int LAYOUT = decltype(layout_c)::value, FUSE = decltype(fuse_c)::value;
        constexpr uint32_t wpb = kGroupBlock / 64;
        const dim3 b(kGroupBlock);
        const uint64_t cap = kMaxBlocks * 4 / wpb;
        if (lanes == 4)
            hipLaunchKernelGGL((rx_group_kernel<4, LAYOUT, FUSE>), dim3(grid_for(p.n, 16, cap, wpb)), b, 0, s, p);
        else if (lanes == 8)
            hipLaunchKernelGGL((rx_group_kernel<8, LAYOUT, FUSE>), dim3(grid_for(p.n, 8, cap, wpb)), b, 0, s, p);
        else
            hipLaunchKernelGGL((rx_group_kernel<16, LAYOUT, FUSE>), dim3(grid_for(p.n, 4, cap, wpb)), b, 0, s, p);
        return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
    });
}

}  // namespace halo
