// rx_stream.hip — the rx kernels for batches of mixed sizes, and their launches: the byte-stream
// kernel (frames packed densely in memory, mixed sizes or one size up to 1 KB) and the size-class mix
// kernel (mixed sizes that are not dense: a wave sorts its window by size class and runs one pass of
// G lanes per frame per class). The per-frame code is rx_frame.h, the histogram rx_hist.h.
#include <hip/hip_runtime.h>

#include "rx_frame.h"
#include "rx_launch.h"

namespace halo {
namespace {

// Mixed sizes (IMIX): each wave takes a window of 256 consecutive frames (four per lane), sorts
// them by size class into LDS (ballot ranks; the frame address and length travel with the
// entry, so nothing is re-loaded), then runs one pass per class with the lanes-per-frame that
// the uniform sweep found best for that size: <= 128 B (and frames failing the length check)
// lane per frame, <= 1024 B 4 lanes, <= 4096 B 8 lanes, longer 16 lanes. Every pass keeps all
// groups busy with frames of one class, so no lane waits behind a longer neighbour.
constexpr uint32_t kMixWindow = 256;                 // frames per wave window (a multiple of 64)
constexpr int kMixPer = (int)(kMixWindow / 64);      // frames per lane in the classification
// (Tried: frames > 4096 B on the 8-lane pass, no 16-lane pass compiled; in git history up to 9ac2a89.)

// Later-round chunks per lane in the mix passes: just enough for each class's size range in one
// later round trip (<= 128 B: 64 + 4*16 B; 570 B on 4 lanes: 256 + 5*64 B; 1500 B on 8 lanes:
// 512 + 8*128 B), so the short classes' passes do not hold the buffers the long ones need.
// IMIX 1.60 -> 1.58 ms, 570 B 150 -> 147 us (profiles/r01/ab_r43_mix_later_small.log, 5 vs 6
// chunks for 570 B: ab_r43_mix_later_g4.log; tried: kLaterChunks for every class; in git history
// up to 9ac2a89).
template <int G>
constexpr int kMixLater = G == 1 ? 4 : G == 4 ? 5 : kLaterChunks;

// Round 0 of the mix passes is kRound0 chunks per lane, as everywhere. Tried: 570 B on 4 lanes in
// one round trip (9 x 64 B >= 576 B), 1500 B on 8 lanes in one (12 x 128 B >= 1536 B): the bigger
// round 0 spills at occupancy 4 (IMIX 2.06 ms) and at occupancy 3 is slower still than two round
// trips (IMIX 1.69 ms, 570 B 173 us; profiles/r01/ab_r43_mix_round0_rejected.log; in git history up
// to 9ac2a89).

template <int G, int FUSE, bool L3>
__device__ __forceinline__ void mix_pass(const RxParams& p, uint32_t e_begin, uint32_t e_end, uint32_t lane,
                                         const uint64_t* s_ptr, const uint32_t* s_idx, const uint16_t* s_len,
                                         uint32_t len_max, Hist& hist) {
    constexpr uint32_t FPW = 64 / G;
    const uint32_t gl = lane & (G - 1);
    const uint32_t grp_base = lane & ~(uint32_t)(G - 1);
    for (uint32_t e0 = e_begin; e0 < e_end; e0 += FPW) {
        const uint32_t e = e0 + lane / G;
        const bool has = e < e_end;
        FrameState<G> st;
        st.frame = has ? reinterpret_cast<const uint8_t*>(s_ptr[e]) : p.bytes;
        st.L = has ? s_len[e] : 0u;
        st.ndw = (has && st.L >= (L3 ? 20u : kEthMin) && st.L <= len_max) ? (st.L + 3) >> 2 : 0;
        frame_loads(gl, st);
        frame_finish<G, FUSE, kMixLater<G>, kRound0, L3>(p, has ? s_idx[e] : 0u, has, gl, grp_base, st, hist);
    }
}

template <int LAYOUT, int FUSE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) rx_mix_kernel(const RxParams p) {
    __shared__ uint32_t s_hist[HALO_RX_STATUS_COUNT];
    __shared__ uint64_t s_ptr[4][kMixWindow];
    __shared__ uint32_t s_idx[4][kMixWindow];
    __shared__ uint16_t s_len[4][kMixWindow];
    if (threadIdx.x < HALO_RX_STATUS_COUNT) s_hist[threadIdx.x] = 0;
    __syncthreads();
    Hist hist = hist_open(p, s_hist);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = threadIdx.x >> 6;
    constexpr bool L3 = kL3<LAYOUT>;
    const bool jumbo = (p.flags & HALO_RX_JUMBO_EXT) != 0;
    const uint32_t len_max = L3 ? (jumbo ? kIpMaxJumbo : kIpMax) : (jumbo ? kEthMaxJumbo : kEthMax);
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t base = wave * kMixWindow; base < p.n; base += nwaves * kMixWindow) {
        // classify: frame base + 64k + lane, k < kMixPer
        const uint8_t* fp[kMixPer];
        uint32_t fl[kMixPer], cls[kMixPer];
#pragma unroll
        for (int k = 0; k < kMixPer; ++k) {
            const uint32_t i = base + 64 * k + lane;
            fp[k] = p.bytes;
            fl[k] = 0;
            if (i < p.n) frame_at<LAYOUT>(p, i, fp[k], fl[k]);
            cls[k] = i >= p.n ? 4u
                   : (fl[k] <= 128 || fl[k] > len_max) ? 0u
                   : fl[k] <= 1024 ? 1u : fl[k] <= 4096 ? 2u : 3u;
        }
        // counting sort by class: one ballot live at a time
        uint32_t pos[kMixPer];
        uint32_t start[5];
        uint32_t run = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            start[c] = run;
#pragma unroll
            for (int k = 0; k < kMixPer; ++k) {
                const uint64_t b = __ballot(cls[k] == (uint32_t)c);
                if (cls[k] == (uint32_t)c)
                    pos[k] = run + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32),
                                                  __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
                run += (uint32_t)__popcll(b);
            }
        }
        start[4] = run;
#pragma unroll
        for (int k = 0; k < kMixPer; ++k) {
            if (cls[k] < 4u) {
                s_ptr[w][pos[k]] = reinterpret_cast<uint64_t>(fp[k]);
                s_idx[w][pos[k]] = base + 64 * k + lane;
                s_len[w][pos[k]] = (uint16_t)fl[k];
            }
        }
        const uint32_t st0 = start[0], st1 = start[1], st2 = start[2], st3 = start[3], nall = start[4];
        __builtin_amdgcn_wave_barrier();
        mix_pass<1, FUSE, L3>(p, st0, st1, lane, s_ptr[w], s_idx[w], s_len[w], len_max, hist);
        mix_pass<4, FUSE, L3>(p, st1, st2, lane, s_ptr[w], s_idx[w], s_len[w], len_max, hist);
        mix_pass<8, FUSE, L3>(p, st2, st3, lane, s_ptr[w], s_idx[w], s_len[w], len_max, hist);
        mix_pass<16, FUSE, L3>(p, st3, nall, lane, s_ptr[w], s_idx[w], s_len[w], len_max, hist);
        __builtin_amdgcn_wave_barrier();
    }
    flush_hist(p, hist);
}

// ---- Byte-stream kernel (ragged batches of mixed sizes, DESIGN.md §4.3 "stream").
// A wave takes a window of 64 consecutive frames, one per lane. Each lane reads its frame's
// 48-byte header and runs the header checks (as the lane kernel). The L4 segment sums then come
// from ONE coalesced pass over the window's bytes: the wave streams [min segment start, max
// segment end) in 4 KB steps (64 contiguous bytes per lane), and a running prefix P of the
// 16-bit halves of every dword gives each frame's sum as P(end) - P(start). Halves sums keep the
// sum's value mod 0xFFFF and its zero-ness, which is all fold16 looks at; the u32 difference is
// exact for any segment (< 2^32 whatever the prefix wraps to). So every byte of a window is
// fetched once, in full 128-byte lines, whatever the sizes, and no lane waits on a longer
// neighbour. The step's bytes and its prefix at each 16-byte sub-chunk go to LDS; a lane whose
// segment starts or ends in the step reads its prefix back from there. A window whose frames are
// not dense in memory (span > 2 x their segment bytes + 8 KB, or a 4 KB page of the span holding
// no frame byte: window_pages_covered) sums each frame on its own lane.
constexpr uint32_t kStreamStep = 4096;  // bytes per wave per step: 64 lanes x 64 B

template <typename Op>
__device__ __forceinline__ uint32_t wave_allreduce(uint32_t x, Op op) {
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, false));
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, false));
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, kDppHalfMirror, 0xF, 0xF, false));
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, kDppMirror, 0xF, 0xF, false));
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)x, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)x, 16);
    const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)x, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)x, 48);
    return op(op(r0, r1), op(r2, r3));
}

// Exclusive prefix sum of x over the wave (lane order) and the wave total: row scans over DPP
// row_shr, row totals by v_readlane.
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t x, uint32_t lane, uint32_t& total) {
    uint32_t v = x;
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);  // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);  // row_shr:8
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 15), r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 31);
    const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 47), r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
    total = r0 + r1 + r2 + r3;
    const uint32_t row = lane >> 4;
    const uint32_t off = row == 0 ? 0u : row == 1 ? r0 : row == 2 ? r0 + r1 : r0 + r1 + r2;
    return v + off - x;
}

// one dword's two 16-bit halves added to acc (v_dot2_u32_u16)
__device__ __forceinline__ uint32_t halves_acc(uint32_t w, uint32_t acc) {
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const u16x2 one = {1, 1};
    return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, w), one, acc, false);
}

// P at step byte r, counting nb (0..4) bytes of the dword holding r: the sub-chunk's base plus
// the halves of its dwords below r's and of the low nb bytes of r's own.
__device__ __forceinline__ uint32_t stream_prefix(const uint32_t* s_base, const uint4* s_x, uint32_t r, uint32_t nb) {
    const uint32_t k = r >> 4, j = (r >> 2) & 3u;
    const uint4 q = s_x[k];
    const uint32_t part = nb >= 4 ? 0xFFFFFFFFu : (1u << (8 * nb)) - 1u;
    uint32_t acc = s_base[k];
    acc = halves_acc(q.x & (j > 0 ? 0xFFFFFFFFu : part), acc);
    acc = halves_acc(q.y & (j > 1 ? 0xFFFFFFFFu : j == 1 ? part : 0u), acc);
    acc = halves_acc(q.z & (j > 2 ? 0xFFFFFFFFu : j == 2 ? part : 0u), acc);
    return halves_acc(q.w & (j == 3 ? part : 0u), acc);
}

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Stream origin alignment (bytes; the first step starts at the window's lowest byte rounded
// down to it). Measured and removed (profiles/r02/stream/stream1-3.log): software-pipelining the
// step loads (+16 VGPRs: 570 B 132 -> 156 us), issuing the next step's loads before this step's
// lookups, and prefetching the next window's addresses / headers (neutral or slower).
constexpr uint32_t kStreamAlign = 128;

// This lane's 64 bytes of the step at s0 (sub-chunk u at s0 + 1024u + 16 lane, so each load
// instruction reads 1 KB contiguous): always four 16-byte loads, no branch, so the load counter
// stays exact across steps. Positions are 16-byte aligned in memory and a window streams only
// when every page of [lo, hi) holds a frame dword (window_pages_covered), so every block in
// [lo, hi) is readable; a sub-chunk wholly outside reads the nearest such block instead. Bytes
// outside the frames are never inside a segment or header, and P differences cancel them.
__device__ __forceinline__ void stream_load(uint64_t B, uint32_t s0, uint32_t lane, uint32_t lo, uint32_t hi,
                                            uint32_t (&x)[4][4]) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(16)));
    const uint32_t first = lo & ~15u, last = (hi - 1u) & ~15u;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        uint32_t a = s0 + 1024u * u + 16 * lane;
        a = a < first ? first : a > last ? last : a;
        const u32x4 q = *(const __attribute__((address_space(1))) u32x4*)(B + a);
        x[u][0] = q.x; x[u][1] = q.y; x[u][2] = q.z; x[u][3] = q.w;
    }
}

// The read contract of include/halo_rx.h: no kernel reads a page that holds no frame byte. The
// stream reads every 16-byte block in [lo, hi) (clamped to it), so a window streams only when
// every 4 KB page of [lo, hi) holds a readable dword of one of its frames (member lanes `in`,
// frame dwords [ps, ps + nb)); pg0 = the stream base's offset in its page, so (position + pg0)
// >> 12 counts real pages. Pages are checked 32 at a time: each member lane ORs in the pages its
// frame touches, and the wave's union must be all of them. A window with a page-sized hole
// (frames in two allocations addressed from one base, or a sparse layout the 2x density test
// lets through) sums its frames lane by lane, reading nothing outside them.
__device__ __forceinline__ bool window_pages_covered(bool in, uint32_t ps, uint32_t nb, uint32_t lo, uint32_t hi,
                                                     uint32_t pg0) {
    const uint32_t P0 = (lo + pg0) >> 12;
    const uint32_t np = ((hi - 1u + pg0) >> 12) - P0 + 1u;
    const uint32_t a = in ? ((ps + pg0) >> 12) - P0 : 1u, b = in ? ((ps + nb - 1u + pg0) >> 12) - P0 : 0u;
    const auto uor = [](uint32_t x, uint32_t y) { return x | y; };
    for (uint32_t w0 = 0; w0 < np; w0 += 32) {
        const uint32_t w1 = np - 1u < w0 + 31u ? np - 1u : w0 + 31u;
        const uint32_t lb = a > w0 ? a : w0, hb = b < w1 ? b : w1;
        const uint32_t m = lb <= hb ? ((2u << (hb - lb)) - 1u) << (lb - w0) : 0u;
        if (wave_allreduce(m, uor) != (2u << (w1 - w0)) - 1u) return false;
    }
    return true;
}

// Threads per block and waves per EU of the stream kernel. (Tried: dynamic LDS padding per block
// for uniform batches, the next step's loads issued before this step is summed, and every call on
// the instance without HDR; in git history up to 9ac2a89.)
constexpr int kStreamBlock = 256, kStreamWaves = 6;

// One stream step's 64 bytes of this lane: their 16-byte sub-chunk prefixes (P at each sub-chunk
// start; carry = P at the step start) and the bytes, to the wave's LDS.
__device__ __forceinline__ void stream_sum(const uint32_t (&x)[4][4], uint32_t lane, uint32_t& carry,
                                           uint32_t* s_base, uint4* s_x) {
    uint32_t s[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
        s[u] = halves_acc(x[u][3], halves_acc(x[u][2], halves_acc(x[u][1], halves_acc(x[u][0], 0u))));
    uint32_t total;
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // sub-chunk k = 64u + lane in stream order
        s_base[u * 64 + lane] = carry + wave_excl_scan(s[u], lane, total);
        carry += total;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) s_x[u * 64 + lane] = make_uint4(x[u][0], x[u][1], x[u][2], x[u][3]);
    wave_lds_sync();
}

// HDR (chosen per call: checksums on): the headers come out of the stream too. Each lane copies
// its frame's 48 header bytes from the step buffer as the stream passes them, and its segment end
// follows from the IPv4 total length (the parse's seg_end = O + totalLen) as soon as that field
// has passed; the header checks run once after the stream. Every byte of a dense window is then
// fetched from HBM exactly once. Without HDR (checksums off: only ICMP frames have a segment),
// the lane reads its header first and the stream covers only the windows' segments.
// Mixed-size batches (IMIX) take the stream kernel in one-wave blocks with 1.5 KB of LDS padding
// (22 blocks = 5.5 waves per SIMD resident): IMIX 1.27 -> 1.25 ms; uniform batches keep 256-thread
// blocks, which the 570 B line prefers (127 vs 133 us; profiles/r02/ab_stream_group_block_uncapped.log).
constexpr int kStreamMixedBlock = 64;
constexpr uint32_t kStreamMixedLdsPad = 1536;
template <int LAYOUT, int FUSE, bool HDR, int BLK = kStreamBlock>
__global__ void __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu(kStreamWaves)))
rx_stream_kernel(const RxParams p) {
    constexpr int kW = BLK / 64;
    __shared__ uint32_t s_hist[HALO_RX_STATUS_COUNT];
    __shared__ uint4 s_x[kW][kStreamStep / 16];       // per wave: the step's bytes (records at the end)
    __shared__ uint32_t s_base[kW][kStreamStep / 16];  // per wave: P at each 16-byte sub-chunk
    if (threadIdx.x < HALO_RX_STATUS_COUNT) s_hist[threadIdx.x] = 0;
    __syncthreads();
    Hist hist = hist_open(p, s_hist);
    constexpr bool L3 = kL3<LAYOUT>;
    constexpr uint32_t O = kIpOff<L3>;
    constexpr uint32_t kSeg = O + 20u;        // L4 segment start in the frame (34 or 20)
    constexpr uint32_t kTlDw = (O + 2u) / 4u;  // the header dword holding the IPv4 total length
    constexpr uint32_t kNone = 0xFFFFFFFFu;    // a position no step holds
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = threadIdx.x >> 6;
    const bool compact = (p.flags & HALO_RX_RECORD_COMPACT) != 0;
    const bool aligned = (reinterpret_cast<uint64_t>(p.bytes) & 3u) == 0;  // positions are dword-exact
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    const auto umin = [](uint32_t a, uint32_t b) { return a < b ? a : b; };
    const auto umax = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
    const auto uadd = [](uint32_t a, uint32_t b) { return a + b; };
    for (uint32_t wbase = wave * 64; wbase < p.n; wbase += nwaves * 64) {
        const uint32_t i = wbase + lane;
        const bool present = i < p.n;
        FrameState<1, 3> st;
        frame_meta<LAYOUT>(p, i, present, st);
        uint32_t h[12];
        Verdict v;
        uint64_t c = 0;
        bool done = false;  // wave-uniform: the window went through the stream
        if constexpr (HDR) {
            const bool rd = st.ndw != 0;
            const uint64_t rds = __ballot(rd);
            if (rds && aligned) {
                // positions relative to a base 2^30 below the first readable frame's 128-byte line
                const uint32_t first = (uint32_t)__builtin_ctzll(rds);
                const uint64_t fa = reinterpret_cast<uint64_t>(st.frame);
                const uint64_t ref = (((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(fa >> 32), first) << 32) |
                                      (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)fa, first)) & ~127ull;
                const uint64_t B = ref - (1ull << 30);
                const uint64_t d64 = fa - B;
                const uint32_t ps = (uint32_t)d64;
                const uint32_t lo = wave_allreduce(rd ? ps : kNone, umin);
                const uint32_t hi = wave_allreduce(rd ? ps + 4 * st.ndw : 0u, umax);
                const uint32_t sum = wave_allreduce(rd ? st.L : 0u, uadd);
                const uint32_t G0 = lo & ~(kStreamAlign - 1);
                const uint32_t span = hi - G0;
                if (!__ballot(rd && d64 >= (1ull << 31)) && span <= 2 * sum + 8192u &&
                    window_pages_covered(rd, ps, 4 * st.ndw, lo, hi, (uint32_t)B & 4095u)) {
#pragma unroll
                    for (int j = 0; j < 12; ++j) h[j] = 0;
                    const uint32_t pa = ps + kSeg;
                    uint32_t pb = kNone;  // the segment's last byte, once the total length has passed
                    uint32_t PA = 0, PB = 0, carry = 0;
                    const uint32_t nsteps = (span + kStreamStep - 1) / kStreamStep;
                    for (uint32_t t = 0; t < nsteps; ++t) {
                        const uint32_t s0 = G0 + t * kStreamStep;
                        uint32_t x[4][4];
                        stream_load(B, s0, lane, lo, hi, x);
                        stream_sum(x, lane, carry, s_base[w], s_x[w]);
                        const uint32_t* xw = reinterpret_cast<const uint32_t*>(s_x[w]);
                        const uint32_t r0 = ps - s0;  // header start in this step (wraps below it)
                        if (__ballot(rd && (r0 < kStreamStep || r0 + 48u < 48u + kStreamStep))) {
#pragma unroll
                            for (int j = 0; j < 12; ++j) {
                                const uint32_t r = r0 + 4u * j;
                                const uint32_t wv = xw[(r >> 2) & (kStreamStep / 4 - 1)];
                                if (rd && r < kStreamStep && (uint32_t)j < st.ndw) h[j] = wv;
                            }
                            if (rd && pb == kNone && r0 + 4u * kTlDw < kStreamStep && kTlDw < st.ndw) {
                                const uint32_t tl = L3 ? bswap16(h[0] >> 16) : bswap16(h[kTlDw] & 0xFFFFu);
                                pb = (tl >= 20u && O + tl <= st.L) ? ps + O + tl - 1u : kNone - 1u;
                            }
                        }
                        const uint32_t ra = pa - s0, rb = pb - s0;
                        if (rd && ra < kStreamStep) PA = stream_prefix(s_base[w], s_x[w], ra, ra & 3u);
                        if (rd && rb < kStreamStep) PB = stream_prefix(s_base[w], s_x[w], rb, (rb & 3u) + 1u);
                        wave_lds_sync();
                    }
                    v = parse_header<L3>(h, st.L, present, p);
                    if (v.seg_end) c = (uint32_t)(PB - PA);
                    done = true;
                }
            }
        }
        if (!done) {
            frame_loads(0u, st);
            frame_header(st, lane, h);
            v = parse_header<L3>(h, st.L, present, p);
            const bool seg = v.seg_end != 0;
            const uint64_t segs = __ballot(seg);
            bool streamed = false;
            if (!HDR && segs && aligned) {
                // positions relative to a base 2^30 below the first segment frame's 128-byte line
                const uint32_t first = (uint32_t)__builtin_ctzll(segs);
                const uint64_t fa = reinterpret_cast<uint64_t>(st.frame);
                const uint64_t ref = (((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(fa >> 32), first) << 32) |
                                      (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)fa, first)) & ~127ull;
                const uint64_t B = ref - (1ull << 30);
                const uint64_t d64 = fa - B;
                const uint32_t ps = (uint32_t)d64;
                const uint32_t pa = ps + kSeg, pe = ps + v.seg_end;  // the segment is [pa, pe)
                const uint32_t S = wave_allreduce(seg ? pa : kNone, umin);
                const uint32_t E = wave_allreduce(seg ? pe : 0u, umax);
                const uint32_t lo = wave_allreduce(seg ? ps : kNone, umin);
                const uint32_t hi = wave_allreduce(seg ? ps + 4 * st.ndw : 0u, umax);
                const uint32_t sum = wave_allreduce(seg ? v.seg_end - kSeg : 0u, uadd);
                const uint32_t G0 = S & ~(kStreamAlign - 1);
                const uint32_t span = E - G0;
                if (!__ballot(seg && d64 >= (1ull << 31)) && span <= 2 * sum + 8192u &&
                    window_pages_covered(seg, ps, 4 * st.ndw, lo, hi, (uint32_t)B & 4095u)) {
                    uint32_t PA = 0, PB = 0, carry = 0;
                    const uint32_t ea = pe - 1;  // the segment's last byte
                    const uint32_t nsteps = (span + kStreamStep - 1) / kStreamStep;
                    for (uint32_t t = 0; t < nsteps; ++t) {
                        const uint32_t s0 = G0 + t * kStreamStep;
                        uint32_t x[4][4];
                        stream_load(B, s0, lane, lo, hi, x);
                        stream_sum(x, lane, carry, s_base[w], s_x[w]);
                        const uint32_t ra = pa - s0, rb = ea - s0;
                        if (seg && ra < kStreamStep) PA = stream_prefix(s_base[w], s_x[w], ra, ra & 3u);
                        if (seg && rb < kStreamStep) PB = stream_prefix(s_base[w], s_x[w], rb, (rb & 3u) + 1u);
                        wave_lds_sync();
                    }
                    c = (uint32_t)(PB - PA);
                    streamed = true;
                }
            }
            if (seg && !streamed) {  // not dense (or unaligned data): this lane sums its own segment
                const uint32_t seg_dw = (v.seg_end + 3) >> 2;
                for (uint32_t d0 = (kSeg / 4) & ~3u; d0 < seg_dw; d0 += 4) {
                    uint32_t x[4];
                    load4(st.frame, d0, seg_dw, x);
                    acc_segment<L3>(x, d0, v.seg_end, c);
                }
            }
        }
        uint4* stage = reinterpret_cast<uint4*>(s_x[w]);
        frame_store<1, FUSE, L3>(p, i, present, 0, h, v, c, hist, &stage[compact ? lane : 2 * lane]);
        wave_lds_sync();
        const uint32_t nrec = p.n - wbase < 64 ? p.n - wbase : 64;
        if (compact) {
            if (lane < nrec) store16<kStoreStream>(reinterpret_cast<uint4*>(p.out) + wbase + lane, stage[lane]);
        } else {
            uint4* out4 = reinterpret_cast<uint4*>(p.out) + 2ull * wbase;
            if (lane < 2 * nrec) store16<kStoreStream>(out4 + lane, stage[lane]);
            if (64 + lane < 2 * nrec) store16<kStoreStream>(out4 + 64 + lane, stage[64 + lane]);
        }
        wave_lds_sync();
    }
    flush_hist(p, hist);
}

template <int BLK>
int launch_stream_blocks(const RxParams& p, int layout, int fuse, uint32_t dyn_lds, hipStream_t s) {
    return each_layout_fuse(layout, fuse, [&](auto layout_c, auto fuse_c) {
        constexpr int LAYOUT = decltype(layout_c)::value, FUSE = decltype(fuse_c)::value;
        constexpr uint32_t wpb = BLK / 64;
        const dim3 g(grid_for(p.n, 64, kMaxBlocks * 4 / wpb, wpb)), b(BLK);
        if (p.flags & HALO_RX_CSUM_ENABLE)
            hipLaunchKernelGGL((rx_stream_kernel<LAYOUT, FUSE, true, BLK>), g, b, dyn_lds, s, p);
        else
            hipLaunchKernelGGL((rx_stream_kernel<LAYOUT, FUSE, false, BLK>), g, b, dyn_lds, s, p);
        return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
    });
}

}  // namespace

int launch_mix(const RxParams& p, int layout, int fuse, hipStream_t s) {
    return each_layout_fuse(layout, fuse, [&](auto layout_c, auto fuse_c) {
        constexpr int LAYOUT = decltype(layout_c)::value, FUSE = decltype(fuse_c)::value;
        hipLaunchKernelGGL((rx_mix_kernel<LAYOUT, FUSE>), dim3(grid_for(p.n, kMixWindow)), dim3(256), 0, s, p);
        return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
    });
}

int launch_stream(const RxParams& p, int layout, int fuse, bool mixed, hipStream_t s) {
    return mixed ? launch_stream_blocks<kStreamMixedBlock>(p, layout, fuse, kStreamMixedLdsPad, s)
                 : launch_stream_blocks<kStreamBlock>(p, layout, fuse, 0, s);
}

}  // namespace halo
