// rx_lane.hip — the lane-per-frame rx kernels: a wave's window of 64 consecutive frames, a lane each
// (lane_window: the straight-line fast path for windows of plain frames, frame_finish otherwise),
// run by rx_lane_kernel, its lean instance for launches without a histogram (rx_lane_lean1_kernel,
// one window per wave and no loop, when the grid covers the batch; rx_lane_lean_kernel otherwise), the
// several-batches kernel, and the resident small-poll consumer (ring_service_kernel); and their launches.
// The per-frame code is rx_frame.h, the histogram rx_hist.h.
#include <hip/hip_runtime.h>

#include "rx_frame.h"
#include "rx_launch.h"

namespace halo {
namespace {

// Lane per frame. The build lands at 76 VGPRs = 6 waves per SIMD; forcing 7 (72 VGPRs) or 8
// (64, with scratch spills) was not faster (profiles/r01/ab_r2o_lane_waves.log: 22.2 / 27.8 µs vs
// 21.9 µs on config 2; in git history up to 9ac2a89), so no waves-per-EU attribute. A wave's 64 records are
// consecutive: they are staged in LDS and written with fully coalesced 16-byte stores (a lane
// writing its own 32 B record at a 32 B stride stored the same bytes 25 % slower:
// profiles/r01/probe_store_patterns.log).
// One wave's window of 64 consecutive frames, a lane each (frames base .. base + 63): parse, stage
// the 64 records in the wave's LDS (s_rec_w: 128 x 16 B) and store them fully coalesced.
// ST: the store policy of the 64 records (store16). The default is what the ring service kernel
// takes; the two batch kernels pass kStoreLane.
//
// The fast path: a window whose 64 frames are all plain takes straight-line code (DESIGN.md
// §15.12). Plain: an Ethernet frame of 61..64 bytes (so each of the four round-0 chunks is one
// 16-byte load and nothing of the frame lies beyond them), IPv4 with header byte 0x45, not a
// fragment, UDP, and 28 <= totalLen <= L - 14 (the UDP length check of udp.go:22 included). Whether
// the lengths qualify is one ballot before the loads, which then carry no bounds test; the header
// tests are a second ballot once they land. Any other window, a partial last one included, takes
// frame_finish as before. LoChan packets (LAYOUT 3) always do.
constexpr uint32_t kLaneFastMaxWaves = 65536u;  // 4M frames: the largest launch measured to gain
template <int LAYOUT>
constexpr bool kLaneFast = !kL3<LAYOUT>;

// bswap16 of a dword's low half with one v_perm_b32 (selector bytes >= 0x0C give 0x00)
__device__ __forceinline__ uint32_t lane_total_len(const FrameState<1>& st) {
    return __builtin_amdgcn_perm(st.buf[1][0], st.buf[1][0], 0x0C0C0001u);
}

// The header part of "plain", for a lane whose st.ndw == 16.
__device__ __forceinline__ bool lane_plain(const FrameState<1>& st) {
    return (st.buf[0][3] & 0x00FFFFFFu) == 0x00450008u     // ethertype 0x0800, IP byte 0 == 0x45
        && (st.buf[1][1] & 0xFF00FFBFu) == 0x11000000u     // flags/fragment bytes 0x40|0x00, 0x00; UDP
        && lane_total_len(st) - 28u <= st.L - 42u;         // 28 <= totalLen <= L - 14
}

// frame_store's fused tails (FUSE, there) for a record of the fast path: they read only the 32 B
// record's fields (lo / hi: its two halves).
template <int FUSE>
__device__ __forceinline__ void fuse_tail(const RxParams& p, uint64_t i, const uint4& lo, const uint4& hi) {
    if constexpr (FUSE == 1) {  // the flow key from the record's own fields (flow_key.h)
        const uint64_t fh = flowkey::nat_hash(lo.y & 0xFFu, lo.z, lo.w, hi.x & 0xFFFFu, hi.x >> 16,
                                              p.flow_kind, p.flow_nat);
        p.flow_hash[i] = fh;
        if (p.flow_bucket) p.flow_bucket[i] = (uint32_t)(fh % p.flow_buckets);  // hashmap/hashmap.go:64
    }
    if constexpr (FUSE == 2)  // FindRoute(dst) (route_view.h)
        p.route_out[i] = find_route(LpmView{p.rt_tbl24, p.rt_tbl8, p.rt_lists, p.rt_ids}, lo.w);
}

// The record of a plain frame (parse_header + the segment sum + frame_store for that case), with no
// branch: the two statuses still possible are selects in the reference's order, IP_HDR_CKSUM before
// L4_CKSUM. Every sum is a chain of v_dot2_u32_u16 over the frame's dwords: a multiplier of 0 drops
// a half that lies outside the region, and dword 9's (1, 2) adds the UDP length field a second time
// for the pseudo-header. The segment [34, 14 + totalLen) ends in dwords 10..15, the only ones that
// need a mask: dword 10 + j keeps its low clamp(sh - 32 j, 0, 32) bits, sh = 8 (totalLen - 26).
template <int FUSE>
__device__ __forceinline__ void lane_fast_record(const RxParams& p, uint32_t i, uint32_t lane, const FrameState<1>& st, Hist& hist,
                                                 uint4* stage) {
    constexpr uint32_t kLo = 0x00000001u, kHi = 0x00010000u, kBoth = 0x00010001u;
    const uint32_t(&a)[4] = st.buf[0], (&b)[4] = st.buf[1], (&c)[4] = st.buf[2], (&d)[4] = st.buf[3];
    const bool csum = (p.flags & HALO_RX_CSUM_ENABLE) != 0;
    const uint32_t tl = lane_total_len(st);

    // IPv4 header bytes 14..33 (ipv4.go:74-78)
    uint32_t hs = dot2_halves(a[3], kHi, 0);
    hs = dot2_halves(b[0], kBoth, hs);
    hs = dot2_halves(b[1], kBoth, hs);
    hs = dot2_halves(b[2], kBoth, hs);
    hs = dot2_halves(b[3], kBoth, hs);
    hs = dot2_halves(c[0], kLo, hs);
    hs = dot2_halves(dot2_halves(hs, kBoth, 0), kBoth, 0);  // fold16
    const bool ip_bad = csum && hs != 0xFFFFu;

    // pseudo-header (src + dst, 0x0011 and the UDP length field, LE domain) + segment (udp.go:30-42)
    uint32_t s = dot2_halves(b[2], kHi, 0);
    s = dot2_halves(b[3], kBoth, s);
    s = dot2_halves(c[0], kBoth, s);
    s = dot2_halves(c[1], 0x00020001u, s);
    const int32_t sh = (int32_t)(8u * tl) - 208;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const uint32_t w = j < 2 ? c[2 + j] : d[j - 2];
        const int32_t x = sh - 32 * j, amt = x < 0 ? 0 : (x > 32 ? 32 : x);
        s = dot2_halves(w & ~(uint32_t)(~0ull << amt), kBoth, s);
    }
    s = dot2_halves(dot2_halves(s + 0x1100u, kBoth, 0), kBoth, 0);
    const bool l4_bad = csum && s != 0xFFFFu;

    // Only constants a VALU operand can hold inline from here on (selects take no literal, and a
    // constant in a register would live across the whole window loop).
    const uint32_t dm_hi = a[1] & 0xFFFFu;
    const bool mac = (a[0] == p.mac_lo && dm_hi == p.mac_hi) || (a[0] == 0xFFFFFFFFu && dm_hi == 0xFFFFu);
    // a frame failing the header sum carries what ParseEthFrm left (parse_header's early return)
    const uint32_t keep = ip_bad ? 0u : ~0u;
    const uint32_t src = __builtin_amdgcn_perm(b[3], b[2], 0x02030405u);   // bytes 26..29, big-endian
    const uint32_t dst = __builtin_amdgcn_perm(c[0], b[3], 0x02030405u);   // bytes 30..33
    const uint32_t ports = __builtin_amdgcn_perm(c[1], c[0], 0x04050203u); // sport | dport << 16
    const uint32_t flags_ip = ((c[0] & 0xFF00u) == 0xFF00u ? HALO_RX_F_IP_BCAST : 0u) |
                              (dst == p.own_ip ? HALO_RX_F_DST_IS_OWN : 0u);
    const uint32_t flags = (mac ? HALO_RX_F_MAC_MATCH : 0u) | (flags_ip & keep);
    const uint32_t status = ip_bad ? HALO_RX_IP_HDR_CKSUM : l4_bad ? HALO_RX_L4_CKSUM : HALO_RX_OK;
    // payload: 14, L - 14 / 34, totalLen - 20 / 42, totalLen - 28 (udp.go:47)
    const uint32_t no_udp = l4_bad ? 8u : 0u;  // the UDP header stays in the payload
    const uint32_t pay_off = ip_bad ? 14u : 42u - no_udp;
    const uint32_t pay_len = ip_bad ? st.L - 14u : tl + no_udp - 28u;
    uint4 lo, hi;
    lo.x = status | (flags << 8) | ((uint32_t)kEthIpv4 << 16);
    lo.y = ((ip_bad ? ~0u : (uint32_t)kIpUdp) & 0xFFu) | ((tl & keep) << 16);  // kIpUnknown == 0xFF
    lo.z = src & keep;
    lo.w = dst & keep;
    hi.x = ports & keep;
    hi.y = pay_off | (pay_len << 16);
    hi.z = 0;
    hi.w = 0;
    if (p.flags & HALO_RX_RECORD_COMPACT) {  // halo_rx_record16_t
        stage[0] = make_uint4((lo.x & 0xFFFFu) | (lo.y << 16 & 0xFF0000u), lo.z, lo.w, hi.x);
    } else {
        stage[0] = lo;
        stage[1] = hi;
    }
    if (p.hist) {
        // The window's OK count goes to the block's LDS counter in one add, where flush_hist puts
        // hist.ok too: a per-lane count would be one more register live across the general path.
        const uint64_t ok = __builtin_amdgcn_ballot_w64(status == HALO_RX_OK);
        if (status != HALO_RX_OK) atomicAdd(&hist.s[status], 1u);
        else if (lane == (uint32_t)__builtin_ctzll(ok)) atomicAdd(&hist.s[HALO_RX_OK], (uint32_t)__builtin_popcountll(ok));
    }
    fuse_tail<FUSE>(p, i, lo, hi);
}

// A wave's 64 staged records (fewer in the batch's last window) from s_rec_w to p.out.
template <int ST>
__device__ __forceinline__ void lane_window_store(const RxParams& p, uint32_t base, uint32_t lane, const uint4* s_rec_w) {
    __builtin_amdgcn_wave_barrier();
    const uint32_t nrec = p.n - base < 64 ? p.n - base : 64;  // records of this wave
    if (p.flags & HALO_RX_RECORD_COMPACT) {
        if (lane < nrec) store16<ST>(reinterpret_cast<uint4*>(p.out) + base + lane, s_rec_w[lane]);
    } else {
        uint4* out4 = reinterpret_cast<uint4*>(p.out) + 2ull * base;
        if (lane < 2 * nrec) store16<ST>(out4 + lane, s_rec_w[lane]);
        if (64 + lane < 2 * nrec) store16<ST>(out4 + 64 + lane, s_rec_w[64 + lane]);
    }
    __builtin_amdgcn_wave_barrier();
}

// Tried and removed (HALO_RX_LANE_SPAN): a window whose 64 frames lie back to back
// read as its 4096-byte span (four 1 KB rows per wave instead of four loads at a 64 B stride) and
// transposed through a 5120 B LDS window at an odd pitch. The counters showed there was nothing to
// win: the per-lane loads already cost one TCP->TCC request per 128 B line (35.1 per wave before and
// after) and the same 168 TCP accesses per wave; the span added 8 LDS instructions and 63 LDS cycles
// per wave. 1M x 64 B 18.74-18.91 -> 18.67-18.95 us, 4M 72.85-73.56 -> 72.38-73.62, 16M 279.9-282.7
// -> 279.5-282.2 (five interleaved rounds, profiles/r10/ab_span_lean.log).

// The whole window on the fast path, after frame_meta: false (nothing stored, st.buf not to be
// used) when some frame of it is not plain.
template <int FUSE, int ST>
__device__ __forceinline__ bool lane_window_fast(const RxParams& p, uint32_t base, uint32_t lane, FrameState<1>& st,
                                                uint4* s_rec_w, Hist& hist) {
    if (__builtin_amdgcn_ballot_w64(st.ndw != 16u) != 0) return false;
#pragma unroll
    for (int u = 0; u < 4; ++u) load4_inside(st.frame, u * 4, st.buf[u]);
    // The header tests read chunks 0 and 1 only; this use keeps the compiler from moving the last
    // chunk's load below the branch, where it would be a second memory round trip.
    asm volatile("" ::"v"(st.buf[3][3]));
    if (__builtin_amdgcn_ballot_w64(!lane_plain(st)) != 0) return false;
    const bool compact = (p.flags & HALO_RX_RECORD_COMPACT) != 0;
    lane_fast_record<FUSE>(p, base + lane, lane, st, hist, &s_rec_w[compact ? lane : 2 * lane]);
    lane_window_store<ST>(p, base, lane, s_rec_w);
    return true;
}

// The window on the general path, after frame_loads.
template <int LAYOUT, int FUSE, int ST>
__device__ __forceinline__ void lane_window_finish(const RxParams& p, uint32_t base, uint32_t lane, FrameState<1>& st,
                                                   uint4* s_rec_w, Hist& hist) {
    const bool compact = (p.flags & HALO_RX_RECORD_COMPACT) != 0;
    const uint32_t i = base + lane;
    frame_finish<1, FUSE, kLaterChunks, kRound0, kL3<LAYOUT>>(p, i, i < p.n, 0, lane, st, hist,
                                                              &s_rec_w[compact ? lane : 2 * lane]);
    lane_window_store<ST>(p, base, lane, s_rec_w);
}

// The kernel arguments a plain window reads, asked for in SGPRs at one point: the loads are then
// issued together and waited for once (one s_waitcnt lgkmcnt ahead of the metadata loads), not sunk
// to their uses in three dependent trips. The fused passes' arguments stay where the compiler puts them.
template <int LAYOUT>
__device__ __forceinline__ void lane_args(const RxParams& p) {
    asm volatile("" ::"s"(p.bytes), "s"(p.n), "s"(p.flags), "s"(p.mac_lo), "s"(p.mac_hi), "s"(p.own_ip), "s"(p.out));
    if constexpr (LAYOUT == 0 || LAYOUT == 3) asm volatile("" ::"s"(p.offsets_dw));
    if constexpr (LAYOUT != 2) asm volatile("" ::"s"(p.lens));
    if constexpr (LAYOUT == 1 || LAYOUT == 2) asm volatile("" ::"s"(p.stride));
    if constexpr (LAYOUT == 2) asm volatile("" ::"s"(p.len));
}

template <int LAYOUT, int FUSE, int ST = kStorePlain>
__device__ __forceinline__ void lane_window(const RxParams& p, uint32_t base, uint32_t lane, uint4* s_rec_w,
                                           Hist& hist, bool try_fast = true) {
    const uint32_t i = base + lane;
    FrameState<1> st;
    frame_meta<LAYOUT>(p, i, i < p.n, st);
    if (kLaneFast<LAYOUT> && try_fast) {
        // The outcome passes through an empty asm so that the compiler cannot thread the fast
        // attempt's two exits into the general path's entry: as one if / else the blocks are laid out
        // general first, the attempt's loads stay live across all of it, and the kernel needs 87
        // VGPRs instead of 72.
        // Tried and removed (part A): the outcome as a wave-uniform integer in an SGPR
        // instead of a bool through readfirstlane. The join then writes no VGPR, needs no
        // s_waitcnt vmcnt(0), and a plain window's wave ends with its record stores in flight (the
        // failing exits wait where the general path first rewrites a loaded register). Alone, in the
        // looping lean kernel: 1M x 64 B 18.56-18.88 -> 18.27-18.66 us, ranges overlap, median -0.20
        // against a parent spread of 0.32; on top of the one-window kernel 18.11-18.55 -> 17.98-18.33,
        // median -0.18: not told from noise either way (five interleaved rounds,
        // profiles/r11/ab_one_window.log). Ending the wave at the stores with s_endpgm moved the
        // fast blocks behind the general path: 58 -> 76 VGPRs.
        uint32_t done = __builtin_amdgcn_readfirstlane(lane_window_fast<FUSE, ST>(p, base, lane, st, s_rec_w, hist));
        asm volatile("" : "+s"(done));
        if (done == 1) return;
    }
    frame_loads<1>(0, st);
    lane_window_finish<LAYOUT, FUSE, ST>(p, base, lane, st, s_rec_w, hist);
}

// Threads per block of the lane kernel and 16-byte chunks per lane in its later load rounds
// (frames > 64 B only; kLaterChunks). One-wave blocks with 4.5 KB of LDS padding (22 blocks =
// 5.5 waves per SIMD resident, against 6 by registers) beat 256-thread blocks at every size
// measured: 1M x 64 B 22.2 -> 21.5 us, 16M x 64 B 321 -> 313 us, 128 B 49.8 -> 49.3 us
// (profiles/r02/lane_ab/: fewer frame bytes in flight per CU stream faster
// from HBM; occupancy 8 (4 later chunks: 60 VGPRs) was 2-8 % slower, 4 waves 2-9 % slower).
constexpr uint32_t kLaneBlock = 64;
// Dynamic LDS bytes per lane-kernel block: caps resident blocks per CU, i.e. the frame bytes in flight.
constexpr uint32_t kLaneLdsPad = 4608;
// Tried (in git history up to 9ac2a89): prefetching the next window's address/length in waves that
// loop: no gain at 1M (22.0 vs 22.1 us) and 3 % slower at 16M; with capped grids 2-11 % slower
// (profiles/r02/ab_lane_prefetch.log). XCD-contiguous block order (blocks b, b+8, ... share an XCD;
// with the remap each XCD's blocks took one contiguous range of the batch): rejected.

// The lean instance: a launch that keeps no status histogram (p.hist null, the
// headline call) runs an instance with HIST false: no s_hist and no block barrier, no hist_open /
// flush_hist, and p.hist a null constant wherever the window code tests it, so lane_fast_record and
// frame_store carry no counting. That instance also drops amdgpu_num_sgpr(80): SGPRs do not limit
// the occupancy of a 71-VGPR kernel on gfx950, and the cap only turned 39 SGPRs into v_writelane /
// v_readlane pairs. Its dynamic LDS grows by the bytes of the s_hist it lacks, so both instances
// allocate the same total per block and the resident blocks per CU do not change. Five interleaved
// rounds against the parent (profiles/r10/ab_span_lean.log): 1M x 64 B 18.74-18.91 -> 18.39-18.63 us,
// 4M 72.85-73.56 -> 72.13-72.97, 16M 279.9-282.7 -> 278.8-282.4
// (tried: every launch through rx_lane_kernel; in git history up to 9ac2a89).
constexpr uint32_t kLaneHistLds = sizeof(uint32_t) * HALO_RX_STATUS_COUNT;
constexpr uint32_t lane_dyn_lds(bool hist) { return kLaneLdsPad + (hist ? 0u : kLaneHistLds); }

template <int LAYOUT, int FUSE>
__global__ void __launch_bounds__(kLaneBlock) __attribute__((amdgpu_num_sgpr(80)))
rx_lane_kernel(const RxParams p) {
    __shared__ uint32_t s_hist[HALO_RX_STATUS_COUNT];
    __shared__ uint4 s_rec[kLaneBlock / 64][128];  // per wave: 64 records of 32 B
    if (threadIdx.x < HALO_RX_STATUS_COUNT) s_hist[threadIdx.x] = 0;
    __syncthreads();
    Hist hist = hist_open(p, s_hist);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t base = wave * 64; base < p.n; base += nwaves * 64) {
        // A 16M-frame launch is bound by memory and ran 2 % slower with the fast path (waves that
        // finish sooner put more requests in flight), 4M 3 % and 1M 14 % faster:
        // launches of up to kLaneFastMaxWaves waves only.
        lane_window<LAYOUT, FUSE, kStoreLane>(p, base, lane, s_rec[w], hist, nwaves <= kLaneFastMaxWaves);
    }
    flush_hist(p, hist);
}

// rx_lane_kernel for a launch without a histogram (the lean instance, above): the same windows
// from the same waves.
template <int LAYOUT, int FUSE>
__global__ void __launch_bounds__(kLaneBlock) rx_lane_lean_kernel(const RxParams p_in) {
    __shared__ uint4 s_rec[kLaneBlock / 64][128];
    RxParams p = p_in;
    p.hist = nullptr;  // a constant for the window code: no counting is compiled in
    Hist hist{nullptr, 0, 0};
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t base = wave * 64; base < p.n; base += nwaves * 64) {
        lane_window<LAYOUT, FUSE, kStoreLane>(p, base, lane, s_rec[w], hist, nwaves <= kLaneFastMaxWaves);
    }
}

// The lean instance for a launch whose grid covers the batch (launch_lane: every batch up to 2^30
// frames): block b is one wave and takes window b, nothing else. Without the loop
// the compiler no longer hoists the general path's constants (thirty scalar moves, eight v_dot2 of
// constants) in front of the window: a plain window executes 8 scalar and 7 vector instructions
// ahead of its metadata loads instead of 62 and 30, 126 VALU / 65 SALU per wave by the counters
// instead of 154 / 91, in 58 VGPRs instead of 68. The fast path's size gate reads p.n, which here is
// the grid: ceil(n / 64) <= kLaneFastMaxWaves. Launched with any other grid a block past the batch
// would store outside it, so launch_lane alone chooses it. Five interleaved rounds against the
// parent (profiles/r11/ab_one_window.log): 1M x 64 B 18.56-18.88 -> 18.11-18.55 us,
// 4M 72.05-72.91 -> 71.99-72.92, 16M 279.6-280.3 -> 279.1-280.1. kLaneLdsPad 4096 / 5120 and
// kLaneFastMaxWaves 262144 re-swept in the same job (on the build with lane_window's part A still in): no
// default changes (4096 and 262144 lose 1-3 % at 16M, 5120 equals 4608).
template <int LAYOUT, int FUSE>
__global__ void __launch_bounds__(kLaneBlock) rx_lane_lean1_kernel(const RxParams p_in) {
    static_assert(kLaneBlock == 64, "one wave per block");
    __shared__ uint4 s_rec[128];
    RxParams p = p_in;
    p.hist = nullptr;
    Hist hist{nullptr, 0, 0};
    lane_args<LAYOUT>(p);
    lane_window<LAYOUT, FUSE, kStoreLane>(p, blockIdx.x * 64u, threadIdx.x, s_rec, hist,
                                          p.n <= kLaneFastMaxWaves * 64u);
}

// Several batches in one launch (halo_rx_parse_batches_device): the batch stream of the reference's
// unbounded poll loop (engine/engine.go:344-351) handed over K batches at a time. A 1M-frame launch
// spends a fixed ramp and tail filling and draining 256 CUs — config 2 ran at 0.62 of 8 TB/s while
// the same kernel reached 0.74 on 16M frames — so the K batches' 64-frame windows are
// one grid: window w belongs to the batch whose cumulative window count first exceeds w (a
// wave-uniform scan over <= kMultiMax kernel arguments), and each wave runs the lane kernel's window
// code on that batch's arrays. Records, histogram and read contract are those of K separate launches.
// (The kernel's argument keeps the name it had before the launch moved behind rx_launch.h: a
// kernel's symbol spells its argument types, and traces name kernels by symbol.)
struct MultiParams : MultiBatches {};

template <int LAYOUT, bool HIST = true>  // HIST false: the launch keeps no histogram (the lean instance)
__global__ void __launch_bounds__(kLaneBlock) rx_lane_multi_kernel(const MultiParams mp) {
    __shared__ uint32_t s_hist[HALO_RX_STATUS_COUNT];
    __shared__ uint4 s_rec[kLaneBlock / 64][128];
    RxParams lean;
    if constexpr (HIST) {
        if (threadIdx.x < HALO_RX_STATUS_COUNT) s_hist[threadIdx.x] = 0;
        __syncthreads();
    } else {
        lean = mp.p;
        lean.hist = nullptr;
    }
    const RxParams& p0 = HIST ? mp.p : lean;
    Hist hist = hist_open(p0, HIST ? s_hist : nullptr);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t total = mp.win_end[mp.k - 1];
    for (uint32_t win = wave; win < total; win += nwaves) {
        uint32_t b = 0;
        while (win >= mp.win_end[b]) ++b;  // k <= 32, uniform across the wave
        RxParams p = p0;
        p.bytes = mp.bytes[b];
        p.offsets_dw = mp.offsets_dw[b];
        p.lens = mp.lens[b];
        p.out = mp.out[b];
        p.n = mp.n[b];
        const uint32_t base = (win - (b ? mp.win_end[b - 1] : 0u)) * 64u;
        lane_window<LAYOUT, 0, kStoreLane>(p, base, lane, s_rec[w], hist, nwaves <= kLaneFastMaxWaves);
    }
    if constexpr (HIST) flush_hist(p0, hist);
}

// The resident small-poll consumer (RingServiceCtl, halo_common.h), kSvcGroups workgroups of
// kSvcWaves waves. In each group wave 0 waits for a request: all its lanes load the request line
// (one 64-byte read of pinned host memory, system scope), s_sleep between tries, bounded by the
// stop flag and an idle timeout on the 100 MHz real-time counter, so every wave reaches the exit.
// A new req_seq whose check matches the fields of the same read is taken (the fields arrive with
// the sequence number: no second round trip); an acquire fence, then the group's waves parse their
// 64-frame windows (window k goes to group k % kSvcGroups, spreading a 1k-frame request over 8
// CUs' memory pipelines) with the lane kernel's window code; after a block barrier thread 0 fences
// and publishes the group's done_seq slot. Measured on one box (profiles/r03/r3j/ab_svc.log, 1 /
// 1000 frames per poll): 1 group x 16 waves 17.5 us at 1000; 8 x 8 9.2 / 11.8-12.6 us; 16 x 4
// 10.3 / 13.2-13.9; 32 x 2 16.5 / 20.4. Rejected: each group also reading its window's lengths
// with the request (offsets derived in-wave, no metadata read after the request: 11.5 / 13.3-13.6,
// the wider poll read cost more than the read it saved), and four poll reads in flight per group
// (profiles/r03/r3h: 25.9 us at 1000: the reads queued ahead of the frame reads).
// Idle exit is one decision for the grid: the first group whose timer runs out sets *quit (device
// memory) and every other group leaves at its next empty read of the request line, so a request
// that races the exit finds the whole kernel gone (the host relaunches within microseconds) rather
// than some groups alive for another 20 ms. Requests whose flags carry
// HALO_RX_L3_START (a LoChan drain through a host context) take the L3 layout.
__global__ void __launch_bounds__(64 * kSvcWaves) ring_service_kernel(RingServiceCtl* ctl, const uint8_t* data,
                                                                      const uint32_t* off, const uint16_t* len,
                                                                      uint32_t* quit_all, uint32_t last,
                                                                      uint64_t idle_ticks) {
    __shared__ uint32_t s_cmd[12];  // seq, exit, n, flags, mac_lo, mac_hi, own_ip, out_lo, out_hi, uni_off/stride/len
    __shared__ uint32_t s_hist[HALO_RX_STATUS_COUNT];
    __shared__ uint4 s_rec[kSvcWaves][128];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, g = blockIdx.x;
    uint32_t* line = reinterpret_cast<uint32_t*>(ctl);
    if (threadIdx.x < HALO_RX_STATUS_COUNT) s_hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) __hip_atomic_store(&ctl->alive[g], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    uint64_t t_idle = __builtin_amdgcn_s_memrealtime();
    for (;;) {
        if (w == 0) {
            uint32_t v, seq, quit = 0;
            for (;;) {
                v = __hip_atomic_load(&line[lane & 15u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                seq = __builtin_amdgcn_readlane(v, 0);
                if (seq != last) {
                    const uint32_t ck = svc_check(seq, __builtin_amdgcn_readlane(v, 1), __builtin_amdgcn_readlane(v, 2),
                                                  __builtin_amdgcn_readlane(v, 3), __builtin_amdgcn_readlane(v, 4),
                                                  __builtin_amdgcn_readlane(v, 5), __builtin_amdgcn_readlane(v, 6),
                                                  __builtin_amdgcn_readlane(v, 7), __builtin_amdgcn_readlane(v, 10),
                                                  __builtin_amdgcn_readlane(v, 11), __builtin_amdgcn_readlane(v, 12));
                    if (ck == __builtin_amdgcn_readlane(v, 9)) break;
                }
                const uint32_t others = __hip_atomic_load(quit_all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__builtin_amdgcn_readlane(v, 8) || others) {
                    quit = 1;
                    break;
                }
                if (__builtin_amdgcn_s_memrealtime() - t_idle > idle_ticks) {
                    if (lane == 0) __hip_atomic_store(quit_all, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    quit = 1;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            if (lane == 0) {
                s_cmd[0] = seq;
                s_cmd[1] = quit;
                s_cmd[2] = __builtin_amdgcn_readlane(v, 1);
                s_cmd[3] = __builtin_amdgcn_readlane(v, 2);
                s_cmd[4] = __builtin_amdgcn_readlane(v, 3);
                s_cmd[5] = __builtin_amdgcn_readlane(v, 4);
                s_cmd[6] = __builtin_amdgcn_readlane(v, 5);
                s_cmd[7] = __builtin_amdgcn_readlane(v, 6);
                s_cmd[8] = __builtin_amdgcn_readlane(v, 7);
                s_cmd[9] = __builtin_amdgcn_readlane(v, 10);
                s_cmd[10] = __builtin_amdgcn_readlane(v, 11);
                s_cmd[11] = __builtin_amdgcn_readlane(v, 12);
                if (!quit) ctl->t_seen[g] = __builtin_amdgcn_s_memrealtime();
            }
            // the request's off / len / frames are read after the request was seen
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        }
        __syncthreads();
        if (s_cmd[1]) break;
        RxParams p{};
        p.bytes = data;
        p.offsets_dw = off;
        p.lens = len;
        p.n = s_cmd[2];
        p.flags = s_cmd[3];
        p.mac_lo = s_cmd[4];
        p.mac_hi = s_cmd[5];
        p.own_ip = s_cmd[6];
        p.out = reinterpret_cast<halo_rx_result_t*>((uint64_t)s_cmd[7] | ((uint64_t)s_cmd[8] << 32));
        Hist hist{s_hist, 0, 0};  // the consumer keeps no histogram
        if (s_cmd[11]) {  // one length, consecutive records: the strided layout, no array reads
            p.bytes = data + 4ull * s_cmd[9];
            p.stride = 4ull * s_cmd[10];
            p.len = s_cmd[11];
            for (uint32_t base = (w * kSvcGroups + g) * 64; base < p.n; base += kSvcGroups * kSvcWaves * 64)
                lane_window<2, 0>(p, base, lane, s_rec[w], hist);
        } else if (p.flags & HALO_RX_L3_START) {
            for (uint32_t base = (w * kSvcGroups + g) * 64; base < p.n; base += kSvcGroups * kSvcWaves * 64)
                lane_window<3, 0>(p, base, lane, s_rec[w], hist);
        } else {
            for (uint32_t base = (w * kSvcGroups + g) * 64; base < p.n; base += kSvcGroups * kSvcWaves * 64)
                lane_window<0, 0>(p, base, lane, s_rec[w], hist);
        }
        __syncthreads();  // every record of this group stored
        if (threadIdx.x == 0) {
            ctl->t_done[g] = __builtin_amdgcn_s_memrealtime();
            __threadfence_system();
            __hip_atomic_store(&ctl->done_seq[g], s_cmd[0], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        last = s_cmd[0];
        t_idle = __builtin_amdgcn_s_memrealtime();
        __syncthreads();  // s_cmd is rewritten by the next wait
    }
    if (threadIdx.x == 0) __hip_atomic_store(&ctl->alive[g], 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

constexpr uint32_t kHistHalveMax = 16384u;  // lane-kernel grids up to this many blocks are halved when a histogram is kept

template <int LAYOUT>
void launch_multi(const MultiParams& mp, dim3 grid, hipStream_t s) {
    if (!mp.p.hist) {
        hipLaunchKernelGGL((rx_lane_multi_kernel<LAYOUT, false>), grid, dim3(kLaneBlock), lane_dyn_lds(false), s, mp);
        return;
    }
    hipLaunchKernelGGL((rx_lane_multi_kernel<LAYOUT, true>), grid, dim3(kLaneBlock), lane_dyn_lds(true), s, mp);
}

}  // namespace

// The launchers (rx_launch.h).

int launch_lane(const RxParams& p, int layout, int fuse, hipStream_t s) {
    return each_layout_fuse(layout, fuse, [&](auto layout_c, auto fuse_c) {
        constexpr int LAYOUT = decltype(layout_c)::value, FUSE = decltype(fuse_c)::value;
        constexpr uint32_t wpb = kLaneBlock / 64;
        uint32_t grid = grid_for(p.n, 64, kMaxBlocks * 4 / wpb, wpb);
        // with a status histogram, batches up to 1M frames take half the waves, two frame groups
        // each: half the arrivals in the histogram tree, whose tail is a fixed cost per launch
        // (1M x 64 B: +2.1 instead of +2.7 us, 8192 blocks; 4096 gave no gain, profiles/r05/r5zm)
        if (p.hist && grid <= kHistHalveMax) grid = (grid + 1) / 2;
        // one window per wave whenever the grid covers the batch (always, below the grid cap)
        if (!p.hist && (uint64_t)grid * 64u >= p.n)
            hipLaunchKernelGGL((rx_lane_lean1_kernel<LAYOUT, FUSE>), dim3(grid), dim3(kLaneBlock), lane_dyn_lds(false), s, p);
        else if (!p.hist)
            hipLaunchKernelGGL((rx_lane_lean_kernel<LAYOUT, FUSE>), dim3(grid), dim3(kLaneBlock), lane_dyn_lds(false), s, p);
        else
            hipLaunchKernelGGL((rx_lane_kernel<LAYOUT, FUSE>), dim3(grid), dim3(kLaneBlock), lane_dyn_lds(true), s, p);
        return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
    });
}

int launch_lane_multi(const MultiBatches& mb, int layout, uint64_t windows, hipStream_t s) {
    if (layout != 0 && layout != 3) return HALO_E_INVAL;
    constexpr uint32_t wpb = kLaneBlock / 64;
    const dim3 grid(grid_for(windows * 64u, 64, kMaxBlocks * 4 / wpb, wpb));
    const MultiParams mp{mb};
    if (layout == 3)
        launch_multi<3>(mp, grid, s);
    else
        launch_multi<0>(mp, grid, s);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

int launch_ring_service(RingServiceCtl* d_ctl, const uint8_t* d_data, const uint32_t* d_off, const uint16_t* d_len,
                        uint32_t* d_quit, uint32_t last, uint32_t idle_us, hipStream_t s) {
    if (hipMemsetAsync(d_quit, 0, sizeof(uint32_t), s) != hipSuccess) return HALO_E_HIP;
    hipLaunchKernelGGL(ring_service_kernel, dim3(kSvcGroups), dim3(64 * kSvcWaves), 0, s, d_ctl, d_data, d_off, d_len,
                       d_quit, last, (uint64_t)idle_us * 100u);  // s_memrealtime: 100 MHz
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

}  // namespace halo
