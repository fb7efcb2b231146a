// port_streams.h — the stable multi-way partition of a device-resident ragged batch into one stream
// per port, written once for the stages that run it: the egress step (tx_egress.hip: ring records,
// three selector kinds) and the loopback gather (lo_gather.hip: L3 packets, two modes). On
// stream_scan.h and host_layout.h. gfx950 only. DESIGN.md §22.4.
//
// Three launches, as the switch's probe / scan / admit and the ARP gather's count / scan / scatter:
//   count    one workgroup per tile of kPortTile frames (grid-stride over tiles): per port the tile's
//            record count and record bytes through LDS atomics (totals are order-free): one pair
//            per wave and port when a wave's frames all go the same way, else one per frame.
//   scan     one workgroup per port: the streams' scan (stream_scan.h) over the port's tiles, u32
//            rank bases and u64 byte bases; writes the port's summary. With a cut, the written
//            prefix is that of the whole tiles before it, and the scatter adds the cut tile's own
//            part (one workgroup per port: no atomics).
//   scatter  recomputes the masks; then per port that any frame of the tile goes to (a loop that is
//            uniform over the workgroup): ballot + mbcnt ranks and a wave scan of record sizes, wave
//            totals through LDS, the tile's bases added; the owning lane lists its record; every
//            record that fits leaves a descriptor in LDS and the workgroup copies them,
//            kLanesPerRec lanes per short record (a wave per long one).
//
// A stage is a struct of static __device__ __forceinline__ functions, and the kernels are templates
// over it (not helpers that take the callers' LDS slots: §22.1 measured what those cost):
//   Params                                     PortStreamParams, or a struct that starts as one
//   frame_ports(q, i, &len, &skip) -> uint64_t frame i's ports (0: none, or not sendable) and the
//                                              length its record is made from; *skip: selected but
//                                              not sendable. Loads nothing at i >= q.n.
//   size(len)                                  a record's bytes in its port's region, a multiple of 4
//   word(src, len, j)                          dword j < size(len) / 4 of the record of the frame
//                                              whose dwords start at src
//   list(q, slot, i, len, fits, byte_off)      the per-record entries at slot < n_ports * index_cap
#pragma once
#include <hip/hip_runtime.h>

#include "halo_common.h"
#include "host_layout.h"
#include "stream_scan.h"

namespace halo {
namespace {

constexpr uint32_t kPortTile = 256;      // frames per tile = lanes per workgroup of the count and scatter kernels
constexpr uint32_t kMaxStreamPorts = 64; // a frame's ports are the bits of a u64
constexpr uint32_t kLanesPerRec = 16;    // lanes that copy one short record together (a wave per long one)
constexpr uint32_t kSmallRecordDw = 32;  // "short": two dwords per lane cover the record

struct PortStreamParams {
    const uint8_t* bytes;
    const uint32_t* offsets_dw;
    const uint16_t* lens;
    const void* sel;  // the stage's selectors: u64 masks, ARP results or switch results
    uint64_t flood, valid, region;
    uint32_t n, n_tiles, n_ports, flags, index_cap;
    uint8_t* out;
    halo_egress_port_t* ports;
    uint32_t* index;
    uint32_t* skipped;
    // workspace, [port * n_tiles + tile]
    uint64_t* byte_base;   // scan: bytes of the port's records in earlier tiles
    uint32_t* rank_base;   // count: the tile's records; scan: the records in earlier tiles
    uint32_t* tile_bytes;  // count: the tile's record bytes
};
static_assert(sizeof(uint64_t) + 2 * sizeof(uint32_t) == kPortStreamCellBytes, "the workspace's bytes per port and tile");

template <class Stage>
__global__ void __launch_bounds__(kPortTile) port_count_kernel(const typename Stage::Params q) {
    __shared__ uint32_t s_cnt[kMaxStreamPorts], s_bytes[kMaxStreamPorts];
    uint32_t skips = 0;  // wave-uniform
    for (uint32_t tile = blockIdx.x; tile < q.n_tiles; tile += gridDim.x) {
        if (threadIdx.x < kMaxStreamPorts) s_cnt[threadIdx.x] = 0, s_bytes[threadIdx.x] = 0;
        __syncthreads();
        uint32_t len;
        bool skip;
        uint64_t m = Stage::frame_ports(q, tile * kPortTile + threadIdx.x, &len, &skip);
        skips += (uint32_t)__popcll(__ballot(skip));
        const uint32_t rec = Stage::size(len);
        // A wave whose selected frames all go to the same ports (one port, or a flood) adds its
        // count and one wave sum of record bytes per port from one lane; a lane per frame would
        // serialise on the port's slot. A wave of mixed ports adds lane by lane: aggregating port by
        // port costs a wave sum per distinct port and measured slower from four ports up.
        const uint64_t act = __ballot(m != 0);
        if (act) {
            const unsigned long long lead = __shfl((unsigned long long)m, (int)__builtin_ctzll(act), 64);
            if (__ballot(m != 0 && m != lead) == 0) {
                const uint32_t bytes = wave_sum(m ? rec : 0u);
                if ((threadIdx.x & 63u) == 0) {
                    for (uint64_t rest = lead; rest; rest &= rest - 1) {
                        const uint32_t p = (uint32_t)__builtin_ctzll(rest);
                        atomicAdd(&s_cnt[p], (uint32_t)__popcll(act));
                        atomicAdd(&s_bytes[p], bytes);
                    }
                }
            } else {
                while (m) {
                    const uint32_t p = (uint32_t)__builtin_ctzll(m);
                    m &= m - 1;
                    atomicAdd(&s_cnt[p], 1u);
                    atomicAdd(&s_bytes[p], rec);
                }
            }
        }
        __syncthreads();
        if (threadIdx.x < q.n_ports) {  // the lanes that zero these slots for the next tile
            q.rank_base[(uint64_t)threadIdx.x * q.n_tiles + tile] = s_cnt[threadIdx.x];
            q.tile_bytes[(uint64_t)threadIdx.x * q.n_tiles + tile] = s_bytes[threadIdx.x];
        }
    }
    if ((threadIdx.x & 63u) == 0 && skips && q.skipped) atomicAdd(q.skipped, skips);
}

// One workgroup per port: stream_scan.h's scan over the port's tiles, then the port's totals.
template <class Params>
__global__ void __launch_bounds__(256) port_scan_kernel(const Params q) {
    __shared__ StreamScanLds s_scan;
    const uint64_t first = (uint64_t)blockIdx.x * q.n_tiles;
    StreamSummary* o = reinterpret_cast<StreamSummary*>(q.ports + blockIdx.x);
    const StreamTotals all = scan_stream_tiles(s_scan, q.rank_base + first, q.tile_bytes + first, q.byte_base + first, q.n_tiles,
                                             q.region, o, [](uint32_t, bool) {});
    if (threadIdx.x == 0) write_stream_totals(o, all, q.region);
}

// The tile's nfit described records, LANES lanes per record: a group takes one record and walks
// its dwords. (Taking four records at a time with two dwords per lane of each loaded before the
// first store was measured and not kept: DESIGN.md §19.)
template <class Stage, uint32_t LANES>
__device__ __forceinline__ void copy_records(const typename Stage::Params& q, const uint4* desc, uint32_t nfit) {
    const uint32_t g = threadIdx.x % LANES;
    for (uint32_t k = threadIdx.x / LANES; k < nfit; k += kPortTile / LANES) {
        const uint4 d = desc[k];
        const uint32_t* src = reinterpret_cast<const uint32_t*>(q.bytes) + d.x;
        uint32_t* dst = reinterpret_cast<uint32_t*>(q.out + ((uint64_t)d.w << 32 | d.z));
        const uint32_t rec_dw = Stage::size(d.y) / 4;
        for (uint32_t j = g; j < rec_dw; j += LANES) dst[j] = Stage::word(src, d.y, j);
    }
}

template <class Stage>
__global__ void __launch_bounds__(kPortTile) port_scatter_kernel(const typename Stage::Params q) {
    __shared__ unsigned long long s_any;  // the ports any frame of the tile goes to
    // of the port in hand; two sets, so that a port's writes do not wait for the last port's reads
    __shared__ uint32_t s_wcnt[2][kPortTile / 64], s_wbytes[2][kPortTile / 64], s_nfit[2], s_fit_end[2];
    __shared__ uint4 s_desc[2][kPortTile];  // source dword offset, len, destination byte offset (lo, hi)
    __shared__ unsigned long long s_base_b[kMaxStreamPorts];  // the tile's bases, one load per tile and port
    __shared__ uint32_t s_base_r[kMaxStreamPorts];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t par = 0;
    for (uint32_t tile = blockIdx.x; tile < q.n_tiles; tile += gridDim.x) {
        if (threadIdx.x == 0) s_any = 0;
        __syncthreads();
        const uint32_t i = tile * kPortTile + threadIdx.x;
        uint32_t len;
        bool skip;
        const uint64_t m = Stage::frame_ports(q, i, &len, &skip);
        // the offset is loaded here, not by the stage, and the listing below stands before `fits`:
        // either moved, the egress instantiations are no longer the text they were (§22.4)
        const uint32_t rec = Stage::size(len), off = m ? q.offsets_dw[i] : 0u;
        if (m) atomicOr(&s_any, (unsigned long long)m);
        __syncthreads();
        uint64_t any = s_any;
        if (threadIdx.x < kMaxStreamPorts && ((any >> threadIdx.x) & 1)) {  // read behind the loop's first barrier
            s_base_b[threadIdx.x] = q.byte_base[(uint64_t)threadIdx.x * q.n_tiles + tile];
            s_base_r[threadIdx.x] = q.rank_base[(uint64_t)threadIdx.x * q.n_tiles + tile];
        }
        while (any) {  // uniform over the workgroup
            const uint32_t p = (uint32_t)__builtin_ctzll(any);
            any &= any - 1;
            const bool sel = (m >> p) & 1;
            const uint64_t b = __ballot(sel);
            const uint32_t size = sel ? rec : 0u;
            const uint32_t inc = wave_inclusive(size, lane);
            if (lane == 63) s_wcnt[par][wave] = (uint32_t)__popcll(b), s_wbytes[par][wave] = inc;
            if (threadIdx.x == 0) s_nfit[par] = 0, s_fit_end[par] = 0;
            __syncthreads();
            uint32_t rank = lanes_below(b), excl = inc - size, tile_cnt = 0;
            for (uint32_t w = 0; w < kPortTile / 64; ++w) {
                if (w < wave) rank += s_wcnt[par][w], excl += s_wbytes[par][w];
                tile_cnt += s_wcnt[par][w];
            }
            const uint64_t base_b = s_base_b[p];
            const uint32_t base_r = s_base_r[p];
            if (sel && base_r + rank < q.index_cap)
                Stage::list(q, (uint64_t)p * q.index_cap + base_r + rank, i, len, base_b + excl + size <= q.region, base_b + excl);
            const bool fits = sel && base_b + excl + size <= q.region;  // monotone: the fitting records are a prefix
            const uint64_t fb = __ballot(fits);
            if (fits) {
                const uint64_t dst = p * q.region + base_b + excl;
                s_desc[par][rank] = make_uint4(off, len, (uint32_t)dst, (uint32_t)(dst >> 32));
            }
            if (fb && lane == 63u - (uint32_t)__builtin_clzll(fb)) {  // the wave's last fitting record
                atomicAdd(&s_nfit[par], (uint32_t)__popcll(fb));
                atomicMax(&s_fit_end[par], excl + size);
            }
            __syncthreads();
            const uint32_t nfit = s_nfit[par];
            if (threadIdx.x == 0 && nfit < tile_cnt && base_b <= q.region) {  // the cut falls in this tile
                q.ports[p].frames_written += nfit;
                q.ports[p].bytes_written += s_fit_end[par];
            }
            if (s_fit_end[par] <= nfit * 4u * kSmallRecordDw)  // records of 128 bytes on average, or less
                copy_records<Stage, kLanesPerRec>(q, s_desc[par], nfit);
            else
                copy_records<Stage, 64>(q, s_desc[par], nfit);
            par ^= 1;
        }
    }
}

inline uint32_t port_stream_blocks(uint64_t tiles) {
    const uint64_t kMax = 256ull * 8;  // 8 workgroups per CU
    return (uint32_t)(tiles > kMax ? kMax : (tiles ? tiles : 1));
}

template <class Stage>
void launch_port_streams(const typename Stage::Params& q, hipStream_t st) {
    const uint32_t grid = port_stream_blocks(q.n_tiles);
    port_count_kernel<Stage><<<dim3(grid), dim3(kPortTile), 0, st>>>(q);
    port_scan_kernel<typename Stage::Params><<<dim3(q.n_ports), dim3(256), 0, st>>>(q);
    port_scatter_kernel<Stage><<<dim3(grid), dim3(kPortTile), 0, st>>>(q);
}

// What every stage fills alike: the batch's shape and the workspace's three arrays
// (port_stream_workspace bytes at d_workspace, 8-byte aligned).
inline void fill_port_streams(PortStreamParams& q, uint32_t n, uint32_t n_ports, uint32_t flags, uint64_t region,
                              void* d_workspace) {
    q.n = n, q.n_tiles = (uint32_t)tiles_of(n, kPortTile), q.n_ports = n_ports, q.flags = flags, q.region = region;
    const uint64_t cells = (uint64_t)q.n_tiles * n_ports;
    q.byte_base = static_cast<uint64_t*>(d_workspace);
    q.rank_base = reinterpret_cast<uint32_t*>(q.byte_base + cells);
    q.tile_bytes = q.rank_base + cells;
}

}  // namespace
}  // namespace halo
