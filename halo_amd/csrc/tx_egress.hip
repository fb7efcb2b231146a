// tx_egress.hip — the device side of the egress step (include/halo_rx.h, "egress") on gfx950: a
// stable multi-way partition of a device-resident ragged batch into one stream of ring records per
// egress port. tx_egress_host.cc checks the arguments and holds the host loop; tx_egress.h holds the
// layout arithmetic both share.
//
// Three launches, as the switch's probe / scan / admit and the ARP gather's count / scan / scatter:
//   count    one workgroup per tile of kTile frames (grid-stride over tiles): per port the tile's
//            record count and record bytes through LDS atomics (totals are order-free): one pair
//            per wave and port when a wave's frames all go the same way, else one per frame.
//   scan     one workgroup per port: the streams' scan (stream_scan.h) over the port's tiles, u32
//            rank bases and u64 byte bases; writes the port's summary. With a cut, the written
//            prefix is that of the whole tiles before it, and the scatter adds the cut tile's own
//            part (one workgroup per port: no atomics).
//   scatter  recomputes the masks; then per port that any frame of the tile goes to (a loop that is
//            uniform over the workgroup): ballot + mbcnt ranks and a wave scan of record sizes, wave
//            totals through LDS, the tile's bases added; every record that fits leaves a descriptor
//            in LDS and the workgroup copies them, kLanesPerRec lanes
//            per short record (a wave per long one). Source and destination are 4-byte aligned by
//            construction. The last source dword is masked to len, the rest of the record is zeros.
// The three front ends instantiate one body that differs only in how a frame's port mask is decoded.
#include <hip/hip_runtime.h>

#include "halo_common.h"
#include "stream_scan.h"
#include "tx_egress.h"

namespace halo {
namespace {

using egress::kTile;
constexpr uint32_t kLanesPerRec = 16;   // lanes that copy one short record together (a wave per long one)
constexpr uint32_t kSmallRecordDw = 32; // "short": two dwords per lane cover the record

struct EgressParams {
    const uint8_t* bytes;
    const uint32_t* offsets_dw;
    const uint16_t* lens;
    const void* sel;  // u64 masks, ARP results or switch results
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

template <uint32_t KIND>
__device__ __forceinline__ uint64_t frame_mask(const EgressParams& q, uint32_t i) {
    if (KIND == HALO_EGRESS_KIND_MASKS) return egress::mask_of_masks(static_cast<const uint64_t*>(q.sel)[i]);
    if (KIND == HALO_EGRESS_KIND_ARP) return egress::mask_of_arp(static_cast<const uint32_t*>(q.sel)[2ull * i]);
    return egress::mask_of_switch(static_cast<const uint32_t*>(q.sel)[i], q.flood);
}

// Frame i's ports (0: none, or not sendable) and length; *skip: selected but not sendable.
template <uint32_t KIND>
__device__ __forceinline__ uint64_t frame_ports(const EgressParams& q, uint32_t i, uint32_t* len, bool* skip) {
    *len = 0;
    *skip = false;
    if (i >= q.n) return 0;
    const uint64_t m = frame_mask<KIND>(q, i) & q.valid;
    if (!m) return 0;
    *len = q.lens[i];
    if (egress::sendable(*len, q.flags)) return m;
    *skip = true;
    return 0;
}

template <uint32_t KIND>
__global__ void __launch_bounds__(kTile) egress_count_kernel(const EgressParams q) {
    __shared__ uint32_t s_cnt[HALO_EGRESS_MAX_PORTS], s_bytes[HALO_EGRESS_MAX_PORTS];
    uint32_t skips = 0;  // wave-uniform
    for (uint32_t tile = blockIdx.x; tile < q.n_tiles; tile += gridDim.x) {
        if (threadIdx.x < HALO_EGRESS_MAX_PORTS) s_cnt[threadIdx.x] = 0, s_bytes[threadIdx.x] = 0;
        __syncthreads();
        uint32_t len;
        bool skip;
        uint64_t m = frame_ports<KIND>(q, tile * kTile + threadIdx.x, &len, &skip);
        skips += (uint32_t)__popcll(__ballot(skip));
        const uint32_t rec = egress::record_size(len);
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
__global__ void __launch_bounds__(256) egress_scan_kernel(const EgressParams q) {
    __shared__ StreamScanLds s_scan;
    const uint64_t first = (uint64_t)blockIdx.x * q.n_tiles;
    StreamSummary* o = reinterpret_cast<StreamSummary*>(q.ports + blockIdx.x);
    const StreamTotals all = scan_stream_tiles(s_scan, q.rank_base + first, q.tile_bytes + first, q.byte_base + first, q.n_tiles,
                                             q.region, o, [](uint32_t, bool) {});
    if (threadIdx.x == 0) write_stream_totals(o, all, q.region);
}

// Dword j of the record of a frame of len bytes at src: the length word, the frame's dwords with
// the last one masked to len, zeros to the record's end. The load stays inside the frame's words.
__device__ __forceinline__ uint32_t record_word(const uint32_t* __restrict__ src, uint32_t len, uint32_t j) {
    const uint32_t data_dw = (len + 3) / 4;
    const uint32_t at = j == 0 ? 0u : (j > data_dw ? data_dw - 1 : j - 1);
    uint32_t w = src[at];
    if (j == data_dw && (len & 3u)) w &= (1u << 8 * (len & 3u)) - 1u;
    return j == 0 ? egress::tx_len(len) : (j > data_dw ? 0u : w);
}

// The tile's nfit described records, LANES lanes per record: a group takes one record and walks
// its dwords. (Taking four records at a time with two dwords per lane of each loaded before the
// first store was measured and not kept: DESIGN.md §19.)
template <uint32_t LANES>
__device__ __forceinline__ void copy_records(const EgressParams& q, const uint4* desc, uint32_t nfit) {
    const uint32_t g = threadIdx.x % LANES;
    for (uint32_t k = threadIdx.x / LANES; k < nfit; k += kTile / LANES) {
        const uint4 d = desc[k];
        const uint32_t* src = reinterpret_cast<const uint32_t*>(q.bytes) + d.x;
        uint32_t* dst = reinterpret_cast<uint32_t*>(q.out + ((uint64_t)d.w << 32 | d.z));
        const uint32_t rec_dw = egress::record_size(d.y) / 4;
        for (uint32_t j = g; j < rec_dw; j += LANES) dst[j] = record_word(src, d.y, j);
    }
}

template <uint32_t KIND>
__global__ void __launch_bounds__(kTile) egress_scatter_kernel(const EgressParams q) {
    __shared__ unsigned long long s_any;  // the ports any frame of the tile goes to
    // of the port in hand; two sets, so that a port's writes do not wait for the last port's reads
    __shared__ uint32_t s_wcnt[2][kTile / 64], s_wbytes[2][kTile / 64], s_nfit[2], s_fit_end[2];
    __shared__ uint4 s_desc[2][kTile];  // source dword offset, len, destination byte offset (lo, hi)
    __shared__ unsigned long long s_base_b[HALO_EGRESS_MAX_PORTS];  // the tile's bases, one load per tile and port
    __shared__ uint32_t s_base_r[HALO_EGRESS_MAX_PORTS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t par = 0;
    for (uint32_t tile = blockIdx.x; tile < q.n_tiles; tile += gridDim.x) {
        if (threadIdx.x == 0) s_any = 0;
        __syncthreads();
        const uint32_t i = tile * kTile + threadIdx.x;
        uint32_t len;
        bool skip;
        const uint64_t m = frame_ports<KIND>(q, i, &len, &skip);
        const uint32_t rec = egress::record_size(len), off = m ? q.offsets_dw[i] : 0u;
        if (m) atomicOr(&s_any, (unsigned long long)m);
        __syncthreads();
        uint64_t any = s_any;
        if (threadIdx.x < HALO_EGRESS_MAX_PORTS && ((any >> threadIdx.x) & 1)) {  // read behind the loop's first barrier
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
            for (uint32_t w = 0; w < kTile / 64; ++w) {
                if (w < wave) rank += s_wcnt[par][w], excl += s_wbytes[par][w];
                tile_cnt += s_wcnt[par][w];
            }
            const uint64_t base_b = s_base_b[p];
            const uint32_t base_r = s_base_r[p];
            if (sel && base_r + rank < q.index_cap) q.index[(uint64_t)p * q.index_cap + base_r + rank] = i;
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
                copy_records<kLanesPerRec>(q, s_desc[par], nfit);
            else
                copy_records<64>(q, s_desc[par], nfit);
            par ^= 1;
        }
    }
}

uint32_t egress_blocks(uint64_t tiles) {
    const uint64_t kMax = 256ull * 8;  // 8 workgroups per CU
    return (uint32_t)(tiles > kMax ? kMax : (tiles ? tiles : 1));
}

template <uint32_t KIND>
void launch(const EgressParams& q, hipStream_t st) {
    const uint32_t grid = egress_blocks(q.n_tiles);
    egress_count_kernel<KIND><<<dim3(grid), dim3(kTile), 0, st>>>(q);
    egress_scan_kernel<<<dim3(q.n_ports), dim3(256), 0, st>>>(q);
    egress_scatter_kernel<KIND><<<dim3(grid), dim3(kTile), 0, st>>>(q);
}

int ops_run(const halo_egress_config_t* cfg, uint32_t kind, const uint8_t* d_bytes, const uint32_t* d_offsets_dw,
            const uint16_t* d_lens, uint32_t n, const void* d_selectors, uint64_t flood_mask, uint8_t* d_out,
            halo_egress_port_t* d_ports, uint32_t* d_index, uint32_t* d_skipped, void* d_workspace, halo_stream_t stream) {
    const int rc = check_device();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0)
        return hipMemsetAsync(d_ports, 0, cfg->n_ports * sizeof(halo_egress_port_t), st) == hipSuccess ? HALO_OK : HALO_E_HIP;
    EgressParams q{};
    q.bytes = d_bytes, q.offsets_dw = d_offsets_dw, q.lens = d_lens, q.sel = d_selectors;
    q.flood = flood_mask, q.valid = egress::port_bits(cfg->n_ports), q.region = cfg->region_bytes;
    q.n = n, q.n_tiles = (uint32_t)tiles_of(n, kTile), q.n_ports = cfg->n_ports, q.flags = cfg->flags;
    q.index_cap = d_index ? cfg->index_cap : 0u;
    q.out = d_out, q.ports = d_ports, q.index = d_index, q.skipped = d_skipped;
    const uint64_t cells = (uint64_t)q.n_tiles * q.n_ports;
    q.byte_base = static_cast<uint64_t*>(d_workspace);
    q.rank_base = reinterpret_cast<uint32_t*>(q.byte_base + cells);
    q.tile_bytes = q.rank_base + cells;
    if (kind == HALO_EGRESS_KIND_MASKS) launch<HALO_EGRESS_KIND_MASKS>(q, st);
    else if (kind == HALO_EGRESS_KIND_ARP) launch<HALO_EGRESS_KIND_ARP>(q, st);
    else launch<HALO_EGRESS_KIND_SWITCH>(q, st);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

const egress::DeviceOps kDeviceOps = {ops_run};

}  // namespace

namespace egress {
const DeviceOps* device_ops() { return &kDeviceOps; }
}  // namespace egress
}  // namespace halo
