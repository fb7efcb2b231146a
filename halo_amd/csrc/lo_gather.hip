// lo_gather.hip — the device side of the loopback gather (include/halo_rx.h, "loopback") on gfx950: a
// stable multi-way partition of a decided, device-resident ragged batch into one L3 batch per out
// NetIf, the packets a NetIf's LoChan receives in the order its sender sends them.
// lo_gather_host.cc checks the arguments and holds the host loop; lo_gather.h holds the selection
// and layout arithmetic both share.
//
// The egress step's three launches (tx_egress.hip), on stream_scan.h and tile_scan.h:
//   count    one workgroup per tile of kTile frames (grid-stride over tiles): the first word of the
//            ARP result and the length, in tx mode the frame dword with bytes 16-19; per NetIf the
//            tile's packet count and packet bytes through LDS atomics, one pair per wave when a
//            wave's packets all go to one NetIf.
//   scan     one workgroup per NetIf: scan_stream_tiles with the region cut; writes the summary.
//   scatter  recomputes the selection; per NetIf that any frame of the tile goes to: ballot + mbcnt
//            ranks and a wave scan of packet sizes, the tile's bases added. The owning lane writes
//            the three per-packet entries; every packet that fits leaves a descriptor in LDS and
//            the workgroup copies them, kLanesPerPkt lanes per short packet (a wave per long one).
// The copy: a frame starts on a dword and the packet 14 bytes in, so destination dword j is
// funnelled out of source dwords 3 + j and 4 + j at a fixed shift of 2 bytes (v_alignbyte_b32).
// The upper one is loaded only when a packet byte lies in it; the last destination dword is masked
// to pkt_len, so the zeros up to the 4-byte boundary come with it.
#include <hip/hip_runtime.h>

#include "halo_common.h"
#include "lo_gather.h"
#include "stream_scan.h"

namespace halo {
namespace {

using lo::kTile;
constexpr uint32_t kLanesPerPkt = 16;  // lanes that copy one short packet together (a wave per long one)
constexpr uint32_t kSmallPktDw = 32;   // "short": two dwords per lane cover the packet
constexpr uint32_t kNone = 0xFFFFFFFFu;

struct LoParams {
    const uint8_t* bytes;
    const uint32_t* offsets_dw;
    const uint16_t* lens;
    const uint32_t* results;  // halo_arp_result_t: two u32 per frame
    uint64_t region;
    uint32_t n, n_tiles, n_netifs, flags, index_cap;
    uint8_t* out;
    halo_egress_port_t* ports;
    uint32_t* pkt_off_dw;
    uint16_t* pkt_len;
    uint32_t* index;
    uint32_t* skipped;
    // workspace, [netif * n_tiles + tile]
    uint64_t* byte_base;   // scan: bytes of the NetIf's packets in earlier tiles
    uint32_t* rank_base;   // count: the tile's packets; scan: the packets in earlier tiles
    uint32_t* tile_bytes;  // count: the tile's packet bytes
};

// Frame i's NetIf (kNone: not selected, or not sendable), its packet length and its dword offset;
// *skip: selected but not sendable. Nothing of an unselected frame is loaded but its result word.
template <bool kTx>
__device__ __forceinline__ uint32_t frame_netif(const LoParams& q, uint32_t i, uint32_t* plen, uint32_t* off, bool* skip) {
    *plen = 0, *off = 0;
    *skip = false;
    if (i >= q.n) return kNone;
    const uint32_t p = lo::netif_of(q.results[2ull * i], q.n_netifs);
    if (p == kNone) return kNone;
    const uint32_t len = q.lens[i];
    bool ok;
    if (kTx) {
        ok = lo::tx_has_total_len(len);
        if (ok) {
            *off = q.offsets_dw[i];
            *plen = lo::tx_total_len(reinterpret_cast<const uint32_t*>(q.bytes)[(uint64_t)*off + 4]);
            ok = lo::tx_sendable(*plen, len);
        }
    } else {
        ok = lo::fwd_sendable(len, q.flags);
        if (ok) *off = q.offsets_dw[i], *plen = len - lo::kEthHeader;
    }
    if (ok) return p;
    *plen = 0;
    *skip = true;
    return kNone;
}

template <bool kTx>
__global__ void __launch_bounds__(kTile) lo_count_kernel(const LoParams q) {
    __shared__ uint32_t s_cnt[HALO_ARP_MAX_NETIFS], s_bytes[HALO_ARP_MAX_NETIFS];
    uint32_t skips = 0;  // wave-uniform
    for (uint32_t tile = blockIdx.x; tile < q.n_tiles; tile += gridDim.x) {
        if (threadIdx.x < HALO_ARP_MAX_NETIFS) s_cnt[threadIdx.x] = 0, s_bytes[threadIdx.x] = 0;
        __syncthreads();
        uint32_t plen, off;
        bool skip;
        const uint32_t p = frame_netif<kTx>(q, tile * kTile + threadIdx.x, &plen, &off, &skip);
        skips += (uint32_t)__popcll(__ballot(skip));
        const uint32_t size = p != kNone ? lo::packet_size(plen) : 0u;
        // A wave whose packets all go to one NetIf (the common case: one address is pinged) adds its
        // count and one wave sum of bytes from one lane; a wave of mixed NetIfs adds lane by lane.
        const uint64_t act = __ballot(p != kNone);
        if (act) {
            const uint32_t lead = __shfl(p, (int)__builtin_ctzll(act), 64);
            if (__ballot(p != kNone && p != lead) == 0) {
                const uint32_t bytes = wave_sum(size);
                if ((threadIdx.x & 63u) == 0) {
                    atomicAdd(&s_cnt[lead], (uint32_t)__popcll(act));
                    atomicAdd(&s_bytes[lead], bytes);
                }
            } else if (p != kNone) {
                atomicAdd(&s_cnt[p], 1u);
                atomicAdd(&s_bytes[p], size);
            }
        }
        __syncthreads();
        if (threadIdx.x < q.n_netifs) {  // the lanes that zero these slots for the next tile
            q.rank_base[(uint64_t)threadIdx.x * q.n_tiles + tile] = s_cnt[threadIdx.x];
            q.tile_bytes[(uint64_t)threadIdx.x * q.n_tiles + tile] = s_bytes[threadIdx.x];
        }
    }
    if ((threadIdx.x & 63u) == 0 && skips && q.skipped) atomicAdd(q.skipped, skips);
}

// One workgroup per NetIf: stream_scan.h's scan over the NetIf's tiles, then its totals.
__global__ void __launch_bounds__(256) lo_scan_kernel(const LoParams q) {
    __shared__ StreamScanLds s_scan;
    const uint64_t first = (uint64_t)blockIdx.x * q.n_tiles;
    StreamSummary* o = reinterpret_cast<StreamSummary*>(q.ports + blockIdx.x);
    const StreamTotals all = scan_stream_tiles(s_scan, q.rank_base + first, q.tile_bytes + first, q.byte_base + first, q.n_tiles,
                                             q.region, o, [](uint32_t, bool) {});
    if (threadIdx.x == 0) write_stream_totals(o, all, q.region);
}

// Dword j of the packet of plen bytes in the frame at src (j < packet_size(plen) / 4): frame bytes
// 14 + 4j .. 17 + 4j, the last dword masked to plen. The upper source dword holds frame bytes
// 16 + 4j and up: it is loaded only when the packet reaches it, so no load goes past the word that
// holds the packet's last byte.
__device__ __forceinline__ uint32_t packet_word(const uint32_t* __restrict__ src, uint32_t plen, uint32_t j) {
    const uint32_t lo_w = src[3 + j];
    const uint32_t hi_w = plen > 4 * j + 2 ? src[4 + j] : 0u;
    uint32_t w = __builtin_amdgcn_alignbyte(hi_w, lo_w, 2);
    const uint32_t rest = plen - 4 * j;  // >= 1
    if (rest < 4) w &= (1u << 8 * rest) - 1u;
    return w;
}

// The tile's nfit described packets, LANES lanes per packet: a group takes one packet and walks its
// aligned destination dwords.
template <uint32_t LANES>
__device__ __forceinline__ void copy_packets(const LoParams& q, const uint4* desc, uint32_t nfit) {
    const uint32_t g = threadIdx.x % LANES;
    for (uint32_t k = threadIdx.x / LANES; k < nfit; k += kTile / LANES) {
        const uint4 d = desc[k];
        const uint32_t* src = reinterpret_cast<const uint32_t*>(q.bytes) + d.x;
        uint32_t* dst = reinterpret_cast<uint32_t*>(q.out + ((uint64_t)d.w << 32 | d.z));
        const uint32_t dw = lo::packet_size(d.y) / 4;
        for (uint32_t j = g; j < dw; j += LANES) dst[j] = packet_word(src, d.y, j);
    }
}

template <bool kTx>
__global__ void __launch_bounds__(kTile) lo_scatter_kernel(const LoParams q) {
    __shared__ unsigned long long s_any;  // the NetIfs any frame of the tile goes to
    // of the NetIf in hand; two sets, so that a NetIf's writes do not wait for the last one's reads
    __shared__ uint32_t s_wcnt[2][kTile / 64], s_wbytes[2][kTile / 64], s_nfit[2], s_fit_end[2];
    __shared__ uint4 s_desc[2][kTile];  // source dword offset, pkt_len, destination byte offset (lo, hi)
    __shared__ unsigned long long s_base_b[HALO_ARP_MAX_NETIFS];  // the tile's bases, one load per tile and NetIf
    __shared__ uint32_t s_base_r[HALO_ARP_MAX_NETIFS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t par = 0;
    for (uint32_t tile = blockIdx.x; tile < q.n_tiles; tile += gridDim.x) {
        if (threadIdx.x == 0) s_any = 0;
        __syncthreads();
        const uint32_t i = tile * kTile + threadIdx.x;
        uint32_t plen, off;
        bool skip;
        const uint32_t mine = frame_netif<kTx>(q, i, &plen, &off, &skip);
        const uint32_t size = lo::packet_size(plen);
        if (mine != kNone) atomicOr(&s_any, 1ull << mine);
        __syncthreads();
        uint64_t any = s_any;
        if (threadIdx.x < HALO_ARP_MAX_NETIFS && ((any >> threadIdx.x) & 1)) {  // read behind the loop's first barrier
            s_base_b[threadIdx.x] = q.byte_base[(uint64_t)threadIdx.x * q.n_tiles + tile];
            s_base_r[threadIdx.x] = q.rank_base[(uint64_t)threadIdx.x * q.n_tiles + tile];
        }
        while (any) {  // uniform over the workgroup
            const uint32_t p = (uint32_t)__builtin_ctzll(any);
            any &= any - 1;
            const bool sel = mine == p;
            const uint64_t b = __ballot(sel);
            const uint32_t sz = sel ? size : 0u;
            const uint32_t inc = wave_inclusive(sz, lane);
            if (lane == 63) s_wcnt[par][wave] = (uint32_t)__popcll(b), s_wbytes[par][wave] = inc;
            if (threadIdx.x == 0) s_nfit[par] = 0, s_fit_end[par] = 0;
            __syncthreads();
            uint32_t rank = lanes_below(b), excl = inc - sz, tile_cnt = 0;
            for (uint32_t w = 0; w < kTile / 64; ++w) {
                if (w < wave) rank += s_wcnt[par][w], excl += s_wbytes[par][w];
                tile_cnt += s_wcnt[par][w];
            }
            const uint64_t base_b = s_base_b[p];
            const uint32_t base_r = s_base_r[p];
            const bool fits = sel && base_b + excl + sz <= q.region;  // monotone: the fitting packets are a prefix
            if (sel && base_r + rank < q.index_cap) {
                const uint64_t at = (uint64_t)p * q.index_cap + base_r + rank;
                q.pkt_off_dw[at] = fits ? (uint32_t)((base_b + excl) / 4) : lo::kNotWritten;
                q.pkt_len[at] = (uint16_t)plen;
                q.index[at] = i;
            }
            const uint64_t fb = __ballot(fits);
            if (fits) {
                const uint64_t dst = p * q.region + base_b + excl;
                s_desc[par][rank] = make_uint4(off, plen, (uint32_t)dst, (uint32_t)(dst >> 32));
            }
            if (fb && lane == 63u - (uint32_t)__builtin_clzll(fb)) {  // the wave's last fitting packet
                atomicAdd(&s_nfit[par], (uint32_t)__popcll(fb));
                atomicMax(&s_fit_end[par], excl + sz);
            }
            __syncthreads();
            const uint32_t nfit = s_nfit[par];
            if (threadIdx.x == 0 && nfit < tile_cnt && base_b <= q.region) {  // the cut falls in this tile
                q.ports[p].frames_written += nfit;
                q.ports[p].bytes_written += s_fit_end[par];
            }
            if (s_fit_end[par] <= nfit * 4u * kSmallPktDw)  // packets of 128 bytes on average, or less
                copy_packets<kLanesPerPkt>(q, s_desc[par], nfit);
            else
                copy_packets<64>(q, s_desc[par], nfit);
            par ^= 1;
        }
    }
}

uint32_t lo_blocks(uint64_t tiles) {
    const uint64_t kMax = 256ull * 8;  // 8 workgroups per CU
    return (uint32_t)(tiles > kMax ? kMax : (tiles ? tiles : 1));
}

template <bool kTx>
void launch(const LoParams& q, hipStream_t st) {
    const uint32_t grid = lo_blocks(q.n_tiles);
    lo_count_kernel<kTx><<<dim3(grid), dim3(kTile), 0, st>>>(q);
    lo_scan_kernel<<<dim3(q.n_netifs), dim3(256), 0, st>>>(q);
    lo_scatter_kernel<kTx><<<dim3(grid), dim3(kTile), 0, st>>>(q);
}

int ops_run(const halo_lo_config_t* cfg, const uint8_t* d_bytes, const uint32_t* d_offsets_dw, const uint16_t* d_lens,
            uint32_t n, const halo_arp_result_t* d_results, uint8_t* d_out, halo_egress_port_t* d_ports,
            uint32_t* d_pkt_off_dw, uint16_t* d_pkt_len, uint32_t* d_index, uint32_t* d_skipped, void* d_workspace,
            halo_stream_t stream) {
    const int rc = check_device();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0)
        return hipMemsetAsync(d_ports, 0, cfg->n_netifs * sizeof(halo_egress_port_t), st) == hipSuccess ? HALO_OK : HALO_E_HIP;
    LoParams q{};
    q.bytes = d_bytes, q.offsets_dw = d_offsets_dw, q.lens = d_lens, q.results = reinterpret_cast<const uint32_t*>(d_results);
    q.region = cfg->region_bytes;
    q.n = n, q.n_tiles = (uint32_t)tiles_of(n, kTile), q.n_netifs = cfg->n_netifs, q.flags = cfg->flags;
    q.index_cap = cfg->index_cap;
    q.out = d_out, q.ports = d_ports, q.pkt_off_dw = d_pkt_off_dw, q.pkt_len = d_pkt_len, q.index = d_index;
    q.skipped = d_skipped;
    const uint64_t cells = (uint64_t)q.n_tiles * q.n_netifs;
    q.byte_base = static_cast<uint64_t*>(d_workspace);
    q.rank_base = reinterpret_cast<uint32_t*>(q.byte_base + cells);
    q.tile_bytes = q.rank_base + cells;
    if (cfg->flags & HALO_LO_TX) launch<true>(q, st);
    else launch<false>(q, st);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

const lo::DeviceOps kDeviceOps = {ops_run};

}  // namespace

namespace lo {
const DeviceOps* device_ops() { return &kDeviceOps; }
}  // namespace lo
}  // namespace halo
