// rx_deliver.hip — the device side of local delivery (include/halo_rx.h, "local delivery") on
// gfx950: from a parsed, device-resident ragged batch to one stream of delivery records (24-byte
// header, payload, zero padding) in frame order. rx_deliver_host.cc checks the arguments and holds
// the host loop; rx_deliver.h holds the decision and the layout arithmetic both share.
//
// Three launches, the shape of the egress step (tx_egress.hip) with one stream in place of a
// stream per port:
//   count    one lane per frame, one tile of kTile frames per workgroup: the decision from the
//            record (two 16-byte loads; the served-port word and the length only for a frame that
//            needs them), per wave a ballot per kind and a sum of record bytes, gathered in LDS;
//            the tile's record count, record bytes and packed UDP / TCP / skipped counts go to the
//            workspace. (One atomic per workgroup and counter into the summary was measured
//            first: the atomics of 4,096 workgroups on one address took 40 of the kernel's 52 us.)
//   scan     one workgroup: the streams' scan (stream_scan.h) over the tiles, u32 rank bases and
//            u64 byte bases together, and the sums of the packed counts; writes the whole summary,
//            so nothing has to be cleared first. With a cut, the written prefix is that of the
//            whole tiles before it, and the scatter adds the cut tile's own part.
//   scatter  a tile without deliveries, or wholly beyond the region and the index, ends at once.
//            Else the decision again, ranks from tile_votes / tile_rank, byte offsets from a wave
//            scan of record sizes plus the wave totals in LDS. The owning lane writes the header
//            (a 16-byte and an 8-byte store) and the index entry and leaves a descriptor in LDS; the
//            workgroup then copies the payloads, a group of lanes per record walking the record's
//            ALIGNED DESTINATION dwords: each is funnelled out of the two source dwords it spans
//            with v_alignbyte_b32 at shift payload_off & 3 — the upper one is not loaded when no
//            payload byte lies in it, so no load leaves the words that hold the payload — and the
//            last is masked to payload_len. kLanesShort lanes per record for tiles of short
//            payloads, a wave per record otherwise.
#include <hip/hip_runtime.h>

#include "halo_common.h"
#include "rx_deliver.h"
#include "stream_scan.h"

namespace halo {
namespace {

using deliver::kNone;
using deliver::kTile;
using deliver::Rec;

constexpr uint32_t kLanesShort = 8;       // lanes that copy one short payload together (a wave per long one)
constexpr uint32_t kShortPayloadDw = 16;  // "short": a tile whose payloads average this many dwords or fewer

static_assert(sizeof(halo_rx_result_t) == 32 && sizeof(halo_deliver_hdr_t) == 24 && sizeof(halo_deliver_summary_t) == 40 &&
                  sizeof(halo_deliver_index_t) == 8,
              "layouts the kernels index by hand");
static_assert(HALO_DELIVER_KIND_COUNT == 3, "UDP and TCP are counted, DHCP is the rest");

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));  // a record starts 4-byte aligned
typedef uint32_t u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));

struct DeliverParams {
    const uint8_t* bytes;
    const uint32_t* offsets_dw;
    const uint16_t* lens;
    const halo_rx_result_t* recs;
    const uint32_t* udp_ports;  // optional
    const uint32_t* tcp_ports;  // optional
    uint64_t region;
    uint32_t n, n_tiles, flags, nat_enable, index_cap;
    uint8_t* out;
    halo_deliver_summary_t* summary;
    uint2* index;
    // workspace, [tile]
    uint64_t* byte_base;   // scan: bytes of the records in earlier tiles
    uint32_t* rank_base;   // count: the tile's records; scan: the records in earlier tiles
    uint32_t* tile_bytes;  // count: the tile's record bytes
    uint32_t* tile_kinds;  // count: the tile's UDP, TCP and skipped counts (deliver::pack_kinds)
};

// Frame i's kind (kNone: not delivered) and record; *skip: selected, but the payload overruns the frame.
__device__ __forceinline__ uint32_t frame_kind(const DeliverParams& q, uint32_t i, Rec* r, bool* skip) {
    *skip = false;
    if (i >= q.n) return kNone;
    const uint4* p = reinterpret_cast<const uint4*>(q.recs) + 2ull * i;
    const uint4 lo = p[0], hi = p[1];
    *r = Rec{lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, hi.w};
    const uint32_t kind = deliver::kind_of(*r, q.udp_ports, q.tcp_ports, q.nat_enable != 0, q.flags);
    if (kind == kNone) return kNone;
    if (deliver::inside(*r, q.lens[i])) return kind;
    *skip = true;
    return kNone;
}

__global__ void __launch_bounds__(kTile) deliver_count_kernel(const DeliverParams q) {
    __shared__ uint32_t s_acc[5];  // records, record bytes, UDP, TCP, skipped
    if (threadIdx.x < 5) s_acc[threadIdx.x] = 0;
    __syncthreads();
    Rec r;
    bool skip;
    const uint32_t kind = frame_kind(q, blockIdx.x * kTile + threadIdx.x, &r, &skip);
    const uint64_t sel = __ballot(kind != kNone), skips = __ballot(skip);
    if (sel) {  // wave-uniform
        const uint32_t bytes = wave_sum(kind != kNone ? deliver::record_size(deliver::payload_len(r)) : 0u);
        const uint32_t udp = (uint32_t)__popcll(__ballot(kind == HALO_DELIVER_UDP));
        const uint32_t tcp = (uint32_t)__popcll(__ballot(kind == HALO_DELIVER_TCP));
        if ((threadIdx.x & 63u) == 0) {
            atomicAdd(&s_acc[0], (uint32_t)__popcll(sel));
            atomicAdd(&s_acc[1], bytes);
            if (udp) atomicAdd(&s_acc[2], udp);
            if (tcp) atomicAdd(&s_acc[3], tcp);
        }
    }
    if (skips && (threadIdx.x & 63u) == 0) atomicAdd(&s_acc[4], (uint32_t)__popcll(skips));
    __syncthreads();
    if (threadIdx.x == 0) {
        q.rank_base[blockIdx.x] = s_acc[0];
        q.tile_bytes[blockIdx.x] = s_acc[1];
        q.tile_kinds[blockIdx.x] = deliver::pack_kinds(s_acc[2], s_acc[3], s_acc[4]);
    }
}

// One workgroup: stream_scan.h's scan over the tiles, the packed per-kind counts summed on the way.
__global__ void __launch_bounds__(256) deliver_scan_kernel(const DeliverParams q) {
    __shared__ StreamScanLds s_scan;
    __shared__ uint32_t s_kind[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    StreamSummary* o = reinterpret_cast<StreamSummary*>(q.summary);
    uint32_t udp = 0, tcp = 0, skipped = 0;  // this lane's tiles only, until the end
    const StreamTotals all =
        scan_stream_tiles(s_scan, q.rank_base, q.tile_bytes, q.byte_base, q.n_tiles, q.region, o, [&](uint32_t t, bool in) {
            const uint32_t kinds = in ? q.tile_kinds[t] : 0u;
            udp += deliver::packed_udp(kinds), tcp += deliver::packed_tcp(kinds), skipped += deliver::packed_skipped(kinds);
        });
    // the per-kind totals: order-free sums, one reduction after the last pass
    udp = wave_sum(udp), tcp = wave_sum(tcp), skipped = wave_sum(skipped);
    __syncthreads();  // the last pass's readers of s_scan are done: its count slots serve again
    if (lane == 0) s_scan.c[0][wave] = udp, s_scan.c[1][wave] = tcp, s_kind[wave] = skipped;
    __syncthreads();
    if (threadIdx.x == 0) {
        udp = s_scan.c[0][0] + s_scan.c[0][1] + s_scan.c[0][2] + s_scan.c[0][3];
        tcp = s_scan.c[1][0] + s_scan.c[1][1] + s_scan.c[1][2] + s_scan.c[1][3];
        write_stream_totals(o, all, q.region);
        q.summary->kind_counts[HALO_DELIVER_UDP] = udp;
        q.summary->kind_counts[HALO_DELIVER_TCP] = tcp;
        q.summary->kind_counts[HALO_DELIVER_DHCP] = all.c - udp - tcp;
        q.summary->skipped = s_kind[0] + s_kind[1] + s_kind[2] + s_kind[3];
    }
}

// The tile's nfit described payloads, LANES lanes per record: a group takes one record and walks
// its destination dwords. desc: the frame's dword offset, payload_off | payload_len << 16, the
// payload's byte offset in the output.
template <uint32_t LANES>
__device__ __forceinline__ void copy_payloads(const DeliverParams& q, const uint4* desc, uint32_t nfit) {
    const uint32_t g = threadIdx.x % LANES;
    for (uint32_t k = threadIdx.x / LANES; k < nfit; k += kTile / LANES) {
        const uint4 d = desc[k];
        const uint32_t poff = d.y & 0xFFFFu, plen = d.y >> 16, n_dw = deliver::payload_dwords(plen);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(q.bytes) + ((uint64_t)d.x + (poff >> 2));
        uint32_t* dst = reinterpret_cast<uint32_t*>(q.out + d.z);
        for (uint32_t j = g; j < n_dw; j += LANES) {
            const uint32_t lo = src[j];
            const uint32_t hi = deliver::needs_upper(poff, plen, j) ? src[j + 1] : 0u;
            dst[j] = deliver::funnel(lo, hi, poff & 3u) & deliver::tail_mask(plen, j);
        }
    }
}

__global__ void __launch_bounds__(kTile) deliver_scatter_kernel(const DeliverParams q) {
    __shared__ uint32_t s_wbytes[kTile / 64], s_nfit, s_fit_end;
    __shared__ uint4 s_desc[kTile];
    const uint32_t tile = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (q.tile_bytes[tile] == 0) return;  // uniform over the workgroup: no delivery in this tile
    const uint64_t base_b = q.byte_base[tile];
    const uint32_t base_r = q.rank_base[tile];
    if (base_b > q.region && base_r >= q.index_cap) return;  // nothing of this tile is written
    if (threadIdx.x == 0) s_nfit = 0, s_fit_end = 0;  // read behind tile_votes' barrier
    const uint32_t i = tile * kTile + threadIdx.x;
    Rec r;
    bool skip;
    const uint32_t kind = frame_kind(q, i, &r, &skip);
    const bool sel = kind != kNone;
    const uint32_t size = sel ? deliver::record_size(deliver::payload_len(r)) : 0u;
    const uint32_t inc = wave_inclusive(size, lane);
    if (lane == 63) s_wbytes[wave] = inc;
    const uint64_t votes = tile_votes<kTile>(sel);
    const uint32_t rank = tile_rank<kTile>(votes, 0u);
    uint32_t excl = inc - size, tile_cnt = 0;
    for (uint32_t w = 0; w < kTile / 64; ++w) {
        if (w < wave) excl += s_wbytes[w];
        tile_cnt += tile_wave_counts<kTile>()[w];
    }
    const uint64_t at = base_b + excl;
    const bool fits = sel && at + size <= q.region;  // monotone: the fitting records are a prefix
    const uint64_t fb = __ballot(fits);
    if (fits) {  // region <= 2^32 - 16: `at` fits 32 bits
        uint32_t w[6];
        deliver::header_words(r, i, kind, w);
        *reinterpret_cast<u32x4_a4*>(q.out + at) = (u32x4_a4){w[0], w[1], w[2], w[3]};
        *reinterpret_cast<u32x2_a4*>(q.out + at + 16) = (u32x2_a4){w[4], w[5]};
        s_desc[rank] = make_uint4(q.offsets_dw[i], r.w5, (uint32_t)at + deliver::kHdrBytes, 0u);
    }
    if (sel && base_r + rank < q.index_cap) q.index[base_r + rank] = make_uint2(i, fits ? (uint32_t)at : 0xFFFFFFFFu);
    if (fb && lane == 63u - (uint32_t)__builtin_clzll(fb)) {  // the wave's last fitting record
        atomicAdd(&s_nfit, (uint32_t)__popcll(fb));
        atomicMax(&s_fit_end, excl + size);
    }
    __syncthreads();
    const uint32_t nfit = s_nfit, fit_end = s_fit_end;
    if (threadIdx.x == 0 && nfit < tile_cnt && base_b <= q.region) {  // the cut falls in this tile
        q.summary->records_written += nfit;
        q.summary->bytes_written += fit_end;
    }
    if (fit_end - nfit * deliver::kHdrBytes <= nfit * 4u * kShortPayloadDw)
        copy_payloads<kLanesShort>(q, s_desc, nfit);
    else
        copy_payloads<64>(q, s_desc, nfit);
}

int ops_run(const halo_deliver_config_t* cfg, const uint8_t* d_bytes, const uint32_t* d_offsets_dw, const uint16_t* d_lens,
            const halo_rx_result_t* d_records, uint32_t n, const halo_rx_netif_t* netif, const uint32_t* d_udp_ports,
            const uint32_t* d_tcp_ports, uint8_t* d_out, halo_deliver_summary_t* d_summary, halo_deliver_index_t* d_index,
            void* d_workspace, halo_stream_t stream) {
    const int rc = check_device();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0)
        return hipMemsetAsync(d_summary, 0, sizeof(halo_deliver_summary_t), st) == hipSuccess ? HALO_OK : HALO_E_HIP;
    DeliverParams q{};
    q.bytes = d_bytes, q.offsets_dw = d_offsets_dw, q.lens = d_lens, q.recs = d_records;
    q.udp_ports = d_udp_ports, q.tcp_ports = d_tcp_ports;
    q.region = cfg->region_bytes;
    q.n = n, q.n_tiles = (uint32_t)tiles_of(n, kTile), q.flags = cfg->flags, q.nat_enable = netif->nat_enable ? 1u : 0u;
    q.index_cap = d_index ? cfg->index_cap : 0u;
    q.out = d_out, q.summary = d_summary, q.index = reinterpret_cast<uint2*>(d_index);
    q.byte_base = static_cast<uint64_t*>(d_workspace);
    q.rank_base = reinterpret_cast<uint32_t*>(q.byte_base + q.n_tiles);
    q.tile_bytes = q.rank_base + q.n_tiles;
    q.tile_kinds = q.tile_bytes + q.n_tiles;
    hipLaunchKernelGGL(deliver_count_kernel, dim3(q.n_tiles), dim3(kTile), 0, st, q);
    hipLaunchKernelGGL(deliver_scan_kernel, dim3(1), dim3(256), 0, st, q);
    hipLaunchKernelGGL(deliver_scatter_kernel, dim3(q.n_tiles), dim3(kTile), 0, st, q);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

const deliver::DeviceOps kDeviceOps = {ops_run};

}  // namespace

namespace deliver {
const DeviceOps* device_ops() { return &kDeviceOps; }
}  // namespace deliver
}  // namespace halo
