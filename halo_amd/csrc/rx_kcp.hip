// rx_kcp.hip — the device side of KCP ingest (include/halo_rx.h, "KCP ingest") on gfx950: from a
// delivery stream in HBM to datagram records and segment descriptors whose structural checks and
// byte checks are done. rx_kcp_host.cc checks the arguments and holds the host loop; rx_kcp.h
// holds the walk, the record words and the CRC arithmetic both share.
//
// Launches, all on the caller's stream, the record count read on the device:
//   count   one lane per delivery index entry, a tile of kTile entries per workgroup: selection
//           from the record's header, ParseEnet or Input's HEADER-ONLY walk (H bytes per segment,
//           read as the aligned dwords that hold them and funnelled with v_alignbyte_b32); the
//           tile's datagram count and walked-segment count go to the workspace.
//   scan    one workgroup: tile_scan.h's scan over both counts; writes the whole summary (totals,
//           zeros elsewhere), so nothing has to be cleared first.
//   write   the walk again, now with the datagram's rank and first segment: the datagram record,
//           one 32-byte descriptor per walked segment (two 16-byte stores) and the header's hash
//           field into the workspace, while the datagram fits both capacities; per workgroup one
//           atomic per non-zero counter into the summary.
//   hash    CRC32: crc_kernel, a group of kCrcLanes lanes per PUSH descriptor, each lane a
//           contiguous kCrcChunk-byte chunk read as whole aligned dwords (rx_kcp.h says how chunks
//           combine; the group's code is kcp_crc_device.h's, shared with tx_kcp.hip). The chunk CRC is shift/xor arithmetic, 32 steps per dword, not LDS slice
//           tables: the lanes of a wave index a table with unrelated bytes, so a 64-bank LDS serves
//           such a wave-wide lookup in several conflict passes, four lookups per dword, and every
//           workgroup would first have to build 4 KiB of tables; the arithmetic needs no memory at
//           all (DESIGN.md §26 has its time against the copy floor; what bounds it was not measured).
//           XXH3: list_kernel writes a (byte offset, length) entry per descriptor slot — length 0
//           for a non-PUSH descriptor and for the slots from segs_written to seg_cap — then
//           flow_hash.hip's run kernel, unchanged and through its public entry
//           halo_xxh3_64_batch_device, hashes seg_cap strings, and flag_kernel compares. Padding
//           to seg_cap instead of a launch that reads the count from device memory keeps that
//           kernel and its launch as they are; a padded slot costs one hashSmall iteration of a
//           4-lane group (16 per 256-slot window and wave) and 20 workspace bytes written and read.
//   final   one lane per written datagram: the first failed check among its descriptors becomes
//           n_segs / ret = -4; ret, error and segment counters into the summary.
// Zero and disabled modes skip the hash launches: the write kernel already knows every check.
#include <hip/hip_runtime.h>

#include "halo_common.h"
#include "kcp_crc_device.h"
#include "rx_kcp.h"
#include "tile_scan.h"

namespace halo {
namespace {

using kcp::Dgram;
using kcp::Hdr;
using kcp::kTile;

static_assert(sizeof(halo_kcp_dgram_t) == 40 && sizeof(halo_kcp_seg_t) == 32 && sizeof(halo_kcp_summary_t) == 96 &&
                  sizeof(halo_kcp_config_t) == 16 && sizeof(halo_deliver_index_t) == 8 && sizeof(halo_deliver_hdr_t) == 24,
              "layouts the kernels index by hand");
static_assert(offsetof(halo_kcp_summary_t, bytes_hashed) == 56 && offsetof(halo_kcp_dgram_t, conv0) == 8 &&
                  offsetof(halo_kcp_seg_t, check) == 28 && offsetof(halo_kcp_dgram_t, n_segs) == 16,
              "layouts the kernels index by hand");

struct KcpParams {
    const uint32_t* stream;  // the delivery stream as dwords
    const halo_deliver_summary_t* dsum;
    const uint2* index;
    uint32_t index_cap, n_tiles, port, dgram_cap, seg_cap;
    int32_t mode;
    uint2* dgrams;  // 40-byte records as five 8-byte words
    uint4* segs;    // 32-byte records as two 16-byte words
    halo_kcp_summary_t* summary;
    // workspace
    uint32_t* tile_dg;  // [tile] count: the tile's datagrams; scan: the datagrams before the tile
    uint32_t* tile_sg;  // [tile] the same for walked segments
    uint64_t* hash;     // [seg_cap] XXH3-64 of the list's entries
    uint64_t* list_off; // [seg_cap]
    uint32_t* want;     // [seg_cap] the header's hash field
    uint32_t* list_len; // [seg_cap]
};

// A payload in the stream: little-endian u32 at any payload offset from the aligned dwords that
// hold its bytes (the upper one is loaded only when one of the four bytes lies in it).
struct DevBytes {
    const uint32_t* dw;
    uint32_t base;  // the payload's byte offset in the stream
    __device__ __forceinline__ uint32_t u32(uint32_t pos) const {
        const uint32_t a = base + pos, s = a & 3u;
        const uint32_t lo = dw[a >> 2], hi = s ? dw[(a >> 2) + 1] : 0u;
        return deliver::funnel(lo, hi, s);
    }
};

// Index entry k — Dgram.what: 0 not selected, 1 ignored, 2 a datagram, its payload at stream byte
// `base`; emit as kcp::walk's.
template <typename Emit>
__device__ __forceinline__ Dgram entry(const KcpParams& q, uint32_t k, uint32_t& base, Emit emit) {
    const uint32_t records = q.dsum->records;
    base = 0;
    if (k >= q.index_cap || k >= records) return Dgram{};
    const uint32_t off = q.index[k].y;
    if (off == kcp::kNotWritten) return Dgram{};
    const uint32_t* rec = q.stream + (off >> 2);  // a record starts 4-byte aligned
    const uint32_t w1 = rec[1];
    if (!kcp::selected(w1, rec[3], q.port)) return Dgram{};
    base = off + deliver::kHdrBytes;
    return kcp::classify(DevBytes{q.stream, base}, w1 >> 16, q.mode, emit);
}

__global__ void __launch_bounds__(kTile) kcp_count_kernel(const KcpParams q) {
    __shared__ uint32_t s_acc[2];
    if (threadIdx.x < 2) s_acc[threadIdx.x] = 0;
    __syncthreads();
    uint32_t base;
    const Dgram d = entry(q, blockIdx.x * kTile + threadIdx.x, base, [](uint32_t, const Hdr&, uint32_t) {});
    const bool sel = d.what == 2u;
    const uint64_t votes = __ballot(sel);
    if (votes) {  // wave-uniform
        const uint32_t lane = threadIdx.x & 63u;
        const uint32_t segs = wave_inclusive(sel ? d.n_walked : 0u, lane);
        if (lane == 63) {
            atomicAdd(&s_acc[0], (uint32_t)__popcll(votes));
            if (segs) atomicAdd(&s_acc[1], segs);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) q.tile_dg[blockIdx.x] = s_acc[0], q.tile_sg[blockIdx.x] = s_acc[1];
}

__global__ void __launch_bounds__(256) kcp_scan_kernel(const KcpParams q) {
    const uint32_t dgrams = scan_tiles(q.tile_dg, q.n_tiles);
    __syncthreads();  // scan_tiles' LDS serves the second scan
    const uint32_t segs = scan_tiles(q.tile_sg, q.n_tiles);
    uint32_t* s = reinterpret_cast<uint32_t*>(q.summary);
    if (threadIdx.x < sizeof(halo_kcp_summary_t) / 4) s[threadIdx.x] = threadIdx.x == 0 ? dgrams : threadIdx.x == 2 ? segs : 0u;
}

// the workgroup's counters: LDS adds, then one global atomic per non-zero counter
enum : uint32_t { kDgW, kSgW, kIgn, kEnet0, kInPkts = kEnet0 + 4, kInBytes, kHashed, kWriteCounters };

__global__ void __launch_bounds__(kTile) kcp_write_kernel(const KcpParams q) {
    __shared__ uint32_t s_wsegs[kTile / 64];
    __shared__ unsigned long long s_cnt[kWriteCounters];
    const uint32_t tile = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x < kWriteCounters) s_cnt[threadIdx.x] = 0;
    const uint32_t k = tile * kTile + threadIdx.x;
    uint32_t base;
    Dgram d = entry(q, k, base, [](uint32_t, const Hdr&, uint32_t) {});
    const uint32_t what = d.what;
    const DevBytes b{q.stream, base};
    const bool sel = what == 2u;
    const uint32_t nw = sel ? d.n_walked : 0u;
    const uint32_t inc = wave_inclusive(nw, lane);
    if (lane == 63) s_wsegs[wave] = inc;
    const uint64_t votes = tile_votes<kTile>(sel);  // the barrier: s_wsegs and s_cnt are set
    const uint32_t j = tile_rank<kTile>(votes, q.tile_dg[tile]);
    uint32_t first = q.tile_sg[tile] + inc - nw;
    for (uint32_t w = 0; w < wave; ++w) first += s_wsegs[w];
    // monotone in k: the datagrams that fit are a prefix
    const bool fits = sel && j < q.dgram_cap && (uint64_t)first + nw <= q.seg_cap;
    const uint64_t fb = __ballot(fits), ib = __ballot(what == 1u);
    if (ib && lane == 0) atomicAdd(&s_cnt[kIgn], (unsigned long long)__popcll(ib));
    if (fb) {  // wave-uniform
        uint32_t n_segs = nw;
        uint32_t hashed = 0;
        if (fits && d.kind == HALO_KCP_DGRAM_KCP) {
            kcp::walk(b, d.payload_len, kcp::overhead(q.mode), d.conv0_lo, d.conv0_hi, [&](uint32_t i, const Hdr& h, uint32_t pos) {
                const uint32_t chk = kcp::check_without_hash(q.mode, h);
                if (chk == HALO_KCP_SEG_CHECK_FAILED && i < n_segs) n_segs = i;
                if (kcp::hashes(q.mode)) {
                    q.want[first + i] = h.hash;
                    if (kcp::cmd_of(h) == kcp::kCmdPush) hashed += h.length;
                }
                uint32_t w[8];
                kcp::seg_words(h, j, b.base + pos, chk, w);
                q.segs[2ull * (first + i)] = make_uint4(w[0], w[1], w[2], w[3]);
                q.segs[2ull * (first + i) + 1] = make_uint4(w[4], w[5], w[6], w[7]);
            });
            if (n_segs < nw) d.ret = -4;  // zero mode; the final kernel counts it
        }
        if (fits) {
            uint32_t w[10];
            kcp::dgram_words(d, k, n_segs, first, w);
            uint2* o = q.dgrams + 5ull * j;
            for (uint32_t x = 0; x < 5; ++x) o[x] = make_uint2(w[2 * x], w[2 * x + 1]);
        }
        const bool is_kcp = fits && d.kind == HALO_KCP_DGRAM_KCP;
        const uint32_t segs_w = wave_inclusive(fits ? nw : 0u, lane), bytes_w = wave_inclusive(is_kcp ? d.payload_len : 0u, lane);
        const uint64_t hashed_w = wave_inclusive((uint64_t)hashed, lane);
        const uint64_t kb = __ballot(is_kcp);
        for (uint32_t t = 0; t < 4; ++t) {
            const uint64_t eb = __ballot(fits && d.kind == HALO_KCP_DGRAM_ENET && d.conn_type == t);
            if (eb && lane == 0) atomicAdd(&s_cnt[kEnet0 + t], (unsigned long long)__popcll(eb));
        }
        if (lane == 63) {
            atomicAdd(&s_cnt[kDgW], (unsigned long long)__popcll(fb));
            if (segs_w) atomicAdd(&s_cnt[kSgW], (unsigned long long)segs_w);
            if (kb) atomicAdd(&s_cnt[kInPkts], (unsigned long long)__popcll(kb));
            if (bytes_w) atomicAdd(&s_cnt[kInBytes], (unsigned long long)bytes_w);
            if (hashed_w) atomicAdd(&s_cnt[kHashed], (unsigned long long)hashed_w);
        }
    }
    __syncthreads();
    if (threadIdx.x < kWriteCounters && s_cnt[threadIdx.x]) {
        const unsigned long long v = s_cnt[threadIdx.x];
        halo_kcp_summary_t* s = q.summary;
        switch (threadIdx.x) {
            case kDgW: atomicAdd(&s->dgrams_written, (uint32_t)v); break;
            case kSgW: atomicAdd(&s->segs_written, (uint32_t)v); break;
            case kIgn: atomicAdd(&s->ignored, (uint32_t)v); break;
            case kInPkts: atomicAdd(reinterpret_cast<unsigned long long*>(&s->in_pkts), v); break;
            case kInBytes: atomicAdd(reinterpret_cast<unsigned long long*>(&s->in_bytes), v); break;
            case kHashed: atomicAdd(reinterpret_cast<unsigned long long*>(&s->bytes_hashed), v); break;
            default: atomicAdd(&s->enet_counts[threadIdx.x - kEnet0], (uint32_t)v); break;
        }
    }
}

constexpr uint32_t kHashBlock = 256;
// workgroups of a hash-step kernel that walks `items` slots, `per` lanes each, grid-stride
uint32_t hash_grid(uint64_t items, uint32_t per) {
    const uint64_t b = (items * per + kHashBlock - 1) / kHashBlock, cap = 256ull * 16;
    return (uint32_t)(b > cap ? cap : (b ? b : 1));
}

__global__ void __launch_bounds__(kHashBlock) kcp_crc_kernel(const KcpParams q) {
    const uint32_t written = q.summary->segs_written;
    const uint32_t g = threadIdx.x % kcp::kCrcLanes;
    const uint32_t per = kHashBlock / kcp::kCrcLanes;
    for (uint32_t s = blockIdx.x * per + threadIdx.x / kcp::kCrcLanes; s < written; s += gridDim.x * per) {  // group-uniform
        const uint4 lo = q.segs[2ull * s], hi = q.segs[2ull * s + 1];
        if ((lo.y & 0xFFu) != kcp::kCmdPush) continue;
        const uint32_t crc = crc_group(q.stream, hi.z, hi.y, g);
        if (g == 0)
            reinterpret_cast<uint32_t*>(q.segs)[8ull * s + 7] = crc == q.want[s] ? HALO_KCP_SEG_CHECK_PASSED : HALO_KCP_SEG_CHECK_FAILED;
    }
}

__global__ void __launch_bounds__(kHashBlock) kcp_list_kernel(const KcpParams q) {
    const uint32_t written = q.summary->segs_written;
    for (uint32_t s = blockIdx.x * kHashBlock + threadIdx.x; s < q.seg_cap; s += gridDim.x * kHashBlock) {
        uint32_t off = 0, len = 0;
        if (s < written) {
            const uint4 lo = q.segs[2ull * s], hi = q.segs[2ull * s + 1];
            if ((lo.y & 0xFFu) == kcp::kCmdPush) off = hi.z, len = hi.y;
        }
        q.list_off[s] = off, q.list_len[s] = len;
    }
}

__global__ void __launch_bounds__(kHashBlock) kcp_flag_kernel(const KcpParams q) {
    const uint32_t written = q.summary->segs_written;
    for (uint32_t s = blockIdx.x * kHashBlock + threadIdx.x; s < written; s += gridDim.x * kHashBlock) {
        uint32_t* seg = reinterpret_cast<uint32_t*>(q.segs) + 8ull * s;
        if ((seg[1] & 0xFFu) != kcp::kCmdPush) continue;
        seg[7] = (uint32_t)q.hash[s] == q.want[s] ? HALO_KCP_SEG_CHECK_PASSED : HALO_KCP_SEG_CHECK_FAILED;
    }
}

enum : uint32_t { kRet0, kInErrs = kRet0 + 5, kInSegs, kFinalCounters };

__global__ void __launch_bounds__(kHashBlock) kcp_final_kernel(const KcpParams q) {
    __shared__ unsigned long long s_cnt[kFinalCounters];
    if (threadIdx.x < kFinalCounters) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t written = q.summary->dgrams_written;
    for (uint32_t j = blockIdx.x * kHashBlock + threadIdx.x; j < written; j += gridDim.x * kHashBlock) {
        uint2* o = q.dgrams + 5ull * j;
        const uint32_t w1 = o[0].y;
        if ((w1 & 0xFFu) != HALO_KCP_DGRAM_KCP) continue;
        const uint2 w45 = o[2];
        const uint32_t nw = w45.x >> 16, first = w45.y;
        uint32_t n_segs = w45.x & 0xFFFFu;
        int ret = (int)(int8_t)(w1 >> 16);
        const uint32_t* chk = reinterpret_cast<const uint32_t*>(q.segs) + 8ull * first + 7;
        for (uint32_t i = 0; i < n_segs; ++i)
            if (chk[8ull * i] == HALO_KCP_SEG_CHECK_FAILED) n_segs = i;  // ends the loop
        if (n_segs < nw && ret != -4) {
            ret = -4;
            o[0].y = (w1 & 0xFF00FFFFu) | 0xFCu << 16;
            o[2].x = n_segs | nw << 16;
        }
        atomicAdd(&s_cnt[kRet0 + (uint32_t)-ret], 1ull);
        if (ret) atomicAdd(&s_cnt[kInErrs], 1ull);
        else if (n_segs) atomicAdd(&s_cnt[kInSegs], (unsigned long long)n_segs);
    }
    __syncthreads();
    if (threadIdx.x < kFinalCounters && s_cnt[threadIdx.x]) {
        const unsigned long long v = s_cnt[threadIdx.x];
        halo_kcp_summary_t* s = q.summary;
        if (threadIdx.x < kInErrs) atomicAdd(&s->ret_counts[threadIdx.x - kRet0], (uint32_t)v);
        else atomicAdd(reinterpret_cast<unsigned long long*>(threadIdx.x == kInErrs ? &s->in_errs : &s->in_segs), v);
    }
}

int ops_run(const halo_kcp_config_t* cfg, const uint8_t* d_stream, const halo_deliver_summary_t* d_deliver_summary,
            const halo_deliver_index_t* d_index, uint32_t index_cap, halo_kcp_dgram_t* d_dgrams, halo_kcp_seg_t* d_segs,
            halo_kcp_summary_t* d_summary, void* d_workspace, halo_stream_t stream) {
    const int rc = check_device();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (index_cap == 0)
        return hipMemsetAsync(d_summary, 0, sizeof(halo_kcp_summary_t), st) == hipSuccess ? HALO_OK : HALO_E_HIP;
    KcpParams q{};
    q.stream = reinterpret_cast<const uint32_t*>(d_stream), q.dsum = d_deliver_summary;
    q.index = reinterpret_cast<const uint2*>(d_index);
    q.index_cap = index_cap, q.n_tiles = (uint32_t)tiles_of(index_cap, kTile), q.port = cfg->port;
    q.dgram_cap = cfg->dgram_cap, q.seg_cap = cfg->seg_cap, q.mode = cfg->byte_check_mode;
    q.dgrams = reinterpret_cast<uint2*>(d_dgrams), q.segs = reinterpret_cast<uint4*>(d_segs), q.summary = d_summary;
    q.tile_dg = static_cast<uint32_t*>(d_workspace);
    q.tile_sg = q.tile_dg + q.n_tiles;
    q.hash = reinterpret_cast<uint64_t*>(q.tile_sg + q.n_tiles);
    q.list_off = q.hash + q.seg_cap;
    q.want = reinterpret_cast<uint32_t*>(q.list_off + q.seg_cap);
    q.list_len = q.want + q.seg_cap;
    hipLaunchKernelGGL(kcp_count_kernel, dim3(q.n_tiles), dim3(kTile), 0, st, q);
    hipLaunchKernelGGL(kcp_scan_kernel, dim3(1), dim3(256), 0, st, q);
    hipLaunchKernelGGL(kcp_write_kernel, dim3(q.n_tiles), dim3(kTile), 0, st, q);
    if (q.mode == HALO_KCP_CHECK_CRC32 && q.seg_cap) {
        hipLaunchKernelGGL(kcp_crc_kernel, dim3(hash_grid(q.seg_cap, kcp::kCrcLanes)), dim3(kHashBlock), 0, st, q);
    } else if (q.mode == HALO_KCP_CHECK_XXH3 && q.seg_cap) {
        hipLaunchKernelGGL(kcp_list_kernel, dim3(hash_grid(q.seg_cap, 1)), dim3(kHashBlock), 0, st, q);
        if (hipGetLastError() != hipSuccess) return HALO_E_HIP;
        const int hrc = halo_xxh3_64_batch_device(d_stream, q.list_off, q.list_len, q.seg_cap, q.hash, stream);
        if (hrc) return hrc;
        hipLaunchKernelGGL(kcp_flag_kernel, dim3(hash_grid(q.seg_cap, 1)), dim3(kHashBlock), 0, st, q);
    }
    if (q.dgram_cap) hipLaunchKernelGGL(kcp_final_kernel, dim3(hash_grid(q.dgram_cap, 1)), dim3(kHashBlock), 0, st, q);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

const kcp::DeviceOps kDeviceOps = {ops_run};

}  // namespace

namespace kcp {
const DeviceOps* device_ops() { return &kDeviceOps; }
}  // namespace kcp
}  // namespace halo
