// tx_kcp.hip — the device side of KCP emit (include/halo_rx.h, "KCP emit") on gfx950: from a flush
// batch's entries and segment descriptors, with the data in HBM, to the stream of UDP payloads and
// the descriptors halo_tx_build_batch_device takes. tx_kcp_host.cc checks the arguments and holds
// the host loop; tx_kcp.h holds the status, the packing walk, the record words and the rule that
// gives every stream dword one writer.
//
// Launches, all on the caller's stream:
//   count   one lane per entry, a tile of kTile entries per workgroup: the entry's checks against
//           its predecessor and the segment list, then flush's packing over its descriptors' second
//           halves (one 16-byte load per segment). Status to d_status, the entry's datagram, dword
//           and segment counts to the workspace, the tile's sums beside them.
//   scan    one workgroup: tile_scan.h's scan over the three counts; writes the whole summary
//           (totals, zeros elsewhere), so nothing has to be cleared first.
//   place   the entry's bases from the tile's and a wave scan; while the entry fits, the walk again:
//           per datagram the 16-byte record and the 40-byte build descriptor, per segment its list
//           index, entry and header offset by OUTPUT rank (and the XXH3 list entry), an ENet packet
//           whole as five dwords; per workgroup one atomic per non-zero counter into the summary.
//   hash    over the SOURCE payload, so that every stream byte has one writer. CRC32: a group of
//           kCrcLanes lanes per written PUSH segment (kcp_crc_device.h, ingest's arithmetic). XXH3:
//           pad_kernel zeroes the list's lengths from segs_written to n_segs, then flow_hash.hip's
//           kernel through halo_xxh3_64_batch_device, unchanged. Zero and disabled modes: nothing.
//   encode  a group of kEncodeLanes lanes per written segment: each lane the stream dwords j, j +
//           kEncodeLanes, .. the segment owns (tx_kcp.h) — a header dword from two header words, a
//           data dword from the two aligned source dwords that hold it (v_alignbyte_b32), and the
//           at most two dwords that mix header, data and fill byte by byte.
#include <hip/hip_runtime.h>

#include "halo_common.h"
#include "kcp_crc_device.h"
#include "tile_scan.h"
#include "tx_kcp.h"

namespace halo {
namespace {

using kcp_emit::kTile;
using kcp_emit::Sess;
using kcp_emit::Shape;
using kcp_emit::Tail;

static_assert(sizeof(halo_kcp_out_session_t) == 40 && sizeof(halo_kcp_out_dgram_t) == 16 && sizeof(halo_kcp_seg_t) == 32 &&
                  sizeof(halo_kcp_emit_summary_t) == 88 && sizeof(halo_kcp_emit_config_t) == 24 &&
                  sizeof(halo_tx_build_desc_t) == 40,
              "layouts the kernels index by hand");
static_assert(offsetof(halo_kcp_out_session_t, first_seg) == 8 && offsetof(halo_kcp_out_session_t, mtu) == 22 &&
                  offsetof(halo_kcp_out_session_t, kind) == 24 && offsetof(halo_kcp_emit_summary_t, dgrams) == 8 &&
                  offsetof(halo_kcp_emit_summary_t, segs) == 16 && offsetof(halo_kcp_emit_summary_t, bytes) == 40 &&
                  offsetof(halo_tx_build_desc_t, mode) == 38 && offsetof(halo_kcp_seg_t, len) == 20,
              "layouts the kernels index by hand");

struct EmitParams {
    const uint2* sessions;    // 40-byte records as five 8-byte words
    const uint4* segs;        // 32-byte records as two 16-byte words
    const uint32_t* payload;  // as dwords
    uint64_t payload_bytes;
    uint32_t n_sessions, n_segs, n_tiles, dgram_cap, stream_cap, src_ip, src_port, H;
    int32_t mode;
    uint32_t* stream;  // as dwords
    uint4* dgrams;
    uint2* descs;
    uint8_t* status;
    halo_kcp_emit_summary_t* summary;
    // workspace
    uint32_t *tile_dg, *tile_dw, *tile_sg;  // [tile] count: the tile's sums; scan: the sums before the tile
    uint32_t *sess_dg, *sess_dw, *sess_sg;  // [entry] its Shape
    uint64_t* hash64;                       // [n_segs] by output rank: XXH3-64 of the list's entries
    uint64_t* list_off;
    uint32_t *list_len, *src, *sess, *dst, *crc;
};

__device__ __forceinline__ Sess load_sess(const EmitParams& q, uint32_t s) {
    const uint2* p = q.sessions + 5ull * s;
    const uint2 a = p[0], b = p[1], c = p[2], d = p[3], e = p[4];
    return Sess{a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y, e.x, e.y};
}
__device__ __forceinline__ Tail load_tail(const EmitParams& q, uint32_t i) {
    const uint4 t = q.segs[2ull * i + 1];
    return Tail{t.x, t.y, t.z, t.w};
}

__global__ void __launch_bounds__(kTile) emit_count_kernel(const EmitParams q) {
    __shared__ uint32_t s_acc[3];
    if (threadIdx.x < 3) s_acc[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t s = blockIdx.x * kTile + threadIdx.x, lane = threadIdx.x & 63u;
    Shape sh{HALO_KCP_EMIT_BAD_RANGE, 0, 0, 0};
    if (s < q.n_sessions) {
        const Sess x = load_sess(q, s);
        uint64_t prev_end = 0;
        if (s) {
            const uint2 r = q.sessions[5ull * (s - 1) + 1];  // first_seg, n_segs
            prev_end = (uint64_t)r.x + r.y;
        }
        sh.status = kcp_emit::entry_status(x, prev_end, q.n_segs, q.H);
        if (sh.status == HALO_KCP_EMIT_OK)
            sh = kcp_emit::kind_of(x) == HALO_KCP_DGRAM_ENET
                     ? kcp_emit::enet_shape()
                     : kcp_emit::walk(x, q.H, q.payload_bytes, [&](uint32_t i) { return load_tail(q, x.first_seg + i); },
                                      [](uint32_t, uint32_t, uint32_t, uint32_t) {},
                                      [](uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) {});
        q.status[s] = (uint8_t)sh.status;
        q.sess_dg[s] = sh.dgrams, q.sess_dw[s] = sh.dwords, q.sess_sg[s] = sh.segs;
    }
    const uint32_t dg = wave_inclusive(sh.dgrams, lane), dw = wave_inclusive(sh.dwords, lane), sg = wave_inclusive(sh.segs, lane);
    if (lane == 63) {
        if (dg) atomicAdd(&s_acc[0], dg);
        if (dw) atomicAdd(&s_acc[1], dw);
        if (sg) atomicAdd(&s_acc[2], sg);
    }
    __syncthreads();
    if (threadIdx.x == 0) q.tile_dg[blockIdx.x] = s_acc[0], q.tile_dw[blockIdx.x] = s_acc[1], q.tile_sg[blockIdx.x] = s_acc[2];
}

__global__ void __launch_bounds__(256) emit_scan_kernel(const EmitParams q) {
    const uint32_t dgrams = scan_tiles(q.tile_dg, q.n_tiles);
    __syncthreads();  // scan_tiles' LDS serves the next scan
    const uint32_t dwords = scan_tiles(q.tile_dw, q.n_tiles);
    __syncthreads();
    const uint32_t segs = scan_tiles(q.tile_sg, q.n_tiles);
    uint32_t* s = reinterpret_cast<uint32_t*>(q.summary);
    if (threadIdx.x < sizeof(halo_kcp_emit_summary_t) / 4) {
        const uint32_t t = threadIdx.x;  // dgrams, segs and the u64 bytes = 4 * dwords
        s[t] = t == 2 ? dgrams : t == 4 ? segs : t == 10 ? dwords << 2 : t == 11 ? dwords >> 30 : 0u;
    }
}

// the workgroup's counters: LDS adds, then one global atomic per non-zero counter
enum : uint32_t { kSess, kSessW, kDgW, kSgW, kSt0, kBytesW = kSt0 + 4, kHashed, kOutBytes, kPlaceCounters };

__global__ void __launch_bounds__(kTile) emit_place_kernel(const EmitParams q) {
    __shared__ uint32_t s_w[3][kTile / 64];
    __shared__ unsigned long long s_cnt[kPlaceCounters];
    const uint32_t tile = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x < kPlaceCounters) s_cnt[threadIdx.x] = 0;
    const uint32_t s = tile * kTile + threadIdx.x;
    const bool in = s < q.n_sessions;
    Shape sh{in ? (uint32_t)q.status[s] : HALO_KCP_EMIT_BAD_RANGE, 0, 0, 0};
    if (in) sh.dgrams = q.sess_dg[s], sh.dwords = q.sess_dw[s], sh.segs = q.sess_sg[s];  // zeros for a non-OK entry
    const uint32_t dgi = wave_inclusive(sh.dgrams, lane), dwi = wave_inclusive(sh.dwords, lane), sgi = wave_inclusive(sh.segs, lane);
    if (lane == 63) s_w[0][wave] = dgi, s_w[1][wave] = dwi, s_w[2][wave] = sgi;
    __syncthreads();  // s_w and s_cnt are set
    uint32_t dg_base = q.tile_dg[tile] + dgi - sh.dgrams, dw_base = q.tile_dw[tile] + dwi - sh.dwords;
    uint32_t seg_base = q.tile_sg[tile] + sgi - sh.segs;
    for (uint32_t w = 0; w < wave; ++w) dg_base += s_w[0][w], dw_base += s_w[1][w], seg_base += s_w[2][w];
    const bool ok = in && sh.status == HALO_KCP_EMIT_OK;
    const bool fit = ok && kcp_emit::fits(sh, dg_base, dw_base, seg_base, q.dgram_cap, q.stream_cap, q.n_segs);
    if (in) atomicAdd(&s_cnt[kSt0 + sh.status], 1ull);
    if (ok) atomicAdd(&s_cnt[kSess], 1ull);
    if (fit) {
        const Sess x = load_sess(q, s);
        const uint32_t base = 4u * dw_base;  // the entry's first stream byte
        uint32_t hashed = 0, out_bytes = 0;
        const auto put_records = [&](uint32_t j, uint32_t rel, uint32_t size, uint32_t n, uint32_t first_i) {
            uint32_t w[4], d[10];
            kcp_emit::dgram_words(base + rel, size, n, s, x.first_seg + first_i, w);
            kcp_emit::desc_words(base + rel, size, q.src_ip, q.src_port, x, d);
            q.dgrams[dg_base + j] = make_uint4(w[0], w[1], w[2], w[3]);
            uint2* o = q.descs + 5ull * (dg_base + j);
            for (uint32_t k = 0; k < 5; ++k) o[k] = make_uint2(d[2 * k], d[2 * k + 1]);
            out_bytes += size;
        };
        if (kcp_emit::kind_of(x) == HALO_KCP_DGRAM_ENET) {
            uint32_t w[5];
            kcp_emit::enet_words(x, w);
            for (uint32_t k = 0; k < 5; ++k) q.stream[(base >> 2) + k] = w[k];
            put_records(0, 0, kcp::kEnetBytes, 0, 0);
        } else {
            kcp_emit::walk(
                x, q.H, q.payload_bytes, [&](uint32_t i) { return load_tail(q, x.first_seg + i); },
                [&](uint32_t i, uint32_t len, uint32_t data_off, uint32_t rel) {
                    const uint32_t k = seg_base + i;
                    q.src[k] = x.first_seg + i, q.sess[k] = s, q.dst[k] = base + rel;
                    if (kcp::hashes(q.mode)) {
                        const bool push = (reinterpret_cast<const uint32_t*>(q.segs)[8ull * (x.first_seg + i) + 1] & 0xFFu) == kcp::kCmdPush;
                        if (push) hashed += len;
                        if (q.mode == HALO_KCP_CHECK_XXH3) q.list_off[k] = data_off, q.list_len[k] = push ? len : 0u;
                    }
                },
                put_records);
        }
        atomicAdd(&s_cnt[kSessW], 1ull);
        if (sh.dgrams) atomicAdd(&s_cnt[kDgW], (unsigned long long)sh.dgrams);
        if (sh.segs) atomicAdd(&s_cnt[kSgW], (unsigned long long)sh.segs);
        if (sh.dwords) atomicAdd(&s_cnt[kBytesW], 4ull * sh.dwords);
        if (hashed) atomicAdd(&s_cnt[kHashed], (unsigned long long)hashed);
        if (out_bytes) atomicAdd(&s_cnt[kOutBytes], (unsigned long long)out_bytes);
    }
    __syncthreads();
    if (threadIdx.x < kPlaceCounters && s_cnt[threadIdx.x]) {
        const unsigned long long v = s_cnt[threadIdx.x];
        halo_kcp_emit_summary_t* o = q.summary;
        const auto add64 = [](uint64_t* p, unsigned long long x) { atomicAdd(reinterpret_cast<unsigned long long*>(p), x); };
        switch (threadIdx.x) {
            case kSess: atomicAdd(&o->sessions, (uint32_t)v); break;
            case kSessW: atomicAdd(&o->sessions_written, (uint32_t)v); break;
            case kDgW: atomicAdd(&o->dgrams_written, (uint32_t)v), add64(&o->out_pkts, v); break;
            case kSgW: atomicAdd(&o->segs_written, (uint32_t)v), add64(&o->out_segs, v); break;
            case kBytesW: add64(&o->bytes_written, v); break;
            case kHashed: add64(&o->bytes_hashed, v); break;
            case kOutBytes: add64(&o->out_bytes, v); break;
            default: atomicAdd(&o->status_counts[threadIdx.x - kSt0], (uint32_t)v); break;
        }
    }
}

constexpr uint32_t kBlock = kcp_emit::kEncodeBlock;
// workgroups of a kernel that walks `items` slots, `per` lanes each, grid-stride
uint32_t slot_grid(uint64_t items, uint32_t per) {
    const uint64_t b = (items * per + kBlock - 1) / kBlock, cap = 256ull * 16;
    return (uint32_t)(b > cap ? cap : (b ? b : 1));
}

__global__ void __launch_bounds__(kBlock) emit_crc_kernel(const EmitParams q) {
    const uint32_t written = q.summary->segs_written;
    const uint32_t g = threadIdx.x % kcp::kCrcLanes, per = kBlock / kcp::kCrcLanes;
    for (uint32_t k = blockIdx.x * per + threadIdx.x / kcp::kCrcLanes; k < written; k += gridDim.x * per) {  // group-uniform
        const uint32_t i = q.src[k];
        if ((reinterpret_cast<const uint32_t*>(q.segs)[8ull * i + 1] & 0xFFu) != kcp::kCmdPush) continue;
        const uint4 hi = q.segs[2ull * i + 1];
        const uint32_t crc = crc_group(q.payload, hi.z, hi.y, g);
        if (g == 0) q.crc[k] = crc;
    }
}

__global__ void __launch_bounds__(kBlock) emit_pad_kernel(const EmitParams q) {
    const uint32_t written = q.summary->segs_written;
    for (uint32_t k = written + blockIdx.x * kBlock + threadIdx.x; k < q.n_segs; k += gridDim.x * kBlock)
        q.list_off[k] = 0, q.list_len[k] = 0;
}

// header dword i of nine held in registers: a select chain, so that no lane indexes an array
__device__ __forceinline__ uint32_t pick(const uint32_t hw[9], uint32_t i) {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 9; ++k) v = i == k ? hw[k] : v;
    return v;
}

__global__ void __launch_bounds__(kBlock) emit_encode_kernel(const EmitParams q) {
    const uint32_t written = q.summary->segs_written, H = q.H;
    const uint32_t g = threadIdx.x % kcp_emit::kEncodeLanes, per = kBlock / kcp_emit::kEncodeLanes;
    for (uint32_t k = blockIdx.x * per + threadIdx.x / kcp_emit::kEncodeLanes; k < written; k += gridDim.x * per) {
        const uint32_t i = q.src[k], D = q.dst[k];
        const uint4 lo = q.segs[2ull * i], hi = q.segs[2ull * i + 1];
        const uint2 conv = q.sessions[5ull * q.sess[k]];
        const uint32_t len = hi.y, a = hi.z, n = H + len, end = D + n;
        uint32_t hash = 0;
        if ((lo.y & 0xFFu) == kcp::kCmdPush && kcp::hashes(q.mode)) hash = q.mode == HALO_KCP_CHECK_CRC32 ? q.crc[k] : (uint32_t)q.hash64[k];
        uint32_t hw[9];
        kcp_emit::header_words(conv.x, conv.y, lo.y, lo.z, lo.w, hi.x, len, hash, hw);
        // the bytes behind the segment: the next header's when it follows at once (then it is of the
        // same datagram: a datagram starts 4-byte aligned, and `end` is asked only when it is not)
        uint32_t fill = 0;
        if ((end & 3u) && k + 1 < written && q.dst[k + 1] == end) fill = conv.x;
        const uint32_t r = kcp_emit::owned_first(D), cnt = kcp_emit::owned_dwords(D, n);
        for (uint32_t j = g; j < cnt; j += kcp_emit::kEncodeLanes) {
            const uint32_t o = r + 4u * j;
            uint32_t v;
            if (o + 4u <= H) {
                v = deliver::funnel(pick(hw, j), pick(hw, j + 1), r);
            } else if (o >= H && o + 4u <= n) {
                const uint32_t x = a + (o - H), sh = x & 3u;
                const uint32_t l = q.payload[x >> 2], u = sh ? q.payload[(x >> 2) + 1] : 0u;
                v = deliver::funnel(l, u, sh);
            } else {
                v = 0;
                for (uint32_t b = 0; b < 4; ++b)
                    v |= kcp_emit::s_byte([&](uint32_t w) { return pick(hw, w); }, H, n, fill, o + b,
                                          [&](uint32_t d) { return q.payload[(a + d) >> 2] >> 8u * ((a + d) & 3u) & 0xFFu; })
                         << 8u * b;
            }
            q.stream[(D + o) >> 2] = v;
        }
    }
}

int ops_run(const halo_kcp_emit_config_t* cfg, const halo_kcp_out_session_t* d_sessions, uint32_t n_sessions,
            const halo_kcp_seg_t* d_segs, uint32_t n_segs, const uint8_t* d_payload, uint64_t payload_bytes, uint8_t* d_stream,
            halo_kcp_out_dgram_t* d_dgrams, halo_tx_build_desc_t* d_descs, uint8_t* d_status, halo_kcp_emit_summary_t* d_summary,
            void* d_workspace, halo_stream_t stream) {
    const int rc = check_device();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_sessions == 0)
        return hipMemsetAsync(d_summary, 0, sizeof(halo_kcp_emit_summary_t), st) == hipSuccess ? HALO_OK : HALO_E_HIP;
    EmitParams q{};
    q.sessions = reinterpret_cast<const uint2*>(d_sessions), q.segs = reinterpret_cast<const uint4*>(d_segs);
    q.payload = reinterpret_cast<const uint32_t*>(d_payload), q.payload_bytes = payload_bytes;
    q.n_sessions = n_sessions, q.n_segs = n_segs, q.n_tiles = (uint32_t)tiles_of(n_sessions, kTile);
    q.dgram_cap = cfg->dgram_cap, q.stream_cap = cfg->stream_cap, q.src_ip = cfg->src_ip, q.src_port = cfg->src_port;
    q.mode = cfg->byte_check_mode, q.H = kcp::overhead(q.mode);
    q.stream = reinterpret_cast<uint32_t*>(d_stream), q.dgrams = reinterpret_cast<uint4*>(d_dgrams);
    q.descs = reinterpret_cast<uint2*>(d_descs), q.status = d_status, q.summary = d_summary;
    q.tile_dg = static_cast<uint32_t*>(d_workspace);
    q.tile_dw = q.tile_dg + q.n_tiles, q.tile_sg = q.tile_dw + q.n_tiles;
    q.sess_dg = q.tile_sg + q.n_tiles, q.sess_dw = q.sess_dg + n_sessions, q.sess_sg = q.sess_dw + n_sessions;
    q.hash64 = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(d_workspace) + kcp_emit::workspace_head(n_sessions));
    q.list_off = q.hash64 + n_segs;
    q.list_len = reinterpret_cast<uint32_t*>(q.list_off + n_segs);
    q.src = q.list_len + n_segs, q.sess = q.src + n_segs, q.dst = q.sess + n_segs, q.crc = q.dst + n_segs;
    hipLaunchKernelGGL(emit_count_kernel, dim3(q.n_tiles), dim3(kTile), 0, st, q);
    hipLaunchKernelGGL(emit_scan_kernel, dim3(1), dim3(256), 0, st, q);
    hipLaunchKernelGGL(emit_place_kernel, dim3(q.n_tiles), dim3(kTile), 0, st, q);
    if (n_segs == 0) return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
    if (q.mode == HALO_KCP_CHECK_CRC32) {
        hipLaunchKernelGGL(emit_crc_kernel, dim3(slot_grid(n_segs, kcp::kCrcLanes)), dim3(kBlock), 0, st, q);
    } else if (q.mode == HALO_KCP_CHECK_XXH3) {
        hipLaunchKernelGGL(emit_pad_kernel, dim3(slot_grid(n_segs, 1)), dim3(kBlock), 0, st, q);
        if (hipGetLastError() != hipSuccess) return HALO_E_HIP;
        const int hrc = halo_xxh3_64_batch_device(d_payload, q.list_off, q.list_len, n_segs, q.hash64, stream);
        if (hrc) return hrc;
    }
    hipLaunchKernelGGL(emit_encode_kernel, dim3(slot_grid(n_segs, kcp_emit::kEncodeLanes)), dim3(kBlock), 0, st, q);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

const kcp_emit::DeviceOps kDeviceOps = {ops_run};

}  // namespace

namespace kcp_emit {
const DeviceOps* device_ops() { return &kDeviceOps; }
}  // namespace kcp_emit
}  // namespace halo
