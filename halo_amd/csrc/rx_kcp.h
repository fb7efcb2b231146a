// rx_kcp.h — KCP ingest (include/halo_rx.h, "KCP ingest"): what the host loop (rx_kcp_host.cc) and
// the kernels (rx_kcp.hip) must agree on — which delivery records are selected, ParseEnet's match,
// Input's header walk and its three structural checks, the words of the two output records, the
// CRC-32 arithmetic (bit steps, the multiplication mod the IEEE polynomial and the powers of x the
// lane groups combine their chunks with) and the workspace layout. Plain C++17, no HIP:
// rx_kcp_host.cc compiles alone with g++ (tools/fuzz_kcp.cc drives it under ASan/UBSan) and into
// libhalo_rx.so.
#pragma once
#include "rx_deliver.h"

#define HALO_KCP_FN HALO_DELIVER_FN

namespace halo {
namespace kcp {

constexpr uint32_t kTile = 256;  // index entries per tile = lanes per workgroup of the count and write kernels
constexpr uint32_t kNotWritten = 0xFFFFFFFFu;
constexpr uint32_t kCmdPush = 81, kCmdWins = 84;  // IKCP_CMD_PUSH .. IKCP_CMD_WINS (kcp.go:22-25)
constexpr uint32_t kEnetBytes = 20;

HALO_KCP_FN bool mode_ok(int32_t mode) { return mode >= HALO_KCP_CHECK_DISABLED && mode <= HALO_KCP_CHECK_XXH3; }
HALO_KCP_FN uint32_t overhead(int32_t mode) { return mode == HALO_KCP_CHECK_DISABLED ? 28u : 32u; }  // IKCP_OVERHEAD
HALO_KCP_FN bool hashes(int32_t mode) { return mode == HALO_KCP_CHECK_CRC32 || mode == HALO_KCP_CHECK_XXH3; }

// A delivery header's words 1 and 3 (rx_deliver.h, header_words): selected?
HALO_KCP_FN bool selected(uint32_t w1, uint32_t w3, uint32_t port) {
    return (w1 & 0xFFu) == HALO_DELIVER_UDP && (w3 >> 16) == port;
}

// ParseEnet (enet.go:100-145) from the payload's first and last little-endian dwords: the conn
// type, or 4 when no head / tail pair matches.
HALO_KCP_FN uint32_t enet_type_of(uint32_t head_le, uint32_t tail_le) {
    const uint32_t h = __builtin_bswap32(head_le), t = __builtin_bswap32(tail_le);
    if (h == 0x000000FFu && t == 0xFFFFFFFFu) return HALO_KCP_ENET_SYN;
    if (h == 0x00000145u && t == 0x14514545u) return HALO_KCP_ENET_EST;
    if (h == 0x00000194u && t == 0x19419494u) return HALO_KCP_ENET_FIN;
    if (h == 0x00000227u && t == 0x22722727u) return HALO_KCP_ENET_PING;
    return 4u;
}

// One segment header (kcp.go:630-641). w2 = cmd | frg << 8 | wnd << 16.
struct Hdr {
    uint32_t conv_lo, conv_hi, w2, ts, sn, una, length, hash;
};
HALO_KCP_FN uint32_t cmd_of(const Hdr& h) { return h.w2 & 0xFFu; }

// Input's loop (kcp.go:624-709) over a payload of L bytes behind `b`, which reads a little-endian
// u32 at any payload offset (b.u32(pos)); H = overhead(mode). emit(i, hdr, data_pos) is called for
// every segment that passes the conv, length and cmd checks. Returns the walked count and ret: 0,
// or the first failing check's -1 / -2 / -3.
struct Walked {
    uint32_t n;
    int ret;
};
template <typename Bytes, typename Emit>
HALO_KCP_FN Walked walk(const Bytes& b, uint32_t L, uint32_t H, uint32_t conv0_lo, uint32_t conv0_hi, Emit emit) {
    uint32_t pos = 0, n = 0;
    int ret = 0;
    while (L - pos >= H) {
        Hdr h;
        h.conv_lo = b.u32(pos), h.conv_hi = b.u32(pos + 4), h.w2 = b.u32(pos + 8), h.ts = b.u32(pos + 12);
        h.sn = b.u32(pos + 16), h.una = b.u32(pos + 20), h.length = b.u32(pos + 24);
        h.hash = H == 32u ? b.u32(pos + 28) : 0u;
        pos += H;
        if (h.conv_lo != conv0_lo || h.conv_hi != conv0_hi) { ret = -1; break; }
        if (h.length > L - pos) { ret = -2; break; }
        if (cmd_of(h) < kCmdPush || cmd_of(h) > kCmdWins) { ret = -3; break; }
        emit(n, h, pos);
        ++n;
        pos += h.length;
    }
    return Walked{n, ret};
}

// The check byte a segment gets without hashing: not applicable, or zero mode's comparison.
// CRC32 / XXH3 PUSH segments get theirs from the hash.
HALO_KCP_FN uint32_t check_without_hash(int32_t mode, const Hdr& h) {
    if (mode == HALO_KCP_CHECK_DISABLED || cmd_of(h) != kCmdPush) return HALO_KCP_SEG_CHECK_NA;
    if (mode == HALO_KCP_CHECK_ZERO) return h.hash == 0u ? HALO_KCP_SEG_CHECK_PASSED : HALO_KCP_SEG_CHECK_FAILED;
    return HALO_KCP_SEG_CHECK_NA;  // provisional: the hash step sets it
}

// halo_kcp_seg_t as eight little-endian dwords, halo_kcp_dgram_t as ten
HALO_KCP_FN void seg_words(const Hdr& h, uint32_t dgram, uint32_t data_off, uint32_t check, uint32_t w[8]) {
    w[0] = dgram, w[1] = h.w2, w[2] = h.ts, w[3] = h.sn, w[4] = h.una, w[5] = h.length, w[6] = data_off, w[7] = check;
}
struct Dgram {
    uint32_t what, kind, conn_type, n_walked, payload_len, conv0_lo, conv0_hi, session_id, conv, enet_type;
    int ret;
};
HALO_KCP_FN uint32_t dgram_w1(uint32_t kind, uint32_t conn_type, int ret) { return kind | conn_type << 8 | ((uint32_t)ret & 0xFFu) << 16; }
HALO_KCP_FN void dgram_words(const Dgram& d, uint32_t index, uint32_t n_segs, uint32_t first_seg, uint32_t w[10]) {
    w[0] = index, w[1] = dgram_w1(d.kind, d.conn_type, d.ret), w[2] = d.conv0_lo, w[3] = d.conv0_hi;
    w[4] = n_segs | d.n_walked << 16, w[5] = first_seg, w[6] = d.payload_len, w[7] = d.session_id, w[8] = d.conv, w[9] = d.enet_type;
}

// What a selected payload is — Dgram.what: 1 ignored, 2 a datagram record (the other fields
// filled). emit as walk's.
template <typename Bytes, typename Emit>
HALO_KCP_FN Dgram classify(const Bytes& b, uint32_t L, int32_t mode, Emit emit) {
    const uint32_t H = overhead(mode);
    Dgram d{};
    d.payload_len = L;
    d.what = 1u;
    if (L == kEnetBytes) {
        const uint32_t t = enet_type_of(b.u32(0), b.u32(16));
        if (t > HALO_KCP_ENET_PING) return d;
        d.kind = HALO_KCP_DGRAM_ENET, d.conn_type = t;
        d.conv0_lo = b.u32(4), d.conv0_hi = b.u32(8);  // rawConv
        d.session_id = __builtin_bswap32(d.conv0_lo), d.conv = __builtin_bswap32(d.conv0_hi);
        d.enet_type = __builtin_bswap32(b.u32(12));
        d.what = 2u;
        return d;
    }
    if (L < H) return d;
    d.kind = HALO_KCP_DGRAM_KCP;
    d.conv0_lo = b.u32(0), d.conv0_hi = b.u32(4);
    const Walked w = walk(b, L, H, d.conv0_lo, d.conv0_hi, emit);
    d.n_walked = w.n, d.ret = w.ret;
    d.what = 2u;
    return d;
}

// ---- CRC-32 (IEEE 802.3, reflected: bit 31 of a register is x^0) --------------------------------
constexpr uint32_t kCrcPoly = 0xEDB88320u;
// the register after `bits` more zero message bits (the message bits themselves are XORed in first)
HALO_KCP_FN constexpr uint32_t crc_steps(uint32_t c, uint32_t bits) {
    for (uint32_t i = 0; i < bits; ++i) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
    return c;
}
// a * b mod the polynomial (zlib's multmodp, without its early exit)
HALO_KCP_FN constexpr uint32_t crc_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t i = 0; i < 32; ++i) {
        p ^= b & (0u - ((a >> (31u - i)) & 1u));
        b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
    }
    return p;
}
// x^(2^k) mod the polynomial (zlib's x2n_table)
HALO_KCP_FN constexpr uint32_t crc_x2n(uint32_t k) {
    uint32_t p = 0x40000000u;  // x^1
    for (uint32_t i = 0; i < k; ++i) p = crc_mulmod(p, p);
    return p;
}
// A group of kCrcLanes lanes takes one segment: each lane a contiguous chunk of kCrcChunk bytes, the
// group kCrcStride bytes per pass. Chunks are aligned to the segment's END, so that only the first
// pass is partial and its missing bytes are leading zeros under a zero register, which leave it
// zero; the lane that holds the first data byte starts from 0xFFFFFFFF. A lane carries its value
// from pass to pass by multiplying with x^(8 * kCrcStride), and the group then folds the lanes'
// values pairwise with x^(8 * kCrcChunk * 2^level) — zlib's crc32_combine with fixed lengths, so
// every power is a compile-time constant.
constexpr uint32_t kCrcLanes = 16, kCrcChunk = 32, kCrcStride = kCrcLanes * kCrcChunk;
constexpr uint32_t kCrcLevels = 4;
static_assert(kCrcChunk == 32 && (1u << kCrcLevels) == kCrcLanes, "x^(8 * 32 * 2^l) = x2n(8 + l)");
constexpr uint32_t kCrcXStride = crc_x2n(8 + kCrcLevels);
HALO_KCP_FN constexpr uint32_t crc_xlevel(uint32_t level) { return crc_x2n(8 + level); }
HALO_KCP_FN uint32_t crc_passes(uint32_t len) { return (len + kCrcStride - 1) / kCrcStride; }
// Lane g's byte range [*b0, *b1) of the data in pass p of P; empty when *b1 <= *b0. *first: the
// range holds data byte 0.
HALO_KCP_FN void crc_lane_range(uint32_t len, uint32_t P, uint32_t p, uint32_t g, uint32_t* b0, uint32_t* b1, bool* first) {
    const int64_t lo = (int64_t)len - (int64_t)(P - p) * kCrcStride + (int64_t)g * kCrcChunk, hi = lo + kCrcChunk;
    *first = lo <= 0 && hi > 0;
    *b0 = lo > 0 ? (uint32_t)lo : 0u;
    *b1 = hi > 0 ? (uint32_t)hi : 0u;
}

// Workspace of a device call: per tile a u32 datagram count and a u32 walked-segment count (the
// scan turns both into the sums before the tile); then per segment slot the XXH3 list's u64 hash
// and u64 byte offset, the header's u32 hash field and the list's u32 length.
HALO_KCP_FN uint64_t workspace_bytes(uint32_t index_cap, uint32_t seg_cap) {
    return 8ull * tiles_of(index_cap, kTile) + 24ull * seg_cap;
}

// The device side (rx_kcp.hip); rx_kcp_host.cc reaches it only through this, after it has checked
// every argument.
struct DeviceOps {
    int (*run)(const halo_kcp_config_t* cfg, const uint8_t* d_stream, const halo_deliver_summary_t* d_deliver_summary,
               const halo_deliver_index_t* d_index, uint32_t index_cap, halo_kcp_dgram_t* d_dgrams, halo_kcp_seg_t* d_segs,
               halo_kcp_summary_t* d_summary, void* d_workspace, halo_stream_t stream);
};
// Defined by rx_kcp.hip; absent (null) in a host-only build, where the device call is HALO_E_NODEV.
const DeviceOps* device_ops() __attribute__((weak));

}  // namespace kcp
}  // namespace halo
