// tx_kcp.h — KCP emit (include/halo_rx.h, "KCP emit"): what the host loop (tx_kcp_host.cc) and the
// kernels (tx_kcp.hip) must agree on — an entry's status, flush's packing rule as one walk over a
// session's descriptors, the words of a segment header, of BuildEnet's packet and of the two output
// records, which dwords of the stream a segment owns and what their bytes are, and the workspace
// layout. Plain C++17, no HIP: tx_kcp_host.cc compiles alone with g++ (tools/fuzz_kcp_emit.cc
// drives it under ASan/UBSan) and into libhalo_rx.so.
#pragma once
#include "rx_kcp.h"

namespace halo {
namespace kcp_emit {

constexpr uint32_t kTile = 256;         // entries per tile = lanes per workgroup of the count and place kernels
constexpr uint32_t kMaxMtu = 1472;      // BuildUdpPkt's payload limit (protocol/udp.go:55)
constexpr uint32_t kEncodeLanes = 16;   // lanes that encode one segment
constexpr uint32_t kEncodeBlock = 256;  // lanes per workgroup of the encode kernel

// halo_kcp_out_session_t as ten little-endian dwords: w5 = dst_port | mtu << 16, w6 = kind | conn_type << 8
struct Sess {
    uint32_t conv_lo, conv_hi, first_seg, n_segs, dst_ip, w5, w6, session_id, enet_conv, enet_type;
};
HALO_KCP_FN uint32_t mtu_of(const Sess& s) { return s.w5 >> 16; }
HALO_KCP_FN uint32_t kind_of(const Sess& s) { return s.w6 & 0xFFu; }
HALO_KCP_FN uint32_t conn_type_of(const Sess& s) { return (s.w6 >> 8) & 0xFFu; }

// The checks that need no descriptor. prev_end: the previous entry's first_seg + n_segs (0 for entry 0).
HALO_KCP_FN uint32_t entry_status(const Sess& s, uint64_t prev_end, uint32_t n_segs_total, uint32_t H) {
    if ((uint64_t)s.first_seg + s.n_segs > n_segs_total || s.first_seg < prev_end) return HALO_KCP_EMIT_BAD_RANGE;
    if (kind_of(s) == HALO_KCP_DGRAM_ENET)
        return conn_type_of(s) > HALO_KCP_ENET_PING || s.n_segs ? HALO_KCP_EMIT_BAD_RANGE : HALO_KCP_EMIT_OK;
    if (kind_of(s) != HALO_KCP_DGRAM_KCP) return HALO_KCP_EMIT_BAD_RANGE;  // neither kind
    return mtu_of(s) <= H || mtu_of(s) > kMaxMtu ? HALO_KCP_EMIT_BAD_MTU : HALO_KCP_EMIT_OK;
}

// What an entry puts out: datagrams, stream dwords (each datagram rounded up to 4 bytes), segments.
struct Shape {
    uint32_t status, dgrams, dwords, segs;
};
HALO_KCP_FN Shape enet_shape() { return Shape{HALO_KCP_EMIT_OK, 1u, kcp::kEnetBytes / 4u, 0u}; }

// flush's packing over a KCP session whose entry_status is OK. tail(i) gives descriptor first_seg +
// i's second half as {una, len, data_off, -}. on_seg(i, len, data_off, rel) is called per segment
// with the byte offset of its header from the session's first stream byte; on_dgram(j, rel, size,
// n, first_i) per datagram j as it closes: its offset (a multiple of 4), bytes, segment count and
// first segment. A failing segment ends the walk with its status: the callbacks made until then
// are the caller's to ignore (the count walk passes none, the write walk runs on OK sessions only).
struct Tail {
    uint32_t una, len, data_off, w7;
};
template <typename TailOf, typename OnSeg, typename OnDgram>
HALO_KCP_FN Shape walk(const Sess& s, uint32_t H, uint64_t payload_bytes, TailOf tail, OnSeg on_seg, OnDgram on_dgram) {
    const uint32_t mtu = mtu_of(s);
    uint32_t size = 0, dg = 0, dw = 0, first_i = 0;
    for (uint32_t i = 0; i < s.n_segs; ++i) {
        const Tail t = tail(i);
        if ((uint64_t)t.data_off + t.len > payload_bytes) return Shape{HALO_KCP_EMIT_BAD_RANGE, 0, 0, 0};
        if ((uint64_t)H + t.len > mtu) return Shape{HALO_KCP_EMIT_SEG_TOO_LONG, 0, 0, 0};
        const uint32_t need = H + t.len;
        if (size + need > mtu) {  // makeSpace: flushBuffer
            on_dgram(dg, 4u * dw, size, i - first_i, first_i);
            dw += (size + 3u) >> 2, ++dg, size = 0, first_i = i;
        }
        on_seg(i, t.len, t.data_off, 4u * dw + size);
        size += need;
    }
    if (size) {
        on_dgram(dg, 4u * dw, size, s.n_segs - first_i, first_i);
        dw += (size + 3u) >> 2, ++dg;
    }
    return Shape{HALO_KCP_EMIT_OK, dg, dw, s.n_segs};
}

// An OK entry with these sums of dgrams / dwords / segs before it is written?
HALO_KCP_FN bool fits(const Shape& x, uint32_t dg_base, uint32_t dw_base, uint32_t seg_base, uint32_t dgram_cap,
                      uint32_t stream_cap, uint32_t n_segs_total) {
    return (uint64_t)dg_base + x.dgrams <= dgram_cap && 4ull * ((uint64_t)dw_base + x.dwords) <= stream_cap &&
           (uint64_t)seg_base + x.segs <= n_segs_total;
}

// segment.encode's header as dwords (w1: the descriptor's cmd | frg << 8 | wnd << 16); hw[7] is the
// hash field, and the zero behind the header that a funnel over a 28-byte header's last word takes in
HALO_KCP_FN void header_words(uint32_t conv_lo, uint32_t conv_hi, uint32_t w1, uint32_t ts, uint32_t sn, uint32_t una,
                              uint32_t len, uint32_t hash, uint32_t hw[9]) {
    hw[0] = conv_lo, hw[1] = conv_hi, hw[2] = w1, hw[3] = ts, hw[4] = sn, hw[5] = una, hw[6] = len, hw[7] = hash, hw[8] = 0;
}

// BuildEnet's 20 bytes as five little-endian dwords
HALO_KCP_FN void enet_words(const Sess& s, uint32_t w[5]) {
    constexpr uint32_t head[4] = {0xFF000000u, 0x45010000u, 0x94010000u, 0x27020000u};
    constexpr uint32_t tail[4] = {0xFFFFFFFFu, 0x45455114u, 0x94944119u, 0x27277222u};
    const uint32_t t = conn_type_of(s) & 3u;
    w[0] = head[t], w[1] = __builtin_bswap32(s.session_id), w[2] = __builtin_bswap32(s.enet_conv);
    w[3] = __builtin_bswap32(s.enet_type), w[4] = tail[t];
}

// halo_kcp_out_dgram_t as four dwords, halo_tx_build_desc_t as ten
HALO_KCP_FN void dgram_words(uint32_t offset, uint32_t len, uint32_t n_segs, uint32_t session, uint32_t first_seg, uint32_t w[4]) {
    w[0] = offset, w[1] = len | n_segs << 16, w[2] = session, w[3] = first_seg;
}
HALO_KCP_FN void desc_words(uint32_t offset, uint32_t len, uint32_t src_ip, uint32_t src_port, const Sess& s, uint32_t w[10]) {
    w[0] = offset, w[1] = 0;                       // payload_off
    w[2] = len | 17u << 16;                        // payload_len, proto = UDP, aux 0
    w[3] = src_port | (s.w5 & 0xFFFFu) << 16;      // src_port, dst_port
    w[4] = src_ip, w[5] = s.dst_ip, w[6] = 0, w[7] = 0;  // seq, ack
    w[8] = 0, w[9] = HALO_TX_BUILD_ETH << 16;      // dst_mac, mode, pad
}

// A segment of n = H + len bytes whose header starts at stream byte D is the byte string S = header
// | data | fill, fill = the three bytes behind it: the next segment's first bytes when that one
// follows in the same datagram (the session's conv, low bytes first), zeros when the datagram ends
// (its padding). The segment OWNS the aligned stream dwords whose first byte is one of its n: dword
// j of them is S[r + 4j, r + 4j + 4), r = -D & 3, for r + 4j < n. Every dword of [0,
// bytes_written) has one owner this way; the bytes before a segment's first owned dword are its
// predecessor's fill.
HALO_KCP_FN uint32_t owned_first(uint32_t D) { return (0u - D) & 3u; }
HALO_KCP_FN uint32_t owned_dwords(uint32_t D, uint32_t n) { return (n - owned_first(D) + 3u) >> 2; }
// Byte p of S (p < n + 3); hword(q) is header dword q, data(i) data byte i
template <typename Hword, typename Data>
HALO_KCP_FN uint32_t s_byte(Hword hword, uint32_t H, uint32_t n, uint32_t fill, uint32_t p, Data data) {
    if (p < H) return hword(p >> 2) >> 8u * (p & 3u) & 0xFFu;
    if (p < n) return data(p - H);
    return fill >> 8u * (p - n) & 0xFFu;
}

// Workspace of a device call: per tile a u32 datagram, dword and segment count (the scan turns each
// into the sum before the tile); per entry the same three (the count kernel's walk, kept for the
// place kernel); then per OUTPUT segment slot the XXH3 list's u64 hash and u64 byte offset, its
// u32 length, the segment's index in the list, its entry, its header's stream offset and its
// CRC-32. A multiple of 8.
HALO_KCP_FN uint64_t workspace_head(uint32_t n_sessions) { return (12ull * tiles_of(n_sessions, kTile) + 12ull * n_sessions + 7) & ~7ull; }
HALO_KCP_FN uint64_t workspace_bytes(uint32_t n_sessions, uint32_t n_segs) {
    return workspace_head(n_sessions) + ((36ull * n_segs + 7) & ~7ull);
}

// The device side (tx_kcp.hip); tx_kcp_host.cc reaches it only through this, after it has checked
// every argument.
struct DeviceOps {
    int (*run)(const halo_kcp_emit_config_t* cfg, const halo_kcp_out_session_t* d_sessions, uint32_t n_sessions,
               const halo_kcp_seg_t* d_segs, uint32_t n_segs, const uint8_t* d_payload, uint64_t payload_bytes,
               uint8_t* d_stream, halo_kcp_out_dgram_t* d_dgrams, halo_tx_build_desc_t* d_descs, uint8_t* d_status,
               halo_kcp_emit_summary_t* d_summary, void* d_workspace, halo_stream_t stream);
};
// Defined by tx_kcp.hip; absent (null) in a host-only build, where the device call is HALO_E_NODEV.
const DeviceOps* device_ops() __attribute__((weak));

}  // namespace kcp_emit
}  // namespace halo
