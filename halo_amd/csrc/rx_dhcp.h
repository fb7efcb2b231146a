// rx_dhcp.h — the DHCP service (include/halo_rx.h, "DHCP"): what the host twins (rx_dhcp_host.cc,
// tx_dhcp_host.cc) and the kernels (rx_dhcp.hip, tx_dhcp.hip) must agree on — RxDhcp's direction
// test, ParseDhcpPkt's two checks, ParseDhcpOption's loop with the places where the Go code would
// panic, the words of the 128-byte message record, the byte function of a built reply and its
// descriptor's words, and the workspace layout. Plain C++17, no HIP: the host files compile alone
// with g++ (tools/fuzz_dhcp.cc drives them under ASan/UBSan) and into libhalo_rx.so.
#pragma once
#include "rx_deliver.h"

#define HALO_DHCP_FN HALO_DELIVER_FN
#if defined(__HIPCC__)
#define HALO_DHCP_UNROLL _Pragma("unroll")
#else
#define HALO_DHCP_UNROLL
#endif

namespace halo {
namespace dhcp {

constexpr uint32_t kTile = 256;  // index entries per tile = lanes per workgroup of the count and write kernels
constexpr uint32_t kNotWritten = 0xFFFFFFFFu;
constexpr uint32_t kFixedBytes = 240;           // BOOTP header and the magic cookie
constexpr uint32_t kCookieLe = 0x63538263u;     // 63 82 53 63 as a little-endian dword
constexpr uint32_t kMsgWords = 32, kSummaryWords = 16;

// a delivery header's word 1: a DHCP record?
HALO_DHCP_FN bool selected(uint32_t w1) { return (w1 & 0xFFu) == HALO_DELIVER_DHCP; }

// RxDhcp's first test, from the header's word 3 = remote_port | local_port << 16
HALO_DHCP_FN uint32_t dir_of(uint32_t w3) {
    const uint32_t remote = w3 & 0xFFFFu, local = w3 >> 16;
    if (remote == 68u && local == 67u) return HALO_DHCP_TO_SERVER;
    if (remote == 67u && local == 68u) return HALO_DHCP_TO_CLIENT;
    return HALO_DHCP_DIR_NONE;
}

// ParseDhcpOption's loop (dhcp_engine.go:70-122) over the n = L - 240 bytes at payload offset 240
// behind `b`, which gives bytes pos .. pos + cnt - 1 (cnt 1..4) as a little-endian value:
// b.span(pos, cnt). The state is registers only: of every kept code the data's position and length
// (the last one wins: a plain overwrite), no array indexed by code.
struct Options {
    uint32_t panic;  // the Go code would panic
    uint32_t bits;   // HALO_DHCP_OPT_* of the codes seen (DNS / DNS_SHORT settled by the caller)
    uint32_t msg_type;
    uint32_t p1, l1, p3, l3, p6, l6, p12, l12, p50, l50;  // payload positions of the data, lengths
};
template <typename Bytes>
HALO_DHCP_FN Options walk(const Bytes& b, uint32_t L) {
    Options o{};
    const uint32_t n = L - kFixedBytes;
    uint32_t i = 0;
    for (;;) {
        if (i == n) {  // optionData[i]: index out of range (i never passes n: the overrun test below)
            o.panic = 1u;
            break;
        }
        const uint32_t code = b.span(kFixedBytes + i, 1);
        if (code == 0xFFu) break;
        if (i + 1u >= n) break;
        const uint32_t len = b.span(kFixedBytes + i + 1u, 1);
        if (i + 2u + len > n) break;
        const uint32_t p = kFixedBytes + i + 2u;
        if (code == 1u) o.bits |= HALO_DHCP_OPT_MASK, o.p1 = p, o.l1 = len;
        else if (code == 3u) o.bits |= HALO_DHCP_OPT_ROUTER, o.p3 = p, o.l3 = len;
        else if (code == 6u) o.bits |= HALO_DHCP_OPT_DNS, o.p6 = p, o.l6 = len;
        else if (code == 12u) o.bits |= HALO_DHCP_OPT_HOSTNAME, o.p12 = p, o.l12 = len;
        else if (code == 50u) o.bits |= HALO_DHCP_OPT_REQ_IP, o.p50 = p, o.l50 = len;
        else if (code == 53u) {
            if (len == 0u) {  // data[0] of an empty slice
                o.panic = 1u;
                break;
            }
            o.bits |= HALO_DHCP_OPT_MSG_TYPE, o.msg_type = b.span(p, 1);
        }
        i += 2u + len;
    }
    return o;
}

HALO_DHCP_FN uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }

// halo_dhcp_msg_t as 32 little-endian dwords, from the delivery header's words 1..3 (hw1 = kind |
// tcp_flags << 8 | payload_len << 16, hw2 = remote_ip, hw3 = the ports) and the payload behind b.
// Returns the status. Nothing of the payload is read for PORTS and SHORT; for COOKIE dword 59 only.
template <typename Bytes>
HALO_DHCP_FN uint32_t msg_words(const Bytes& b, uint32_t k, uint32_t hw1, uint32_t hw2, uint32_t hw3, uint32_t w[kMsgWords]) {
    const uint32_t L = hw1 >> 16, dir = dir_of(hw3);
    HALO_DHCP_UNROLL
    for (uint32_t x = 0; x < kMsgWords; ++x) w[x] = 0u;
    w[0] = k, w[6] = L << 16, w[7] = hw2;
    uint32_t status = HALO_DHCP_OK;
    if (dir == HALO_DHCP_DIR_NONE) status = HALO_DHCP_PORTS;
    else if (L < kFixedBytes) status = HALO_DHCP_SHORT;
    else if (b.span(236u, 4) != kCookieLe) status = HALO_DHCP_COOKIE;
    if (status != HALO_DHCP_OK) {
        w[1] = status | dir << 8;
        return status;
    }
    w[3] = b.span(4u, 4);
    w[4] = __builtin_bswap32(b.span(16u, 4));
    w[5] = b.span(28u, 4);
    w[6] |= b.span(32u, 2);
    const Options o = walk(b, L);
    if (o.panic) {
        w[1] = HALO_DHCP_REF_PANIC | dir << 8;
        return HALO_DHCP_REF_PANIC;
    }
    uint32_t bits = o.bits;
    w[1] = status | dir << 8 | o.msg_type << 16;
    if ((bits & HALO_DHCP_OPT_REQ_IP) && o.l50 == 4u) w[8] = __builtin_bswap32(b.span(o.p50, 4));
    uint32_t mask_n = 0, gw_n = 0;
    if (bits & HALO_DHCP_OPT_MASK) {
        mask_n = min_u32(o.l1, 4u);
        if (mask_n) w[9] = b.span(o.p1, mask_n);
    }
    if (bits & HALO_DHCP_OPT_ROUTER) {
        gw_n = min_u32(o.l3, 4u);
        if (gw_n) w[10] = b.span(o.p3, gw_n);
    }
    if (bits & HALO_DHCP_OPT_DNS) {
        if (o.l6 >= 4u) w[11] = b.span(o.p6, 4);
        else bits = (bits & ~HALO_DHCP_OPT_DNS) | HALO_DHCP_OPT_DNS_SHORT;  // build-defined: absent
    }
    w[12] = mask_n | gw_n << 8;
    w[2] = bits;
    if (bits & HALO_DHCP_OPT_HOSTNAME) {
        const uint32_t hn = min_u32(o.l12, 63u);
        HALO_DHCP_UNROLL
        for (uint32_t j = 0; j < 16u; ++j)
            if (4u * j < hn) w[16 + j] = b.span(o.p12 + 4u * j, min_u32(hn - 4u * j, 4u));
        w[31] |= hn << 24;  // byte 63; hn <= 63, so never a name byte
    }
    return status;
}

// the type_counts slot of an OK message
HALO_DHCP_FN uint32_t type_slot(uint32_t bits, uint32_t msg_type) {
    return (bits & HALO_DHCP_OPT_MSG_TYPE) && msg_type < HALO_DHCP_TYPE_COUNT ? msg_type : 0u;
}

// Workspace of a decode call: per tile a u32 count of DHCP records, which the scan turns into the
// count before the tile; rounded up to the 8-byte alignment.
HALO_DHCP_FN uint64_t workspace_bytes(uint32_t index_cap) { return (4ull * tiles_of(index_cap, kTile) + 7) & ~7ull; }

// ---- reply build ---------------------------------------------------------------------------------
constexpr uint32_t kSlot = HALO_DHCP_SLOT_BYTES, kSlotWords = kSlot / 4, kDescWords = 10;

// halo_dhcp_reply_t as the eight dwords a kernel loads, and the three addresses of the config
struct Reply {
    uint32_t w[8];
};
struct Addrs {
    uint32_t ip, mask, dns;
};
HALO_DHCP_FN uint32_t kind_of(const Reply& r) { return r.w[0] & 0xFFu; }
HALO_DHCP_FN bool server_kind(uint32_t kind) { return kind == HALO_DHCP_OFFER || kind == HALO_DHCP_ACK || kind == HALO_DHCP_NAK; }
// the message's length (BuildDhcpPkt's 240 bytes and BuildDhcpOption's, in the fixed order); 0: no such kind
HALO_DHCP_FN uint32_t reply_len(uint32_t kind) {
    switch (kind) {
        case HALO_DHCP_OFFER:
        case HALO_DHCP_ACK: return 286u;
        case HALO_DHCP_NAK: return 250u;
        case HALO_DHCP_REQUEST: return 270u;
        case HALO_DHCP_DISCOVER: return 258u;
        default: return 0u;
    }
}
HALO_DHCP_FN uint32_t be_byte(uint32_t v, uint32_t i) { return (v >> (24u - 8u * i)) & 0xFFu; }  // UToIpAddr(v)[i]
HALO_DHCP_FN uint32_t le_byte(uint32_t v, uint32_t i) { return (v >> (8u * i)) & 0xFFu; }
HALO_DHCP_FN uint32_t mac_byte(const Reply& r, uint32_t i) { return i < 4u ? le_byte(r.w[3], i) : le_byte(r.w[4], i - 4u); }
// a six-byte option {code, 4, value big-endian} at offset q of it
HALO_DHCP_FN uint32_t tlv4(uint32_t code, uint32_t v, uint32_t q) { return q == 0u ? code : q == 1u ? 4u : be_byte(v, q - 2u); }

// byte `pos` (< 288) of the slot of reply r
HALO_DHCP_FN uint32_t reply_byte(const Reply& r, const Addrs& a, uint32_t pos) {
    const uint32_t kind = kind_of(r), len = reply_len(kind);
    if (pos >= len) return 0u;
    if (pos < kFixedBytes) {  // BuildDhcpPkt (dhcp_engine.go:197-209)
        if (pos == 0u) return server_kind(kind) ? 2u : 1u;  // DhcpBootMsgTypeReply / Request
        if (pos == 1u) return 1u;
        if (pos == 2u) return 6u;
        if (pos >= 4u && pos < 8u) return le_byte(r.w[1], pos - 4u);
        if (pos == 10u) return 0x80u;
        if (pos >= 16u && pos < 20u) return be_byte(r.w[2], pos - 16u);
        if (pos >= 28u && pos < 34u) return mac_byte(r, pos - 28u);
        if (pos >= 236u) return le_byte(kCookieLe, pos - 236u);
        return 0u;
    }
    const uint32_t p = pos - kFixedBytes;
    if (pos + 1u == len) return 0xFFu;
    if (p < 3u) return p == 0u ? 53u : p == 1u ? 1u : kind;
    const uint32_t q = p - 3u;
    if (kind == HALO_DHCP_NAK) return tlv4(54u, a.ip, q);
    if (kind == HALO_DHCP_OFFER || kind == HALO_DHCP_ACK) {
        const uint32_t t = q / 6u, x = q % 6u;
        switch (t) {
            case 0: return tlv4(1u, a.mask, x);
            case 1: return tlv4(3u, a.ip, x);
            case 2: return tlv4(6u, a.dns, x);
            case 3: return tlv4(51u, 3600u, x);   // DhcpLeaseTime
            case 4: return tlv4(59u, 3150u, x);   // * 0.875
            case 5: return tlv4(58u, 1800u, x);   // * 0.5
            default: return tlv4(54u, a.ip, x);
        }
    }
    // REQUEST / DISCOVER: 61, 7, 1, the MAC; then REQUEST's 50 and 54; then 55, 3, 1, 3, 6
    if (q < 9u) return q == 0u ? 61u : q == 1u ? 7u : q == 2u ? 1u : mac_byte(r, q - 3u);
    uint32_t z = q - 9u;
    if (kind == HALO_DHCP_REQUEST) {
        if (z < 6u) return tlv4(50u, r.w[5], z);
        if (z < 12u) return tlv4(54u, r.w[6], z - 6u);
        z -= 12u;
    }
    return z == 0u ? 55u : z == 1u ? 3u : z == 2u ? 1u : z == 3u ? 3u : 6u;
}
HALO_DHCP_FN uint32_t reply_word(const Reply& r, const Addrs& a, uint32_t d) {
    return reply_byte(r, a, 4u * d) | reply_byte(r, a, 4u * d + 1u) << 8 | reply_byte(r, a, 4u * d + 2u) << 16 |
           reply_byte(r, a, 4u * d + 3u) << 24;
}
// halo_tx_build_desc_t of reply i as ten little-endian dwords
HALO_DHCP_FN void desc_words(const Reply& r, const Addrs& a, uint32_t i, uint32_t w[kDescWords]) {
    const uint32_t kind = kind_of(r), len = reply_len(kind);
    HALO_DHCP_UNROLL
    for (uint32_t x = 0; x < kDescWords; ++x) w[x] = 0u;
    if (!len) return;
    const uint64_t off = (uint64_t)i * kSlot;
    w[0] = (uint32_t)off, w[1] = (uint32_t)(off >> 32);
    w[2] = len | 17u << 16;  // payload_len, proto; aux 0
    w[3] = server_kind(kind) ? 67u | 68u << 16 : 68u | 67u << 16;
    w[4] = a.ip, w[5] = 0xFFFFFFFFu;
    w[8] = 0xFFFFFFFFu, w[9] = 0xFFFFu | HALO_TX_BUILD_ETH << 16;
}

// The device sides; the host files reach them only through these, after every argument is checked.
struct DeviceOps {
    int (*decode)(const uint8_t* d_stream, const halo_deliver_summary_t* d_deliver_summary, const halo_deliver_index_t* d_index,
                  uint32_t index_cap, halo_dhcp_msg_t* d_msgs, uint32_t msg_cap, halo_dhcp_summary_t* d_summary,
                  void* d_workspace, halo_stream_t stream);
};
struct BuildOps {
    int (*build)(const halo_dhcp_config_t* cfg, const halo_dhcp_reply_t* d_replies, uint32_t n, uint8_t* d_payload,
                 halo_tx_build_desc_t* d_descs, halo_stream_t stream);
};
// Defined by rx_dhcp.hip / tx_dhcp.hip; absent (null) in a host-only build, where the device calls
// are HALO_E_NODEV.
const DeviceOps* device_ops() __attribute__((weak));
const BuildOps* build_ops() __attribute__((weak));

}  // namespace dhcp
}  // namespace halo
