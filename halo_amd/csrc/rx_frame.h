// rx_frame.h — the per-frame device code every rx kernel (rx_lane.hip, rx_group.hip, rx_stream.hip)
// is built from: the record store policies, the L4 segment sums, the header checks in reference
// order (parse_header / finish_l4; the functions restated are listed in rx_parse.hip), a frame's
// address and length per layout, and one frame's chain on a group of G lanes (FrameState,
// frame_loads / frame_header / frame_finish / frame_store, process_frame). Device-only; gfx950 only.
//
// Checksum arithmetic (DESIGN.md "Checksum in the little-endian domain"): the frame is summed
// as little-endian dwords. A one's-complement sum of byte-swapped 16-bit words is the byte
// swap of the sum (RFC 1071 §2B); swapping maps 0xFFFF to itself, and 2^16 == 1 (mod 0xFFFF),
// so "GetCheckSum(region) == 0" <=> fold16(sum of the LE dwords of the region) == 0xFFFF.
// Every region on the path starts at an even frame offset (14, 26, 34), so region edges fall
// on half-dwords and an odd trailing byte lands in the low byte of its half, which is the
// HIGH byte of its big-endian word: exactly protocol/utils.go:21-24.
#pragma once
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "flow_key.h"
#include "halo_common.h"
#include "route_view.h"
#include "rx_hist.h"

namespace halo {
namespace {

// NT: a non-temporal store. The byte-stream kernel's records take it: IMIX 1.272 -> 1.244 /
// 1.240 ms on one box (profiles/r06/r6c/ab_nt.log); tried: the lane kernel's too, 1M x 64 B
// 21.5 -> 22.2 us in the same A/B (§15.4), and every other record store (a measurement knob).
// WT: a write-through store at agent scope (global_store_dwordx4 ... sc1): the line goes through
// the XCD's L2 to memory at once, so the release at the end of the launch finds no dirty record
// lines to write back before the next dependent launch may start. Only for stores
// that write whole 128-byte lines from one wave instruction (64 lanes x 16 B), or every partial
// line would go to memory on its own. Five interleaved rounds each, kernel time, plain (or, for the
// stream kernel, non-temporal) stores against write-through ones (profiles/r07/; in git history up
// to 9ac2a89):
//   the two batch lane kernels (never the ring service kernel, whose hand-off to the host is its
//     own protocol): write-through. 1M x 64 B 22.28-22.70 -> 21.58-22.01 us,
//     4M 75.9-77.8 -> 75.1-75.9 us, 16M 281.9-285.1 -> 279.4-280.5 us; HBM writes per 1M launch
//     33,554,432 B before and after (no partial lines). kLaneLdsPad re-swept with it:
//     4096 gains 1 % at 1M and loses 1.3 % at 16M, 5120 equals 4608; 4608 stays.
//   the 32 B records of the group kernels and the mix kernel's group passes: plain. Tried:
//     1500 B 276.5-295.0 -> 275.3-293.5 us (overlap); jumbo 5760-5777 -> 5736-5759 us, 0.3 %,
//     the ranges 1.3 us apart: too small to call.
//   the byte-stream kernel: non-temporal. Tried: 570 B 115.7-119.7 -> 120.9-125.7 us,
//     IMIX 1178-1241 -> 1194-1263 us: slower.
enum : int { kStorePlain = 0, kStoreNt = 1, kStoreWt = 2 };
constexpr int kStoreLane = kStoreWt, kStoreGroup = kStorePlain, kStoreStream = kStoreNt;
template <int ST = kStorePlain>
__device__ __forceinline__ void store16(uint4* dst, uint4 v) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    if constexpr (ST == kStoreWt) {
        // The compiler does not count this store in vmcnt (it can only wait for more, never less)
        // and does not know the data registers are read after issue: the s_nop keeps the next
        // instructions from redefining them while the 16-byte store still reads them.
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1"
                     :
                     : "v"(dst), "v"((u32x4){v.x, v.y, v.z, v.w})
                     : "memory");
    } else if constexpr (ST == kStoreNt) {
        __builtin_nontemporal_store((u32x4){v.x, v.y, v.z, v.w}, reinterpret_cast<u32x4*>(dst));
    } else {
        *dst = v;
    }
}

// Byte offset of the IPv4 header in the buffer: 14 in an Ethernet frame, 0 for a LoChan packet
// (HALO_RX_L3_START). Both are even, so every region stays on half-dword boundaries.
template <bool L3>
constexpr uint32_t kIpOff = L3 ? 0u : 14u;

// Accumulate the L4-segment bytes [kIpOff + 20, seg_end) held in dwords [d0, d0+4).
template <bool L3>
__device__ __forceinline__ void acc_segment(const uint32_t (&w)[4], uint32_t d0, uint32_t seg_end, uint64_t& c) {
    constexpr uint32_t kSeg = kIpOff<L3> + 20u;  // 34 (dword 8, high half) or 20 (dword 5)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t d = d0 + j;
        const int32_t rel = (int32_t)seg_end - (int32_t)(4u * d);  // segment bytes left in this dword
        uint32_t keep = rel >= 4 ? 0xFFFFFFFFu : (rel <= 0 ? 0u : ((1u << (rel * 8)) - 1u));
        keep &= d >= (kSeg + 3u) / 4u ? 0xFFFFFFFFu : ((kSeg & 2u) && d == kSeg / 4u ? 0xFFFF0000u : 0u);
        c += (uint64_t)(w[j] & keep);
    }
}

// Lane-per-frame form of acc_segment (G = 1): the end mask from one clamped shift (v_med3 + a
// 64-bit shift) instead of two compares and selects, and each dword's two 16-bit halves added into
// a u32 with one v_dot2_u32_u16 instead of a 64-bit add. A halves sum keeps the value mod 0xFFFF
// (2^16 == 1) and is zero exactly when the masked bytes are, which is all fold16 looks at; it stays
// below 2^32 for any frame (<= 2254 dwords x 2 x 0xFFFF). e8 = 8 * seg_end.
// (Still a macro: deleting frame_finish's unreachable acc_segment branch reorders scalar moves in
// the LoChan lane kernels, and the knob retirement changed no kernel. DESIGN.md §24.)
#ifndef HALO_RX_LANE_DOT2
#define HALO_RX_LANE_DOT2 1
#endif
template <bool L3>
__device__ __forceinline__ void acc_segment_dot2(const uint32_t (&w)[4], uint32_t d0, int32_t e8, uint32_t& h) {
    constexpr uint32_t kSeg = kIpOff<L3> + 20u;
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const u16x2 one = {1, 1};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t d = d0 + j;
        const int32_t r8 = e8 - (int32_t)(32u * d);
        const int32_t sh = r8 < 0 ? 0 : (r8 > 32 ? 32 : r8);  // segment bits left in this dword
        uint32_t keep = (uint32_t)~(~0ull << sh);
        keep &= d >= (kSeg + 3u) / 4u ? 0xFFFFFFFFu : ((kSeg & 2u) && d == kSeg / 4u ? 0xFFFF0000u : 0u);
        h = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, w[j] & keep), one, h, false);
    }
}

// Group form (G > 1): the halves sum (v_dot2_u32_u16, as acc_segment_dot2) of the segment bytes in
// dwords [d0, d0+4). A chunk wholly inside the segment needs no mask, and whether every lane's chunk
// is is one wave-uniform test, so the common case costs four v_dot2 per chunk; only a wave whose
// chunk meets the segment's start or end (FIRST: round 0's header chunk) takes the masked path.
template <bool L3, bool FIRST = false>
__device__ __forceinline__ void acc_chunk(const uint32_t (&w)[4], uint32_t d0, uint32_t seg_end, uint32_t& hs) {
    constexpr uint32_t kSeg = kIpOff<L3> + 20u;
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const u16x2 one = {1, 1};
    const bool inside = 4u * d0 >= kSeg && 4u * d0 + 16u <= seg_end;
    if (!FIRST && __builtin_amdgcn_ballot_w64(!inside) == 0) {  // wave-uniform: no masks
#pragma unroll
        for (int j = 0; j < 4; ++j) hs = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, w[j]), one, hs, false);
        return;
    }
    acc_segment_dot2<L3>(w, d0, (int32_t)(8u * seg_end), hs);
}

struct Verdict {
    uint32_t status, flags, ethertype, ip_proto, ip_total_len, src_ip, dst_ip, sport, dport;
    uint32_t pay_off, pay_len, l4_aux, l4_seq, l4_ack;
    uint32_t seg_end;   // end of the L4 segment whose sum is needed (0: none)
    uint32_t l4_extra;  // pseudo-header + header-field part of the L4 sum, LE domain
    bool check_l4;      // L4 checksum decides the verdict after the reduction
};

#define HB(b) ((h[(b) >> 2] >> (((b)&3) * 8)) & 0xFFu)

// Frames failing ParseEthFrm's length check (or, for LoChan packets, ParseIpv4Pkt's) are never
// read: the reference looks at no byte of them.
template <bool L3>
__device__ __forceinline__ bool len_readable(uint32_t L, uint32_t flags) {
    const bool jumbo = (flags & HALO_RX_JUMBO_EXT) != 0;
    if constexpr (L3) return L >= 20u && L <= (jumbo ? kIpMaxJumbo : kIpMax);
    return L >= kEthMin && L <= (jumbo ? kEthMaxJumbo : kEthMax);
}

// Header checks, in reference order, up to (not including) the L4 checksum. h = buffer dwords
// 0..11: an Ethernet frame (IPv4 header at byte 14) or, with L3, a LoChan packet (at byte 0).
template <bool L3>
__device__ __forceinline__ Verdict parse_header(const uint32_t (&h)[12], uint32_t L, bool present,
                                                const RxParams& p) {
    constexpr uint32_t O = kIpOff<L3>;
    Verdict v;
    v.status = HALO_RX_OK; v.flags = 0; v.ethertype = kEthUnknown; v.ip_proto = kIpUnknown;
    v.ip_total_len = 0; v.src_ip = 0; v.dst_ip = 0; v.sport = 0; v.dport = 0;
    v.pay_off = 0; v.pay_len = 0; v.l4_aux = 0; v.l4_seq = 0; v.l4_ack = 0;
    v.seg_end = 0; v.l4_extra = 0; v.check_l4 = false;
    const bool jumbo = (p.flags & HALO_RX_JUMBO_EXT) != 0;
    const bool csum = (p.flags & HALO_RX_CSUM_ENABLE) != 0;
    const uint32_t ip_max = jumbo ? kIpMaxJumbo : kIpMax;
    const uint32_t l4_max = jumbo ? kL4MaxJumbo : kL4Max;

    uint32_t iplen;
    if constexpr (L3) {  // a LoChan packet: IPv4 only, no Ethernet layer (engine/engine.go:361)
        v.ethertype = kEthIpv4;
        iplen = L;
    } else {
        // ---- ParseEthFrm (protocol/ethernet.go:29-55)
        const uint32_t eth_max = jumbo ? kEthMaxJumbo : kEthMax;
        if (!present || L < kEthMin || L > eth_max) { v.status = HALO_RX_ETH_LEN; return v; }
        const uint32_t et = bswap16(h[3] & 0xFFFFu);
        if (et != kEthIeee8023 && et != kEthIpv4 && et != kEthArp && et != kEthIpv6) {
            v.status = HALO_RX_ETH_TYPE; return v;
        }
        v.ethertype = et;
        v.pay_off = 14; v.pay_len = L - 14;
        // RxEthernet's filter (engine/ethernet_engine.go:22)
        const uint32_t dm_lo = h[0], dm_hi = h[1] & 0xFFFFu;
        if ((dm_lo == p.mac_lo && dm_hi == p.mac_hi) || (dm_lo == 0xFFFFFFFFu && dm_hi == 0xFFFFu))
            v.flags |= HALO_RX_F_MAC_MATCH;
        if (et != kEthIpv4) return v;
        iplen = L - 14;
    }

    // ---- ParseIpv4Pkt (protocol/ipv4.go:48-86) on pkt = frm[14:L] (or the LoChan packet)
    if ((L3 && !present) || iplen < 20 || iplen > ip_max) { v.status = HALO_RX_IP_LEN; return v; }
    if (HB(O + 0) != 0x45u) { v.status = HALO_RX_IP_VER; return v; }
    if ((HB(O + 6) != 0x40u && HB(O + 6) != 0x00u) || HB(O + 7) != 0x00u) { v.status = HALO_RX_IP_FRAG; return v; }
    const uint32_t proto = HB(O + 9);
    if (proto != kIpIcmp && proto != kIpTcp && proto != kIpUdp) { v.status = HALO_RX_IP_PROTO; return v; }
    // pseudo-header src+dst (IP bytes 12..19), LE domain; sum_a = the rest of the IP header
    const uint32_t sum_b = L3 ? hsum(h[3]) + hsum(h[4]) : (h[6] >> 16) + hsum(h[7]) + (h[8] & 0xFFFFu);
    if (csum) {
        const uint32_t sum_a = L3 ? hsum(h[0]) + hsum(h[1]) + hsum(h[2])
                                  : (h[3] >> 16) + hsum(h[4]) + hsum(h[5]) + (h[6] & 0xFFFFu);
        if (fold16(sum_a + sum_b) != 0xFFFFu) { v.status = HALO_RX_IP_HDR_CKSUM; return v; }
    }
    const uint32_t total_len = L3 ? bswap16(h[0] >> 16) : bswap16(h[4] & 0xFFFFu);
    // pkt[20:totalLen] (protocol/ipv4.go:84): Go panics below 20 and reads stale bytes or
    // panics past len(pkt); both are reported as build-defined statuses.
    if (total_len < 20) { v.status = HALO_RX_IP_TOTLEN_UNDERFLOW; return v; }
    if (total_len > iplen) { v.status = HALO_RX_IP_TOTLEN_OVERRUN; return v; }
    v.ip_proto = proto;
    v.ip_total_len = total_len;
    v.src_ip = (HB(O + 12) << 24) | (HB(O + 13) << 16) | (HB(O + 14) << 8) | HB(O + 15);
    v.dst_ip = (HB(O + 16) << 24) | (HB(O + 17) << 16) | (HB(O + 18) << 8) | HB(O + 19);
    if (HB(O + 19) == 255u) v.flags |= HALO_RX_F_IP_BCAST;
    if (v.dst_ip == p.own_ip) v.flags |= HALO_RX_F_DST_IS_OWN;
    // NatGetSrcDstPort (protocol/ipv4.go:229-246) on the untrimmed packet: (0, 0) below 26 B,
    // which only a LoChan packet can be (an Ethernet frame's IPv4 part is >= 28 B)
    if (L3 && iplen < 26) {
        v.sport = v.dport = 0;
    } else if (proto == kIpIcmp) {
        v.sport = v.dport = (HB(O + 24) << 8) | HB(O + 25);
    } else {
        v.sport = (HB(O + 20) << 8) | HB(O + 21);
        v.dport = (HB(O + 22) << 8) | HB(O + 23);
    }
    v.pay_off = O + 20; v.pay_len = total_len - 20;

    // ---- L4 pre-checksum checks on pkt = ipPayload (len = totalLen - 20)
    const uint32_t l4len = total_len - 20;
    const uint32_t seg_end = total_len + O;
    if (proto == kIpUdp) {        // protocol/udp.go:21-49
        if (l4len < 8 || l4len > l4_max) { v.status = HALO_RX_L4_LEN; return v; }
        if (csum) {  // pseudo length = the UDP header's own length field (udp.go:30,38)
            v.check_l4 = true; v.seg_end = seg_end;
            v.l4_extra = sum_b + 0x1100u + (L3 ? h[6] & 0xFFFFu : h[9] >> 16);  // IP bytes 24..25
        }
    } else if (proto == kIpTcp) { // protocol/tcp.go:36-70
        if (l4len < 20 || l4len > l4_max) { v.status = HALO_RX_L4_LEN; return v; }
        if (csum) {  // pseudo length = len(pkt) (tcp.go:54-59)
            v.check_l4 = true; v.seg_end = seg_end;
            v.l4_extra = sum_b + 0x0600u + bswap16(l4len);
        }
    } else {                      // ICMP, protocol/icmp.go:33-63: checksum ALWAYS verified
        if (l4len < 8 || l4len > l4_max) { v.status = HALO_RX_L4_LEN; return v; }
        const uint32_t type = HB(O + 20);
        if (type != kIcmpRequest && type != kIcmpReply && type != kIcmpTtl) { v.status = HALO_RX_ICMP_TYPE; return v; }
        if (HB(O + 21) != 0u) { v.status = HALO_RX_ICMP_CODE; return v; }
        v.check_l4 = true; v.seg_end = seg_end; v.l4_extra = 0;
    }
    return v;
}

// L4 outputs once the whole chain succeeded.
template <bool L3>
__device__ __forceinline__ void finish_l4(const uint32_t (&h)[12], Verdict& v) {
    constexpr uint32_t S = kIpOff<L3> + 20u;  // L4 segment start
    const uint32_t l4len = v.ip_total_len - 20;
    if (v.ip_proto == kIpUdp) {
        v.pay_off = S + 8; v.pay_len = l4len - 8;                       // udp.go:47
    } else if (v.ip_proto == kIpTcp) {
        v.l4_aux = HB(S + 13);                                         // tcp.go:50
        v.l4_seq = (HB(S + 4) << 24) | (HB(S + 5) << 16) | (HB(S + 6) << 8) | HB(S + 7);
        v.l4_ack = (HB(S + 8) << 24) | (HB(S + 9) << 16) | (HB(S + 10) << 8) | HB(S + 11);
        const uint32_t hl = HB(S + 12) >> 4;                           // tcp.go:49 (words used as bytes)
        v.pay_off = S + hl; v.pay_len = l4len - hl;                    // tcp.go:68
    } else {
        v.l4_aux = HB(S);                                              // icmp.go:38
        v.l4_seq = (HB(S + 4) << 24) | (HB(S + 5) << 16) | (HB(S + 6) << 8) | HB(S + 7);
        v.pay_off = S + 8; v.pay_len = l4len - 8;                       // icmp.go:62
    }
}
#undef HB

// LAYOUT 0: ragged (u32 dword offsets + u16 lengths); 1: strided with per-frame lengths;
// 2: strided, one length; 3: ragged LoChan packets (HALO_RX_L3_START).
template <int LAYOUT>
constexpr bool kL3 = LAYOUT == 3;

template <int LAYOUT>
__device__ __forceinline__ void frame_at(const RxParams& p, uint64_t i, const uint8_t*& frame, uint32_t& L) {
    if constexpr (LAYOUT == 0 || LAYOUT == 3) {
        frame = p.bytes + ((uint64_t)p.offsets_dw[i] << 2);
        L = p.lens[i];
    } else if constexpr (LAYOUT == 1) {
        frame = p.bytes + i * p.stride;
        L = p.lens[i];
    } else {
        frame = p.bytes + i * p.stride;
        L = p.len;
    }
}

// 16-byte chunks per lane issued before the header is parsed (a lane-per-frame lane needs its
// first 64 bytes). Eight for groups would let a 570 B frame finish in one round trip, but costs
// ~55 VGPRs (occupancy 5 -> 3) and lost more than it gained (tried for the 8-lane kernel; in git
// history up to 9ac2a89).
constexpr int kRound0 = 4;
// Later-round loads of the widest groups (jumbo frames) are non-temporal: 9000 B frames 6.08-6.10
// -> 5.76 ms; for 1500 B on 8 lanes the same hint costs 12 % (290-296 -> 332 us), IMIX 2 %
// (profiles/r03/r3y/ab_nt.log: tried from 16 lanes / off / from 8 lanes, two rounds on one box; in
// git history up to 9ac2a89).
constexpr int kLaterNtG = 16;
constexpr uint32_t kGroupXcd = 8;  // runs of this many blocks per XCD in the 4- and 8-lane kernels
// One frame's state between "fetch" (addresses + round-0 loads issued) and "finish".
template <int G, int R0 = kRound0>
struct FrameState {
    static constexpr int kR0 = R0;
    const uint8_t* frame;
    uint32_t L, ndw;
    uint32_t buf[R0][4];  // round 0: chunks (u*G + gl) of 16 bytes
};

template <int LAYOUT, typename FS>
__device__ __forceinline__ void frame_meta(const RxParams& p, uint64_t i, bool present, FS& st) {
    st.frame = p.bytes;
    st.L = 0;
    if (present) frame_at<LAYOUT>(p, i, st.frame, st.L);
    st.ndw = (present && len_readable<kL3<LAYOUT>>(st.L, p.flags)) ? (st.L + 3) >> 2 : 0;
}

// Round 0: four 16-byte chunks per lane issued back to back, bounded by the frame length (the
// L4 end is not known before the header is parsed, and never exceeds the frame length).
template <int G, int R0>
__device__ __forceinline__ void frame_loads(uint32_t gl, FrameState<G, R0>& st) {
#pragma unroll
    for (int u = 0; u < R0; ++u) load4(st.frame, (u * G + gl) * 4, st.ndw, st.buf[u]);
}

// Header dwords 0..11 of the frame: the lane's own chunks (G = 1) or chunk 0 of group lanes 0..2.
template <int G, int R0>
__device__ __forceinline__ void frame_header(const FrameState<G, R0>& st, uint32_t grp_base, uint32_t (&h)[12]) {
    if constexpr (G == 1) {
#pragma unroll
        for (int j = 0; j < 12; ++j) h[j] = st.buf[j >> 2][j & 3];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            h[j] = group_bcast<G, 0>(st.buf[0][j], grp_base);
            h[4 + j] = group_bcast<G, 1>(st.buf[0][j], grp_base);
            h[8 + j] = group_bcast<G, 2>(st.buf[0][j], grp_base);
        }
    }
}

// Verdict after the L4 segment sum (this lane's or group's partial `c`), record store and count.
// `stage` (lane-per-frame only): write the record to this wave's LDS staging slot instead of
// global memory; the wave then stores its 64 consecutive records fully coalesced.
// FUSE (compile time, so the plain parse carries none of it): 1 = hash every record's NAT flow
// key (halo_rx_parse_flow_batch_device), 2 = FindRoute of every record's dst
// (halo_rx_parse_route_batch_device).
template <int G, int FUSE = 0, bool L3 = false>
__device__ __forceinline__ void frame_store(const RxParams& p, uint64_t i, bool present, uint32_t gl,
                                            const uint32_t (&h)[12], Verdict& v, uint64_t c, Hist& hist,
                                            uint4* stage = nullptr) {
    const uint32_t c32 = group_sum<G>(fold64(c));
    if (v.status == HALO_RX_OK && v.check_l4 && fold16(c32 + v.l4_extra) != 0xFFFFu) v.status = HALO_RX_L4_CKSUM;
    if (v.status == HALO_RX_OK && v.ip_proto != kIpUnknown) finish_l4<L3>(h, v);

    if (present && gl < 2) {
        uint4 lo, hi;
        lo.x = v.status | (v.flags << 8) | (v.ethertype << 16);
        lo.y = v.ip_proto | (v.l4_aux << 8) | (v.ip_total_len << 16);
        lo.z = v.src_ip;
        lo.w = v.dst_ip;
        hi.x = v.sport | (v.dport << 16);
        hi.y = v.pay_off | (v.pay_len << 16);
        hi.z = v.l4_seq;
        hi.w = v.l4_ack;
        if (p.flags & HALO_RX_RECORD_COMPACT) {  // halo_rx_record16_t
            if (gl == 0) {
                const uint32_t et_class = v.ethertype == kEthArp ? HALO_RX_F_ET_ARP
                                        : v.ethertype == kEthIpv6 ? HALO_RX_F_ET_IPV6
                                        : v.ethertype == kEthIeee8023 ? HALO_RX_F_ET_8023 : 0u;
                const uint4 r16 =
                    make_uint4(v.status | ((v.flags | et_class) << 8) | (v.ip_proto << 16) | (v.l4_aux << 24),
                               v.src_ip, v.dst_ip, hi.x);
                if constexpr (G == 1) {
                    if (stage) stage[0] = r16;
                    else reinterpret_cast<uint4*>(p.out)[i] = r16;
                } else {  // 16 B per group: 64 B rows at G = 16, never write-through
                    reinterpret_cast<uint4*>(p.out)[i] = r16;
                }
            }
        } else if (G == 1 && stage) {
            stage[0] = lo;
            stage[1] = hi;
        } else {
            uint4* rec = reinterpret_cast<uint4*>(p.out + i);
            if constexpr (G == 1) {
                rec[0] = lo;
                rec[1] = hi;
            } else {  // lane 0 writes bytes 0..15, lane 1 bytes 16..31 (per-component select: no scratch)
                const bool h1 = gl != 0;
                // a wave instruction writes 64/G consecutive records: rows of 128 B (G = 16) to 512 B
                const uint4 half = make_uint4(h1 ? hi.x : lo.x, h1 ? hi.y : lo.y, h1 ? hi.z : lo.z, h1 ? hi.w : lo.w);
                if constexpr (kStoreGroup == kStorePlain) rec[gl] = half;
                else store16<kStoreGroup>(rec + gl, half);
            }
        }
        if (gl == 0 && p.hist) hist.add(v.status);
        if (FUSE == 1 && gl == 0) {  // the flow key from the record's own fields (flow_key.h)
            const uint64_t fh = flowkey::nat_hash(lo.y & 0xFFu, lo.z, lo.w, hi.x & 0xFFFFu, hi.x >> 16,
                                                  p.flow_kind, p.flow_nat);
            p.flow_hash[i] = fh;
            if (p.flow_bucket) p.flow_bucket[i] = (uint32_t)(fh % p.flow_buckets);  // hashmap/hashmap.go:64
        }
        if (FUSE == 2 && gl == 0)  // FindRoute(dst) (route_view.h)
            p.route_out[i] = find_route(LpmView{p.rt_tbl24, p.rt_tbl8, p.rt_lists, p.rt_ids}, lo.w);
    }
}

// Everything after round 0 for frame i on a group of G lanes (G = 1: one lane, no cross-lane
// traffic). Every lane of a group calls it with the same i / present (other groups may be doing
// the same for other frames); `present` false means "no frame": nothing is read or written,
// but the group still executes the collective steps.
constexpr int kLaterChunks = 8;
template <int G, int FUSE = 0, int U = kLaterChunks, int R0 = kRound0, bool L3 = false>  // U: 16-byte chunks in flight per lane per later round
__device__ __forceinline__ void frame_finish(const RxParams& p, uint64_t i, bool present, uint32_t gl,
                                             uint32_t grp_base, FrameState<G, R0>& st, Hist& hist,
                                             uint4* stage = nullptr) {
    constexpr uint32_t STEP = 4 * G;  // dwords per group per load step
    constexpr int U0 = R0;            // chunks already loaded
    uint32_t h[12];
    frame_header(st, grp_base, h);
    uint64_t c = 0;
    uint32_t hs = 0;  // group kernels: halves sum of this lane's segment dwords
    if constexpr (G > 1) {
        // Round 0 is summed before the header checks run, so its buffers are dead during them (a
        // group kernel can then issue more of the frame in round 0). The segment end is the one
        // parse_header computes (IPv4 offset + totalLen) whenever the L4 sum decides the verdict;
        // for any other frame the sum is never read.
        const uint32_t tl = L3 ? bswap16(h[0] >> 16) : bswap16(h[4] & 0xFFFFu);
        acc_chunk<L3, true>(st.buf[0], gl * 4, kIpOff<L3> + tl, hs);
#pragma unroll
        for (int u = 1; u < U0; ++u) acc_chunk<L3>(st.buf[u], (u * G + gl) * 4, kIpOff<L3> + tl, hs);
    }
    Verdict v = parse_header<L3>(h, st.L, present, p);

    // L4 segment sum over [kIpOff + 20, seg_end): round 0 from registers, then U chunks per round
    if (v.seg_end && G == 1 && HALO_RX_LANE_DOT2) {
        uint32_t hs = 0;
        const int32_t e8 = (int32_t)(8u * v.seg_end);
#pragma unroll
        for (int u = 0; u < U0; ++u) acc_segment_dot2<L3>(st.buf[u], u * 4, e8, hs);
        const uint32_t seg_dw = (v.seg_end + 3) >> 2;
        for (uint32_t r0 = U0 * STEP; r0 < seg_dw; r0 += U * STEP) {
            uint32_t x[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u) load4(st.frame, r0 + u * 4, seg_dw, x[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) acc_segment_dot2<L3>(x[u], r0 + u * 4, e8, hs);
        }
        c = hs;
    } else if (v.seg_end && G == 1) {
#pragma unroll
        for (int u = 0; u < U0; ++u) acc_segment<L3>(st.buf[u], u * 4, v.seg_end, c);
        const uint32_t seg_dw = (v.seg_end + 3) >> 2;
        for (uint32_t r0 = U0 * STEP; r0 < seg_dw; r0 += U * STEP) {
            uint32_t x[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u) load4(st.frame, r0 + u * 4, seg_dw, x[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) acc_segment<L3>(x[u], r0 + u * 4, v.seg_end, c);
        }
    } else if constexpr (G > 1) {
        // later rounds: the group's loop bound is wave-uniform in practice (one length per batch),
        // and a group with no segment (or a frame not present) loads nothing
        const uint32_t seg_dw = v.seg_end ? (v.seg_end + 3) >> 2 : 0u;
        for (uint32_t r0 = U0 * STEP; r0 < seg_dw; r0 += U * STEP) {
            uint32_t x[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if constexpr (G >= kLaterNtG) load4_nt(st.frame, r0 + (u * G + gl) * 4, seg_dw, x[u]);
                else load4(st.frame, r0 + (u * G + gl) * 4, seg_dw, x[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) acc_chunk<L3>(x[u], r0 + (u * G + gl) * 4, v.seg_end, hs);
        }
        c = hs;
    }
    frame_store<G, FUSE, L3>(p, i, present, gl, h, v, c, hist, stage);
}

// The whole chain for frame i on a group of G lanes: R0 chunks per lane in round 0, U per later round.
template <int G, int LAYOUT, int FUSE, int R0, int U>
__device__ __forceinline__ void process_frame(const RxParams& p, uint64_t i, bool present, uint32_t gl,
                                              uint32_t grp_base, Hist& hist) {
    FrameState<G, R0> st;
    frame_meta<LAYOUT>(p, i, present, st);
    frame_loads(gl, st);
    frame_finish<G, FUSE, U, R0, kL3<LAYOUT>>(p, i, present, gl, grp_base, st, hist);
}

}  // namespace
}  // namespace halo
