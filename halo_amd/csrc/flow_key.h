// flow_key.h — the NAT flow key of a parsed record and its XXH3-64, shared
// by the standalone flow-hash kernel (flow_hash.hip) and the rx kernels' fused pass (rx_frame.h,
// halo_rx_parse_flow_batch_device), so the two produce the same bits by construction.
//
//   key (13 bytes, little-endian): remote ip u32 | remote port u16 | local ip u32 | local port u16
//   | proto u8 — NatFlowHash / NatWanFlowHash (engine/ipv4_engine.go:451-479) as NatGetFlowByHash /
//   NatGetFlowByWan build them (:524-581); hashed by hashcode.GetHashCodeXXH3 (hashcode/xxh3.go,
//   hashSmall for 9..16 bytes, :62-66: default secret, seed 0).
//
// Host code (nat_table.cc, which places the device NAT table's entries) includes this header too,
// without HIP: the functions are then plain inline C++ and the 64x64 high multiply is a 128-bit one.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HALO_FLOWKEY_FN __host__ __device__ __forceinline__
#else
#define HALO_FLOWKEY_FN inline
#endif
#include <stdint.h>

#include "../../include/halo_rx.h"

namespace halo {
namespace flowkey {

// secret64(24) ^ secret64(32) and secret64(40) ^ secret64(48) of hashcode/xxh3.go:27-40
constexpr uint64_t kSecLo = 0x1f67b3b7a4a44072ull ^ 0x78e5c0cc4ee679cbull;
constexpr uint64_t kSecHi = 0x2172ffcc7dd05a82ull ^ 0x8e2443f7744608b8ull;

HALO_FLOWKEY_FN uint64_t mul_fold64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (a * b) ^ __umul64hi(a, b);
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    return (uint64_t)p ^ (uint64_t)(p >> 64);
#endif
}

// hashSmall for 9..16 bytes (xxh3.go:62-66) given the two overlapping 8-byte words
HALO_FLOWKEY_FN uint64_t hash_9to16(uint64_t w_lo, uint64_t w_hi, uint32_t len) {
    const uint64_t lo = w_lo ^ kSecLo, hi = w_hi ^ kSecHi;
    uint64_t v = (uint64_t)len + __builtin_bswap64(lo) + hi + mul_fold64(lo, hi);
    v ^= v >> 37;  // avalanche (xxh3.go:238-243)
    v *= 0x165667919e3779f9ull;
    return v ^ (v >> 32);
}

// The normalised flow key: the five fields of NatFlowHash / NatWanFlowHash (ports and proto widened).
struct Key {
    uint32_t rip, rport, lip, lport, proto;
};

// XXH3-64 of the 13-byte little-endian image of a key (GetHashCode, engine/ipv4_engine.go:451-479)
HALO_FLOWKEY_FN uint64_t key_hash(const Key& k) {
    const uint64_t w_lo = (uint64_t)k.rip | (uint64_t)k.rport << 32 | (uint64_t)(k.lip & 0xFFFFu) << 48;
    const uint64_t w_hi = (uint64_t)(k.rport >> 8) | (uint64_t)k.lip << 8 | (uint64_t)k.lport << 40 |
                          (uint64_t)k.proto << 56;  // key bytes 5..12
    return hash_9to16(w_lo, w_hi, 13);
}

// The flow key of a record (proto, IpAddrToU src/dst, ports as NatGetSrcDstPort gives them).
// kind: HALO_FLOW_NAT_LAN / HALO_FLOW_NAT_WAN; nat_type: HALO_NAT_SYMMETRIC or other.
HALO_FLOWKEY_FN Key nat_key(uint32_t proto, uint32_t src, uint32_t dst, uint32_t sport, uint32_t dport,
                            uint32_t kind, uint32_t nat_type) {
    const bool wan = kind == HALO_FLOW_NAT_WAN;
    // NatGetFlowByWan(src, sport, dst, dport) / NatGetFlowByHash(dst, dport, src, sport)
    uint32_t rip = wan ? src : dst, rport = wan ? sport : dport;
    const uint32_t lip = wan ? dst : src, lport = wan ? dport : sport;
    if (nat_type != HALO_NAT_SYMMETRIC) { rip = 0; rport = 0; }  // :528-534
    if (proto == 1u) rport = 0;                                    // ICMP, :535-537
    return Key{rip, rport, lip, lport, proto};
}

// ... and its hash
HALO_FLOWKEY_FN uint64_t nat_hash(uint32_t proto, uint32_t src, uint32_t dst, uint32_t sport,
                                  uint32_t dport, uint32_t kind, uint32_t nat_type) {
    return key_hash(nat_key(proto, src, dst, sport, dport, kind, nat_type));
}

// The tag word of a used slot of a device flow table (nat_table.h, pmflow_table.h) is
// kSlotUsed | proto; 0 = empty.
constexpr uint32_t kSlotUsed = 0x80000000u;

#if defined(__HIPCC__)
// One probe sequence over a table of mask + 1 32-byte slots {rip, lip, rport | lport << 16, tag;
// four value words}, placed by linear probing from key_hash & mask: the value words of the slot
// whose key equals k, or false when the chain ends (an empty slot) first. One aligned 32-byte slot
// per step, as two 16-byte loads of one sector.
__device__ __forceinline__ bool probe(const uint4* __restrict__ tab, uint32_t mask, const Key& k, uint4* hit) {
    const uint32_t ports = k.rport | k.lport << 16, tag = kSlotUsed | k.proto;
    uint32_t s = (uint32_t)key_hash(k) & mask;
    for (uint32_t step = 0; step <= mask; ++step) {  // bounded: a full table cannot spin
        const uint4* p = tab + 2ull * s;
        const uint4 key = p[0];
        const uint4 val = p[1];
        if (key.w == 0) return false;
        if (key.x == k.rip && key.y == k.lip && key.z == ports && key.w == tag) {
            *hit = val;
            return true;
        }
        s = (s + 1) & mask;
    }
    return false;
}
#endif

}  // namespace flowkey
}  // namespace halo
