// kcp_check_host.h — kcp.go's byte_check_hash on the host, for the two sequential loops
// (rx_kcp_host.cc compares with it, tx_kcp_host.cc fills the header's field with it): a bytewise
// CRC-32 and an XXH3-64 written from hashcode/xxh3.go (flow_key.h's covers the 13-byte flow key
// only); the tests hold both against zlib and oracle/ref_xxh3_py.py. Plain C++17, host code only.
#pragma once
#include <string.h>

#include "rx_kcp.h"

namespace halo {
namespace kcp {
namespace {

struct CrcTable {  // the register after one more byte, by the byte XORed into its low end
    uint32_t t[256];
    constexpr CrcTable() : t() {
        for (uint32_t i = 0; i < 256; ++i) t[i] = crc_steps(i, 8);
    }
};
constexpr CrcTable kCrcTable;

uint32_t crc32_bytes(const uint8_t* d, uint32_t n) {  // crc32.ChecksumIEEE, a byte and a table lookup at a time
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i) c = kCrcTable.t[(c ^ d[i]) & 0xFFu] ^ (c >> 8);
    return ~c;
}

// ---- XXH3-64, default secret, seed 0 (hashcode/xxh3.go) -----------------------------------------
const uint8_t kSecret[192] = {
    0xb8, 0xfe, 0x6c, 0x39, 0x23, 0xa4, 0x4b, 0xbe, 0x7c, 0x01, 0x81, 0x2c, 0xf7, 0x21, 0xad, 0x1c, 0xde, 0xd4, 0x6d, 0xe9,
    0x83, 0x90, 0x97, 0xdb, 0x72, 0x40, 0xa4, 0xa4, 0xb7, 0xb3, 0x67, 0x1f, 0xcb, 0x79, 0xe6, 0x4e, 0xcc, 0xc0, 0xe5, 0x78,
    0x82, 0x5a, 0xd0, 0x7d, 0xcc, 0xff, 0x72, 0x21, 0xb8, 0x08, 0x46, 0x74, 0xf7, 0x43, 0x24, 0x8e, 0xe0, 0x35, 0x90, 0xe6,
    0x81, 0x3a, 0x26, 0x4c, 0x3c, 0x28, 0x52, 0xbb, 0x91, 0xc3, 0x00, 0xcb, 0x88, 0xd0, 0x65, 0x8b, 0x1b, 0x53, 0x2e, 0xa3,
    0x71, 0x64, 0x48, 0x97, 0xa2, 0x0d, 0xf9, 0x4e, 0x38, 0x19, 0xef, 0x46, 0xa9, 0xde, 0xac, 0xd8, 0xa8, 0xfa, 0x76, 0x3f,
    0xe3, 0x9c, 0x34, 0x3f, 0xf9, 0xdc, 0xbb, 0xc7, 0xc7, 0x0b, 0x4f, 0x1d, 0x8a, 0x51, 0xe0, 0x4b, 0xcd, 0xb4, 0x59, 0x31,
    0xc8, 0x9f, 0x7e, 0xc9, 0xd9, 0x78, 0x73, 0x64, 0xea, 0xc5, 0xac, 0x83, 0x34, 0xd3, 0xeb, 0xc3, 0xc5, 0x81, 0xa0, 0xff,
    0xfa, 0x13, 0x63, 0xeb, 0x17, 0x0d, 0xdd, 0x51, 0xb7, 0xf0, 0xda, 0x49, 0xd3, 0x16, 0x55, 0x26, 0x29, 0xd4, 0x68, 0x9e,
    0x2b, 0x16, 0xbe, 0x58, 0x7d, 0x47, 0xa1, 0xfc, 0x8f, 0xf8, 0xb8, 0xd1, 0x7a, 0xd0, 0x31, 0xce, 0x45, 0xcb, 0x3a, 0x8f,
    0x95, 0x16, 0x04, 0x28, 0xaf, 0xd7, 0xfb, 0xca, 0xbb, 0x4b, 0x40, 0x7e};
constexpr uint64_t P32_1 = 2654435761ull, P32_2 = 2246822519ull, P32_3 = 3266489917ull;
constexpr uint64_t P64_1 = 11400714785074694791ull, P64_2 = 14029467366897019727ull, P64_3 = 1609587929392839161ull,
                   P64_4 = 9650029242287828579ull, P64_5 = 2870177450012600261ull;

uint64_t r64(const uint8_t* p) {
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
}
uint64_t r32(const uint8_t* p) { return load_u32(p); }
uint64_t sec64(uint32_t off) { return r64(kSecret + off); }
uint64_t mul_fold(uint64_t a, uint64_t b) {
    const unsigned __int128 p = (unsigned __int128)a * b;
    return (uint64_t)p ^ (uint64_t)(p >> 64);
}
uint64_t aval(uint64_t v) {
    v ^= v >> 37;
    v *= 0x165667919e3779f9ull;
    return v ^ (v >> 32);
}
uint64_t rotl(uint64_t v, int r) { return (v << r) | (v >> (64 - r)); }
uint64_t mix16(const uint8_t* d, uint32_t soff) { return mul_fold(r64(d) ^ sec64(soff), r64(d + 8) ^ sec64(soff + 8)); }

uint64_t xxh3_64(const uint8_t* d, uint32_t n) {
    if (n == 0) return 0x2d06800538d394c2ull;
    if (n <= 3) {  // xxh3.go:71-80
        uint64_t v = ((uint64_t)d[0] << 16 | (uint64_t)d[n >> 1] << 24 | d[n - 1] | (uint64_t)n << 8) ^ (r32(kSecret) ^ r32(kSecret + 4));
        v ^= v >> 33;
        v *= P64_2;
        v ^= v >> 29;
        v *= P64_3;
        return v ^ (v >> 32);
    }
    if (n <= 8) {  // :67-70
        uint64_t v = (r32(d + n - 4) + (r32(d) << 32)) ^ (sec64(8) ^ sec64(16));
        v ^= rotl(v, 49) ^ rotl(v, 24);
        v *= 0x9fb21c651e98df25ull;
        v ^= (v >> 35) + n;
        v *= 0x9fb21c651e98df25ull;
        return v ^ (v >> 28);
    }
    if (n <= 16) {  // :62-66
        const uint64_t lo = r64(d) ^ (sec64(24) ^ sec64(32)), hi = r64(d + n - 8) ^ (sec64(40) ^ sec64(48));
        return aval((uint64_t)n + __builtin_bswap64(lo) + hi + mul_fold(lo, hi));
    }
    uint64_t acc = (uint64_t)n * P64_1;
    if (n <= 128) {  // hashMedium, :94-113
        for (uint32_t i = 0; 32u * i < n && i < 4; ++i) acc += mix16(d + 16 * i, 32 * i) + mix16(d + n - 16 - 16 * i, 32 * i + 16);
        return aval(acc);
    }
    if (n <= 240) {  // hashLarge, :116-129
        for (uint32_t o = 0; o < 128; o += 16) acc += mix16(d + o, o);
        acc = aval(acc);
        for (uint32_t o = 128; o < (n & ~15u); o += 16) acc += mix16(d + o, o - 125);
        return aval(acc + mix16(d + n - 16, 119));
    }
    uint64_t a[8] = {P32_3, P64_1, P64_2, P64_3, P64_4, P32_2, P64_5, P32_1};  // hashLong, :132-209
    auto stripe = [&](const uint8_t* in, uint32_t soff) {
        for (uint32_t j = 0; j < 8; ++j) {
            const uint64_t v = r64(in + 8 * j), k = v ^ sec64(soff + 8 * j);
            a[j ^ 1] += v;
            a[j] += (k & 0xFFFFFFFFull) * (k >> 32);
        }
    };
    const uint32_t nblocks = (n - 1) / 1024;
    for (uint32_t blk = 0; blk < nblocks; ++blk) {
        for (uint32_t s = 0; s < 16; ++s) stripe(d + 1024 * blk + 64 * s, 8 * s);
        for (uint32_t j = 0; j < 8; ++j) a[j] = ((a[j] ^ (a[j] >> 47)) ^ sec64(128 + 8 * j)) * P32_1;
    }
    const uint32_t base = nblocks * 1024;
    for (uint32_t s = 0; s < (n - 1 - base) / 64; ++s) stripe(d + base + 64 * s, 8 * s);
    stripe(d + n - 64, 121);
    uint64_t r = (uint64_t)n * P64_1;
    for (uint32_t i = 0; i < 4; ++i) r += mul_fold(a[2 * i] ^ sec64(11 + 16 * i), a[2 * i + 1] ^ sec64(19 + 16 * i));
    return aval(r);
}

uint32_t byte_check_hash(int32_t mode, const uint8_t* d, uint32_t n) {  // kcp.go's byte_check_hash
    return mode == HALO_KCP_CHECK_CRC32 ? crc32_bytes(d, n) : mode == HALO_KCP_CHECK_XXH3 ? (uint32_t)xxh3_64(d, n) : 0u;
}

}  // namespace
}  // namespace kcp
}  // namespace halo
