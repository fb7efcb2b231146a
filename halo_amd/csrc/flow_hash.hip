// flow_hash.hip — SURVEY.md §8f row f3 on gfx950: XXH3-64 (hashcode/xxh3.go, the reference's
// trimmed port of github.com/zeebo/xxh3 v1.1.0: default secret, seed 0) over batches of byte
// strings, and the NAT flow-table keys of the forward path (NatFlowHash / NatWanFlowHash,
// engine/ipv4_engine.go:451-479) hashed straight from parsed rx records.
//
// Shape. One kernel, the run kernel (xxh3_run_kernel below): a one-wave block owns a window of
// kRunWin consecutive strings and splits it into 16 contiguous runs, one per 4-lane group. Lane j
// of a group owns accumulators 2j and 2j+1 of hashLong's eight (xxh3.go:132-209) and reads bytes
// [16j, 16j+16) of each 64-byte stripe, so accumulateStripe's i ^ 1 exchange stays inside the
// lane; strings of 17..240 B (hashMedium / hashLarge, :94-129) put their mix16 terms on the same
// four lanes and the same loads, strings of <= 16 B take hashSmall (:59-91). The window's hashes
// leave as whole lines in string order.
//
// String data are read 16 bytes at a time at any byte address, every byte a string byte; the
// <= 16 B path reads aligned dwords merged with v_alignbyte. Either way no read touches a dword
// that holds none of the string's bytes (so never a page the string is not on).
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "flow_key.h"
#include "halo_common.h"

namespace halo {
namespace {

// hashcode/xxh3.go:27-40 (192 bytes) as little-endian dwords, + 2 zero dwords for the
// unaligned-read overhang
__constant__ uint32_t kSecretDw[50] = {
    0x396cfeb8u, 0xbe4ba423u, 0x2c81017cu, 0x1cad21f7u, 0xe96dd4deu, 0xdb979083u, 0xa4a44072u, 0x1f67b3b7u,
    0x4ee679cbu, 0x78e5c0ccu, 0x7dd05a82u, 0x2172ffccu, 0x744608b8u, 0x8e2443f7u, 0xe69035e0u, 0x4c263a81u,
    0xbb52283cu, 0xcb00c391u, 0x8b65d088u, 0xa32e531bu, 0x97486471u, 0x4ef90da2u, 0x46ef1938u, 0xd8acdea9u,
    0x3f76faa8u, 0x3f349ce3u, 0xc7bbdcf9u, 0x1d4f0bc7u, 0x4be0518au, 0x3159b4cdu, 0xc97e9fc8u, 0x647378d9u,
    0x83acc5eau, 0xc3ebd334u, 0xffa081c5u, 0xeb6313fau, 0x51dd0d17u, 0x49daf0b7u, 0x265516d3u, 0x9e68d429u,
    0x58be162bu, 0xfca1477du, 0xd1b8f88fu, 0xce31d07au, 0x8f3acb45u, 0x28041695u, 0xcafbd7afu, 0x7e404bbbu,
    0u, 0u};

constexpr uint64_t P32_1 = 2654435761ull, P32_2 = 2246822519ull, P32_3 = 3266489917ull;
constexpr uint64_t P64_1 = 11400714785074694791ull, P64_2 = 14029467366897019727ull,
                   P64_3 = 1609587929392839161ull, P64_4 = 9650029242287828579ull,
                   P64_5 = 2870177450012600261ull;

__device__ __forceinline__ uint64_t join64(uint32_t lo, uint32_t hi) { return (uint64_t)hi << 32 | lo; }

// secret64(off) (xxh3.go:282-284) for any byte offset
__device__ __forceinline__ uint64_t sec64(uint32_t off) {
    const uint32_t a = off >> 2, s = off & 3u;
    const uint32_t w0 = kSecretDw[a], w1 = kSecretDw[a + 1], w2 = kSecretDw[a + 2];
    return join64(__builtin_amdgcn_alignbyte(w1, w0, s), __builtin_amdgcn_alignbyte(w2, w1, s));
}
__device__ __forceinline__ uint32_t sec32(uint32_t off) { return (uint32_t)sec64(off); }

typedef const __attribute__((address_space(1))) uint32_t gdw;

// little-endian reads of string bytes at any address (xxh3.go:262-279)
__device__ __forceinline__ uint64_t ld64(const uint8_t* p) {
    const uintptr_t u = reinterpret_cast<uintptr_t>(p);
    gdw* q = (gdw*)(u & ~(uintptr_t)3);
    const uint32_t s = (uint32_t)(u & 3u);
    const uint32_t w0 = q[0], w1 = q[1];
    const uint32_t w2 = s ? q[2] : 0u;
    return join64(__builtin_amdgcn_alignbyte(w1, w0, s), __builtin_amdgcn_alignbyte(w2, w1, s));
}
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) {
    const uintptr_t u = reinterpret_cast<uintptr_t>(p);
    gdw* q = (gdw*)(u & ~(uintptr_t)3);
    const uint32_t s = (uint32_t)(u & 3u);
    const uint32_t w0 = q[0];
    const uint32_t w1 = s ? q[1] : 0u;
    return __builtin_amdgcn_alignbyte(w1, w0, s);
}
__device__ __forceinline__ uint32_t ld8(const uint8_t* p) {
    return *(const __attribute__((address_space(1))) uint8_t*)p;
}

__device__ __forceinline__ uint64_t mul_fold64(uint64_t a, uint64_t b) { return (a * b) ^ __umul64hi(a, b); }
__device__ __forceinline__ uint64_t avalanche_small(uint64_t v) {  // xxh3.go:228-235
    v ^= v >> 33; v *= P64_2; v ^= v >> 29; v *= P64_3; v ^= v >> 32;
    return v;
}
__device__ __forceinline__ uint64_t avalanche(uint64_t v) {  // xxh3.go:238-243
    v ^= v >> 37; v *= 0x165667919e3779f9ull; v ^= v >> 32;
    return v;
}
__device__ __forceinline__ uint64_t rotl64(uint64_t v, int r) { return (v << r) | (v >> (64 - r)); }
__device__ __forceinline__ uint64_t rrmxmx(uint64_t v, uint64_t len) {  // xxh3.go:246-253
    v ^= rotl64(v, 49) ^ rotl64(v, 24);
    v *= 0x9fb21c651e98df25ull;
    v ^= (v >> 35) + len;
    v *= 0x9fb21c651e98df25ull;
    v ^= v >> 28;
    return v;
}

// hashSmall for 9..16 bytes given the two overlapping 8-byte words (xxh3.go:62-66)
__device__ __forceinline__ uint64_t hash_9to16(uint64_t w_lo, uint64_t w_hi, uint32_t len) {
    const uint64_t lo = w_lo ^ (sec64(24) ^ sec64(32));
    const uint64_t hi = w_hi ^ (sec64(40) ^ sec64(48));
    return avalanche((uint64_t)len + __builtin_bswap64(lo) + hi + mul_fold64(lo, hi));
}

// hashSmall (xxh3.go:59-91), len <= 16, one lane
__device__ __forceinline__ uint64_t hash_upto16(const uint8_t* d, uint32_t len) {
    if (len > 8) return hash_9to16(ld64(d), ld64(d + len - 8), len);
    if (len > 3) {
        const uint64_t in = (uint64_t)ld32(d + len - 4) + ((uint64_t)ld32(d) << 32);
        return rrmxmx(in ^ (sec64(8) ^ sec64(16)), len);
    }
    uint64_t acc;
    if (len == 3) acc = ((uint64_t)(ld8(d) | ld8(d + 1) << 8) << 16) + ld8(d + 2) + (3u << 8);
    else if (len == 2) acc = ((uint64_t)(ld8(d) | ld8(d + 1) << 8) * ((1u << 24) + 1) >> 8) + (2u << 8);
    else if (len == 1) acc = (uint64_t)ld8(d) * ((1u << 24) + (1u << 16) + 1) + (1u << 8);
    else return 0x2d06800538d394c2ull;
    acc ^= (uint64_t)(sec32(0) ^ sec32(4));
    return avalanche_small(acc);
}

// a 64-bit DPP move (both halves with the same control)
template <int CTRL>
__device__ __forceinline__ uint64_t dpp64(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, false);
    return join64(lo, hi);
}

// Secret words the long path needs, staged in LDS once per block: the 64-bit word at byte 8k
// (k = 0..23: stripe secrets, k = 16 + j: scramble), at 121 + 8j (last stripe) and at 11 + 8j
// (merge). Lane j of a group reads word st + j for stripe st: one ds_read_b64, no constant-cache
// gathers.
struct LongSecrets {
    uint64_t w8[24];
    uint64_t last[8];
    uint64_t merge[8];
    uint64_t mid3[16];  // hashLarge's middle terms: the word at 3 + 8k (xxh3.go:124-126)
    uint64_t mlast[2];  // hashLarge's last term: the words at 119 and 127 (:127)
};

__device__ __forceinline__ void load_secrets(LongSecrets& s) {  // needs >= 58 threads
    const uint32_t t = threadIdx.x;
    if (t < 24) s.w8[t] = sec64(8 * t);
    else if (t < 32) s.last[t - 24] = sec64(121 + 8 * (t - 24));
    else if (t < 40) s.merge[t - 32] = sec64(11 + 8 * (t - 32));
    else if (t < 56) s.mid3[t - 40] = sec64(3 + 8 * (t - 40));
    else if (t < 58) s.mlast[t - 56] = sec64(119 + 8 * (t - 56));
}

// hashLong on a group of 4 lanes: lane j owns accumulators 2j and 2j+1 and reads input words 2j
// and 2j+1 of each stripe (bytes [16j, 16j+16): one 16-byte load), so the i ^ 1 exchange of
// accumulateStripe (xxh3.go:181-209) stays inside the lane — no DPP swap — and a wave-instruction
// reads 16 strings' 64-byte stripes. The load is unaligned (gfx9 global loads accept any byte
// address; the 16 bytes are all string bytes, so no other page is touched).
typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(1)));
__device__ __forceinline__ void ld128u(const uint8_t* p, uint64_t& lo, uint64_t& hi) {
    const u32x4u v = *(const __attribute__((address_space(1))) u32x4u*)p;
    lo = join64(v.x, v.y);
    hi = join64(v.z, v.w);
}

struct XxhParams {
    const uint8_t* bytes;
    const uint64_t* offsets;
    const uint32_t* lens;
    uint32_t n;
    uint64_t* out;
    uint32_t win;  // strings per wave of the run kernel (<= kRunWin)
};

// ---- the run kernel ---------------------------------------------------------------------------
// the per-class kernels fetched 1.29x the algorithmic bytes — strings packed one byte
// apart share their first and last 128-byte lines with their neighbours, and a neighbour was hashed
// at another time (a length-ranked round, or the short-string pass), by then evicted from the L2 —
// and wrote every 8-byte hash on its own (3.2x the hash bytes).
//
// Shape. A wave owns a window of kRunWin consecutive strings and splits it into 16 contiguous RUNS
// of strings, one per 4-lane group, balanced by their cost in loop iterations (a long string: one
// iteration per 4 stripes, counting the last stripe; a string <= 240 B: one). Each group hashes its
// run in index order, so the line a string shares with the next one is read twice in a row by the
// same group (an L2 hit, often a TCP one), and only the 15 boundaries between runs can miss. Every
// iteration a group issues up to four 16-byte loads for whatever its current string needs: four
// stripes of a long string (hashLong, xxh3.go:132-209; accumulateStripe's terms do not depend on the
// accumulators, so the last stripe is simply one more term of the final block), or the mix16 terms of
// hashMedium / hashLarge (:94-129, two or four per lane), so all groups share one memory round trip
// per iteration whatever mix of strings they hold. Strings of <= 16 B take hashSmall (:59-91). The
// window's hashes collect in LDS and leave as whole lines in string order.
constexpr uint32_t kRunWin = 256;  // strings per wave (a multiple of 64)
constexpr uint32_t kRunPer = kRunWin / 64;
struct RunLds {
    uint64_t off[kRunWin];
    uint64_t hash[kRunWin];
    uint32_t len[kRunWin];
    uint32_t pref[kRunWin];  // exclusive prefix of the strings' iteration counts
};

// Stripes per iteration of a long string (16-byte loads per lane in flight): 8 halves the
// dependent memory round trips a wave makes (a window of 256 KCP-sized strings is ~56 of them at 4)
constexpr uint32_t kRunB = 8;
static_assert(kRunB == 4 || kRunB == 8 || kRunB == 16, "a batch must not straddle a 16-stripe block");
__device__ __forceinline__ uint32_t run_cost(uint32_t len) {
    return len > 240 ? ((len - 1) / 64 + kRunB) / kRunB : 1u;  // ceil((T + 1) / B), T = loop stripes
}

__device__ __forceinline__ uint64_t quad_sum(uint64_t v) {
    v += dpp64<0xB1>(v);  // quad_perm 1,0,3,2
    v += dpp64<0x4E>(v);  // quad_perm 2,3,0,1
    return v;
}

// Branch-free iteration: every lane issues all kRunB loads, an idle slot (past a string's last
// stripe, a short string, a finished group) reading this zero line instead of branching around
// the load; the long path selects secrets and drops terms past the last stripe.
#ifndef HALO_XXH3_PROBE  // tools only: the run kernel's loads without the hashing (wrong hashes)
#define HALO_XXH3_PROBE 0
#endif
__device__ const uint8_t g_xxh3_pad[64] = {};

__global__ void __launch_bounds__(64) xxh3_run_kernel(const XxhParams p) {
    __shared__ LongSecrets sec;
    __shared__ RunLds s;
    load_secrets(sec);
    const uint32_t lane = threadIdx.x;
    const uint32_t base = blockIdx.x * p.win;
    const uint32_t cnt = p.n - base < p.win ? p.n - base : p.win;
    uint32_t total = 0;
#pragma unroll
    for (uint32_t k = 0; k < kRunPer; ++k) {  // stage the window's metadata; weights' exclusive prefix
        const uint32_t r = 64 * k + lane;
        const bool in = r < cnt;
        const uint32_t len = in ? p.lens[base + r] : 0u;
        s.len[r] = len;
        s.off[r] = in ? p.offsets[base + r] : 0ull;
        const uint32_t w = in ? run_cost(len) : 0u;
        uint32_t incl = w;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d, 64);
            if (lane >= (uint32_t)d) incl += o;
        }
        s.pref[r] = total + incl - w;
        total += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    __syncthreads();
    const uint32_t g = lane >> 2, j = lane & 3u;
    // run of group g: the strings whose cost starts in [ceil(g * total / 16), ceil((g + 1) * total / 16))
    auto first_at = [&](uint32_t t) {
        uint32_t lo = 0, hi = cnt;
        while (lo < hi) {
            const uint32_t m = (lo + hi) >> 1;
            if (s.pref[m] < t) lo = m + 1;
            else hi = m;
        }
        return lo;
    };
    uint32_t idx = first_at((uint32_t)(((uint64_t)g * total + 15) / 16));
    const uint32_t end = g == 15 ? cnt : first_at((uint32_t)(((uint64_t)(g + 1) * total + 15) / 16));
    constexpr uint64_t kInit[8] = {P32_3, P64_1, P64_2, P64_3, P64_4, P32_2, P64_5, P32_1};
    const uint64_t init0 = j == 0 ? kInit[0] : j == 1 ? kInit[2] : j == 2 ? kInit[4] : kInit[6];
    const uint64_t init1 = j == 0 ? kInit[1] : j == 1 ? kInit[3] : j == 2 ? kInit[5] : kInit[7];
    uint32_t len = 0, T = 0, nb = 0, st = 0;
    const uint8_t* d = p.bytes;
    uint64_t a0 = init0, a1 = init1;
    auto begin = [&]() {
        len = s.len[idx];
        d = p.bytes + s.off[idx];
        T = len > 240 ? (len - 1) / 64 : 0u;
        nb = len > 240 ? (len - 1) / 1024 : 0u;
        st = 0;
        a0 = init0;
        a1 = init1;
    };
    if (idx < end) begin();
    for (;;) {
        const bool act = idx < end;
        if (!__builtin_amdgcn_ballot_w64(act)) break;
        const bool lng = act && len > 240, mid = act && len > 16 && len <= 240, sml = act && len <= 16;
        const bool large = len > 128;
        const uint32_t lv = len > 96 ? 4u : len > 64 ? 3u : len > 32 ? 2u : 1u;  // hashMedium's pairs
        const uint32_t nmid = large ? ((len & ~15u) - 128) / 16 : 0u;           // hashLarge's middle terms
        uint64_t lo[kRunB], hi[kRunB];
#pragma unroll
        for (uint32_t u = 0; u < kRunB; ++u) {
            const uint8_t* a = d;
            bool v = false;
            if (lng) {
                const uint32_t x = st + u;
                v = x <= T;
                a = x < T ? d + 64 * x + 16 * j : d + len - 64 + 16 * j;
            } else if (u >= 4) {  // the short hashes need four loads at most
            } else if (mid && !large) {
                v = u < 2 && j < lv;
                a = u == 0 ? d + 16 * j : d + len - 16 - 16 * j;
            } else if (mid) {
                const uint32_t t = 2 * j + (u & 1u);
                v = u < 2 || t <= nmid;
                a = u < 2 ? d + 16 * t : t < nmid ? d + 128 + 16 * t : d + len - 16;
            }
            ld128u(v ? a : g_xxh3_pad, lo[u], hi[u]);
        }
        uint64_t h = 0;
        bool have = false;
#if HALO_XXH3_PROBE
        // measurement probe (tools only, wrong hashes): the same loads and control flow, no hashing
        if (lng) {
#pragma unroll
            for (uint32_t u = 0; u < kRunB; ++u) {
                a0 ^= lo[u];
                a1 ^= hi[u];
            }
            st += kRunB;
            if (st > T) {
                h = a0 ^ a1;
                have = true;
            }
        }
        if (mid) {
            h = lo[0] ^ hi[0] ^ lo[1] ^ hi[1] ^ lo[2] ^ hi[2] ^ lo[3] ^ hi[3];
            have = true;
        }
#else
        if (lng) {
#pragma unroll
            for (uint32_t u = 0; u < kRunB; ++u) {
                const uint32_t x = st + u;
                // select the secret and drop the term past the last stripe instead of branching
                const uint64_t s0 = x < T ? sec.w8[(x & 15u) + 2 * j] : sec.last[2 * j];
                const uint64_t s1 = x < T ? sec.w8[(x & 15u) + 2 * j + 1] : sec.last[2 * j + 1];
                const uint64_t k0 = lo[u] ^ s0, k1 = hi[u] ^ s1;
                const uint64_t t0 = hi[u] + (uint64_t)(uint32_t)k0 * (k0 >> 32);
                const uint64_t t1 = lo[u] + (uint64_t)(uint32_t)k1 * (k1 >> 32);
                a0 += x <= T ? t0 : 0ull;
                a1 += x <= T ? t1 : 0ull;
            }
            st += kRunB;
            if ((st & 15u) == 0 && (st >> 4) <= nb) {  // a full block ended: scramble (xxh3.go:212-218)
                a0 ^= a0 >> 47;
                a1 ^= a1 >> 47;
                a0 ^= sec.w8[16 + 2 * j];
                a1 ^= sec.w8[17 + 2 * j];
                a0 *= P32_1;
                a1 *= P32_1;
            }
            if (st > T) {  // merge (xxh3.go:139-145): pair (2j, 2j+1) with secret 11 + 16j, summed over the quad
                const uint64_t m = quad_sum(mul_fold64(a0 ^ sec.merge[2 * j], a1 ^ sec.merge[2 * j + 1]));
                h = avalanche((uint64_t)len * P64_1 + m);
                have = true;
            }
        }
        if (mid) {
            uint64_t t01 = 0, t23 = 0;
            if (!large) {  // hashMedium: pair j = terms (16j, secret 32j) and (len-16-16j, secret 32j+16)
                if (j < lv)
                    t01 = mul_fold64(lo[0] ^ sec.w8[4 * j], hi[0] ^ sec.w8[4 * j + 1]) +
                          mul_fold64(lo[1] ^ sec.w8[4 * j + 2], hi[1] ^ sec.w8[4 * j + 3]);
                h = avalanche((uint64_t)len * P64_1 + quad_sum(t01));
            } else {       // hashLarge: terms 2j, 2j+1 of the first eight, then of the middle + last
                t01 = mul_fold64(lo[0] ^ sec.w8[4 * j], hi[0] ^ sec.w8[4 * j + 1]) +
                      mul_fold64(lo[1] ^ sec.w8[4 * j + 2], hi[1] ^ sec.w8[4 * j + 3]);
                const uint64_t acc = avalanche((uint64_t)len * P64_1 + quad_sum(t01));
#pragma unroll
                for (uint32_t u = 2; u < 4; ++u) {
                    const uint32_t t = 2 * j + (u & 1u);
                    if (t < nmid) t23 += mul_fold64(lo[u] ^ sec.mid3[2 * t], hi[u] ^ sec.mid3[2 * t + 1]);
                    else if (t == nmid) t23 += mul_fold64(lo[u] ^ sec.mlast[0], hi[u] ^ sec.mlast[1]);
                }
                h = avalanche(acc + quad_sum(t23));
            }
            have = true;
        }
#endif
        if (sml) {  // hashSmall: every lane of the group computes it
            h = hash_upto16(d, len);
            have = true;
        }
        if (have) {
            if (j == 0) s.hash[idx] = h;
            ++idx;
            if (idx < end) begin();
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kRunPer; ++k) {  // the window's hashes as whole lines, in string order
        const uint32_t r = 64 * k + lane;
        if (r < cnt) p.out[base + r] = s.hash[r];
    }
}

// Tried and removed (round 4; in git history up to commit 68eed30): the run kernel
// on 8 groups of 8 lanes (128 contiguous bytes per string per load instruction) and a software-
// pipelined run kernel (step k + 1's loads before step k's arithmetic). Both bit-exact, both slower.
//
// Tried and removed (in git history up to commit 9ac2a89), each bit-exact:
//  - the round-3 pair of kernels the run kernel replaced: a short-string kernel (a wave compacted 256
//    strings by class; 17..240 B on 8-lane groups, one 16-byte mix16 term per lane; lane-per-string
//    for those lengths, every lane gathering 4-byte words of a different string, ran at ~0.5 TB/s) and
//    a long-string kernel (a wave ranked its 64 strings by length and hashed the long ones one per
//    4- or 8-lane group, the short ones optionally in the same wave). Its loads went four stripes at a
//    time from one-wave blocks: 8 / 16 stripes were 11 / 30 % slower, 256-thread blocks 2 % slower
//    (profiles/r02/ab_xxh3_batch_block.log). Non-temporal string loads and dwordx3 loads went with it.
//  - a loop that branched around idle load slots instead of reading the zero line;
//  - one finishing sequence shared by long merges and 17..240 B strings: 0.189 / 0.189 ms against
//    0.188 / 0.186 (profiles/r04/r4i);
//  - dword-aligned loads (an aligned 16-byte load plus one dword, merged with v_alignbyte) instead of
//    one byte-unaligned 16-byte load: 0.214 / 0.214 ms against 0.185 / 0.185 (profiles/r04/r4j);
//  - windows sized so that all waves are resident at once (5120 waves = 5 per SIMD at the kernel's
//    95 VGPRs; 1M strings -> 208-string windows, 5042 waves): 0.199 / 0.200 ms against 0.186 / 0.186
//    for 256-string windows (4096 waves; profiles/r04/r4h/ab_xxh3_bf.log).


// ---- NAT flow keys from parsed records ------------------------------------------------------
struct FlowParams {
    const void* recs;  // halo_rx_result_t (32 B) or, COMPACT, halo_rx_record16_t (16 B)
    uint32_t n, kind, nat_type, buckets;
    uint64_t* hash;
    uint32_t* bucket;
};

// Full records: bytes 0..15 (status..dst_ip) and 16..19 (sport, dport) of each 32-byte record —
// 20 of every 32 bytes, so the memory system delivers the whole record (1.6x the bytes used,
// VERDICT r3). Compact records carry the same five fields in 16 bytes: one load, nothing unused.
template <bool COMPACT>
__global__ void __launch_bounds__(256) flow_hash_kernel(const FlowParams p) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += stride) {
        uint32_t proto, src, dst, ports;
        if constexpr (COMPACT) {  // status, flags, ip_proto, l4_aux | src | dst | sport, dport
            const uint4 a = reinterpret_cast<const uint4*>(p.recs)[i];
            proto = (a.x >> 16) & 0xFFu;
            src = a.y;
            dst = a.z;
            ports = a.w;
        } else {
            const uint4 a = reinterpret_cast<const uint4*>(p.recs)[2ull * i];
            ports = reinterpret_cast<const uint32_t*>(p.recs)[8ull * i + 4];
            proto = a.y & 0xFFu;
            src = a.z;
            dst = a.w;
        }
        const uint64_t h = flowkey::nat_hash(proto, src, dst, ports & 0xFFFFu, ports >> 16, p.kind, p.nat_type);
        p.hash[i] = h;
        if (p.bucket) p.bucket[i] = (uint32_t)(h % p.buckets);  // hashmap/hashmap.go:64
    }
}

uint32_t blocks_for(uint64_t threads) {
    const uint64_t b = (threads + 255) / 256;
    const uint64_t kMax = 256ull * 8 * 8;
    return (uint32_t)(b > kMax ? kMax : (b ? b : 1));
}

}  // namespace
}  // namespace halo

#if HALO_XXH3_PROBE_ENTRY
// The XXH3 line's load-pattern probe (measurement tooling): tools/libhalo_bench.so compiles this
// file a second time with HALO_XXH3_PROBE=1 HALO_XXH3_PROBE_ENTRY=1, and this entry — nothing of the
// product's — launches the run kernel with its hashing replaced by XORs (the same windows, runs,
// loads and control flow; the hashes it writes are not XXH3).
extern "C" __attribute__((visibility("default"))) int halo_bench_xxh3_probe_launch(
    const uint8_t* d_bytes, const uint64_t* d_offsets, const uint32_t* d_lens, uint32_t n, uint64_t* d_hash,
    void* stream) {
    static_assert(HALO_XXH3_PROBE, "the probe entry is the run kernel built as a probe");
    if (n == 0 || !d_bytes || !d_offsets || !d_lens || !d_hash) return HALO_E_INVAL;
    halo::XxhParams p{d_bytes, d_offsets, d_lens, n, d_hash};
    p.win = halo::kRunWin;
    hipLaunchKernelGGL(halo::xxh3_run_kernel, dim3((n + p.win - 1) / p.win), dim3(64), 0,
                       static_cast<hipStream_t>(stream), p);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}
#else
extern "C" HALO_API int halo_xxh3_64_batch_device(const uint8_t* d_bytes, const uint64_t* d_offsets,
                                                  const uint32_t* d_lens, uint32_t n, uint64_t* d_hash,
                                                  halo_stream_t stream) {
    if (n == 0) return HALO_OK;
    if (!d_offsets || !d_lens || !d_hash) return HALO_E_INVAL;
    if (reinterpret_cast<uintptr_t>(d_hash) & 7u) return HALO_E_INVAL;
    int rc = halo::check_device();
    if (rc) return rc;
    halo::XxhParams p{d_bytes, d_offsets, d_lens, n, d_hash};
    const hipStream_t s = static_cast<hipStream_t>(stream);
    // one one-wave block per window of kRunWin strings: no grid-stride loop, no cap on the grid
    const uint32_t win = halo::kRunWin;
    p.win = win;
    hipLaunchKernelGGL(halo::xxh3_run_kernel, dim3((n + win - 1) / win), dim3(64), 0, s, p);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

namespace {
int flow_hash(const void* d_records, bool compact, uint32_t n, uint32_t kind, uint32_t nat_type, uint64_t* d_hash,
              uint32_t bucket_count, uint32_t* d_bucket, halo_stream_t stream) {
    if (kind > HALO_FLOW_NAT_WAN) return HALO_E_INVAL;
    if (d_bucket && bucket_count == 0) return HALO_E_INVAL;
    if (n == 0) return HALO_OK;
    if (!d_records || !d_hash) return HALO_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_records) & 15u) || (reinterpret_cast<uintptr_t>(d_hash) & 7u))
        return HALO_E_INVAL;
    int rc = halo::check_device();
    if (rc) return rc;
    halo::FlowParams p{d_records, n, kind, nat_type, bucket_count, d_hash, d_bucket};
    if (compact)
        hipLaunchKernelGGL(halo::flow_hash_kernel<true>, dim3(halo::blocks_for(n)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), p);
    else
        hipLaunchKernelGGL(halo::flow_hash_kernel<false>, dim3(halo::blocks_for(n)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), p);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}
}  // namespace

extern "C" HALO_API int halo_flow_hash_device(const halo_rx_result_t* d_records, uint32_t n, uint32_t kind,
                                              uint32_t nat_type, uint64_t* d_hash, uint32_t bucket_count,
                                              uint32_t* d_bucket, halo_stream_t stream) {
    return flow_hash(d_records, false, n, kind, nat_type, d_hash, bucket_count, d_bucket, stream);
}

extern "C" HALO_API int halo_flow_hash_compact_device(const halo_rx_record16_t* d_records, uint32_t n, uint32_t kind,
                                                      uint32_t nat_type, uint64_t* d_hash, uint32_t bucket_count,
                                                      uint32_t* d_bucket, halo_stream_t stream) {
    return flow_hash(d_records, true, n, kind, nat_type, d_hash, bucket_count, d_bucket, stream);
}
#endif  // HALO_XXH3_PROBE_ENTRY
