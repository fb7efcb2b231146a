// nat_miss.hip — the device side of the NAT miss path (include/halo_rx.h, "the miss path") on
// gfx950: list, once per key and in ascending record index, the records a lookup left as
// HALO_NAT_V_MISS (collect), and write the host's answers back into the ops, verdicts and refs of
// every record of a key (apply). nat_table.cc checks the arguments and holds the host parts
// (halo_nat_collect_misses_host, halo_nat_resolve_items); nat_lookup.hip reaches these launchers
// through nat::DeviceOps.
//
// Collect is one memset and five launches over a workspace of u32 owner[slots], tiles[n_tiles],
// link[n]:
//   claim    every selected record probes the scratch table linearly from key_hash(key) & mask
//            with atomicCAS(owner[s], EMPTY, i), tried only when a load shows the slot empty (a
//            slot never empties again). An occupied slot holds a record index o whose
//            key is re-derived from the records: equal keys meet in that slot (atomicMin only when
//            i < o — waves run in ascending order, so nearly every duplicate skips the atomic and
//            a one-key batch does not put n atomics on one word), different keys step on. A
//            slot's key never changes once claimed and only its index goes down, so what the table
//            holds at the end does not depend on arrival order, though which slot a key lands in
//            may. link[i] = the record's slot (kAlone for the order-sensitive class, which stays
//            out of the table; kNone when not selected).
//   count    link[i] becomes the representative, owner[link[i]] (i itself for kAlone); tile counts
//            of the records that are their own representative.
//   scan     tile_scan.h's one-workgroup scan; *d_count.
//   scatter  a representative's rank is its list position: its item (rank < cap) and its d_pos.
//   link     every other record: d_pos[i] = d_pos[representative], written by the launch before.
// The outputs are a function of the inputs alone: two runs are byte-identical.
//
// Apply is one lane per record, grid-stride by whole wavefronts; an answer is one 16-byte load;
// counts go through a ballot per verdict and one atomic per wave and counter.
#include <hip/hip_runtime.h>

#include "flow_key.h"
#include "halo_common.h"
#include "nat_table.h"
#include "tile_scan.h"

namespace halo {
namespace {

using nat::kMissTile;

static_assert(sizeof(halo_nat_miss_item_t) == 20 && sizeof(halo_nat_answer_t) == 16, "miss path ABI");
static_assert(kMissTile == 256 && kMissTile % 64 == 0, "whole wavefronts per tile");

constexpr uint32_t kNone = HALO_NAT_NO_FLOW;  // link / owner: not selected / empty
constexpr uint32_t kAlone = 0xFFFFFFFEu;      // link: listed on its own (slot indexes are < 2^31)

struct MissRec {
    uint32_t proto, src, dst, ports;  // ports = sport | dport << 16
};

template <bool COMPACT>
__device__ __forceinline__ MissRec load_rec(const void* __restrict__ recs, uint32_t i) {
    if (COMPACT) {
        const uint4 r = reinterpret_cast<const uint4*>(recs)[i];
        return MissRec{(r.x >> 16) & 0xFFu, r.y, r.z, r.w};
    }
    const uint4 r = reinterpret_cast<const uint4*>(recs)[2ull * i];
    return MissRec{r.y & 0xFFu, r.z, r.w, reinterpret_cast<const uint32_t*>(recs)[8ull * i + 4]};
}

template <uint32_t KIND>
__device__ __forceinline__ flowkey::Key key_of(const MissRec& r, uint32_t nat_type) {
    return flowkey::nat_key(r.proto, r.src, r.dst, r.ports & 0xFFFFu, r.ports >> 16, KIND, nat_type);
}

__device__ __forceinline__ bool same_key(const flowkey::Key& a, const flowkey::Key& b) {
    return a.rip == b.rip && a.rport == b.rport && a.lip == b.lip && a.lport == b.lport && a.proto == b.proto;
}

__device__ __forceinline__ bool selected(const uint8_t* __restrict__ verdict, const uint8_t* __restrict__ select,
                                         uint32_t i) {
    return verdict[i] == HALO_NAT_V_MISS && (!select || select[i]);
}

template <uint32_t KIND, bool COMPACT>
__global__ void __launch_bounds__(256) nat_miss_claim_kernel(const void* __restrict__ recs,
                                                             const uint8_t* __restrict__ verdict,
                                                             const uint8_t* __restrict__ select, uint32_t n,
                                                             uint32_t nat_type, uint32_t* owner, uint32_t mask,
                                                             uint32_t* __restrict__ link) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint32_t at = kNone;
        if (selected(verdict, select, i)) {
            const MissRec r = load_rec<COMPACT>(recs, i);
            // a LAN record with dport == 0 and sport != 0: NatAddFlow refuses it, its key may be shared
            if (KIND == HALO_FLOW_NAT_LAN && (r.ports >> 16) == 0 && (r.ports & 0xFFFFu) != 0) {
                at = kAlone;
            } else {
                const flowkey::Key k = key_of<KIND>(r, nat_type);
                uint32_t s = (uint32_t)flowkey::key_hash(k) & mask;
                // bounded: slots > n, so an empty slot exists; a full table cannot spin
                for (uint32_t step = 0; step <= mask; ++step) {
                    // a slot never empties and whatever index it shows has its key: a load that sees
                    // it taken is as good as a failed CAS, and keeps a one-key batch off the atomic unit
                    uint32_t o = __hip_atomic_load(owner + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (o == kNone) o = atomicCAS(owner + s, kNone, i);
                    if (o == kNone) {
                        at = s;
                        break;
                    }
                    if (same_key(k, key_of<KIND>(load_rec<COMPACT>(recs, o), nat_type))) {
                        if (i < o) atomicMin(owner + s, i);
                        at = s;
                        break;
                    }
                    s = (s + 1) & mask;
                }
            }
        }
        link[i] = at;
    }
}

__global__ void __launch_bounds__(kMissTile) nat_miss_count_kernel(const uint32_t* __restrict__ owner, uint32_t n,
                                                                   uint32_t* tiles, uint32_t* __restrict__ link) {
    const uint32_t i = blockIdx.x * kMissTile + threadIdx.x;
    tile_count(tiles, [&] {
        if (i >= n) return false;
        const uint32_t at = link[i];
        if (at == kNone) return false;
        const uint32_t rep = at == kAlone ? i : owner[at];
        link[i] = rep;
        return rep == i;
    });
}

// One workgroup: tiles[t] becomes the number of items in the tiles before t; *count = all.
__global__ void __launch_bounds__(256) nat_miss_scan_kernel(uint32_t* tiles, uint32_t n_tiles, uint32_t* count) {
    const uint32_t total = scan_tiles(tiles, n_tiles);
    if (threadIdx.x == 0) *count = total;
}

template <bool COMPACT>
__global__ void __launch_bounds__(kMissTile) nat_miss_scatter_kernel(const void* __restrict__ recs, uint32_t n,
                                                                     const uint32_t* __restrict__ tiles,
                                                                     const uint32_t* __restrict__ link,
                                                                     halo_nat_miss_item_t* __restrict__ items, uint32_t cap,
                                                                     uint32_t* __restrict__ pos) {
    const uint32_t i = blockIdx.x * kMissTile + threadIdx.x;
    const uint32_t rep = i < n ? link[i] : kNone;
    const bool sel = rep == i && i < n;
    const uint64_t votes = tile_votes<kMissTile>(sel);
    if (!sel) {
        if (i < n && rep == kNone) pos[i] = kNone;  // a duplicate's is the link launch's
        return;
    }
    const uint32_t rank = tile_rank<kMissTile>(votes, tiles[blockIdx.x]);
    pos[i] = rank;
    if (rank >= cap) return;
    const MissRec r = load_rec<COMPACT>(recs, i);
    uint32_t* o = reinterpret_cast<uint32_t*>(items) + 5ull * rank;  // 20-byte items, 4-byte aligned
    o[0] = i;
    o[1] = r.src;
    o[2] = r.dst;
    o[3] = r.ports;
    o[4] = r.proto;
}

__global__ void __launch_bounds__(256) nat_miss_link_kernel(const uint32_t* __restrict__ link, uint32_t n, uint32_t* pos) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t rep = link[i];
        if (rep != kNone && rep != i) pos[i] = pos[rep];  // rep < n: a record index the claim stored
    }
}

template <uint32_t KIND>
__global__ void __launch_bounds__(256) nat_miss_apply_kernel(const uint32_t* __restrict__ pos, uint32_t n,
                                                             const uint4* __restrict__ answers, uint32_t k,
                                                             halo_tx_op_t* __restrict__ ops, uint8_t* __restrict__ verdict,
                                                             uint32_t* __restrict__ ref, uint32_t* counts) {
    const uint32_t stride = gridDim.x * blockDim.x, lane = threadIdx.x & 63u;
    uint32_t mine = 0;  // lane v < 6: this wave's records answered with verdict v
    // whole wavefronts iterate together (the bound is on the wave's first record), so the ballots
    // below see every lane of the wave
    for (uint32_t base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n; base += stride) {
        const uint32_t i = base + lane;
        uint32_t verd = 0xFFu;  // no answer
        if (i < n) {
            const uint32_t p = pos[i];
            if (p < k) {
                const uint4 a = answers[p];  // ip; ref; port | verdict << 16; pad
                verd = (a.z >> 16) & 0xFFu;
                if (verd == HALO_NAT_V_FLOW || verd == HALO_NAT_V_MAPPING) {
                    halo_tx_op_t* op = ops + i;
                    if (KIND == HALO_FLOW_NAT_WAN) {
                        op->steps |= HALO_TX_NAT_DST;
                        op->dst_port = (uint16_t)a.z;
                        op->dst_ip = a.x;
                    } else {
                        op->steps |= HALO_TX_NAT_SRC;
                        op->src_port = (uint16_t)a.z;
                        op->src_ip = a.x;
                    }
                    verdict[i] = (uint8_t)verd;
                    ref[i] = a.y;
                } else if (verd == HALO_NAT_V_DROP) {
                    verdict[i] = HALO_NAT_V_DROP;
                    ref[i] = HALO_NAT_NO_FLOW;
                }
            }
        }
        if (counts) {
            for (uint32_t v = 0; v <= HALO_NAT_V_DROP; ++v) {
                const uint32_t c = (uint32_t)__popcll(__ballot(verd == v));
                if (lane == v) mine += c;
            }
        }
    }
    if (counts && lane <= HALO_NAT_V_DROP && mine) atomicAdd(counts + lane, mine);
}

uint32_t miss_blocks(uint64_t threads) {
    const uint64_t b = (threads + 255) / 256;
    const uint64_t kMax = 256ull * 8 * 8;  // nat_lookup.hip's cap
    return (uint32_t)(b > kMax ? kMax : (b ? b : 1));
}

template <uint32_t KIND, bool COMPACT>
void launch_collect(const void* d_records, const uint8_t* d_verdict, const uint8_t* d_select, uint32_t n, uint32_t nat_type,
                    uint32_t slots, halo_nat_miss_item_t* d_items, uint32_t cap, uint32_t* d_count, uint32_t* d_pos,
                    uint32_t* owner, uint32_t* tiles, uint32_t* link, hipStream_t st) {
    const uint32_t n_tiles = nat::miss_tiles(n);
    hipLaunchKernelGGL((nat_miss_claim_kernel<KIND, COMPACT>), dim3(miss_blocks(n)), dim3(256), 0, st, d_records, d_verdict,
                       d_select, n, nat_type, owner, slots - 1, link);
    hipLaunchKernelGGL(nat_miss_count_kernel, dim3(n_tiles), dim3(kMissTile), 0, st, owner, n, tiles, link);
    hipLaunchKernelGGL(nat_miss_scan_kernel, dim3(1), dim3(256), 0, st, tiles, n_tiles, d_count);
    hipLaunchKernelGGL(nat_miss_scatter_kernel<COMPACT>, dim3(n_tiles), dim3(kMissTile), 0, st, d_records, n, tiles, link,
                       d_items, cap, d_pos);
    hipLaunchKernelGGL(nat_miss_link_kernel, dim3(miss_blocks(n)), dim3(256), 0, st, link, n, d_pos);
}

}  // namespace

namespace nat {

int miss_collect(uint32_t dir, uint32_t nat_type, bool compact, const void* d_records, const uint8_t* d_verdict,
                 const uint8_t* d_select, uint32_t n, uint32_t slots, halo_nat_miss_item_t* d_items, uint32_t cap,
                 uint32_t* d_count, uint32_t* d_pos, void* d_workspace, halo_stream_t stream) {
    const int rc = check_device();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) return hipMemsetAsync(d_count, 0, sizeof(uint32_t), st) == hipSuccess ? HALO_OK : HALO_E_HIP;
    uint32_t* owner = static_cast<uint32_t*>(d_workspace);
    uint32_t* tiles = owner + slots;
    uint32_t* link = tiles + miss_tiles(n);
    if (hipMemsetAsync(owner, 0xFF, (size_t)slots * sizeof(uint32_t), st) != hipSuccess) return HALO_E_HIP;
    const bool wan = dir == HALO_FLOW_NAT_WAN;
    if (wan && compact)
        launch_collect<HALO_FLOW_NAT_WAN, true>(d_records, d_verdict, d_select, n, nat_type, slots, d_items, cap, d_count, d_pos,
                                                owner, tiles, link, st);
    else if (wan)
        launch_collect<HALO_FLOW_NAT_WAN, false>(d_records, d_verdict, d_select, n, nat_type, slots, d_items, cap, d_count, d_pos,
                                                 owner, tiles, link, st);
    else if (compact)
        launch_collect<HALO_FLOW_NAT_LAN, true>(d_records, d_verdict, d_select, n, nat_type, slots, d_items, cap, d_count, d_pos,
                                                owner, tiles, link, st);
    else
        launch_collect<HALO_FLOW_NAT_LAN, false>(d_records, d_verdict, d_select, n, nat_type, slots, d_items, cap, d_count, d_pos,
                                                 owner, tiles, link, st);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

int miss_apply(uint32_t dir, const uint32_t* d_pos, uint32_t n, const halo_nat_answer_t* d_answers, uint32_t k,
               halo_tx_op_t* d_ops, uint8_t* d_verdict, uint32_t* d_ref, uint32_t* d_counts, halo_stream_t stream) {
    const int rc = check_device();
    if (rc) return rc;
    if (n == 0) return HALO_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint4* answers = reinterpret_cast<const uint4*>(d_answers);
    if (dir == HALO_FLOW_NAT_WAN)
        hipLaunchKernelGGL(nat_miss_apply_kernel<HALO_FLOW_NAT_WAN>, dim3(miss_blocks(n)), dim3(256), 0, st, d_pos, n, answers, k,
                           d_ops, d_verdict, d_ref, d_counts);
    else
        hipLaunchKernelGGL(nat_miss_apply_kernel<HALO_FLOW_NAT_LAN>, dim3(miss_blocks(n)), dim3(256), 0, st, d_pos, n, answers, k,
                           d_ops, d_verdict, d_ref, d_counts);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

}  // namespace nat
}  // namespace halo
