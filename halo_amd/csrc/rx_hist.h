// rx_hist.h — the device half of the rx kernels' status histogram: a block's counts (Hist), the
// tree of its launch's HSA queue (launch_tree) and the block's flush into it (flush_hist). The host
// half, which makes the tree sets, is rx_hist.hip; the layout both agree on is in halo_common.h.
// Device-only; gfx950 (wave64) only.
#pragma once
#include <hip/hip_runtime.h>

#include "halo_common.h"

namespace halo {
namespace {

// Per-block status histogram: OK frames are counted per lane, the rest in LDS.
struct Hist {
    uint32_t* s;  // __shared__ [HALO_RX_STATUS_COUNT]
    uint32_t ok;
    // status threads: the key word the launch queue's tree most likely has (flush_hist), loaded when
    // the block starts so that its latency hides under the frame loads instead of ending the block
    unsigned long long key;
    __device__ __forceinline__ void add(uint32_t status) {
        if (status == HALO_RX_OK) ++ok;
        else atomicAdd(&s[status], 1u);
    }
};

// The launch's HSA queue and the tree-set slot its key is looked up from first.
__device__ __forceinline__ unsigned long long launch_queue() {
    return (unsigned long long)(uintptr_t)(const void*)__builtin_amdgcn_queue_ptr();
}
__device__ __forceinline__ uint32_t tree_slot0(unsigned long long q) {
    return ((uint32_t)(q >> 6) ^ (uint32_t)(q >> 17)) & (kHistTrees - 1u);
}
__device__ __forceinline__ Hist hist_open(const RxParams& p, uint32_t* s_hist) {
    Hist h{s_hist, 0, 0};
    if (p.hist && threadIdx.x < HALO_RX_STATUS_COUNT)
        h.key = reinterpret_cast<const unsigned long long*>(p.hist)[tree_slot0(launch_queue())];
    return h;
}

// The block's counts reach the caller's counters through a two-level tree of partial histograms
// (p.hist, hist_trees) instead of device-scope atomics on the caller's 14 counters: those serialise
// at the memory side, ~10 ns each, and 16384 one-wave blocks cost 170 us on a 21 us launch (bench
// r4b). Every word of the tree is a 64-bit (arrivals << 40 | count) pair, one per status: block b
// adds (1 << 40 | its count) to status k of level-1 slot b % 1024 (16 blocks per slot for 1M
// frames), and the add that brings the arrivals to the slot's block count returns the slot's final
// count, so that thread alone moves it on — to level-2 slot (b % 1024) / 32, whose last arrival
// adds it to the caller's counter (at most 32 x 14 atomics on them per launch) — and zeroes the word
// for the next launch on the queue. Each word carries its own completion, so no fence is needed: a
// __threadfence per block (agent-scope release / acquire, L2 writeback and invalidate across the
// XCDs on gfx950) cost 0.55 ms per 1M-frame launch (bench r4i), and a separate finalize launch
// ~10 us (r4e). Every block of a kernel that counts calls this once, with the whole block.
// The tree is the one of the launch's HSA queue (halo_common.h): the words assume one launch at a
// time per tree, and the dispatch packet's barrier bit is what guarantees it.
// key0: the word at the queue's first probe slot as block thread 0 read it when the block started
// (Hist::key). A key never changes once set, so a stale copy can only read 0, and then the CAS
// (performed at memory) returns the real key.
// Called by the 64 lanes of wave 0 (every kernel that counts has blocks of whole waves, >= 64
// threads). Lane j reads probe slot k0 + j (kHistTrees == 64: every slot in one round trip); the
// first slot in probe order holding this queue's key is the tree; otherwise the slots read as free
// are claimed in probe order by lane 0, one CAS each, until one is this queue's. A queue that finds
// every key held by others (or poisoned) returns nullptr after that one round trip (16 serial probes
// before round 6).
static_assert(kHistTrees == 64, "one probe slot per lane of a wave");
__device__ __forceinline__ unsigned long long* launch_tree(uint32_t* set_u32, unsigned long long key0) {
    unsigned long long* set = reinterpret_cast<unsigned long long*>(set_u32);
    const unsigned long long q = launch_queue();
    const uint32_t k0 = tree_slot0(q), lane = threadIdx.x & 63u;
    const unsigned long long k0key =
        ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(key0 >> 32), 0, 64) << 32) |
        (uint32_t)__shfl((int)(uint32_t)key0, 0, 64);
    if (k0key == q) return set + kHistKeyWords + (uint64_t)k0 * kHistWords;  // uniform
    const unsigned long long key = set[(k0 + lane) & (kHistTrees - 1u)];
    const uint64_t mine = __ballot(key == q);
    if (mine) return set + kHistKeyWords + (uint64_t)((k0 + (uint32_t)__builtin_ctzll(mine)) & (kHistTrees - 1u)) * kHistWords;
    uint64_t free_slots = __ballot(key == 0);
    while (free_slots) {  // uniform
        const uint32_t k = (k0 + (uint32_t)__builtin_ctzll(free_slots)) & (kHistTrees - 1u);
        unsigned long long got = 0;
        if (lane == 0) {  // claim it (device scope: a native compare-and-swap, no retry loop)
            __hip_atomic_compare_exchange_strong(set + k, &got, q, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
        }
        got = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(got >> 32), 0, 64) << 32) |
              (uint32_t)__shfl((int)(uint32_t)got, 0, 64);
        if (got == 0 || got == q) return set + kHistKeyWords + (uint64_t)k * kHistWords;  // claimed now / by a sibling block
        free_slots &= free_slots - 1;  // another queue's key (our read was stale): the next free slot
    }
    return nullptr;  // every key taken by another queue, or poisoned (hist_trees: no barrier bits)
}

__device__ __forceinline__ void flush_hist(const RxParams& p, Hist& hist) {
    if (!p.hist) return;
    const uint32_t t = threadIdx.x;
    uint32_t ok = hist.ok;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) ok += __shfl_xor(ok, m, 64);
    if ((threadIdx.x & 63u) == 0 && ok) atomicAdd(&hist.s[HALO_RX_OK], ok);
    __syncthreads();
    if (t >= 64) return;
    unsigned long long* tree = launch_tree(p.hist, hist.key);  // wave 0: one probe round trip for the block
    if (t >= HALO_RX_STATUS_COUNT) return;
    const uint32_t s = blockIdx.x & (kHistSlots - 1u), g = gridDim.x;
    if (!tree) {  // no tree this launch can own alone: straight into the caller's counters
        if (hist.s[t]) atomicAdd(&p.hist_out[t], hist.s[t]);
        return;
    }
    // What it costs is a fixed tail per launch, not a per-block price (two-level tree: 1M frames
    // +2.7 us, 4M +2.4, 16M +1.4; counting, the LDS adds and the barrier alone +0.4): the last
    // block's chain of dependent round trips. Arrivals in one word with only the statuses a block saw
    // ran 0.6 us slower; one level of 64 / 256 / 1024 slots strided over the grid ran +0.3 / +1.3 / +9
    // us (their completers all finish at the end and queue on one counter, ~10 ns an add). Runs of
    // consecutive blocks complete through the launch instead. DESIGN.md §14.5.
    constexpr unsigned long long kOne = 1ull << 40, kCount = kOne - 1;
    // Tried (profiles/r05/r5zz2; in git history up to 9ac2a89), 1M x 64 B: runs of 16 +1.8-2.0 us
    // against +2.1-2.4 for the two-level tree alone; runs of 8: +5.6, of 32: +1.8-2.0
    constexpr uint32_t kHistRuns = 16;
    if (g <= kHistSlots * kHistRuns) {  // uniform
        // Grids up to 16384 blocks: slot = a run of 16 consecutive blocks. Workgroups are dispatched
        // in order, so the runs complete one after another through the launch instead of all at its
        // end, and each completer adds straight into the caller's counters (one level: the adds
        // arrive spread out, not queued on one counter at the tail).
        constexpr uint32_t R = kHistRuns;
        const uint32_t r = blockIdx.x / R;
        unsigned long long* w = tree + r * kHistStride + t;
        const unsigned long long add = kOne | hist.s[t];
        const unsigned long long now1 = atomicAdd(w, add) + add;
        if ((now1 >> 40) != (g - r * R < R ? g - r * R : R)) return;
        atomicExch(w, 0ull);
        if (now1 & kCount) atomicAdd(&p.hist_out[t], (uint32_t)(now1 & kCount));
        return;
    }
    unsigned long long* l1 = tree + s * kHistStride + t;
    unsigned long long now = atomicAdd(l1, kOne | hist.s[t]) + (kOne | hist.s[t]);
    if ((now >> 40) != g / kHistSlots + (g % kHistSlots > s)) return;
    atomicExch(l1, 0ull);
    const uint32_t used = g < kHistSlots ? g : kHistSlots, first = s & ~(kHistFan - 1u);
    unsigned long long* l2 = tree + (kHistSlots + s / kHistFan) * kHistStride + t;
    now = atomicAdd(l2, kOne | (now & kCount)) + (kOne | (now & kCount));
    if ((now >> 40) != (used - first < kHistFan ? used - first : kHistFan)) return;
    atomicExch(l2, 0ull);
    if (now & kCount) atomicAdd(&p.hist_out[t], (uint32_t)(now & kCount));
}

}  // namespace
}  // namespace halo
