// switch_fwd.hip — the device mode of the L2 switch (include/halo_rx.h, "L2 switch") on gfx950:
// SwitchPort.RxEthernet / HandleEthernet (engine/ethernet_engine.go:58-114) over a batch of frames
// from one ingress port, with the reference's one-frame-at-a-time order reproduced by the closed
// form of DESIGN.md "L2 switch":
//   first[m]  = the lowest index of a learnable frame with source m
//   the MACs with first[m] defined that the table does not hold are admitted in ascending
//   first[m] order while room lasts; frame i is TABLE_FULL iff its source is neither held nor
//   admitted; a destination d resolves to the ingress port when first[d] <= i and d is held or
//   admitted, else to the port the table held for it BEFORE the call, else the frame floods.
//
// State in HBM: the MAC table — a power-of-two array of 16-byte slots {used | mac, port,
// CreateTime}, linear probing from mac_hash, no tombstones (an expiry tick rebuilds the table into
// its second generation) — the entry count, and a per-call scratch set of the batch's source MACs
// (32-byte entries, at least 2 * max_batch of them). A scratch key carries the call's 16-bit epoch
// in its top bits, so entries of earlier calls read as empty and the set is cleared only when the
// epoch wraps (every 65535 calls; halo_switch_debug_set_epoch moves a switch next to the wrap for tests).
//
// Five launches per call, on the caller's stream, one lane per frame:
//   learn   reads bytes 0..15 of each frame once, stashes {dst, len, class} (8 B) per frame, claims
//           the source's scratch entry with a 64-bit CAS and folds the frame index into first[m]
//           with a 64-bit atomicMax of (epoch << 32 | ~i)
//   probe   the frame that owns first[m] probes the table: held (slot, old port) or new; new flags
//           are counted per 256-frame tile
//   scan    one workgroup: exclusive scan of the tile counts, room = capacity - entries,
//           entries += min(new, room)
//   admit   tile-local scan of the new flags -> admission rank; admitted owners insert (CAS on an
//           empty key), owners of held MACs refresh (port, now)
//   resolve every frame: verdict from the scratch entries of its source and destination, or from
//           the table where the destination was no source of this batch; 4-byte result; the six
//           verdict counters go through LDS and one atomic per counter and workgroup
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "device_table.h"
#include "switch_table.h"
#include "tile_scan.h"

namespace halo {
namespace {

using sw::kMacMask;
using sw::kUsed;
using sw::Slot;

struct alignas(32) Scratch {
    uint64_t key;    // epoch << 48 | mac; another epoch = empty
    uint64_t first;  // epoch << 32 | ~(lowest frame index with this source)
    uint32_t info;   // kHeld | kAdmitted | old port << 8, written by the owner
    uint32_t aux;    // held: the MAC's table slot
    uint64_t pad;
};
static_assert(sizeof(Scratch) == 32, "scratch");
constexpr uint32_t kHeld = 1u, kAdmitted = 2u;
// per-frame source reference: the scratch entry, or kNoSlot for a frame that learns nothing
constexpr uint32_t kNoSlot = 0x3FFFFFFFu, kSlotBits = 0x3FFFFFFFu, kOwner = 1u << 31, kNew = 1u << 30;
constexpr uint32_t kLearn = 7u;  // stash class of a frame that passed ParseEthFrm and the source check
constexpr uint32_t kTile = 256;  // frames per workgroup = the tile of the admission scan

struct State {  // device memory
    uint32_t entries;  // MACs in the table
    uint32_t room;     // capacity - entries at the start of the call in flight
    uint32_t survivors;
    uint32_t pad;
};

struct View {  // kernel parameters of one call
    Slot* table;
    Scratch* scratch;
    State* state;
    uint64_t* stash;  // per frame: dst | len << 48 | class << 60 (len 0 for an ETH_LEN frame)
    uint32_t* sref;   // per frame: source reference
    uint32_t* tiles;  // per tile: new-MAC count, then its exclusive prefix
    uint32_t mask;    // table slots - 1
    uint32_t smask;   // scratch entries - 1
    uint32_t epoch;   // 1..65535
    uint32_t capacity;
    uint32_t port, now, n;
};

struct SwitchDevice {
    Slot* gen[2] = {nullptr, nullptr};
    int active = 0;
    Scratch* scratch = nullptr;
    State* state = nullptr;
    uint64_t* stash = nullptr;
    uint32_t* sref = nullptr;
    uint32_t* tiles = nullptr;
    uint32_t scratch_entries = 0;
    uint32_t epoch = 0;  // of the last call; 1..65535 once a call was made
    bool failed = false;  // a HIP call failed part-way: the device state is unknown
    int device = -1;
};

// The table slot holding `mac`, or -1 when its probe chain ends first.
__device__ __forceinline__ int64_t table_find(const Slot* __restrict__ tab, uint32_t mask, uint64_t mac, uint32_t* port) {
    const uint64_t want = kUsed | mac;
    uint32_t s = sw::mac_hash(mac) & mask;
    for (uint32_t step = 0; step <= mask; ++step) {  // bounded: entries < slots, and a full table cannot spin
        const uint4 e = *reinterpret_cast<const uint4*>(tab + s);
        const uint64_t key = (uint64_t)e.y << 32 | e.x;
        if (key == 0) return -1;
        if (key == want) {
            *port = e.z;
            return s;
        }
        s = (s + 1) & mask;
    }
    return -1;
}

__global__ void __launch_bounds__(kTile) sw_learn_kernel(const View v, const uint8_t* __restrict__ bytes,
                                                         const uint32_t* __restrict__ offsets_dw,
                                                         const uint16_t* __restrict__ lens) {
    const uint32_t i = blockIdx.x * kTile + threadIdx.x;
    if (i >= v.n) return;
    const uint32_t len = lens[i];
    uint32_t cls = HALO_SW_V_ETH_LEN, sref = kNoSlot;
    uint32_t slen = 0;  // the stash has 12 bits for it: only a length ParseEthFrm accepts (<= 1514) is kept
    uint64_t dst = 0;
    if (len >= 42u && len <= 1514u) {  // 16 bytes lie inside a frame of >= 42
        slen = len;
        const uint32_t* p = reinterpret_cast<const uint32_t*>(bytes + 4ull * offsets_dw[i]);
        const uint32_t w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3];
        dst = (uint64_t)(w1 & 0xFFFFu) << 32 | w0;
        const uint64_t src = (uint64_t)w2 << 16 | (w1 >> 16);
        const uint32_t et = (w3 & 0xFFu) << 8 | ((w3 >> 8) & 0xFFu);
        if (!sw::ethertype_known(et)) {
            cls = HALO_SW_V_ETH_TYPE;
        } else if (src & 1u) {
            cls = HALO_SW_V_SRC_MCAST;
        } else {
            cls = kLearn;
            const uint64_t mine = (uint64_t)v.epoch << 48 | src;
            uint32_t s = sw::mac_hash(src) & v.smask;
            // at most n <= entries / 2 keys of this epoch exist, so an entry of another epoch is met
            for (uint32_t step = 0; step <= v.smask; ++step) {
                uint64_t k = __hip_atomic_load(&v.scratch[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (k != mine && (uint32_t)(k >> 48) != v.epoch) {
                    const uint64_t old = atomicCAS(reinterpret_cast<unsigned long long*>(&v.scratch[s].key), k, mine);
                    k = old == k ? mine : old;  // ours now, or whoever claimed it in this epoch
                }
                if (k == mine) break;
                s = (s + 1) & v.smask;
            }
            // first[m] only grows within a call, so a frame that reads a value at or above its own has
            // nothing to add: on a batch of few MACs almost every frame stops here
            const uint64_t tag = (uint64_t)v.epoch << 32 | (uint32_t)~i;
            if (__hip_atomic_load(&v.scratch[s].first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < tag)
                atomicMax(reinterpret_cast<unsigned long long*>(&v.scratch[s].first), tag);
            sref = s;
        }
    }
    v.stash[i] = dst | (uint64_t)slen << 48 | (uint64_t)cls << 60;
    v.sref[i] = sref;
}

__global__ void __launch_bounds__(kTile) sw_probe_kernel(const View v) {
    const uint32_t i = blockIdx.x * kTile + threadIdx.x;
    tile_count(v.tiles, [&] {
        bool is_new = false;
        if (i < v.n) {
            const uint32_t s = v.sref[i];
            if (s != kNoSlot) {
                Scratch* e = v.scratch + s;
                if ((uint32_t)e->first == (uint32_t)~i) {  // this frame owns first[m]
                    uint32_t port = 0;
                    const int64_t slot = table_find(v.table, v.mask, e->key & kMacMask, &port);
                    is_new = slot < 0;
                    e->info = is_new ? 0u : (kHeld | (port & 0xFFu) << 8);
                    e->aux = is_new ? 0u : (uint32_t)slot;
                    v.sref[i] = s | kOwner | (is_new ? kNew : 0u);
                }
            }
        }
        return is_new;
    });
}

// One workgroup: tiles[t] becomes the number of new MACs in the tiles before t.
__global__ void __launch_bounds__(256) sw_scan_kernel(const View v, uint32_t n_tiles) {
    const uint32_t fresh = scan_tiles(v.tiles, n_tiles);
    if (threadIdx.x == 0) {
        const uint32_t room = v.capacity - v.state->entries;
        v.state->room = room;
        v.state->entries += fresh < room ? fresh : room;
    }
}

__global__ void __launch_bounds__(kTile) sw_admit_kernel(const View v) {
    const uint32_t i = blockIdx.x * kTile + threadIdx.x;
    const uint32_t r = i < v.n ? v.sref[i] : kNoSlot;
    const bool owner = r != kNoSlot && (r & kOwner), is_new = owner && (r & kNew);
    const uint64_t votes = tile_votes<kTile>(is_new);
    if (!owner) return;
    Scratch* e = v.scratch + (r & kSlotBits);
    const uint2 val = make_uint2(v.port, v.now);  // :92-94
    if (!is_new) {
        *reinterpret_cast<uint2*>(&v.table[e->aux].port) = val;
        return;
    }
    const uint32_t rank = tile_rank<kTile>(votes, v.tiles[blockIdx.x]);
    if (rank >= v.state->room) return;  // MallocType fails from here on (:79-83); info stays 0
    const uint64_t mac = e->key & kMacMask;
    uint32_t s = sw::mac_hash(mac) & v.mask;
    for (uint32_t step = 0; step <= v.mask; ++step) {  // entries <= capacity < slots: an empty slot exists
        if (atomicCAS(reinterpret_cast<unsigned long long*>(&v.table[s].key), 0ull, kUsed | mac) == 0ull) {
            *reinterpret_cast<uint2*>(&v.table[s].port) = val;
            e->info = kAdmitted;
            return;
        }
        s = (s + 1) & v.mask;
    }
}

__global__ void __launch_bounds__(kTile) sw_resolve_kernel(const View v, halo_sw_result_t* __restrict__ results,
                                                           uint32_t* counts) {
    __shared__ uint32_t s_counts[HALO_SW_V_COUNT];
    if (threadIdx.x < HALO_SW_V_COUNT) s_counts[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    // whole workgroups iterate together, so every ballot sees every lane of its wave
    for (uint32_t base = blockIdx.x * kTile; base < v.n; base += gridDim.x * kTile) {
        const uint32_t i = base + threadIdx.x;
        uint32_t verdict = HALO_SW_V_COUNT;  // no frame
        if (i < v.n) {
            const uint64_t st = v.stash[i];
            const uint32_t cls = (uint32_t)(st >> 60), len = (uint32_t)(st >> 48) & 0x7FFu;
            const uint64_t dst = st & kMacMask;
            uint32_t out_port = 0xFFu;
            if (cls != kLearn) {
                verdict = cls;
            } else if (!(v.scratch[v.sref[i] & kSlotBits].info & (kHeld | kAdmitted))) {
                verdict = HALO_SW_V_TABLE_FULL;
            } else {
                verdict = HALO_SW_V_FLOOD;
                if (!(dst & 1u)) {  // a group address is never learned (:71), so it is in neither set
                    const uint64_t want = (uint64_t)v.epoch << 48 | dst;
                    uint32_t s = sw::mac_hash(dst) & v.smask;
                    bool in_batch = false;
                    for (uint32_t step = 0; step <= v.smask; ++step) {
                        const uint64_t k = v.scratch[s].key;
                        if (k == want) {
                            in_batch = true;
                            break;
                        }
                        if ((uint32_t)(k >> 48) != v.epoch) break;
                        s = (s + 1) & v.smask;
                    }
                    if (in_batch) {
                        const Scratch* e = v.scratch + s;
                        const uint32_t info = e->info, first = ~(uint32_t)e->first;
                        if (first <= i && (info & (kHeld | kAdmitted))) {
                            verdict = HALO_SW_V_UNICAST, out_port = v.port;
                        } else if (info & kHeld) {
                            verdict = HALO_SW_V_UNICAST, out_port = (info >> 8) & 0xFFu;  // its port before the call
                        }
                    } else {
                        uint32_t port = 0;
                        if (table_find(v.table, v.mask, dst, &port) >= 0) verdict = HALO_SW_V_UNICAST, out_port = port & 0xFFu;
                    }
                }
            }
            const uint32_t tx = verdict >= HALO_SW_V_UNICAST ? (len < 60u ? 60u : len) : 0u;
            reinterpret_cast<uint32_t*>(results)[i] = verdict | out_port << 8 | tx << 16;
        }
        if (counts) {
            for (uint32_t k = 0; k < HALO_SW_V_COUNT; ++k) {
                const uint32_t c = (uint32_t)__popcll(__ballot(verdict == k));
                if (lane == k && c) atomicAdd(&s_counts[k], c);
            }
        }
    }
    if (counts) {
        __syncthreads();
        if (threadIdx.x < HALO_SW_V_COUNT && s_counts[threadIdx.x]) atomicAdd(counts + threadIdx.x, s_counts[threadIdx.x]);
    }
}

// An expiry tick: the survivors of `from` go into the zeroed `to`.
__global__ void __launch_bounds__(256) sw_rebuild_kernel(const Slot* __restrict__ from, Slot* to, uint32_t mask, uint32_t now,
                                                         State* state) {
    uint32_t kept = 0;  // wave-uniform
    for (uint32_t base = blockIdx.x * 256u + (threadIdx.x & ~63u); base <= mask; base += gridDim.x * 256u) {
        const uint32_t k = base + (threadIdx.x & 63u);
        bool keep = false;
        if (k <= mask) {
            const uint4 e = *reinterpret_cast<const uint4*>(from + k);
            const uint64_t key = (uint64_t)e.y << 32 | e.x;
            keep = key != 0 && !sw::expired(now, e.w);
            if (keep) {
                uint32_t s = sw::mac_hash(key & kMacMask) & mask;
                for (uint32_t step = 0; step <= mask; ++step) {
                    if (atomicCAS(reinterpret_cast<unsigned long long*>(&to[s].key), 0ull, key) == 0ull) {
                        *reinterpret_cast<uint2*>(&to[s].port) = make_uint2(e.z, e.w);
                        break;
                    }
                    s = (s + 1) & mask;
                }
            }
        }
        kept += (uint32_t)__popcll(__ballot(keep));
    }
    if ((threadIdx.x & 63u) == 0 && kept) atomicAdd(&state->survivors, kept);
}

SwitchDevice* dev_of(const halo_switch* s) { return static_cast<SwitchDevice*>(s->dev); }

void free_all(SwitchDevice* d) {
    for (auto* p : d->gen)
        if (p) (void)hipFree(p);
    if (d->scratch) (void)hipFree(d->scratch);
    if (d->state) (void)hipFree(d->state);
    if (d->stash) (void)hipFree(d->stash);
    if (d->sref) (void)hipFree(d->sref);
    if (d->tiles) (void)hipFree(d->tiles);
}

int ops_create(halo_switch* s) {
    int rc = device_present(s->cfg.device);
    if (rc) return rc;
    DeviceScope ds(s->cfg.device);
    if ((rc = check_device())) return rc;
    SwitchDevice* d = new (std::nothrow) SwitchDevice;
    if (!d) return HALO_E_NOMEM;
    d->device = s->cfg.device;
    uint64_t entries = 64;
    while (entries < 2ull * s->cfg.max_batch) entries <<= 1;
    d->scratch_entries = (uint32_t)entries;
    const size_t tab = (size_t)s->slots * sizeof(Slot), n_tiles = (s->cfg.max_batch + kTile - 1) / kTile;
    const bool ok = hipMalloc(&d->gen[0], tab) == hipSuccess && hipMalloc(&d->gen[1], tab) == hipSuccess &&
                    hipMalloc(&d->scratch, entries * sizeof(Scratch)) == hipSuccess &&
                    hipMalloc(&d->state, sizeof(State)) == hipSuccess &&
                    hipMalloc(&d->stash, (size_t)s->cfg.max_batch * sizeof(uint64_t)) == hipSuccess &&
                    hipMalloc(&d->sref, (size_t)s->cfg.max_batch * sizeof(uint32_t)) == hipSuccess &&
                    hipMalloc(&d->tiles, n_tiles * sizeof(uint32_t)) == hipSuccess;
    if (!ok) rc = HALO_E_NOMEM;
    if (!rc && (hipMemset(d->gen[0], 0, tab) != hipSuccess || hipMemset(d->scratch, 0, entries * sizeof(Scratch)) != hipSuccess ||
                hipMemset(d->state, 0, sizeof(State)) != hipSuccess || hipDeviceSynchronize() != hipSuccess))
        rc = HALO_E_HIP;
    if (rc) {
        (void)hipGetLastError();
        free_all(d);
        delete d;
        return rc;
    }
    s->dev = d;
    return HALO_OK;
}

void ops_destroy(halo_switch* s) {
    SwitchDevice* d = dev_of(s);
    if (!d) return;
    {
        DeviceScope ds(d->device);
        ParkResidents park(d->device);  // through the frees: hipFree waits for every kernel
        (void)drain_device(d->device);  // no call may still use the table or the scratch set
        free_all(d);
    }
    delete d;
    s->dev = nullptr;
}

// A HIP call failed after the call had begun to change the device state (the epoch, a memset, a
// half-built generation): the switch answers HALO_E_HIP from now on and can only be destroyed.
int fail(SwitchDevice* d) {
    (void)hipGetLastError();
    d->failed = true;
    return HALO_E_HIP;
}

int ops_forward(halo_switch* s, uint32_t port, const uint8_t* d_bytes, const uint32_t* d_offsets_dw, const uint16_t* d_lens,
                uint32_t n, uint32_t now, halo_sw_result_t* d_results, uint32_t* d_counts, halo_stream_t stream) {
    SwitchDevice* d = dev_of(s);
    DeviceScope ds(d->device);
    const int rc = check_device();
    if (rc) return rc;
    if (d->failed) return HALO_E_HIP;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (d->epoch == 0xFFFFu) {  // the epoch wraps: no entry of an earlier call may read as current
        if (hipMemsetAsync(d->scratch, 0, (size_t)d->scratch_entries * sizeof(Scratch), st) != hipSuccess) return fail(d);
        d->epoch = 0;
    }
    ++d->epoch;
    // the scratch set in use is sized by this call: at least 2 n entries, so short calls stay in cache
    uint32_t entries = 64;
    while (entries < 2 * n) entries <<= 1;
    const View v = {d->gen[d->active], d->scratch, d->state, d->stash, d->sref, d->tiles, s->slots - 1, entries - 1,
                    d->epoch,          s->cfg.capacity, port,  now,      n};
    const uint32_t n_tiles = (n + kTile - 1) / kTile;
    hipLaunchKernelGGL(sw_learn_kernel, dim3(n_tiles), dim3(kTile), 0, st, v, d_bytes, d_offsets_dw, d_lens);
    hipLaunchKernelGGL(sw_probe_kernel, dim3(n_tiles), dim3(kTile), 0, st, v);
    hipLaunchKernelGGL(sw_scan_kernel, dim3(1), dim3(256), 0, st, v, n_tiles);
    hipLaunchKernelGGL(sw_admit_kernel, dim3(n_tiles), dim3(kTile), 0, st, v);
    hipLaunchKernelGGL(sw_resolve_kernel, dim3(n_tiles < 2048u ? n_tiles : 2048u), dim3(kTile), 0, st, v, d_results, d_counts);
    return hipGetLastError() == hipSuccess ? HALO_OK : fail(d);
}

int ops_expire(halo_switch* s, uint32_t now, uint32_t* n_removed) {
    SwitchDevice* d = dev_of(s);
    DeviceScope ds(d->device);
    ParkResidents park(d->device);
    if (d->failed) return HALO_E_HIP;
    if (drain_device(d->device) != HALO_OK) return fail(d);  // every earlier forward has landed
    State before{}, after{};
    Slot* from = d->gen[d->active];
    Slot* to = d->gen[1 - d->active];
    const uint32_t blocks = s->slots / 256u ? (s->slots / 256u < 2048u ? s->slots / 256u : 2048u) : 1u;
    if (hipMemcpy(&before, d->state, sizeof before, hipMemcpyDeviceToHost) != hipSuccess) return fail(d);
    if (hipMemsetAsync(to, 0, (size_t)s->slots * sizeof(Slot), nullptr) != hipSuccess ||
        hipMemsetAsync(&d->state->survivors, 0, sizeof(uint32_t), nullptr) != hipSuccess)
        return fail(d);
    hipLaunchKernelGGL(sw_rebuild_kernel, dim3(blocks), dim3(256), 0, nullptr, from, to, s->slots - 1, now, d->state);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(d);
    if (hipMemcpy(&after, d->state, sizeof after, hipMemcpyDeviceToHost) != hipSuccess) return fail(d);
    if (hipMemcpy(&d->state->entries, &after.survivors, sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess)
        return fail(d);
    d->active = 1 - d->active;
    if (n_removed) *n_removed = before.entries - after.survivors;
    return HALO_OK;
}

int ops_snapshot(halo_switch* s, std::vector<Slot>* out) {
    SwitchDevice* d = dev_of(s);
    DeviceScope ds(d->device);
    ParkResidents park(d->device);
    if (d->failed || drain_device(d->device) != HALO_OK) return HALO_E_HIP;
    out->resize(s->slots);
    if (hipMemcpy(out->data(), d->gen[d->active], (size_t)s->slots * sizeof(Slot), hipMemcpyDeviceToHost) != hipSuccess)
        return HALO_E_HIP;
    return HALO_OK;
}

int ops_set_epoch(halo_switch* s, uint32_t epoch) {
    SwitchDevice* d = dev_of(s);
    if (epoch > 0xFFFFu) return HALO_E_INVAL;
    DeviceScope ds(d->device);
    ParkResidents park(d->device);
    // entries of ANY earlier epoch may be in the set, so it is cleared, as at a wrap
    if (d->failed || drain_device(d->device) != HALO_OK) return HALO_E_HIP;
    if (hipMemset(d->scratch, 0, (size_t)d->scratch_entries * sizeof(Scratch)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(d);
    d->epoch = epoch;
    return HALO_OK;
}

const sw::DeviceOps kDeviceOps = {ops_create, ops_destroy, ops_forward, ops_expire, ops_snapshot, ops_set_epoch};

}  // namespace

namespace sw {
const DeviceOps* device_ops() { return &kDeviceOps; }
}  // namespace sw
}  // namespace halo
