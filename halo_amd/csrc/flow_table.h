// flow_table.h — what the host sides of the open-addressing tables share (nat_table.cc and
// pmflow_table.cc, keyed by flowkey::Key; arp_table.cc takes `place`): the std containers' hash and
// equality, the home slot, the serial-number `later`, the capacity rule, the linear-probe placement
// with its statistics and the merge of device stamps. Plain C++17, no HIP: the *_table.cc files
// compile alone with g++. flow_key.h is not the place for any of it: the kernels include that file.
#pragma once
#include <stdint.h>

#include <map>

#include "../../include/halo_rx.h"
#include "flow_key.h"

namespace halo {
namespace flowtab {

struct KeyHash {
    size_t operator()(const flowkey::Key& k) const { return (size_t)flowkey::key_hash(k); }
};
struct KeyEq {
    bool operator()(const flowkey::Key& a, const flowkey::Key& b) const {
        return a.rip == b.rip && a.rport == b.rport && a.lip == b.lip && a.lport == b.lport && a.proto == b.proto;
    }
};

// home slot of a key: the hash of halo_flow_hash_device, low bits
inline uint32_t home_slot(const flowkey::Key& k, uint32_t mask) { return (uint32_t)flowkey::key_hash(k) & mask; }

// a is later than b in serial-number order (TimeNow wraps)
inline bool later(uint32_t a, uint32_t b) { return (int32_t)(a - b) > 0; }

// Slots of an index of `entries` keys: 1 << capacity_log2 when that is forced, else the power of
// two from 16 with load <= 0.5. HALO_E_RANGE above 2^28 slots, or when a forced index would be
// full: a probe chain must end at an empty slot.
inline int capacity_slots(uint32_t capacity_log2, uint32_t entries, uint32_t* slots) {
    uint32_t log2 = capacity_log2;
    if (log2 == 0) {
        log2 = 4;
        while (log2 < 31 && (1ull << log2) < 2ull * entries) ++log2;
        if (log2 > 28) return HALO_E_RANGE;
    } else if (entries >= (1u << log2)) {
        return HALO_E_RANGE;
    }
    *slots = 1u << log2;
    return HALO_OK;
}

// Linear probing from `home`: the first empty slot (tag == 0), for the caller to fill, counted into
// the index's layout statistics. The index has an empty slot (entries < slots).
template <typename Slot>
uint32_t place(const Slot* index, uint32_t mask, uint32_t home, uint32_t* entries, uint32_t* longest_chain,
               uint32_t* wrapped) {
    uint32_t s = home, chain = 1;
    while (index[s].tag) {
        s = (s + 1) & mask;
        ++chain;
    }
    ++*entries;
    if (chain > *longest_chain) *longest_chain = chain;
    if (s < home) ++*wrapped;
    return s;
}

// Merge device stamps (dev[id] for id < n) into the flows' last_alive(flow): the later of the two.
template <typename Flow, typename LastAlive>
void merge_stamps(std::map<uint32_t, Flow>& flows, const uint32_t* dev, uint32_t n, LastAlive last_alive) {
    for (auto& kv : flows) {
        if (kv.first >= n) break;
        uint32_t& host = last_alive(kv.second);
        if (later(dev[kv.first], host)) host = dev[kv.first];
    }
}

}  // namespace flowtab
}  // namespace halo
