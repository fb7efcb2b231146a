// nat_table.h — the host control plane of a NATing NetIf's flow table (nat_table.cc) and the
// image of it that nat_lookup.hip uploads. Plain C++17, no HIP: nat_table.cc compiles alone with
// g++ (tools/fuzz_nat.cc drives it under ASan/UBSan) and into libhalo_rx.so. Every extern "C" entry
// point is nat_table.cc's; the device side is reached through nat::DeviceOps, as the ARP, switch
// and return-flow tables reach theirs. Hash, placement and capacity rule are flow_table.h's.
//
// Reference state (engine/ipv4_engine.go:423-759), kept as the reference builds it:
//   NatFlowTable     lan : normalised NatFlowHash    -> flow      (ListNat / NatTableClear walk it)
//   NatWanFlowTable  wan : normalised NatWanFlowHash -> flow
//   NatPortAlloc     one used-port set per normalised remote address
//   NatPortMappingTable  a list in call order
// A flow whose LAN key a later NatAddFlow replaced (HashMap.Set overwrites) stays in the WAN index
// with its port taken, as in the reference, where nothing ever removes it.
#pragma once
#include <stdint.h>

#include <atomic>
#include <map>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "../../include/halo_rx.h"
#include "flow_table.h"

namespace halo {
namespace nat {

using flowtab::KeyEq;
using flowtab::KeyHash;

struct Flow {
    halo_nat_flow_t f;
    bool in_lan;  // still the value of its LAN key (false: replaced, reachable by its WAN key only)
};

// PortAlloc.UsePortMap over 32768..65535 as a bitmap that grows with the highest port in use
struct PortSet {
    std::vector<uint64_t> bits;
    uint32_t used = 0;
    uint32_t take();  // the lowest free port from 32768, marked used; 0 when all 32768 are taken
    void release(uint32_t port);
};

struct PortMapping {
    uint16_t wan_port;
    uint16_t lan_port;
    uint32_t lan_ip;
    uint8_t proto;
};

// One slot of a device index (32 bytes, 32-byte aligned): the whole key in the first 16 bytes.
struct alignas(32) Slot {
    uint32_t rip;
    uint32_t lip;
    uint32_t ports;  // rport | lport << 16
    uint32_t tag;    // kSlotUsed | proto; 0 = empty (ends a probe chain)
    uint32_t x_ip;   // the translation: LAN index -> WanIpAddr, WAN index -> LanHostIpAddr
    uint32_t x_port; //                               WanPort                  LanHostPort
    uint32_t id;     // flow id
    uint32_t pad;
};
static_assert(sizeof(Slot) == 32, "slot");
using flowkey::kSlotUsed;
// a port mapping as the kernels stage it in LDS (12 bytes)
struct MapWord {
    uint32_t ports;  // wan_port | lan_port << 16
    uint32_t lan_ip;
    uint32_t proto;
};

struct Image {
    uint32_t slots = 0;          // per index
    std::vector<Slot> index[2];  // [HALO_FLOW_NAT_LAN], [HALO_FLOW_NAT_WAN]
    std::vector<MapWord> maps;
    std::vector<uint32_t> stamps;  // by flow id, next_id entries (0 for ids no longer live)
    halo_nat_layout_stats_t stats{};
};

// The device side of a table (nat_lookup.hip); nat_table.cc reaches it only through these.
struct DeviceOps {
    int (*sync)(halo_nat_table* t, int device);  // t->sync_mu held, as for fold and publish
    int (*fold)(halo_nat_table* t);              // drain the device, merge its stamps into the host table
    int (*publish)(halo_nat_table* t);           // rebuild the copy after an expiry
    void (*destroy)(halo_nat_table* t);
    using Lookup = int (*)(const halo_nat_table* t, const void* d_records, uint32_t n, uint32_t now, const uint8_t* d_skip,
                           halo_tx_op_t* d_ops, uint8_t* d_verdict, uint32_t* d_ref, uint32_t* d_miss_count,
                           halo_stream_t stream);
    Lookup lookup_wan, lookup_lan, lookup_wan_compact, lookup_lan_compact;  // compact: d_records are halo_rx_record16_t
    int (*quote)(const halo_nat_table* t, const halo_rx_result_t* d_quote_records, uint32_t n, halo_tx_deep_nat_t* d_nat,
                 halo_stream_t stream);
    // the miss path (nat_miss.hip); arguments checked by nat_table.cc, `slots` from miss_slots
    using Collect = int (*)(const halo_nat_table* t, uint32_t dir, const void* d_records, const uint8_t* d_verdict,
                            const uint8_t* d_select, uint32_t n, uint32_t slots, halo_nat_miss_item_t* d_items, uint32_t cap,
                            uint32_t* d_count, uint32_t* d_pos, void* d_workspace, halo_stream_t stream);
    Collect collect, collect_compact;
    int (*apply)(uint32_t dir, const uint32_t* d_pos, uint32_t n, const halo_nat_answer_t* d_answers, uint32_t k,
                 halo_tx_op_t* d_ops, uint8_t* d_verdict, uint32_t* d_ref, uint32_t* d_counts, halo_stream_t stream);
};
// The miss path's kernels (nat_miss.hip); nat_lookup.hip puts them behind DeviceOps once it has
// seen a published device copy.
int miss_collect(uint32_t dir, uint32_t nat_type, bool compact, const void* d_records, const uint8_t* d_verdict,
                 const uint8_t* d_select, uint32_t n, uint32_t slots, halo_nat_miss_item_t* d_items, uint32_t cap,
                 uint32_t* d_count, uint32_t* d_pos, void* d_workspace, halo_stream_t stream);
int miss_apply(uint32_t dir, const uint32_t* d_pos, uint32_t n, const halo_nat_answer_t* d_answers, uint32_t k,
               halo_tx_op_t* d_ops, uint8_t* d_verdict, uint32_t* d_ref, uint32_t* d_counts, halo_stream_t stream);

// The collect's geometry, shared by the workspace size and the launch: 256-record tiles; the
// scratch table's slot count (0: out of range); and the workspace as u32 owner[slots], then
// tiles[n_tiles], then link[n].
constexpr uint32_t kMissTile = 256;
inline uint32_t miss_slots(uint32_t n, uint32_t scratch_log2) {
    if (scratch_log2 > 31) return 0;
    if (scratch_log2) return 1u << scratch_log2;
    if (n > (1u << 30)) return 0;
    uint32_t s = 16;
    while (s < 2 * n) s <<= 1;
    return s;
}
inline uint32_t miss_tiles(uint32_t n) { return n / kMissTile + (n % kMissTile ? 1u : 0u); }
// Defined by nat_lookup.hip; absent (null) in a host-only build, where the device calls are HALO_E_NODEV.
const DeviceOps* device_ops() __attribute__((weak));

}  // namespace nat
}  // namespace halo

struct halo_nat_table {
    halo_nat_config_t cfg{};
    mutable std::mutex mu;  // NetIf.NatLock
    std::map<uint32_t, halo::nat::Flow> flows;  // by flow id (ascending = creation order)
    std::unordered_map<halo::flowkey::Key, halo::nat::Flow*, halo::nat::KeyHash, halo::nat::KeyEq> lan, wan;
    std::unordered_map<uint32_t, halo::nat::PortSet> ports;  // NatPortAlloc
    std::vector<halo::nat::PortMapping> maps;
    uint32_t next_id = 0;
    uint32_t n_lan = 0;  // flows with in_lan (== lan.size())
    // device copy (nat_lookup.hip)
    std::mutex sync_mu;  // one sync / expire at a time
    std::atomic<void*> dev{nullptr};  // set once by the first sync (release)
};

namespace halo {
namespace nat {
// Build the image a sync uploads (takes t.mu). with_stamps = false leaves Image::stamps empty.
// HALO_E_RANGE when an index does not fit the forced slot count.
int compile(const halo_nat_table& t, Image* out, bool with_stamps);
// Merge device stamps (dev[id] for id < n) into the live flows: the later in serial-number order.
void merge_stamps(halo_nat_table& t, const uint32_t* dev, uint32_t n);
}  // namespace nat
}  // namespace halo
