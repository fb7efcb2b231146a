// pmflow_table.h — the port-mapping return-flow table (include/halo_rx.h, "port-mapping return
// flows"): the host control plane (pmflow_table.cc) and the slot layout the device side
// (pmflow_fwd.hip) shares with the host compile. Plain C++17, no HIP: pmflow_table.cc compiles
// alone with g++ (tools/fuzz_pmflow.cc drives it under ASan/UBSan) and into libhalo_rx.so. Hash,
// placement, capacity rule and stamp merge are flow_table.h's, shared with the NAT flow table.
//
// Reference state (engine/ipv4_engine.go:489-516, engine/engine.go): Router.NatPortMappingFlowTable,
// NatFlowHash -> NatPortMappingFlow {WanNetIf, WanPort, LastAliveTime}, every flow allocated from
// the Router's StaticAllocator. NetIf names are indices here, as in the ARP cache.
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
namespace pmflow {

using flowtab::KeyEq;
using flowtab::KeyHash;

struct Flow {
    flowkey::Key key;
    uint32_t wan_netif, wan_port, last_alive, id;
};

// One slot of the device table (32 bytes, 32-byte aligned): the whole key in the first 16 bytes,
// the layout of the NAT flow table's slots.
struct alignas(32) Slot {
    uint32_t rip;
    uint32_t lip;
    uint32_t ports;  // rport | lport << 16
    uint32_t tag;    // kSlotUsed | proto; 0 = empty (ends a probe chain)
    uint32_t wan_netif;
    uint32_t wan_port;
    uint32_t id;
    uint32_t pad;
};
static_assert(sizeof(Slot) == 32, "slot");
using flowkey::kSlotUsed;

// A NetIf as the kernels read it (16 bytes)
struct alignas(16) NetIfWord {
    uint32_t ip;
    uint32_t nat_enable;
    uint32_t gateway;
    uint32_t pad;
};

// halo_pmflow_record_device's count / scan / scatter: frames per workgroup, as arp_fwd.hip's gather
// has them (the scan's pass is tile_scan.h's).
constexpr uint32_t kRecordTile = 256;

struct Image {
    std::vector<Slot> slots;
    std::vector<uint32_t> stamps;  // by flow id, next_id entries (0 for ids no longer live)
    halo_pmflow_layout_stats_t stats{};
    uint64_t version = 0;  // halo_pmflow_table::version the image was compiled from
};

// The device side of a table (pmflow_fwd.hip); pmflow_table.cc reaches it only through these.
struct DeviceOps {
    int (*sync)(halo_pmflow_table* t, const halo_route_table_t* routes, int device);
    int (*fold)(halo_pmflow_table* t);     // drain the device, merge its stamps; t->sync_mu held
    int (*publish)(halo_pmflow_table* t);  // rebuild the copy after an expiry; t->sync_mu held
    void (*destroy)(halo_pmflow_table* t);
    int (*lookup)(const halo_pmflow_table* t, const halo_rx_result_t* d_records, uint32_t n, uint32_t now,
                  const uint32_t* d_route_ids, const uint8_t* d_select, halo_tx_op_t* d_ops, halo_pmflow_via_t* d_via,
                  uint8_t* d_hit, uint32_t* d_counts, halo_stream_t stream);
    int (*record)(const halo_pmflow_table* t, uint32_t in_netif, const halo_rx_result_t* d_records,
                  const uint8_t* d_wan_verdict, const halo_tx_op_t* d_ops, const halo_arp_result_t* d_arp_results,
                  uint32_t n, uint32_t now, halo_pmflow_item_t* d_items, uint32_t cap, uint32_t* d_count,
                  void* d_workspace, halo_stream_t stream);
    int (*arp_drop)(halo_arp_result_t* d_results, const uint32_t* d_index, uint32_t k, halo_stream_t stream);
};
// Defined by pmflow_fwd.hip; absent (null) in a host-only build, where the device calls are HALO_E_NODEV.
const DeviceOps* device_ops() __attribute__((weak));

}  // namespace pmflow
}  // namespace halo

struct halo_pmflow_table {
    halo_pmflow_config_t cfg{};
    mutable std::mutex mu;  // Router.NatPortMappingFlowLock
    std::map<uint32_t, halo::pmflow::Flow> flows;  // by flow id (ascending = creation order: the compile order)
    std::unordered_map<halo::flowkey::Key, halo::pmflow::Flow*, halo::pmflow::KeyHash, halo::pmflow::KeyEq> index;
    uint32_t next_id = 0;
    uint64_t version = 1;         // bumped by every insert, changed value and removal
    uint64_t synced_version = 0;  // of the published device copy (0: none)
    // device copy (pmflow_fwd.hip)
    std::mutex sync_mu;  // one sync / expire at a time
    std::atomic<void*> dev{nullptr};  // set once by the first sync (release)
};

namespace halo {
namespace pmflow {
// Build the image a sync uploads (takes t.mu). with_stamps = false leaves Image::stamps empty.
// HALO_E_RANGE when the flows do not fit the forced slot count.
int compile(const halo_pmflow_table& t, Image* out, bool with_stamps);
// Merge device stamps (dev[id] for id < n) into the live flows: the later in serial-number order.
void merge_stamps(halo_pmflow_table& t, const uint32_t* dev, uint32_t n);
// The device copy now equals version `v` of the host table (takes t.mu).
void mark_synced(halo_pmflow_table& t, uint64_t v);
}  // namespace pmflow
}  // namespace halo
