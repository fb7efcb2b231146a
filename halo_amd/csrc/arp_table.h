// arp_table.h — the ARP neighbour cache (include/halo_rx.h, "ARP neighbour cache"): the host
// control plane (arp_table.cc) and the slot layout and hash the device side (arp_fwd.hip) shares
// with the host compile. Plain C++17, no HIP: arp_table.cc compiles alone with g++
// (tools/fuzz_arp.cc drives it under ASan/UBSan) and into libhalo_rx.so.
//
// Reference state (engine/arp_engine.go): per NetIf an ArpCacheTable, IpAddrHash -> ArpCache
// {IpAddr, MacAddr, ExpTime}, every entry allocated from the Router's StaticAllocator. One table
// here holds all NetIfs of a Router, keyed by (netif, ip).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HALO_ARP_FN __host__ __device__ __forceinline__
#else
#define HALO_ARP_FN inline
#endif
#include <stdint.h>

#include <atomic>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/halo_rx.h"

namespace halo {
namespace arp {

// One slot of the device table (16 bytes, one load per probe): tag = kUsed | netif, 0 = empty
// (ends a probe chain).
struct alignas(16) Slot {
    uint32_t ip;
    uint32_t tag;
    uint32_t mac_lo;  // MAC bytes 0..3, little-endian packed
    uint32_t mac_hi;  // MAC bytes 4..5
};
static_assert(sizeof(Slot) == 16, "slot");
constexpr uint32_t kUsed = 0x80000000u;

// A NetIf as the kernels read it (16 bytes)
struct alignas(16) NetIfWord {
    uint32_t ip;
    uint32_t mac_lo;
    uint32_t mac_hi;
    uint32_t nat_enable;
};
// A route as the encap kernel reads it (8 bytes), indexed by route id
struct alignas(8) RouteWord {
    uint32_t next_hop;
    uint32_t netif;
};

// Home slot of a key: a splitmix64 finaliser of (netif << 32 | ip). Internal, not observable.
HALO_ARP_FN uint32_t key_hash(uint32_t netif, uint32_t ip) {
    uint64_t z = ((uint64_t)netif << 32 | ip) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)(z ^ (z >> 31));
}

// ArpTableClear's and ArpTableRefresh's tests, with Go's wrapping u32 arithmetic
HALO_ARP_FN bool expired(uint32_t now, uint32_t exp_time) { return now > exp_time; }
HALO_ARP_FN bool refresh_due(uint32_t now, uint32_t exp_time) { return now > (uint32_t)(exp_time - HALO_ARP_REFRESH_AHEAD); }

constexpr uint32_t kGatherTile = 256;  // frames per workgroup = the tile of the gather's scan

struct HostEntry {
    uint8_t mac[6];
    uint32_t exp_time;
};

struct Image {
    std::vector<Slot> slots;
    halo_arp_layout_stats_t stats{};
    uint64_t version = 0;  // halo_arp_table::version the image was compiled from
};

// The device side of a table (arp_fwd.hip); arp_table.cc reaches it only through these.
struct DeviceOps {
    int (*sync)(halo_arp_table* t, const halo_route_table_t* routes, int device);
    int (*publish)(halo_arp_table* t);  // rebuild the copy after an expiry; t->sync_mu held
    void (*destroy)(halo_arp_table* t);
    int (*lookup)(const halo_arp_table* t, const uint32_t* d_ips, const uint8_t* d_netifs, uint32_t netif, uint32_t n,
                  uint8_t* d_mac8, uint8_t* d_verdict, uint32_t* d_miss_count, halo_stream_t stream);
    int (*encap)(const halo_arp_table* t, uint8_t* d_bytes, const uint32_t* d_offsets_dw, const uint16_t* d_lens, uint32_t n,
                 const uint32_t* d_route_ids, uint32_t in_netif, bool tx, const uint8_t* d_select,
                 const halo_pmflow_via_t* d_via,  // forward path only (tx = false); null: no override
                 halo_arp_result_t* d_results, uint32_t* d_counts, uint32_t* d_miss_count, halo_stream_t stream);
    int (*gather)(const uint8_t* d_bytes, const uint32_t* d_offsets_dw, const uint16_t* d_lens,
                  const halo_rx_result_t* d_records, uint32_t n, uint32_t netif, halo_arp_msg_t* d_msgs, uint32_t cap,
                  uint32_t* d_count, void* d_workspace, uint64_t workspace_bytes, halo_stream_t stream);
    int (*mark)(const halo_arp_table* t, const halo_rx_result_t* d_records, uint32_t n, const uint32_t* d_route_ids,
                uint32_t in_netif, const halo_pmflow_via_t* d_via, uint8_t* d_mark, halo_stream_t stream);
};
// Defined by arp_fwd.hip; absent (null) in a host-only build, where the device calls are HALO_E_NODEV.
const DeviceOps* device_ops() __attribute__((weak));

}  // namespace arp
}  // namespace halo

struct halo_arp_table {
    halo_arp_config_t cfg{};
    uint32_t slots = 0;     // of the device table
    mutable std::mutex mu;  // NetIf.ArpLock
    std::map<uint64_t, halo::arp::HostEntry> cache;  // netif << 32 | ip (ascending: the compile order)
    uint64_t version = 1;         // bumped by every insert, MAC change and removal
    uint64_t synced_version = 0;  // of the published device copy (0: none)
    // device copy (arp_fwd.hip)
    std::mutex sync_mu;  // one sync / expire at a time
    std::atomic<void*> dev{nullptr};  // set once by the first sync (release)
};

namespace halo {
namespace arp {
// Build the image a sync uploads (takes t.mu).
void compile(const halo_arp_table& t, Image* out);
// The device copy now equals version `v` of the host table (takes t.mu).
void mark_synced(halo_arp_table& t, uint64_t v);
}  // namespace arp
}  // namespace halo
