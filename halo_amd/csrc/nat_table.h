// nat_table.h — the host control plane of a NATing NetIf's flow table (nat_table.cc) and the
// image of it that nat_lookup.hip uploads. Plain C++17, no HIP: nat_table.cc compiles alone with
// g++ (tools/fuzz_nat.cc drives it under ASan/UBSan) and into libhalo_rx.so.
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
#include "flow_key.h"

namespace halo {
namespace nat {

struct KeyHash {
    size_t operator()(const flowkey::Key& k) const { return (size_t)flowkey::key_hash(k); }
};
struct KeyEq {
    bool operator()(const flowkey::Key& a, const flowkey::Key& b) const {
        return a.rip == b.rip && a.rport == b.rport && a.lip == b.lip && a.lport == b.lport && a.proto == b.proto;
    }
};

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

// home slot of a key: the hash of halo_flow_hash_device, low bits
inline uint32_t home_slot(const flowkey::Key& k, uint32_t mask) { return (uint32_t)flowkey::key_hash(k) & mask; }

struct Image {
    uint32_t slots = 0;          // per index
    std::vector<Slot> index[2];  // [HALO_FLOW_NAT_LAN], [HALO_FLOW_NAT_WAN]
    std::vector<MapWord> maps;
    std::vector<uint32_t> stamps;  // by flow id, next_id entries (0 for ids no longer live)
    halo_nat_layout_stats_t stats{};
};

// The device side of a table (nat_lookup.hip); nat_table.cc reaches it only through these.
struct DeviceOps {
    int (*fold)(halo_nat_table* t);     // drain the device, merge its stamps into the host table
    int (*publish)(halo_nat_table* t);  // compile and publish a new generation
    void (*destroy)(halo_nat_table* t);
};

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
    std::atomic<void*> dev{nullptr};                 // set once by the first sync (release)
    const halo::nat::DeviceOps* dev_ops = nullptr;  // written and read under sync_mu
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
