// switch_table.h — the L2 switch (include/halo_rx.h, "L2 switch"): configuration, flood masks and
// the host mode of halo_switch_forward (switch_table.cc), and the slot layout and hash the device
// mode (switch_fwd.hip) shares with the host-side statistics. Plain C++17, no HIP: switch_table.cc
// compiles alone with g++ (tools/fuzz_switch.cc drives it under ASan/UBSan) and into libhalo_rx.so.
//
// Reference state (engine/ethernet_engine.go:51-163): Switch.SwitchMacAddrTable, MacAddrHash ->
// SwitchMacAddr {MacAddr, NetIf, CreateTime}, allocated from the switch's StaticAllocator.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HALO_SW_FN __host__ __device__ __forceinline__
#else
#define HALO_SW_FN inline
#endif
#include <stdint.h>

#include <unordered_map>
#include <vector>

#include "../../include/halo_rx.h"

namespace halo {
namespace sw {

// A MAC as a 48-bit integer: byte 0 of the address in bits 0..7 (the little-endian load of the
// six bytes), so the multicast bit of the source is bit 0.
constexpr uint64_t kMacMask = 0xFFFFFFFFFFFFull;
constexpr uint64_t kUsed = 1ull << 63;  // set in the key of every occupied slot (MAC 0 is a MAC)

// One slot of the device table (16 bytes): key = kUsed | mac, 0 = empty (ends a probe chain).
struct alignas(16) Slot {
    uint64_t key;
    uint32_t port;
    uint32_t create_time;
};
static_assert(sizeof(Slot) == 16, "slot");

// Home slot of a MAC: a splitmix64 finaliser of the 48 bits. Internal, not observable.
HALO_SW_FN uint32_t mac_hash(uint64_t mac) {
    uint64_t z = mac + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)(z ^ (z >> 31));
}

// ParseEthFrm's EtherType switch (protocol/ethernet.go:39-50)
HALO_SW_FN bool ethertype_known(uint32_t et) { return et == 0x05DCu || et == 0x0800u || et == 0x0806u || et == 0x86DDu; }

// SwitchMacAddrClear's test, with Go's wrapping u32 add
HALO_SW_FN bool expired(uint32_t now, uint32_t create_time) { return now > (uint32_t)(create_time + HALO_SW_MAC_AGE); }

struct HostEntry {
    uint32_t port;
    uint32_t create_time;
};

// The device side of a switch (switch_fwd.hip); switch_table.cc reaches it only through these.
struct DeviceOps {
    int (*create)(halo_switch* s);  // allocates the table and the scratch set on s->cfg.device
    void (*destroy)(halo_switch* s);
    int (*forward)(halo_switch* s, uint32_t port, const uint8_t* d_bytes, const uint32_t* d_offsets_dw,
                   const uint16_t* d_lens, uint32_t n, uint32_t now, halo_sw_result_t* d_results, uint32_t* d_counts,
                   halo_stream_t stream);
    int (*expire)(halo_switch* s, uint32_t now, uint32_t* n_removed);
    // the whole slot array, after a device drain
    int (*snapshot)(halo_switch* s, std::vector<Slot>* out);
    int (*set_epoch)(halo_switch* s, uint32_t epoch);  // halo_switch_debug_set_epoch
};
// Defined by switch_fwd.hip; absent (null) in a host-only build, where device mode is HALO_E_NODEV.
const DeviceOps* device_ops() __attribute__((weak));

}  // namespace sw
}  // namespace halo

struct halo_switch {
    halo_switch_config_t cfg{};
    uint32_t slots = 0;                 // of the device table (reported in host mode too)
    uint64_t flood[HALO_SW_MAX_PORTS];  // per ingress port
    std::unordered_map<uint64_t, halo::sw::HostEntry> table;  // host mode
    void* dev = nullptr;                                       // device mode (switch_fwd.hip)
    const halo::sw::DeviceOps* ops = nullptr;
};
