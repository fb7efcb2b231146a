// nat_lookup.hip — the device copy of a NAT flow table (nat_table.cc is its host control plane)
// and the batched lookups of the forward path on gfx950: the inbound DNAT and outbound SNAT halves
// of Ipv4RouteForward (engine/ipv4_engine.go:111-130, :203-225) and IcmpTtlDeepNat's
// NatGetFlowByWan (engine/icmp_engine.go:75-82).
//
// Layout: per index (NatFlowTable, NatWanFlowTable) a power-of-two array of 32-byte slots — the
// whole 13-byte key in the first 16 bytes (remote ip, local ip, both ports, used | proto), then
// the translation and the flow id — placed by linear probing from XXH3-64(key) & mask, the hash of
// flow_key.h the host compile and the kernel share. A lookup compares whole keys (HashMap.Get
// does, hashmap/hashmap.go:63-80) and ends at the first empty slot; tables are rebuilt from
// scratch by every sync, so there are no tombstones. Two generations, published with
// release/acquire, under route_lpm.hip's discipline. LastAliveTime is one u32 per flow id in a
// stamp array both generations share. The extern "C" entry points are nat_table.cc's: they reach
// this file through nat::device_ops(), and sync, fold, publish and destroy are device_table.h's
// lifecycle over NatDevice::write and ::free_arrays.
//
// Kernel shape: one lane per record, grid-stride by whole wavefronts; a probe reads one aligned
// 32-byte slot (two 16-byte loads of one 32-byte sector); the port-mapping list (<= 256 entries,
// first match wins) is staged in LDS once per block and scanned there — every lane reads the same
// address, a broadcast; misses are counted per wavefront with a ballot and one atomic add.
#include <hip/hip_runtime.h>

#include <shared_mutex>
#include <vector>

#include "device_table.h"
#include "flow_key.h"
#include "nat_table.h"

namespace halo {
namespace {

using nat::MapWord;
using nat::Slot;

struct NatView {
    const uint4* index[2];  // [HALO_FLOW_NAT_LAN], [HALO_FLOW_NAT_WAN]: 32-byte Slots as flowkey::probe reads them
    const MapWord* maps;
    uint32_t* stamps;
    uint32_t mask;    // slots - 1
    uint32_t n_maps;  // <= HALO_NAT_MAX_PORT_MAPPINGS
    uint32_t nat_type;
    uint32_t wan_ip;
};

struct NatGen {
    Slot* d_index[2] = {nullptr, nullptr};
    size_t cap[2] = {0, 0};
    MapWord* d_maps = nullptr;  // HALO_NAT_MAX_PORT_MAPPINGS entries
    uint32_t slots = 0, n_maps = 0;
};

struct NatDevice : Generations<NatGen> {  // device_table.h's lifecycle runs it
    Stamps stamps;
    static constexpr auto merge_stamps = &nat::merge_stamps;
    int write(halo_nat_table* t);
    void free_arrays();
};

// KIND: HALO_FLOW_NAT_WAN = inbound half (DNAT), HALO_FLOW_NAT_LAN = outbound half (SNAT)
template <uint32_t KIND, bool COMPACT>
__global__ void __launch_bounds__(256) nat_lookup_kernel(const NatView v, const void* __restrict__ recs, uint32_t n,
                                                         uint32_t now, const uint8_t* __restrict__ skip,
                                                         halo_tx_op_t* __restrict__ ops, uint8_t* __restrict__ verdict,
                                                         uint32_t* __restrict__ ref, uint32_t* miss_count) {
    __shared__ MapWord s_maps[HALO_NAT_MAX_PORT_MAPPINGS];
    for (uint32_t k = threadIdx.x; k < v.n_maps; k += blockDim.x) s_maps[k] = v.maps[k];
    __syncthreads();
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t misses = 0;  // wave-uniform
    // whole wavefronts iterate together (the bound is on the wave's first record), so the ballot
    // below sees every lane of the wave
    for (uint32_t base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n; base += stride) {
        const uint32_t i = base + (threadIdx.x & 63u);
        bool miss = false;
        if (i < n) {
            uint32_t proto, src, dst, ports;
            if (COMPACT) {
                const uint4 r = reinterpret_cast<const uint4*>(recs)[i];
                proto = (r.x >> 16) & 0xFFu, src = r.y, dst = r.z, ports = r.w;
            } else {
                const uint4 r = reinterpret_cast<const uint4*>(recs)[2ull * i];
                proto = r.y & 0xFFu, src = r.z, dst = r.w;
                ports = reinterpret_cast<const uint32_t*>(recs)[8ull * i + 4];
            }
            const uint32_t sport = ports & 0xFFFFu, dport = ports >> 16;
            uint32_t verd, rf = HALO_NAT_NO_FLOW, x_ip = 0, x_port = 0;
            if (proto == 0xFFu) {
                verd = HALO_NAT_V_NONE;
            } else if (skip && skip[i]) {
                verd = HALO_NAT_V_SKIP;
            } else {
                verd = HALO_NAT_V_MISS;
                if (proto == 6u || proto == 17u) {  // CheckNatPortMapping (:683-707): first match
                    for (uint32_t k = 0; k < v.n_maps; ++k) {
                        const MapWord m = s_maps[k];
                        const bool match = KIND == HALO_FLOW_NAT_WAN
                                               ? ((m.ports & 0xFFFFu) == dport && m.proto == proto)
                                               : (m.lan_ip == src && (m.ports >> 16) == sport && m.proto == proto);
                        if (match) {
                            verd = HALO_NAT_V_MAPPING;
                            rf = k;
                            x_ip = KIND == HALO_FLOW_NAT_WAN ? m.lan_ip : v.wan_ip;
                            x_port = KIND == HALO_FLOW_NAT_WAN ? (m.ports >> 16) : (m.ports & 0xFFFFu);
                            break;
                        }
                    }
                }
                if (verd == HALO_NAT_V_MISS) {
                    const flowkey::Key k = flowkey::nat_key(proto, src, dst, sport, dport, KIND, v.nat_type);
                    uint4 hit;
                    if (flowkey::probe(v.index[KIND], v.mask, k, &hit)) {  // x_ip, x_port, id
                        verd = HALO_NAT_V_FLOW;
                        x_ip = hit.x, x_port = hit.y, rf = hit.z;
                        v.stamps[rf] = now;  // LastAliveTime = TimeNow (:125, :219)
                    } else {
                        miss = true;
                    }
                }
                if (!miss) {  // only this direction's fields: the caller chains both lookups
                    halo_tx_op_t* op = ops + i;
                    if (KIND == HALO_FLOW_NAT_WAN) {
                        op->steps |= HALO_TX_NAT_DST;
                        op->dst_port = (uint16_t)x_port;
                        op->dst_ip = x_ip;
                    } else {
                        op->steps |= HALO_TX_NAT_SRC;
                        op->src_port = (uint16_t)x_port;
                        op->src_ip = x_ip;
                    }
                }
            }
            verdict[i] = (uint8_t)verd;
            ref[i] = rf;
        }
        misses += (uint32_t)__popcll(__ballot(miss));
    }
    if ((threadIdx.x & 63u) == 0 && misses) atomicAdd(miss_count, misses);
}

__global__ void __launch_bounds__(256) nat_quote_kernel(const NatView v, const halo_rx_result_t* __restrict__ recs,
                                                        uint32_t n, halo_tx_deep_nat_t* __restrict__ out) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint4 r = reinterpret_cast<const uint4*>(recs)[2ull * i];
        const uint32_t ports = reinterpret_cast<const uint32_t*>(recs)[8ull * i + 4];
        uint2 o = make_uint2(0u, 0u);  // lan_ip | lan_port, found, pad
        if ((r.x & 0xFFu) == HALO_RX_OK) {
            // the quote record is laid out so that its WAN key is NatGetFlowByWan's (deep_nat.hip)
            const flowkey::Key k =
                flowkey::nat_key(r.y & 0xFFu, r.z, r.w, ports & 0xFFFFu, ports >> 16, HALO_FLOW_NAT_WAN, v.nat_type);
            uint4 hit;
            if (flowkey::probe(v.index[HALO_FLOW_NAT_WAN], v.mask, k, &hit)) o = make_uint2(hit.x, (hit.y & 0xFFFFu) | 1u << 16);
        }
        reinterpret_cast<uint2*>(out)[i] = o;
    }
}

uint32_t nat_blocks(uint64_t threads) {
    const uint64_t b = (threads + 255) / 256;
    const uint64_t kMax = 256ull * 8 * 8;
    return (uint32_t)(b > kMax ? kMax : (b ? b : 1));
}


// Compile the host table into the unpublished generation and publish it. The caller holds
// t->sync_mu and an Exclusive, and has folded.
int NatDevice::write(halo_nat_table* t) {
    nat::Image img;
    int rc = nat::compile(*t, &img, true);
    if (rc) return rc;
    NatGen* g = begin_write();
    if (!g) return HALO_E_HIP;
    for (int k = 0; k < 2; ++k)
        if ((rc = grow(g->d_index[k], g->cap[k], img.slots))) return rc;
    if (!g->d_maps && hipMalloc(&g->d_maps, HALO_NAT_MAX_PORT_MAPPINGS * sizeof(MapWord)) != hipSuccess) return HALO_E_NOMEM;
    for (int k = 0; k < 2; ++k)
        if (hipMemcpy(g->d_index[k], img.index[k].data(), (size_t)img.slots * sizeof(Slot), hipMemcpyHostToDevice) != hipSuccess)
            return HALO_E_HIP;
    if (!img.maps.empty() &&
        hipMemcpy(g->d_maps, img.maps.data(), img.maps.size() * sizeof(MapWord), hipMemcpyHostToDevice) != hipSuccess)
        return HALO_E_HIP;
    if ((rc = stamps.upload(img.stamps))) return rc;
    g->slots = img.slots;
    g->n_maps = (uint32_t)img.maps.size();
    return publish();
}

void NatDevice::free_arrays() {
    for (auto& g : gen) {
        for (auto* p : g.d_index)
            if (p) (void)hipFree(p);
        if (g.d_maps) (void)hipFree(g.d_maps);
    }
    if (stamps.d_stamps) (void)hipFree(stamps.d_stamps);
}

int ops_sync(halo_nat_table* t, int device) {  // halo_nat_sync_device, t->sync_mu held
    NatDevice* d;
    int rc = sync_begin(t, device, &d);
    if (rc) return rc;
    Exclusive x(*d);
    if ((rc = fold(t, d))) return rc;
    return d->write(t);
}

// The view of the published generation; the caller holds view_mu shared until its launch.
int nat_view(const halo_nat_table* t, NatDevice* d, NatView* out) {
    const NatGen* g = d->published();
    if (!g) return HALO_E_INVAL;  // never synced
    *out = NatView{{reinterpret_cast<const uint4*>(g->d_index[0]), reinterpret_cast<const uint4*>(g->d_index[1])},
                   g->d_maps, d->stamps.d_stamps, g->slots - 1, g->n_maps, t->cfg.nat_type, t->cfg.wan_ip};
    return HALO_OK;
}

template <uint32_t KIND, bool COMPACT>
int lookup(const halo_nat_table* t, const void* d_records, uint32_t n, uint32_t now, const uint8_t* d_skip,
           halo_tx_op_t* d_ops, uint8_t* d_verdict, uint32_t* d_ref, uint32_t* d_miss_count, halo_stream_t stream) {
    NatDevice* d = dev_of<NatDevice>(t);
    if (!d) return HALO_E_INVAL;  // never synced
    std::shared_lock<std::shared_mutex> lk(d->view_mu);
    NatView v;
    if (nat_view(t, d, &v)) return HALO_E_INVAL;
    if (!d_verdict || !d_ref || !d_ops || !d_miss_count) return HALO_E_INVAL;
    if (n == 0) return HALO_OK;
    if (!d_records) return HALO_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_records) | reinterpret_cast<uintptr_t>(d_ops)) & 15u) return HALO_E_INVAL;
    if (reinterpret_cast<uintptr_t>(d_ref) & 3u) return HALO_E_INVAL;
    int rc = check_device();
    if (rc) return rc;
    hipLaunchKernelGGL((nat_lookup_kernel<KIND, COMPACT>), dim3(nat_blocks(n)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), v, d_records, n, now, d_skip, d_ops, d_verdict, d_ref,
                       d_miss_count);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

int ops_quote(const halo_nat_table* t, const halo_rx_result_t* d_quote_records, uint32_t n, halo_tx_deep_nat_t* d_nat,
              halo_stream_t stream) {
    NatDevice* d = dev_of<NatDevice>(t);
    if (!d) return HALO_E_INVAL;  // never synced
    std::shared_lock<std::shared_mutex> lk(d->view_mu);
    NatView v;
    if (nat_view(t, d, &v)) return HALO_E_INVAL;
    if (!d_nat) return HALO_E_INVAL;
    if (n == 0) return HALO_OK;
    if (!d_quote_records) return HALO_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_quote_records) & 15u) || (reinterpret_cast<uintptr_t>(d_nat) & 7u))
        return HALO_E_INVAL;
    int rc = check_device();
    if (rc) return rc;
    hipLaunchKernelGGL(nat_quote_kernel, dim3(nat_blocks(n)), dim3(256), 0, static_cast<hipStream_t>(stream), v,
                       d_quote_records, n, d_nat);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

// The miss path's collect (nat_miss.hip) reads no table, only its NAT type; it is refused before
// the first sync as the lookups are.
template <bool COMPACT>
int ops_collect(const halo_nat_table* t, uint32_t dir, const void* d_records, const uint8_t* d_verdict,
                const uint8_t* d_select, uint32_t n, uint32_t slots, halo_nat_miss_item_t* d_items, uint32_t cap,
                uint32_t* d_count, uint32_t* d_pos, void* d_workspace, halo_stream_t stream) {
    NatDevice* d = dev_of<NatDevice>(t);
    if (!d) return HALO_E_INVAL;  // never synced
    {
        std::shared_lock<std::shared_mutex> lk(d->view_mu);
        if (!d->published()) return HALO_E_INVAL;
    }
    return nat::miss_collect(dir, t->cfg.nat_type, COMPACT, d_records, d_verdict, d_select, n, slots, d_items, cap, d_count,
                             d_pos, d_workspace, stream);
}

// (the lookups in DeviceOps' order: the kernels are emitted in the order they are first named)
const nat::DeviceOps kDeviceOps = {
    ops_sync, fold_entry<NatDevice, halo_nat_table>, publish_entry<NatDevice, halo_nat_table>, destroy<NatDevice, halo_nat_table>,
    lookup<HALO_FLOW_NAT_WAN, false>, lookup<HALO_FLOW_NAT_LAN, false>, lookup<HALO_FLOW_NAT_WAN, true>, lookup<HALO_FLOW_NAT_LAN, true>,
    ops_quote, ops_collect<false>, ops_collect<true>, nat::miss_apply};

}  // namespace

namespace nat {
const DeviceOps* device_ops() { return &kDeviceOps; }
}  // namespace nat
}  // namespace halo
