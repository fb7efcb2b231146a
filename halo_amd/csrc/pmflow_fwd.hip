// pmflow_fwd.hip — the device side of the port-mapping return-flow table (pmflow_table.cc is its
// host control plane) on gfx950: the LAN-side lookup of Ipv4RouteForward (engine/ipv4_engine.go
// :160-186, :203-207) over a batch of parsed records, the WAN-side listing of the frames that
// record a flow (:238-266) and the result edit for the frames the host then dropped.
//
// Layout: a power-of-two array of 32-byte slots — the whole 13-byte NatFlowHash in the first 16
// bytes (remote ip, lan ip, both ports, used | proto), then wan_netif, wan_port and the flow id —
// placed by linear probing from XXH3-64(key) & mask, the hash of flow_key.h the host compile and
// the kernels share. A lookup compares whole keys and ends at the first empty slot; the table is
// rebuilt from scratch by every sync, so there are no tombstones. Beside it the NetIf array {ip,
// nat_enable, gateway} (16 bytes each, fixed at create) and, when the sync was given a route
// table, the NetIf of every route id. Two generations, published with release/acquire, under
// nat_lookup.hip's discipline. LastAliveTime is one u32 per flow id in a stamp array both
// generations share.
//
// Kernel shape: one lane per record, grid-stride by whole wavefronts; a probe reads one aligned
// 32-byte slot (two 16-byte loads of one 32-byte sector); verdict counts go through a ballot per
// wavefront, LDS, and one atomic per counter and workgroup. The listing is tile counts -> a
// one-workgroup scan -> scatter, as arp_fwd.hip's gather is; the count pass probes and leaves one
// flag byte per frame, so the scatter does not probe again.
#include <hip/hip_runtime.h>

#include <shared_mutex>
#include <vector>

#include "arp_table.h"
#include "device_table.h"
#include "flow_key.h"
#include "pmflow_table.h"
#include "tile_scan.h"

namespace halo {
namespace {

using pmflow::kRecordTile;
using pmflow::NetIfWord;
using pmflow::Slot;

// the listing shares its tile and scan geometry with the ARP gather: one set of boundary sizes
static_assert(kRecordTile == arp::kGatherTile, "record tile == the ARP gather's tile");
static_assert(kRecordTile % 64 == 0, "whole wavefronts per tile");

struct PmView {
    const uint4* slots;  // 32-byte Slots as flowkey::probe reads them
    const NetIfWord* netifs;
    const uint32_t* route_netif;  // null: synced without a route table
    uint32_t* stamps;
    uint32_t mask;  // slots - 1
    uint32_t n_netifs;
    uint32_t n_routes;
};

struct PmGen {
    Slot* d_slots = nullptr;
    size_t cap = 0;
    uint32_t* d_routes = nullptr;
    size_t routes_cap = 0;
    uint32_t slots = 0, n_routes = 0;
    bool have_routes = false;
};

struct PmDevice : Generations<PmGen> {  // device_table.h's lifecycle runs it
    NetIfWord* d_netifs = nullptr;  // HALO_ARP_MAX_NETIFS entries, written once
    Stamps stamps;
    std::vector<uint32_t> routes;  // of the last sync: an expiry republishes them
    bool have_routes = false;
    static constexpr auto merge_stamps = &pmflow::merge_stamps;
    int write(halo_pmflow_table* t);
    void free_arrays();
};

__global__ void __launch_bounds__(256) pmflow_lookup_kernel(const PmView v, const halo_rx_result_t* __restrict__ recs,
                                                            uint32_t n, uint32_t now,
                                                            const uint32_t* __restrict__ route_ids,
                                                            const uint8_t* __restrict__ select,
                                                            halo_tx_op_t* __restrict__ ops, uint2* __restrict__ via,
                                                            uint8_t* __restrict__ hit_out, uint32_t* counts) {
    __shared__ uint32_t s_counts[HALO_PMFLOW_V_COUNT];
    if (threadIdx.x < HALO_PMFLOW_V_COUNT) s_counts[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t stride = gridDim.x * blockDim.x, lane = threadIdx.x & 63u;
    // whole wavefronts iterate together (the bound is on the wave's first record), so the ballots
    // below see every lane of the wave
    for (uint32_t base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n; base += stride) {
        const uint32_t i = base + lane;
        uint32_t verdict = HALO_PMFLOW_V_COUNT;  // no record
        if (i < n) {
            const uint4 r = reinterpret_cast<const uint4*>(recs)[2ull * i];
            const uint32_t ports = reinterpret_cast<const uint32_t*>(recs)[8ull * i + 4];
            const uint32_t rid = route_ids[i];
            const bool sel = !select || select[i];
            const uint32_t proto = r.y & 0xFFu, src = r.z, dst = r.w;
            uint2 o = make_uint2(HALO_PMFLOW_V_NONE | 0xFFu << 8, 0u);
            verdict = HALO_PMFLOW_V_NONE;
            if (proto != 0xFFu && sel) {
                verdict = HALO_PMFLOW_V_MISS;
                uint4 f;  // wan_netif, wan_port, id
                // NatFlowHash{remote = dst : dport, lan host = src : sport} (:165-171); only TCP / UDP
                // flows exist (CheckNatPortMapping, :683-707)
                if ((proto == 6u || proto == 17u) &&
                    flowkey::probe(v.slots, v.mask, flowkey::Key{dst, ports >> 16, src, ports & 0xFFFFu, proto}, &f)) {
                    v.stamps[f.z] = now;  // LastAliveTime = TimeNow (:176)
                    const uint4 nif = *reinterpret_cast<const uint4*>(v.netifs + f.x);  // ip, nat_enable, gateway
                    // outNetIfName != WanNetIf (:182): a panicking route is the encap's to report
                    const bool same = rid == HALO_ROUTE_PANIC || (rid < v.n_routes && v.route_netif[rid] == f.x);
                    verdict = same ? HALO_PMFLOW_V_HIT : HALO_PMFLOW_V_OVERRIDE;
                    if (nif.y) {  // outNetIf.Config.NatEnable (:203-207)
                        halo_tx_op_t* op = ops + i;
                        op->steps |= HALO_TX_NAT_SRC;
                        op->src_port = (uint16_t)f.y;
                        op->src_ip = nif.x;
                    }
                    o = make_uint2(verdict | f.x << 8 | f.y << 16, nif.z);
                } else {
                    o.x = HALO_PMFLOW_V_MISS | 0xFFu << 8;
                }
            }
            via[i] = o;
            hit_out[i] = verdict >= HALO_PMFLOW_V_HIT ? 1 : 0;
        }
        for (uint32_t k = 0; k < HALO_PMFLOW_V_COUNT; ++k) {
            const uint32_t c = (uint32_t)__popcll(__ballot(verdict == k));
            if (lane == k && c) atomicAdd(&s_counts[k], c);
        }
    }
    __syncthreads();
    if (counts && threadIdx.x < HALO_PMFLOW_V_COUNT && s_counts[threadIdx.x])
        atomicAdd(counts + threadIdx.x, s_counts[threadIdx.x]);
}

// A frame that records a flow (:238): the inbound lookup found a NatPortMappingEntry and the L2
// step found the neighbour (arp result byte 0).
__device__ __forceinline__ bool is_candidate(const uint8_t* __restrict__ wan_verdict, const uint2* __restrict__ arp,
                                             uint32_t i) {
    return wan_verdict[i] == HALO_NAT_V_MAPPING && (arp[i].x & 0xFFu) == HALO_ARP_V_HIT;
}

// Whether frame i is one to list, also left in flags[i]. A candidate the device copy already holds
// with the same value is stamped here instead.
__device__ __forceinline__ bool to_list(const PmView& v, uint32_t in_netif, const halo_rx_result_t* __restrict__ recs,
                                        const uint8_t* __restrict__ wan_verdict, const halo_tx_op_t* __restrict__ ops,
                                        const uint2* __restrict__ arp, uint32_t n, uint32_t now, uint8_t* __restrict__ flags,
                                        uint32_t i) {
    bool list = false;
    if (i < n) {
        if (is_candidate(wan_verdict, arp, i)) {
            const uint4 r = reinterpret_cast<const uint4*>(recs)[2ull * i];
            const uint32_t ports = reinterpret_cast<const uint32_t*>(recs)[8ull * i + 4];
            const uint2 op = *reinterpret_cast<const uint2*>(ops + i);  // steps, pad, dst_port; dst_ip
            uint4 f;
            list = true;
            // NatFlowHash{remote = src : sport, lan host = the entry's} (:240-247)
            if (flowkey::probe(v.slots, v.mask, flowkey::Key{r.z, ports & 0xFFFFu, op.y, op.x >> 16, r.y & 0xFFu}, &f) &&
                f.x == in_netif && f.y == (ports >> 16)) {
                v.stamps[f.z] = now;  // :264; WanNetIf and WanPort are already these
                list = false;
            }
        }
        flags[i] = list ? 1 : 0;
    }
    return list;
}

// Tile counts of the frames to list.
__global__ void __launch_bounds__(kRecordTile) pmflow_count_kernel(const PmView v, uint32_t in_netif,
                                                                   const halo_rx_result_t* __restrict__ recs,
                                                                   const uint8_t* __restrict__ wan_verdict,
                                                                   const halo_tx_op_t* __restrict__ ops,
                                                                   const uint2* __restrict__ arp, uint32_t n, uint32_t now,
                                                                   uint32_t* tiles, uint8_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * kRecordTile + threadIdx.x;
    tile_count(tiles, [&] { return to_list(v, in_netif, recs, wan_verdict, ops, arp, n, now, flags, i); });
}

// One workgroup: tiles[t] becomes the number of items in the tiles before t; *count = all.
__global__ void __launch_bounds__(256) pmflow_scan_kernel(uint32_t* tiles, uint32_t n_tiles, uint32_t* count) {
    const uint32_t total = scan_tiles(tiles, n_tiles);
    if (threadIdx.x == 0) *count = total;
}

__global__ void __launch_bounds__(kRecordTile) pmflow_scatter_kernel(const halo_rx_result_t* __restrict__ recs,
                                                                     const halo_tx_op_t* __restrict__ ops, uint32_t n,
                                                                     const uint32_t* __restrict__ tiles,
                                                                     const uint8_t* __restrict__ flags,
                                                                     halo_pmflow_item_t* __restrict__ items, uint32_t cap) {
    const uint32_t i = blockIdx.x * kRecordTile + threadIdx.x;
    const bool sel = i < n && flags[i];
    const uint64_t votes = tile_votes<kRecordTile>(sel);
    if (!sel) return;
    const uint32_t rank = tile_rank<kRecordTile>(votes, tiles[blockIdx.x]);
    if (rank >= cap) return;
    const uint4 r = reinterpret_cast<const uint4*>(recs)[2ull * i];
    const uint32_t ports = reinterpret_cast<const uint32_t*>(recs)[8ull * i + 4];
    const uint2 op = *reinterpret_cast<const uint2*>(ops + i);
    uint32_t* o = reinterpret_cast<uint32_t*>(items) + 5ull * rank;  // 20-byte items, 4-byte aligned
    o[0] = i;
    o[1] = r.z;                                 // remote_ip = src
    o[2] = op.y;                                // lan_ip = the entry's LanHostIpAddr
    o[3] = (ports & 0xFFFFu) | (op.x & 0xFFFF0000u);  // remote_port = sport; lan_port = dst_port
    o[4] = (ports >> 16) | (r.y & 0xFFu) << 16;       // wan_port = dport; proto; pad
}

__global__ void __launch_bounds__(256) arp_drop_kernel(uint2* __restrict__ results, const uint32_t* __restrict__ index,
                                                       uint32_t k) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < k; j += stride)
        results[index[j]] = make_uint2(HALO_ARP_V_NONE | 0xFFu << 8, 0u);
}

uint32_t pm_blocks(uint64_t threads) {
    const uint64_t b = (threads + 255) / 256;
    // nat_lookup.hip's cap: the same probe-bound shape. arp_fwd.hip's 256 * 8 measured 2-5 us slower
    // at 2^20 records, with and without the counters
    const uint64_t kMax = 256ull * 8 * 8;
    return (uint32_t)(b > kMax ? kMax : (b ? b : 1));
}

// Compile the host table into the unpublished generation and publish it. The caller holds
// t->sync_mu and an Exclusive, and has folded.
int PmDevice::write(halo_pmflow_table* t) {
    pmflow::Image img;
    int rc = pmflow::compile(*t, &img, true);
    if (rc) return rc;
    PmGen* g = begin_write();
    if (!g) return HALO_E_HIP;
    if ((rc = grow(g->d_slots, g->cap, img.slots.size()))) return rc;
    if (have_routes && (rc = grow(g->d_routes, g->routes_cap, routes.size() ? routes.size() : 1))) return rc;
    if (!d_netifs) {
        NetIfWord w[HALO_ARP_MAX_NETIFS] = {};
        for (uint32_t q = 0; q < t->cfg.n_netifs; ++q)
            w[q] = NetIfWord{t->cfg.netif[q].ip, t->cfg.netif[q].nat_enable ? 1u : 0u, t->cfg.gateway[q], 0};
        if (hipMalloc(&d_netifs, sizeof w) != hipSuccess) return HALO_E_NOMEM;
        if (hipMemcpy(d_netifs, w, sizeof w, hipMemcpyHostToDevice) != hipSuccess) return HALO_E_HIP;
    }
    if (hipMemcpy(g->d_slots, img.slots.data(), img.slots.size() * sizeof(Slot), hipMemcpyHostToDevice) != hipSuccess)
        return HALO_E_HIP;
    if (have_routes && !routes.empty() &&
        hipMemcpy(g->d_routes, routes.data(), routes.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
        return HALO_E_HIP;
    if ((rc = stamps.upload(img.stamps))) return rc;
    g->slots = (uint32_t)img.slots.size();
    g->n_routes = (uint32_t)routes.size();
    g->have_routes = have_routes;
    if ((rc = publish())) return rc;
    pmflow::mark_synced(*t, img.version);
    return HALO_OK;
}

void PmDevice::free_arrays() {
    for (auto& g : gen) {
        if (g.d_slots) (void)hipFree(g.d_slots);
        if (g.d_routes) (void)hipFree(g.d_routes);
    }
    if (d_netifs) (void)hipFree(d_netifs);
    if (stamps.d_stamps) (void)hipFree(stamps.d_stamps);
}

int ops_sync(halo_pmflow_table* t, const halo_route_table_t* routes, int device) {
    std::lock_guard<std::mutex> sg(t->sync_mu);
    std::vector<uint32_t> rw;  // ahead of the device object and the parked residents: the walk needs neither
    int rc;
    if (routes && (rc = route_words(routes, &rw, [](const halo_route_entry_t& e) { return e.netif; }))) return rc;
    PmDevice* d;
    if ((rc = sync_begin(t, device, &d))) return rc;
    Exclusive x(*d);
    if ((rc = fold(t, d))) return rc;
    d->routes.swap(rw);
    d->have_routes = routes != nullptr;
    return d->write(t);
}

// The view of the published generation; the caller holds view_mu shared until its launch.
int pm_view(const halo_pmflow_table* t, PmDevice* d, PmView* out) {
    const PmGen* g = d->published();
    if (!g) return HALO_E_INVAL;  // never synced
    *out = PmView{reinterpret_cast<const uint4*>(g->d_slots), d->d_netifs, g->have_routes ? g->d_routes : nullptr,
                  d->stamps.d_stamps, g->slots - 1, t->cfg.n_netifs, g->n_routes};
    return HALO_OK;
}

int ops_lookup(const halo_pmflow_table* t, const halo_rx_result_t* d_records, uint32_t n, uint32_t now,
               const uint32_t* d_route_ids, const uint8_t* d_select, halo_tx_op_t* d_ops, halo_pmflow_via_t* d_via,
               uint8_t* d_hit, uint32_t* d_counts, halo_stream_t stream) {
    PmDevice* d = dev_of<PmDevice>(t);
    if (!d) return HALO_E_INVAL;  // never synced
    std::shared_lock<std::shared_mutex> lk(d->view_mu);
    PmView v;
    if (pm_view(t, d, &v) || !v.route_netif) return HALO_E_INVAL;  // ... or synced without a route table
    if (n == 0) return HALO_OK;
    const int rc = check_device();
    if (rc) return rc;
    hipLaunchKernelGGL(pmflow_lookup_kernel, dim3(pm_blocks(n)), dim3(256), 0, static_cast<hipStream_t>(stream), v,
                       d_records, n, now, d_route_ids, d_select, d_ops, reinterpret_cast<uint2*>(d_via), d_hit, d_counts);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

int ops_record(const halo_pmflow_table* t, uint32_t in_netif, const halo_rx_result_t* d_records,
               const uint8_t* d_wan_verdict, const halo_tx_op_t* d_ops, const halo_arp_result_t* d_arp_results, uint32_t n,
               uint32_t now, halo_pmflow_item_t* d_items, uint32_t cap, uint32_t* d_count, void* d_workspace,
               halo_stream_t stream) {
    PmDevice* d = dev_of<PmDevice>(t);
    if (!d) return HALO_E_INVAL;  // never synced
    std::shared_lock<std::shared_mutex> lk(d->view_mu);
    PmView v;
    if (pm_view(t, d, &v)) return HALO_E_INVAL;
    const int rc = check_device();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) return hipMemsetAsync(d_count, 0, sizeof(uint32_t), st) == hipSuccess ? HALO_OK : HALO_E_HIP;
    const uint32_t n_tiles = (n + kRecordTile - 1) / kRecordTile;
    uint32_t* tiles = static_cast<uint32_t*>(d_workspace);
    uint8_t* flags = reinterpret_cast<uint8_t*>(tiles + n_tiles);
    hipLaunchKernelGGL(pmflow_count_kernel, dim3(n_tiles), dim3(kRecordTile), 0, st, v, in_netif, d_records, d_wan_verdict,
                       d_ops, reinterpret_cast<const uint2*>(d_arp_results), n, now, tiles, flags);
    hipLaunchKernelGGL(pmflow_scan_kernel, dim3(1), dim3(256), 0, st, tiles, n_tiles, d_count);
    hipLaunchKernelGGL(pmflow_scatter_kernel, dim3(n_tiles), dim3(kRecordTile), 0, st, d_records, d_ops, n, tiles, flags,
                       d_items, cap);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

int ops_arp_drop(halo_arp_result_t* d_results, const uint32_t* d_index, uint32_t k, halo_stream_t stream) {
    const int rc = check_device();
    if (rc) return rc;
    if (k == 0) return HALO_OK;
    hipLaunchKernelGGL(arp_drop_kernel, dim3(pm_blocks(k)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<uint2*>(d_results), d_index, k);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

const pmflow::DeviceOps kDeviceOps = {
    ops_sync, fold_entry<PmDevice, halo_pmflow_table>, publish_entry<PmDevice, halo_pmflow_table>, destroy<PmDevice, halo_pmflow_table>,
    ops_lookup, ops_record, ops_arp_drop};

}  // namespace

namespace pmflow {
const DeviceOps* device_ops() { return &kDeviceOps; }
}  // namespace pmflow
}  // namespace halo
