// arp_fwd.hip — the device side of the ARP neighbour cache (arp_table.cc is its host control
// plane) on gfx950: the bare GetArpCache over a batch of (netif, ip) pairs, the forward path's L2
// step (engine/ipv4_engine.go:180-201, :226-236, :267: route id -> next hop -> GetArpCache -> the
// Ethernet header BuildEthFrm writes) over a device-resident batch — also with the out-interface
// override of a port-mapping return flow (:180-186, halo_arp_encap_via_device; pmflow_fwd.hip makes
// the via array) — that step's LOOPBACK test alone, from records, for the chain to take ahead of the
// NAT lookup (halo_arp_loopback_mark_device; lo_gather.hip makes the LoChan batches), and the gather
// that brings a parsed batch's ARP messages to the host in frame order.
//
// Layout: a power-of-two array of 16-byte slots {ip, used | netif, mac[0..3], mac[4..5]} placed by
// linear probing from key_hash(netif, ip) & mask, the hash the host compile shares. A probe is one
// 16-byte load; a lookup compares the whole key and ends at the first empty slot; the table has
// more slots than `capacity` and is rebuilt from scratch by every sync, so chains end and there
// are no tombstones. Beside it the NetIf array (16 bytes each, fixed at create) and, when the sync
// was given a route table, a {next_hop, netif} array indexed by route id. Two generations,
// published with release/acquire, under nat_lookup.hip's discipline. Lookups only read.
//
// Kernel shape: one lane per entry / frame, grid-stride by whole workgroups so that every ballot
// sees every lane of its wave; verdict counts go through LDS and one atomic per counter and
// workgroup. The encap reads a frame's bytes 12-15 and 28-33 (one line for frames up to 64 B) and
// writes bytes 0-11 of a HIT with three dword stores. The gather is tile counts -> one-workgroup
// scan -> scatter, as the switch's probe / scan / admit kernels are.
#include <hip/hip_runtime.h>

#include <shared_mutex>
#include <vector>

#include "arp_table.h"
#include "device_table.h"
#include "tile_scan.h"

namespace halo {
namespace {

using arp::kGatherTile;
using arp::kUsed;
using arp::NetIfWord;
using arp::RouteWord;
using arp::Slot;

struct ArpView {
    const Slot* slots;
    const NetIfWord* netifs;
    const RouteWord* routes;  // null: synced without a route table
    uint32_t mask;            // slots - 1
    uint32_t n_netifs;
    uint32_t n_routes;
};

struct ArpGen {
    Slot* d_slots = nullptr;
    size_t cap = 0;
    RouteWord* d_routes = nullptr;
    size_t routes_cap = 0;
    uint32_t slots = 0, n_routes = 0;
    bool have_routes = false;
};

struct ArpDevice : Generations<ArpGen> {  // device_table.h's lifecycle runs it; no stamps, so no fold
    NetIfWord* d_netifs = nullptr;  // HALO_ARP_MAX_NETIFS entries, written once
    std::vector<RouteWord> routes;  // of the last sync: an expiry republishes them
    bool have_routes = false;
    int write(halo_arp_table* t);
    void free_arrays();
};

// The slot holding (netif, ip): its MAC words, or false when the probe chain ends first.
__device__ __forceinline__ bool probe(const Slot* __restrict__ tab, uint32_t mask, uint32_t netif, uint32_t ip, uint2* mac) {
    const uint32_t tag = kUsed | netif;
    uint32_t s = arp::key_hash(netif, ip) & mask;
    for (uint32_t step = 0; step <= mask; ++step) {  // bounded: entries < slots, and a full table cannot spin
        const uint4 e = *reinterpret_cast<const uint4*>(tab + s);
        if (e.y == 0) return false;
        if (e.x == ip && e.y == tag) {
            *mac = make_uint2(e.z, e.w);
            return true;
        }
        s = (s + 1) & mask;
    }
    return false;
}

__global__ void __launch_bounds__(256) arp_lookup_kernel(const ArpView v, const uint32_t* __restrict__ ips,
                                                         const uint8_t* __restrict__ netifs, uint32_t uniform_netif,
                                                         uint32_t n, uint2* __restrict__ mac8, uint8_t* __restrict__ verdict,
                                                         uint32_t* miss_count) {
    uint32_t misses = 0;  // wave-uniform
    for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {
        const uint32_t i = base + threadIdx.x;
        bool miss = false;
        if (i < n) {
            const uint32_t netif = netifs ? netifs[i] : uniform_netif, ip = ips[i];
            uint32_t verd = HALO_ARP_V_NONE;
            uint2 mac = make_uint2(0u, 0u);
            if (netif < v.n_netifs) {
                if (ip == v.netifs[netif].ip) {  // :32-34
                    verd = HALO_ARP_V_OWN_IP;
                } else if (probe(v.slots, v.mask, netif, ip, &mac)) {
                    verd = HALO_ARP_V_HIT;
                } else {
                    verd = HALO_ARP_V_MISS;
                    miss = true;
                }
            }
            mac8[i] = mac;
            verdict[i] = (uint8_t)verd;
        }
        misses += (uint32_t)__popcll(__ballot(miss));
    }
    if ((threadIdx.x & 63u) == 0 && misses) atomicAdd(miss_count, misses);
}

// kTx = false: the forward path's step, in_arg = the in NetIf's nat_enable. kTx = true: TxIpv4's
// (engine/ipv4_engine.go:50-99) for frames NetIf in_arg originated: a x.x.x.255 destination goes
// out of that NetIf to the broadcast MAC without a route, and dst == the out NetIf's address is a
// LOOPBACK whatever nat_enable says. The forward instantiation holds none of the Tx branches.
//
// kVia: the return-flow override of :180-186 (halo_arp_encap_via_device). Where via[i] says
// OVERRIDE, (next hop, out NetIf) come from it and the route id is not consulted; everything from
// the LOOPBACK test on is the same code. The body is shared and inlined into each kernel, so the
// instantiations without kVia compile to what they were.
template <bool kTx, bool kVia>
__device__ __forceinline__ void arp_encap_body(const ArpView& v, uint8_t* bytes, const uint32_t* __restrict__ offsets_dw,
                                               const uint16_t* __restrict__ lens, uint32_t n,
                                               const uint32_t* __restrict__ route_ids, uint32_t in_arg,
                                               const uint8_t* __restrict__ select, const uint2* __restrict__ via,
                                               uint2* __restrict__ results, uint32_t* counts, uint32_t* miss_count) {
    __shared__ uint32_t s_counts[HALO_ARP_V_COUNT];
    if (threadIdx.x < HALO_ARP_V_COUNT) s_counts[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {
        const uint32_t i = base + threadIdx.x;
        uint32_t verdict = HALO_ARP_V_COUNT;  // no frame
        if (i < n) {
            verdict = HALO_ARP_V_NONE;
            uint32_t out = 0xFFu, tx = 0, target = 0;
            // the loads that depend on nothing but i go out together, then the frame's and the
            // route's side by side: the chain is index arrays -> {frame, route -> NetIf} -> slot
            const uint32_t len = lens[i], off = offsets_dw[i];
            uint32_t rid = route_ids[i];
            const bool sel = !select || select[i];
            uint2 r = make_uint2(0u, 0xFFFFFFFFu);
            bool routed;
            if (kVia) {
                // the route word is loaded whatever the via says, so that the two loads go out
                // together and the chain to the slot is no longer than without a via
                const uint2 w = via[i];  // verdict | wan_netif << 8 | wan_port << 16; next_hop
                routed = rid < v.n_routes;
                if (routed) r = *reinterpret_cast<const uint2*>(v.routes + rid);
                if ((w.x & 0xFFu) == HALO_PMFLOW_V_OVERRIDE) {
                    r = make_uint2(w.y, (w.x >> 8) & 0xFFu);
                    rid = 0;  // neither NONE nor PANIC: the forced pair stands for the route
                    routed = true;
                }
            }
            if (sel && len >= 34u) {
                uint8_t* f = bytes + 4ull * off;
                uint32_t* p = reinterpret_cast<uint32_t*>(f);
                if (!kVia) routed = rid < v.n_routes;
                const uint32_t w3 = p[3], w7 = p[7], h = *reinterpret_cast<const uint16_t*>(f + 32);
                if (!kVia) r = routed ? *reinterpret_cast<const uint2*>(v.routes + rid) : make_uint2(0u, 0xFFFFFFFFu);
                if ((w3 & 0xFFFFu) != 0x0008u) {  // bytes 12-13 are not 08 00
                } else if (kTx && (h >> 8) == 255u) {  // :60-61, :85-86: no FindRoute, no GetArpCache
                    out = in_arg;
                    const uint4 nif = *reinterpret_cast<const uint4*>(v.netifs + out);
                    verdict = HALO_ARP_V_HIT;
                    tx = len < 60u ? 60u : len;
                    p[0] = 0xFFFFFFFFu;
                    p[1] = 0xFFFFu | nif.y << 16;
                    p[2] = nif.y >> 16 | nif.z << 16;
                } else if (rid == HALO_ROUTE_NONE) {
                    verdict = HALO_ARP_V_NO_ROUTE;
                } else if (rid == HALO_ROUTE_PANIC) {
                    verdict = HALO_ARP_V_ROUTE_PANIC;
                } else if (routed) {  // r = next_hop, netif
                    if (r.y < v.n_netifs) {
                        out = r.y;
                        const uint4 nif = *reinterpret_cast<const uint4*>(v.netifs + out);  // ip, mac_lo, mac_hi, nat
                        // ipv4DstAddr is a slice into the packet: bytes 30-33 as they are now
                        const uint32_t dst = ((w7 >> 16) & 0xFFu) << 24 | (w7 >> 24) << 16 | (h & 0xFFu) << 8 | h >> 8;
                        if (dst == nif.x && (kTx || !in_arg)) {
                            verdict = HALO_ARP_V_LOOPBACK;
                        } else {
                            target = r.x ? r.x : dst;
                            uint2 mac;
                            if (target == nif.x) {
                                verdict = HALO_ARP_V_OWN_IP;
                            } else if (probe(v.slots, v.mask, out, target, &mac)) {
                                verdict = HALO_ARP_V_HIT;
                                tx = len < 60u ? 60u : len;
                                p[0] = mac.x;
                                p[1] = (mac.y & 0xFFFFu) | nif.y << 16;
                                p[2] = nif.y >> 16 | nif.z << 16;
                            } else {
                                verdict = HALO_ARP_V_MISS;
                            }
                        }
                    }
                }
            }
            results[i] = make_uint2(verdict | out << 8 | tx << 16, target);
        }
        for (uint32_t k = 0; k < HALO_ARP_V_COUNT; ++k) {
            const uint32_t c = (uint32_t)__popcll(__ballot(verdict == k));
            if (lane == k && c) atomicAdd(&s_counts[k], c);
        }
    }
    __syncthreads();
    if (threadIdx.x < HALO_ARP_V_COUNT && s_counts[threadIdx.x]) {
        if (counts) atomicAdd(counts + threadIdx.x, s_counts[threadIdx.x]);
        if (threadIdx.x == HALO_ARP_V_MISS) atomicAdd(miss_count, s_counts[threadIdx.x]);
    }
}

template <bool kTx>
__global__ void __launch_bounds__(256) arp_encap_kernel(const ArpView v, uint8_t* bytes, const uint32_t* __restrict__ offsets_dw,
                                                        const uint16_t* __restrict__ lens, uint32_t n,
                                                        const uint32_t* __restrict__ route_ids, uint32_t in_arg,
                                                        const uint8_t* __restrict__ select, uint2* __restrict__ results,
                                                        uint32_t* counts, uint32_t* miss_count) {
    arp_encap_body<kTx, false>(v, bytes, offsets_dw, lens, n, route_ids, in_arg, select, nullptr, results, counts,
                               miss_count);
}

__global__ void __launch_bounds__(256) arp_encap_via_kernel(const ArpView v, uint8_t* bytes,
                                                            const uint32_t* __restrict__ offsets_dw,
                                                            const uint16_t* __restrict__ lens, uint32_t n,
                                                            const uint32_t* __restrict__ route_ids, uint32_t in_arg,
                                                            const uint8_t* __restrict__ select, const uint2* __restrict__ via,
                                                            uint2* __restrict__ results, uint32_t* counts,
                                                            uint32_t* miss_count) {
    arp_encap_body<false, true>(v, bytes, offsets_dw, lens, n, route_ids, in_arg, select, via, results, counts, miss_count);
}

// halo_rx_dispatch's HALO_RX_ACT_ARP: status OK, EtherType 0x0806, MAC_MATCH (the record's first dword)
__device__ __forceinline__ bool is_arp(const halo_rx_result_t* __restrict__ recs, uint32_t i) {
    const uint32_t w = reinterpret_cast<const uint32_t*>(recs)[8ull * i];
    return (w & 0xFFu) == HALO_RX_OK && (w >> 16) == 0x0806u && (w & (HALO_RX_F_MAC_MATCH << 8));
}

__global__ void __launch_bounds__(kGatherTile) arp_count_kernel(const halo_rx_result_t* __restrict__ recs, uint32_t n,
                                                                uint32_t* tiles) {
    const uint32_t i = blockIdx.x * kGatherTile + threadIdx.x;
    tile_count(tiles, [&] { return i < n && is_arp(recs, i); });
}

// One workgroup: tiles[t] becomes the number of messages in the tiles before t; *count = all.
__global__ void __launch_bounds__(256) arp_scan_kernel(uint32_t* tiles, uint32_t n_tiles, uint32_t* count) {
    const uint32_t total = scan_tiles(tiles, n_tiles);
    if (threadIdx.x == 0) *count = total;
}

__global__ void __launch_bounds__(kGatherTile) arp_scatter_kernel(const uint8_t* __restrict__ bytes,
                                                                  const uint32_t* __restrict__ offsets_dw,
                                                                  const halo_rx_result_t* __restrict__ recs, uint32_t n,
                                                                  uint32_t netif, const uint32_t* __restrict__ tiles,
                                                                  halo_arp_msg_t* __restrict__ msgs, uint32_t cap) {
    const uint32_t i = blockIdx.x * kGatherTile + threadIdx.x;
    const bool sel = i < n && is_arp(recs, i);
    const uint64_t votes = tile_votes<kGatherTile>(sel);
    if (!sel) return;
    const uint32_t rank = tile_rank<kGatherTile>(votes, tiles[blockIdx.x]);
    if (rank >= cap) return;
    // a selected frame passed ParseEthFrm: it has at least 42 bytes. Bytes 6-11 and 14-41 only.
    const uint8_t* f = bytes + 4ull * offsets_dw[i];
    const uint32_t* p = reinterpret_cast<const uint32_t*>(f);
    const uint32_t h6 = *reinterpret_cast<const uint16_t*>(f + 6), w2 = p[2];
    const uint32_t h14 = *reinterpret_cast<const uint16_t*>(f + 14), h40 = *reinterpret_cast<const uint16_t*>(f + 40);
    uint32_t q[6];
    for (uint32_t k = 0; k < 6; ++k) q[k] = p[4 + k];  // bytes 16-39
    uint2* o = reinterpret_cast<uint2*>(msgs + rank);
    o[0] = make_uint2(i, (netif & 0xFFu) | h6 << 16);  // index; netif, pad, eth_src[0..1]
    o[1] = make_uint2(w2, h14 | q[0] << 16);            // eth_src[2..5]; arp[0..3]
    o[2] = make_uint2(q[0] >> 16 | q[1] << 16, q[1] >> 16 | q[2] << 16);
    o[3] = make_uint2(q[2] >> 16 | q[3] << 16, q[3] >> 16 | q[4] << 16);
    o[4] = make_uint2(q[4] >> 16 | q[5] << 16, q[5] >> 16 | h40 << 16);
}

// The encap's LOOPBACK test alone, from records, ahead of the NAT lookup (halo_arp_loopback_mark_device):
// no frame byte is touched. One lane per record, one 16-byte load of its first half {status ..,
// ip_proto .., src_ip, dst_ip}, one byte store. nat = the in NetIf's nat_enable.
__global__ void __launch_bounds__(256) arp_loopback_mark_kernel(const ArpView v, const uint4* __restrict__ recs, uint32_t n,
                                                                const uint32_t* __restrict__ route_ids, uint32_t nat,
                                                                const uint2* __restrict__ via, uint8_t* __restrict__ mark) {
    for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {
        const uint32_t i = base + threadIdx.x;
        if (i >= n) continue;
        const uint4 rec = recs[2ull * i];
        const uint32_t rid = route_ids[i];
        uint32_t out = 0xFFFFFFFFu;
        if (rid < v.n_routes) out = v.routes[rid].netif;
        if (via) {
            const uint32_t w = via[i].x;  // verdict | wan_netif << 8 | wan_port << 16
            if ((w & 0xFFu) == HALO_PMFLOW_V_OVERRIDE) out = (w >> 8) & 0xFFu;
        }
        bool m = false;
        if (!nat && (rec.y & 0xFFu) != 0xFFu && out < v.n_netifs) m = rec.w == v.netifs[out].ip;
        mark[i] = m ? 1 : 0;
    }
}

uint32_t arp_blocks(uint64_t threads) {
    const uint64_t b = (threads + 255) / 256;
    const uint64_t kMax = 256ull * 8;  // 8 workgroups per CU; twice as many measured 9 us slower at 2^20 frames
    return (uint32_t)(b > kMax ? kMax : (b ? b : 1));
}

// Compile the host table into the unpublished generation and publish it. The caller holds
// t->sync_mu and an Exclusive.
int ArpDevice::write(halo_arp_table* t) {
    arp::Image img;
    arp::compile(*t, &img);
    ArpGen* g = begin_write();
    if (!g) return HALO_E_HIP;
    int rc;
    if ((rc = grow(g->d_slots, g->cap, img.slots.size()))) return rc;
    if (have_routes && (rc = grow(g->d_routes, g->routes_cap, routes.size() ? routes.size() : 1))) return rc;
    if (!d_netifs) {
        NetIfWord w[HALO_ARP_MAX_NETIFS] = {};
        for (uint32_t q = 0; q < t->cfg.n_netifs; ++q) {
            const halo_rx_netif_t& nif = t->cfg.netif[q];
            const uint8_t* m = nif.mac;
            w[q] = NetIfWord{nif.ip, (uint32_t)m[0] | (uint32_t)m[1] << 8 | (uint32_t)m[2] << 16 | (uint32_t)m[3] << 24,
                             (uint32_t)m[4] | (uint32_t)m[5] << 8, nif.nat_enable};
        }
        if (hipMalloc(&d_netifs, sizeof w) != hipSuccess) return HALO_E_NOMEM;
        if (hipMemcpy(d_netifs, w, sizeof w, hipMemcpyHostToDevice) != hipSuccess) return HALO_E_HIP;
    }
    if (hipMemcpy(g->d_slots, img.slots.data(), img.slots.size() * sizeof(Slot), hipMemcpyHostToDevice) != hipSuccess)
        return HALO_E_HIP;
    if (have_routes && !routes.empty() &&
        hipMemcpy(g->d_routes, routes.data(), routes.size() * sizeof(RouteWord), hipMemcpyHostToDevice) != hipSuccess)
        return HALO_E_HIP;
    g->slots = (uint32_t)img.slots.size();
    g->n_routes = (uint32_t)routes.size();
    g->have_routes = have_routes;
    if ((rc = publish())) return rc;
    arp::mark_synced(*t, img.version);
    return HALO_OK;
}

void ArpDevice::free_arrays() {
    for (auto& g : gen) {
        if (g.d_slots) (void)hipFree(g.d_slots);
        if (g.d_routes) (void)hipFree(g.d_routes);
    }
    if (d_netifs) (void)hipFree(d_netifs);
}

int ops_sync(halo_arp_table* t, const halo_route_table_t* routes, int device) {
    std::lock_guard<std::mutex> sg(t->sync_mu);
    std::vector<RouteWord> rw;  // ahead of the device object and the parked residents: the walk needs neither
    int rc;
    if (routes && (rc = route_words(routes, &rw, [](const halo_route_entry_t& e) { return RouteWord{e.next_hop, e.netif}; })))
        return rc;
    ArpDevice* d;
    if ((rc = sync_begin(t, device, &d))) return rc;
    Exclusive x(*d);
    d->routes.swap(rw);
    d->have_routes = routes != nullptr;
    return d->write(t);
}

// The view of the published generation; the caller holds view_mu shared until its launch.
int arp_view(const halo_arp_table* t, ArpDevice* d, ArpView* out) {
    const ArpGen* g = d->published();
    if (!g) return HALO_E_INVAL;  // never synced
    *out = ArpView{g->d_slots, d->d_netifs, g->have_routes ? g->d_routes : nullptr, g->slots - 1, t->cfg.n_netifs, g->n_routes};
    return HALO_OK;
}

int ops_lookup(const halo_arp_table* t, const uint32_t* d_ips, const uint8_t* d_netifs, uint32_t netif, uint32_t n,
               uint8_t* d_mac8, uint8_t* d_verdict, uint32_t* d_miss_count, halo_stream_t stream) {
    ArpDevice* d = dev_of<ArpDevice>(t);
    if (!d) return HALO_E_INVAL;  // never synced
    std::shared_lock<std::shared_mutex> lk(d->view_mu);
    ArpView v;
    if (arp_view(t, d, &v)) return HALO_E_INVAL;
    if (!d_mac8 || !d_verdict || !d_miss_count) return HALO_E_INVAL;
    if (n == 0) return HALO_OK;
    if (!d_ips) return HALO_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_ips) | reinterpret_cast<uintptr_t>(d_miss_count)) & 3u) return HALO_E_INVAL;
    if (reinterpret_cast<uintptr_t>(d_mac8) & 7u) return HALO_E_INVAL;
    const int rc = check_device();
    if (rc) return rc;
    hipLaunchKernelGGL(arp_lookup_kernel, dim3(arp_blocks(n)), dim3(256), 0, static_cast<hipStream_t>(stream), v, d_ips,
                       d_netifs, netif, n, reinterpret_cast<uint2*>(d_mac8), d_verdict, d_miss_count);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

int ops_encap(const halo_arp_table* t, uint8_t* d_bytes, const uint32_t* d_offsets_dw, const uint16_t* d_lens, uint32_t n,
              const uint32_t* d_route_ids, uint32_t in_netif, bool tx, const uint8_t* d_select,
              const halo_pmflow_via_t* d_via, halo_arp_result_t* d_results, uint32_t* d_counts, uint32_t* d_miss_count,
              halo_stream_t stream) {
    ArpDevice* d = dev_of<ArpDevice>(t);
    if (!d) return HALO_E_INVAL;  // never synced
    std::shared_lock<std::shared_mutex> lk(d->view_mu);
    ArpView v;
    if (arp_view(t, d, &v) || !v.routes) return HALO_E_INVAL;  // ... or synced without a route table
    if (!d_results || !d_miss_count) return HALO_E_INVAL;
    if (n == 0) return HALO_OK;
    if (!d_bytes || !d_offsets_dw || !d_lens || !d_route_ids) return HALO_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_bytes) | reinterpret_cast<uintptr_t>(d_offsets_dw) |
         reinterpret_cast<uintptr_t>(d_route_ids) | reinterpret_cast<uintptr_t>(d_counts) |
         reinterpret_cast<uintptr_t>(d_miss_count)) & 3u)
        return HALO_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_lens) & 1u) || (reinterpret_cast<uintptr_t>(d_results) & 7u)) return HALO_E_INVAL;
    if (reinterpret_cast<uintptr_t>(d_via) & 7u) return HALO_E_INVAL;
    const int rc = check_device();
    if (rc) return rc;
    if (d_via)  // forward path only; without it the plain forward kernel is the same computation
        hipLaunchKernelGGL(arp_encap_via_kernel, dim3(arp_blocks(n)), dim3(256), 0, static_cast<hipStream_t>(stream), v,
                           d_bytes, d_offsets_dw, d_lens, n, d_route_ids, t->cfg.netif[in_netif].nat_enable ? 1u : 0u,
                           d_select, reinterpret_cast<const uint2*>(d_via), reinterpret_cast<uint2*>(d_results), d_counts,
                           d_miss_count);
    else if (tx)
        hipLaunchKernelGGL(arp_encap_kernel<true>, dim3(arp_blocks(n)), dim3(256), 0, static_cast<hipStream_t>(stream), v,
                           d_bytes, d_offsets_dw, d_lens, n, d_route_ids, in_netif, d_select,
                           reinterpret_cast<uint2*>(d_results), d_counts, d_miss_count);
    else
        hipLaunchKernelGGL(arp_encap_kernel<false>, dim3(arp_blocks(n)), dim3(256), 0, static_cast<hipStream_t>(stream), v,
                           d_bytes, d_offsets_dw, d_lens, n, d_route_ids, t->cfg.netif[in_netif].nat_enable ? 1u : 0u,
                           d_select, reinterpret_cast<uint2*>(d_results), d_counts, d_miss_count);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

int ops_mark(const halo_arp_table* t, const halo_rx_result_t* d_records, uint32_t n, const uint32_t* d_route_ids,
             uint32_t in_netif, const halo_pmflow_via_t* d_via, uint8_t* d_mark, halo_stream_t stream) {
    ArpDevice* d = dev_of<ArpDevice>(t);
    if (!d) return HALO_E_INVAL;  // never synced
    std::shared_lock<std::shared_mutex> lk(d->view_mu);
    ArpView v;
    if (arp_view(t, d, &v) || !v.routes) return HALO_E_INVAL;  // ... or synced without a route table
    if (n == 0) return HALO_OK;
    if (!d_records || !d_route_ids || !d_mark) return HALO_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_records) & 15u) || (reinterpret_cast<uintptr_t>(d_route_ids) & 3u) ||
        (reinterpret_cast<uintptr_t>(d_via) & 7u))
        return HALO_E_INVAL;
    const int rc = check_device();
    if (rc) return rc;
    hipLaunchKernelGGL(arp_loopback_mark_kernel, dim3(arp_blocks(n)), dim3(256), 0, static_cast<hipStream_t>(stream), v,
                       reinterpret_cast<const uint4*>(d_records), n, d_route_ids, t->cfg.netif[in_netif].nat_enable ? 1u : 0u,
                       reinterpret_cast<const uint2*>(d_via), d_mark);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

int ops_gather(const uint8_t* d_bytes, const uint32_t* d_offsets_dw, const uint16_t* /*d_lens*/,
               const halo_rx_result_t* d_records, uint32_t n, uint32_t netif, halo_arp_msg_t* d_msgs, uint32_t cap,
               uint32_t* d_count, void* d_workspace, uint64_t /*workspace_bytes*/, halo_stream_t stream) {
    const int rc = check_device();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) return hipMemsetAsync(d_count, 0, sizeof(uint32_t), st) == hipSuccess ? HALO_OK : HALO_E_HIP;
    uint32_t* tiles = static_cast<uint32_t*>(d_workspace);
    const uint32_t n_tiles = (n + kGatherTile - 1) / kGatherTile;
    hipLaunchKernelGGL(arp_count_kernel, dim3(n_tiles), dim3(kGatherTile), 0, st, d_records, n, tiles);
    hipLaunchKernelGGL(arp_scan_kernel, dim3(1), dim3(256), 0, st, tiles, n_tiles, d_count);
    hipLaunchKernelGGL(arp_scatter_kernel, dim3(n_tiles), dim3(kGatherTile), 0, st, d_bytes, d_offsets_dw, d_records, n,
                       netif, tiles, d_msgs, cap);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

const arp::DeviceOps kDeviceOps = {
    ops_sync, publish_entry<ArpDevice, halo_arp_table>, destroy<ArpDevice, halo_arp_table>, ops_lookup, ops_encap, ops_gather,
    ops_mark};

}  // namespace

namespace arp {
const DeviceOps* device_ops() { return &kDeviceOps; }
}  // namespace arp
}  // namespace halo
