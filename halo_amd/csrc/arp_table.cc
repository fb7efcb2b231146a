// arp_table.cc — the ARP neighbour cache of include/halo_rx.h ("ARP neighbour cache"): the host
// control plane — SetArpCache, GetArpCache, HandleArp, SendArpReq / SendFreeArp, ArpTableClear,
// ArpTableRefresh and ListArp (engine/arp_engine.go, protocol/arp.go) restated over one table keyed
// by (netif, ip) — and the compile of the image arp_fwd.hip uploads. The device side is reached
// through arp::DeviceOps. No HIP.
#include "arp_table.h"

#include <string.h>

#include "flow_table.h"

#include <new>

using namespace halo::arp;

namespace {

constexpr uint32_t kOpRequest = 1, kOpReply = 2;  // protocol.ARP_REQUEST / ARP_REPLY

uint64_t key_of(uint32_t netif, uint32_t ip) { return (uint64_t)netif << 32 | ip; }

void put_ip(uint8_t* p, uint32_t ip) {  // UToIpAddr
    p[0] = (uint8_t)(ip >> 24), p[1] = (uint8_t)(ip >> 16), p[2] = (uint8_t)(ip >> 8), p[3] = (uint8_t)ip;
}
uint32_t get_ip(const uint8_t* p) {  // IpAddrToU
    return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
}

// BuildArpPkt inside BuildEthFrm(0x0806), zero-padded to 60 bytes
void build_frame(uint8_t* out, const uint8_t* eth_dst, const uint8_t* own_mac, uint32_t op, uint32_t own_ip,
                 const uint8_t* tha, uint32_t tpa) {
    memset(out, 0, 60);
    memcpy(out, eth_dst, 6);
    memcpy(out + 6, own_mac, 6);
    out[12] = 0x08, out[13] = 0x06;
    static const uint8_t kFixed[6] = {0x00, 0x01, 0x08, 0x00, 0x06, 0x04};
    memcpy(out + 14, kFixed, 6);
    out[20] = (uint8_t)(op >> 8), out[21] = (uint8_t)op;
    memcpy(out + 22, own_mac, 6);
    put_ip(out + 28, own_ip);
    memcpy(out + 32, tha, 6);
    put_ip(out + 38, tpa);
}

// SetArpCache, t->mu held. Returns false when the table was full (nothing stored).
bool set_locked(halo_arp_table* t, uint32_t netif, uint32_t ip, const uint8_t* mac, uint32_t now, uint32_t* changed) {
    auto it = t->cache.find(key_of(netif, ip));
    if (it == t->cache.end()) {
        if (t->cache.size() >= t->cfg.capacity) return false;  // MallocType failed (:67-70)
        it = t->cache.emplace(key_of(netif, ip), HostEntry{}).first;
        ++t->version;
        if (changed) ++*changed;
    } else if (memcmp(it->second.mac, mac, 6) != 0) {
        ++t->version;
        if (changed) ++*changed;
    }
    memcpy(it->second.mac, mac, 6);
    it->second.exp_time = (uint32_t)(now + HALO_ARP_AGE);
    return true;
}

void store_entry(uint64_t key, const HostEntry& e, halo_arp_entry_t* out) {
    out->ip = (uint32_t)key;
    memcpy(out->mac, e.mac, 6);
    out->netif = (uint8_t)(key >> 32);
    out->pad = 0;
    out->exp_time = e.exp_time;
}

}  // namespace

namespace halo {
namespace arp {

void compile(const halo_arp_table& t, Image* out) {
    std::lock_guard<std::mutex> g(t.mu);
    const uint32_t mask = t.slots - 1;
    out->slots.assign(t.slots, Slot{0, 0, 0, 0});
    out->stats = halo_arp_layout_stats_t{t.slots, 0, 0, 0};
    out->version = t.version;
    for (const auto& kv : t.cache) {
        const uint32_t netif = (uint32_t)(kv.first >> 32), ip = (uint32_t)kv.first;
        // entries <= capacity < slots: an empty slot exists
        const uint32_t s = halo::flowtab::place(out->slots.data(), mask, key_hash(netif, ip) & mask, &out->stats.entries,
                                                &out->stats.longest_chain, &out->stats.wrapped);
        const uint8_t* m = kv.second.mac;
        out->slots[s] = Slot{ip, kUsed | netif, (uint32_t)m[0] | (uint32_t)m[1] << 8 | (uint32_t)m[2] << 16 | (uint32_t)m[3] << 24,
                             (uint32_t)m[4] | (uint32_t)m[5] << 8};
    }
}

void mark_synced(halo_arp_table& t, uint64_t v) {
    std::lock_guard<std::mutex> g(t.mu);
    t.synced_version = v;
}

}  // namespace arp
}  // namespace halo

extern "C" HALO_API int halo_arp_table_create(const halo_arp_config_t* cfg, halo_arp_table_t** out) {
    if (!cfg || !out) return HALO_E_INVAL;
    *out = nullptr;
    if (cfg->n_netifs < 1 || cfg->n_netifs > HALO_ARP_MAX_NETIFS || cfg->capacity == 0 || cfg->slots_log2 > 28)
        return HALO_E_INVAL;
    uint64_t slots;
    if (cfg->slots_log2) {
        slots = 1ull << cfg->slots_log2;
    } else {
        slots = 2;
        while (slots < 2ull * cfg->capacity) slots <<= 1;
    }
    if (slots <= cfg->capacity || slots > (1ull << 28)) return HALO_E_INVAL;
    halo_arp_table* t = new (std::nothrow) halo_arp_table;
    if (!t) return HALO_E_NOMEM;
    t->cfg = *cfg;
    for (uint32_t q = cfg->n_netifs; q < HALO_ARP_MAX_NETIFS; ++q) memset(&t->cfg.netif[q], 0, sizeof t->cfg.netif[q]);
    t->slots = (uint32_t)slots;
    *out = t;
    return HALO_OK;
}

extern "C" HALO_API int halo_arp_table_destroy(halo_arp_table_t* t) {
    if (!t) return HALO_E_INVAL;
    if (t->dev.load(std::memory_order_acquire) && device_ops) device_ops()->destroy(t);
    delete t;
    return HALO_OK;
}

extern "C" HALO_API int halo_arp_set(halo_arp_table_t* t, uint32_t netif, uint32_t ip, const uint8_t mac[6], uint32_t now) {
    if (!t || !mac) return HALO_E_INVAL;
    if (netif >= t->cfg.n_netifs) return HALO_E_RANGE;
    std::lock_guard<std::mutex> g(t->mu);
    (void)set_locked(t, netif, ip, mac, now, nullptr);
    return HALO_OK;
}

extern "C" HALO_API int halo_arp_get(const halo_arp_table_t* t, uint32_t netif, uint32_t ip, halo_arp_entry_t* entry,
                                     uint32_t* found) {
    if (!t || !found) return HALO_E_INVAL;
    if (netif >= t->cfg.n_netifs) return HALO_E_RANGE;
    if (ip == t->cfg.netif[netif].ip) {  // :32-34
        *found = HALO_ARP_GET_OWN_IP;
        return HALO_OK;
    }
    std::lock_guard<std::mutex> g(t->mu);
    const auto it = t->cache.find(key_of(netif, ip));
    if (it == t->cache.end()) {
        *found = HALO_ARP_GET_ABSENT;
        return HALO_OK;
    }
    if (entry) store_entry(it->first, it->second, entry);
    *found = HALO_ARP_GET_FOUND;
    return HALO_OK;
}

extern "C" HALO_API int halo_arp_handle_msgs(halo_arp_table_t* t, const halo_arp_msg_t* msgs, uint32_t n, uint32_t now,
                                             uint8_t* verdicts, uint8_t* reply_frames, uint32_t* n_replies,
                                             uint32_t* n_changed) {
    if (!t) return HALO_E_INVAL;
    if (n && (!msgs || !verdicts)) return HALO_E_INVAL;
    for (uint32_t i = 0; i < n; ++i)
        if (msgs[i].netif >= t->cfg.n_netifs) return HALO_E_RANGE;
    uint32_t replies = 0, changed = 0;
    std::lock_guard<std::mutex> g(t->mu);
    for (uint32_t i = 0; i < n; ++i) {
        const halo_arp_msg_t& m = msgs[i];
        const halo_rx_netif_t& nif = t->cfg.netif[m.netif];
        const uint8_t* p = m.arp;
        const uint32_t op = (uint32_t)p[6] << 8 | p[7];  // ParseArpPkt reads nothing of bytes 0-5
        uint8_t v;
        if (op != kOpRequest && op != kOpReply) {
            v = HALO_ARP_H_BAD_OP;
        } else if (memcmp(p + 8, m.eth_src, 6) != 0) {  // :85-89
            v = HALO_ARP_H_SRC_MISMATCH;
        } else if (get_ip(p + 14) == nif.ip) {  // :90-93
            v = HALO_ARP_H_CONFLICT;
        } else {
            v = HALO_ARP_H_ACCEPTED;
            const uint32_t spa = get_ip(p + 14);
            if (!set_locked(t, m.netif, spa, p + 8, now, &changed)) v |= HALO_ARP_H_F_NOT_LEARNED;
            if (op == kOpRequest && get_ip(p + 24) == nif.ip) {  // :96-104, whether or not it learned
                if (reply_frames) build_frame(reply_frames + 60ull * replies, p + 8, nif.mac, kOpReply, nif.ip, p + 8, spa);
                ++replies;
                v |= HALO_ARP_H_F_REPLY;
            }
        }
        verdicts[i] = v;
    }
    if (n_replies) *n_replies = replies;
    if (n_changed) *n_changed = changed;
    return HALO_OK;
}

extern "C" HALO_API int halo_arp_build_request(const halo_arp_table_t* t, uint32_t netif, uint32_t target_ip, uint8_t out[60]) {
    if (!t || !out) return HALO_E_INVAL;
    if (netif >= t->cfg.n_netifs) return HALO_E_RANGE;
    static const uint8_t kBroadcast[6] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF};  // protocol.BROADCAST_MAC_ADDR
    const halo_rx_netif_t& nif = t->cfg.netif[netif];
    build_frame(out, kBroadcast, nif.mac, kOpRequest, nif.ip, kBroadcast, target_ip);
    return HALO_OK;
}

extern "C" HALO_API int halo_arp_expire(halo_arp_table_t* t, uint32_t now, uint32_t* n_removed) {
    if (!t) return HALO_E_INVAL;
    if (n_removed) *n_removed = 0;
    std::lock_guard<std::mutex> sg(t->sync_mu);
    uint32_t removed = 0;
    {
        std::lock_guard<std::mutex> g(t->mu);
        for (auto it = t->cache.begin(); it != t->cache.end();) {
            if (expired(now, it->second.exp_time)) {
                it = t->cache.erase(it);
                ++removed;
            } else {
                ++it;
            }
        }
        if (removed) ++t->version;
    }
    if (n_removed) *n_removed = removed;
    // the device must stop answering with the entries that left
    if (removed && t->dev.load(std::memory_order_acquire) && device_ops) return device_ops()->publish(t);
    return HALO_OK;
}

extern "C" HALO_API int halo_arp_refresh_list(const halo_arp_table_t* t, uint32_t now, uint8_t* netif_out, uint32_t* ip_out,
                                              uint32_t cap, uint32_t* n) {
    if (!t || !n || (cap && (!netif_out || !ip_out))) return HALO_E_INVAL;
    std::lock_guard<std::mutex> g(t->mu);
    uint32_t total = 0;
    for (const auto& kv : t->cache) {
        if (!refresh_due(now, kv.second.exp_time)) continue;
        if (total < cap) {
            netif_out[total] = (uint8_t)(kv.first >> 32);
            ip_out[total] = (uint32_t)kv.first;
        }
        ++total;
    }
    *n = total;
    return HALO_OK;
}

extern "C" HALO_API int halo_arp_list(const halo_arp_table_t* t, halo_arp_entry_t* out, uint32_t cap, uint32_t* n) {
    if (!t || !n || (cap && !out)) return HALO_E_INVAL;
    std::lock_guard<std::mutex> g(t->mu);
    uint32_t total = 0;
    for (const auto& kv : t->cache) {
        if (total < cap) store_entry(kv.first, kv.second, out + total);
        ++total;
    }
    *n = total;
    return HALO_OK;
}

extern "C" HALO_API int halo_arp_layout_stats(const halo_arp_table_t* t, halo_arp_layout_stats_t* out) {
    if (!t || !out) return HALO_E_INVAL;
    Image img;
    compile(*t, &img);
    *out = img.stats;
    return HALO_OK;
}

extern "C" HALO_API int halo_arp_dirty(const halo_arp_table_t* t) {
    if (!t) return HALO_E_INVAL;
    std::lock_guard<std::mutex> g(t->mu);
    return t->version != t->synced_version ? 1 : 0;
}

extern "C" HALO_API int halo_arp_sync_device(halo_arp_table_t* t, const halo_route_table_t* routes, int device) {
    if (!t || device < 0) return HALO_E_INVAL;
    const DeviceOps* ops = device_ops ? device_ops() : nullptr;
    return ops ? ops->sync(t, routes, device) : HALO_E_NODEV;
}

extern "C" HALO_API int halo_arp_lookup_device(const halo_arp_table_t* t, const uint32_t* d_ips, const uint8_t* d_netifs,
                                               uint32_t netif, uint32_t n, uint8_t* d_mac8, uint8_t* d_verdict,
                                               uint32_t* d_miss_count, halo_stream_t stream) {
    if (!t) return HALO_E_INVAL;
    const DeviceOps* ops = device_ops ? device_ops() : nullptr;
    return ops ? ops->lookup(t, d_ips, d_netifs, netif, n, d_mac8, d_verdict, d_miss_count, stream) : HALO_E_NODEV;
}

extern "C" HALO_API int halo_arp_encap_device(const halo_arp_table_t* t, uint8_t* d_bytes, const uint32_t* d_offsets_dw,
                                              const uint16_t* d_lens, uint32_t n, const uint32_t* d_route_ids,
                                              uint32_t in_netif, const uint8_t* d_select, halo_arp_result_t* d_results,
                                              uint32_t* d_counts, uint32_t* d_miss_count, halo_stream_t stream) {
    if (!t) return HALO_E_INVAL;
    if (in_netif >= t->cfg.n_netifs) return HALO_E_RANGE;
    const DeviceOps* ops = device_ops ? device_ops() : nullptr;
    return ops ? ops->encap(t, d_bytes, d_offsets_dw, d_lens, n, d_route_ids, in_netif, false, d_select, nullptr,
                            d_results, d_counts, d_miss_count, stream)
               : HALO_E_NODEV;
}

extern "C" HALO_API int halo_arp_encap_tx_device(const halo_arp_table_t* t, uint8_t* d_bytes, const uint32_t* d_offsets_dw,
                                                 const uint16_t* d_lens, uint32_t n, const uint32_t* d_route_ids,
                                                 uint32_t self_netif, const uint8_t* d_select, halo_arp_result_t* d_results,
                                                 uint32_t* d_counts, uint32_t* d_miss_count, halo_stream_t stream) {
    if (!t) return HALO_E_INVAL;
    if (self_netif >= t->cfg.n_netifs) return HALO_E_RANGE;
    const DeviceOps* ops = device_ops ? device_ops() : nullptr;
    return ops ? ops->encap(t, d_bytes, d_offsets_dw, d_lens, n, d_route_ids, self_netif, true, d_select, nullptr,
                            d_results, d_counts, d_miss_count, stream)
               : HALO_E_NODEV;
}

extern "C" HALO_API int halo_arp_encap_via_device(const halo_arp_table_t* t, uint8_t* d_bytes, const uint32_t* d_offsets_dw,
                                                  const uint16_t* d_lens, uint32_t n, const uint32_t* d_route_ids,
                                                  uint32_t in_netif, const uint8_t* d_select,
                                                  const halo_pmflow_via_t* d_via, halo_arp_result_t* d_results,
                                                  uint32_t* d_counts, uint32_t* d_miss_count, halo_stream_t stream) {
    if (!t) return HALO_E_INVAL;
    if (in_netif >= t->cfg.n_netifs) return HALO_E_RANGE;
    const DeviceOps* ops = device_ops ? device_ops() : nullptr;
    return ops ? ops->encap(t, d_bytes, d_offsets_dw, d_lens, n, d_route_ids, in_netif, false, d_select, d_via,
                            d_results, d_counts, d_miss_count, stream)
               : HALO_E_NODEV;
}

extern "C" HALO_API int halo_arp_loopback_mark_device(const halo_arp_table_t* t, const halo_rx_result_t* d_records,
                                                      uint32_t n, const uint32_t* d_route_ids, uint32_t in_netif,
                                                      const halo_pmflow_via_t* d_via, uint8_t* d_mark,
                                                      halo_stream_t stream) {
    if (!t) return HALO_E_INVAL;
    if (in_netif >= t->cfg.n_netifs) return HALO_E_RANGE;
    const DeviceOps* ops = device_ops ? device_ops() : nullptr;
    return ops ? ops->mark(t, d_records, n, d_route_ids, in_netif, d_via, d_mark, stream) : HALO_E_NODEV;
}

extern "C" HALO_API uint64_t halo_arp_gather_workspace(uint32_t n) {
    const uint64_t tiles = ((uint64_t)n + kGatherTile - 1) / kGatherTile;
    return 4 * (tiles ? tiles : 1);  // one u32 per tile
}

extern "C" HALO_API int halo_arp_gather_device(const uint8_t* d_bytes, const uint32_t* d_offsets_dw, const uint16_t* d_lens,
                                               const halo_rx_result_t* d_records, uint32_t n, uint32_t netif,
                                               halo_arp_msg_t* d_msgs, uint32_t cap, uint32_t* d_count, void* d_workspace,
                                               uint64_t workspace_bytes, halo_stream_t stream) {
    if (!d_count || netif >= HALO_ARP_MAX_NETIFS || (cap && !d_msgs)) return HALO_E_INVAL;
    if (n && (!d_bytes || !d_offsets_dw || !d_lens || !d_records || !d_workspace)) return HALO_E_INVAL;
    if (n && workspace_bytes < halo_arp_gather_workspace(n)) return HALO_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_bytes) | reinterpret_cast<uintptr_t>(d_offsets_dw) |
         reinterpret_cast<uintptr_t>(d_count) | reinterpret_cast<uintptr_t>(d_workspace)) & 3u)
        return HALO_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_records) & 15u) || (reinterpret_cast<uintptr_t>(d_msgs) & 7u)) return HALO_E_INVAL;
    const DeviceOps* ops = device_ops ? device_ops() : nullptr;
    return ops ? ops->gather(d_bytes, d_offsets_dw, d_lens, d_records, n, netif, d_msgs, cap, d_count, d_workspace,
                             workspace_bytes, stream)
               : HALO_E_NODEV;
}
