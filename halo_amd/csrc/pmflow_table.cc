// pmflow_table.cc — the port-mapping return-flow table of include/halo_rx.h ("port-mapping return
// flows"): the host control plane — the Get / MallocType / Set of engine/ipv4_engine.go:238-266, the
// Get of :164-179 and NatPortMappingFlowClear (:497-516) restated over std containers — and the
// compile of the open-addressing image pmflow_fwd.hip uploads. The device side is reached through
// pmflow::DeviceOps. No HIP.
#include "pmflow_table.h"

#include <string.h>

#include <new>

using halo::flowkey::Key;
using namespace halo::pmflow;

namespace {

void store_entry(const Flow& f, halo_pmflow_entry_t* out) {
    out->remote_ip = f.key.rip;
    out->lan_ip = f.key.lip;
    out->last_alive = f.last_alive;
    out->id = f.id;
    out->remote_port = (uint16_t)f.key.rport;
    out->lan_port = (uint16_t)f.key.lport;
    out->wan_port = (uint16_t)f.wan_port;
    out->proto = (uint8_t)f.key.proto;
    out->wan_netif = (uint8_t)f.wan_netif;
}

const DeviceOps* dev_ops() { return device_ops ? device_ops() : nullptr; }

}  // namespace

namespace halo {
namespace pmflow {

int compile(const halo_pmflow_table& t, Image* out, bool with_stamps) {
    std::lock_guard<std::mutex> g(t.mu);
    uint32_t slots;
    const int rc = flowtab::capacity_slots(t.cfg.capacity_log2, (uint32_t)t.flows.size(), &slots);
    if (rc) return rc;
    const uint32_t mask = slots - 1;
    out->slots.assign(slots, Slot{});
    out->stats = halo_pmflow_layout_stats_t{slots, 0, 0, 0};
    out->version = t.version;
    for (const auto& kv : t.flows) {  // ascending id: the layout depends on the table's history only
        const Flow& f = kv.second;
        const uint32_t s = flowtab::place(out->slots.data(), mask, flowtab::home_slot(f.key, mask), &out->stats.entries,
                                          &out->stats.longest_chain, &out->stats.wrapped);
        out->slots[s] = Slot{f.key.rip, f.key.lip, f.key.rport | f.key.lport << 16, kSlotUsed | f.key.proto,
                             f.wan_netif, f.wan_port, f.id, 0};
    }
    out->stamps.clear();
    if (with_stamps) {
        out->stamps.assign(t.next_id, 0u);
        for (const auto& kv : t.flows) out->stamps[kv.first] = kv.second.last_alive;
    }
    return HALO_OK;
}

void merge_stamps(halo_pmflow_table& t, const uint32_t* dev, uint32_t n) {
    std::lock_guard<std::mutex> g(t.mu);
    flowtab::merge_stamps(t.flows, dev, n, [](Flow& f) -> uint32_t& { return f.last_alive; });
}

void mark_synced(halo_pmflow_table& t, uint64_t v) {
    std::lock_guard<std::mutex> g(t.mu);
    t.synced_version = v;
}

}  // namespace pmflow
}  // namespace halo

extern "C" HALO_API int halo_pmflow_table_create(const halo_pmflow_config_t* cfg, halo_pmflow_table_t** out) {
    if (!cfg || !out) return HALO_E_INVAL;
    *out = nullptr;
    if (cfg->n_netifs < 1 || cfg->n_netifs > HALO_ARP_MAX_NETIFS || cfg->capacity == 0) return HALO_E_INVAL;
    if (cfg->capacity_log2 > 28) return HALO_E_RANGE;
    halo_pmflow_table* t = new (std::nothrow) halo_pmflow_table;
    if (!t) return HALO_E_NOMEM;
    t->cfg = *cfg;
    for (uint32_t q = cfg->n_netifs; q < HALO_ARP_MAX_NETIFS; ++q) {
        memset(&t->cfg.netif[q], 0, sizeof t->cfg.netif[q]);
        t->cfg.gateway[q] = 0;
    }
    *out = t;
    return HALO_OK;
}

extern "C" HALO_API int halo_pmflow_table_destroy(halo_pmflow_table_t* t) {
    if (!t) return HALO_E_INVAL;
    if (t->dev.load(std::memory_order_acquire) && dev_ops()) dev_ops()->destroy(t);
    delete t;
    return HALO_OK;
}

extern "C" HALO_API int halo_pmflow_record(halo_pmflow_table_t* t, uint32_t in_netif, const halo_pmflow_item_t* items,
                                           uint32_t k, uint32_t now, uint8_t* dropped_out, uint32_t* n_added) {
    if (!t) return HALO_E_INVAL;
    if (in_netif >= t->cfg.n_netifs) return HALO_E_RANGE;
    if (k && (!items || !dropped_out)) return HALO_E_INVAL;
    for (uint32_t j = 0; j < k; ++j)  // CheckNatPortMapping (:683-707) yields no entry for another protocol
        if (items[j].proto != 6u && items[j].proto != 17u) return HALO_E_INVAL;
    if (n_added) *n_added = 0;
    uint32_t added = 0;
    std::lock_guard<std::mutex> g(t->mu);
    for (uint32_t j = 0; j < k; ++j) {
        const halo_pmflow_item_t& it = items[j];
        const Key key{it.remote_ip, it.remote_port, it.lan_ip, it.lan_port, it.proto};
        dropped_out[j] = 0;
        auto f = t->index.find(key);
        Flow* fl;
        if (f == t->index.end()) {
            // MallocType failed (:251-255); ids are never reused: a spent id space drops as well
            if (t->flows.size() >= t->cfg.capacity || t->next_id == 0xFFFFFFFFu) {
                dropped_out[j] = 1;
                continue;
            }
            const uint32_t id = t->next_id++;
            fl = &t->flows.emplace_hint(t->flows.end(), id, Flow{key, in_netif, it.wan_port, now, id})->second;
            t->index.emplace(key, fl);
            ++t->version;
            ++added;
        } else {
            fl = f->second;
            if (fl->wan_netif != in_netif || fl->wan_port != it.wan_port) ++t->version;
        }
        fl->wan_netif = in_netif;  // :262-264
        fl->wan_port = it.wan_port;
        fl->last_alive = now;
    }
    if (n_added) *n_added = added;
    return HALO_OK;
}

extern "C" HALO_API int halo_pmflow_get(halo_pmflow_table_t* t, uint32_t remote_ip, uint16_t remote_port, uint32_t lan_ip,
                                        uint16_t lan_port, uint8_t proto, const uint32_t* now_or_no_stamp,
                                        halo_pmflow_entry_t* out, uint32_t* found) {
    if (!t || !found) return HALO_E_INVAL;
    std::lock_guard<std::mutex> g(t->mu);
    const auto f = t->index.find(Key{remote_ip, remote_port, lan_ip, lan_port, proto});
    if (f == t->index.end()) {
        *found = 0;
        return HALO_OK;
    }
    if (now_or_no_stamp) f->second->last_alive = *now_or_no_stamp;  // :176
    if (out) store_entry(*f->second, out);
    *found = 1;
    return HALO_OK;
}

extern "C" HALO_API int halo_pmflow_expire(halo_pmflow_table_t* t, uint32_t now, uint32_t* n_removed) {
    if (!t) return HALO_E_INVAL;
    if (n_removed) *n_removed = 0;
    std::lock_guard<std::mutex> sg(t->sync_mu);
    const bool have_dev = t->dev.load(std::memory_order_acquire) && dev_ops();
    int rc;
    if (have_dev && (rc = dev_ops()->fold(t))) return rc;
    uint32_t removed = 0;
    {
        std::lock_guard<std::mutex> g(t->mu);
        for (auto it = t->flows.begin(); it != t->flows.end();) {
            if ((uint32_t)(now - it->second.last_alive) <= 60u) {  // :507
                ++it;
                continue;
            }
            t->index.erase(it->second.key);
            it = t->flows.erase(it);
            ++removed;
        }
        if (removed) ++t->version;
    }
    if (n_removed) *n_removed = removed;
    // the device must stop answering with the flows that left
    if (removed && have_dev) return dev_ops()->publish(t);
    return HALO_OK;
}

extern "C" HALO_API int halo_pmflow_list(const halo_pmflow_table_t* t, halo_pmflow_entry_t* out, uint32_t cap, uint32_t* n) {
    if (!t || !n || (cap && !out)) return HALO_E_INVAL;
    std::lock_guard<std::mutex> g(t->mu);
    uint32_t total = 0;
    for (const auto& kv : t->flows) {
        if (total < cap) store_entry(kv.second, out + total);
        ++total;
    }
    *n = total;
    return HALO_OK;
}

extern "C" HALO_API int halo_pmflow_layout_stats(const halo_pmflow_table_t* t, halo_pmflow_layout_stats_t* out) {
    if (!t || !out) return HALO_E_INVAL;
    Image img;
    const int rc = compile(*t, &img, false);
    if (rc) return rc;
    *out = img.stats;
    return HALO_OK;
}

extern "C" HALO_API int halo_pmflow_dirty(const halo_pmflow_table_t* t) {
    if (!t) return HALO_E_INVAL;
    std::lock_guard<std::mutex> g(t->mu);
    return t->version != t->synced_version ? 1 : 0;
}

extern "C" HALO_API int halo_pmflow_sync_device(halo_pmflow_table_t* t, const halo_route_table_t* routes, int device) {
    if (!t || device < 0) return HALO_E_INVAL;
    const DeviceOps* ops = dev_ops();
    return ops ? ops->sync(t, routes, device) : HALO_E_NODEV;
}

extern "C" HALO_API int halo_pmflow_lookup_device(const halo_pmflow_table_t* t, const halo_rx_result_t* d_records,
                                                  uint32_t n, uint32_t now, const uint32_t* d_route_ids,
                                                  const uint8_t* d_select, halo_tx_op_t* d_ops, halo_pmflow_via_t* d_via,
                                                  uint8_t* d_hit, uint32_t* d_counts, halo_stream_t stream) {
    if (!t) return HALO_E_INVAL;
    if (n && (!d_records || !d_route_ids || !d_ops || !d_via || !d_hit)) return HALO_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_records) | reinterpret_cast<uintptr_t>(d_ops)) & 15u) return HALO_E_INVAL;
    if (reinterpret_cast<uintptr_t>(d_via) & 7u) return HALO_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_route_ids) | reinterpret_cast<uintptr_t>(d_counts)) & 3u) return HALO_E_INVAL;
    const DeviceOps* ops = dev_ops();
    return ops ? ops->lookup(t, d_records, n, now, d_route_ids, d_select, d_ops, d_via, d_hit, d_counts, stream)
               : HALO_E_NODEV;
}

extern "C" HALO_API uint64_t halo_pmflow_record_workspace(uint32_t n) {
    const uint64_t tiles = ((uint64_t)n + kRecordTile - 1) / kRecordTile;
    // one u32 per tile, then one flag byte per frame (the count pass's verdict, read by the scatter)
    return 4 * (tiles ? tiles : 1) + (((uint64_t)n + 3) & ~3ull);
}

extern "C" HALO_API int halo_pmflow_record_device(const halo_pmflow_table_t* t, uint32_t in_netif,
                                                  const halo_rx_result_t* d_records, const uint8_t* d_wan_verdict,
                                                  const halo_tx_op_t* d_ops, const halo_arp_result_t* d_arp_results,
                                                  uint32_t n, uint32_t now, halo_pmflow_item_t* d_items, uint32_t cap,
                                                  uint32_t* d_count, void* d_workspace, uint64_t workspace_bytes,
                                                  halo_stream_t stream) {
    if (!t || !d_count || (cap && !d_items)) return HALO_E_INVAL;
    if (in_netif >= t->cfg.n_netifs) return HALO_E_RANGE;
    if (n && (!d_records || !d_wan_verdict || !d_ops || !d_arp_results || !d_workspace)) return HALO_E_INVAL;
    if (n && workspace_bytes < halo_pmflow_record_workspace(n)) return HALO_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_records) | reinterpret_cast<uintptr_t>(d_ops)) & 15u) return HALO_E_INVAL;
    if (reinterpret_cast<uintptr_t>(d_arp_results) & 7u) return HALO_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_items) | reinterpret_cast<uintptr_t>(d_count) |
         reinterpret_cast<uintptr_t>(d_workspace)) & 3u)
        return HALO_E_INVAL;
    const DeviceOps* ops = dev_ops();
    return ops ? ops->record(t, in_netif, d_records, d_wan_verdict, d_ops, d_arp_results, n, now, d_items, cap, d_count,
                             d_workspace, stream)
               : HALO_E_NODEV;
}

extern "C" HALO_API int halo_arp_drop_device(halo_arp_result_t* d_results, const uint32_t* d_index, uint32_t k,
                                             halo_stream_t stream) {
    if (k && (!d_results || !d_index)) return HALO_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_results) & 7u) || (reinterpret_cast<uintptr_t>(d_index) & 3u)) return HALO_E_INVAL;
    const DeviceOps* ops = dev_ops();
    return ops ? ops->arp_drop(d_results, d_index, k, stream) : HALO_E_NODEV;
}
