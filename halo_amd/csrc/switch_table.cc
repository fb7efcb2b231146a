// switch_table.cc — the L2 switch of include/halo_rx.h ("L2 switch"): configuration, validation,
// flood masks, and the host mode — SwitchPort.RxEthernet / HandleEthernet, SwitchMacAddrClear and
// ListSwitchMacAddr (engine/ethernet_engine.go:58-163) restated as the sequential loop over a
// host table and host frame arrays. The device mode is switch_fwd.hip, reached through
// sw::DeviceOps. No HIP.
#include "switch_table.h"

#include <string.h>

#include <new>

using namespace halo::sw;

namespace {

uint64_t load_mac(const uint8_t* p) {
    uint64_t m = 0;
    for (int k = 5; k >= 0; --k) m = m << 8 | p[k];
    return m;
}

void store_entry(uint64_t mac, uint32_t port, uint32_t create_time, halo_switch_entry_t* e) {
    for (int k = 0; k < 6; ++k) e->mac[k] = (uint8_t)(mac >> (8 * k));
    e->port = (uint8_t)port;
    e->pad = 0;
    e->create_time = create_time;
}

// One batch in host mode: the reference's loop, one frame at a time.
void forward_host(halo_switch* s, uint32_t port, const uint8_t* bytes, const uint32_t* offsets_dw, const uint16_t* lens,
                  uint32_t n, uint32_t now, halo_sw_result_t* results, uint32_t* counts) {
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t len = lens[i];
        halo_sw_result_t r = {HALO_SW_V_ETH_LEN, 0xFF, 0};
        do {
            if (len < 42u || len > 1514u) break;  // ParseEthFrm (protocol/ethernet.go:31)
            const uint8_t* f = bytes + 4ull * offsets_dw[i];
            r.verdict = HALO_SW_V_ETH_TYPE;
            if (!ethertype_known((uint32_t)f[12] << 8 | f[13])) break;
            r.verdict = HALO_SW_V_SRC_MCAST;
            if (f[6] & 1u) break;  // :71
            const uint64_t src = load_mac(f + 6), dst = load_mac(f);
            auto it = s->table.find(src);
            if (it == s->table.end()) {
                r.verdict = HALO_SW_V_TABLE_FULL;
                if (s->table.size() >= s->cfg.capacity) break;  // MallocType failed (:79-83)
                it = s->table.emplace(src, HostEntry{}).first;
            }
            it->second = HostEntry{port, now};  // :92-94
            const auto d = s->table.find(dst);
            if (d != s->table.end()) {
                r.verdict = HALO_SW_V_UNICAST;
                r.out_port = (uint8_t)d->second.port;
            } else {
                r.verdict = HALO_SW_V_FLOOD;
            }
            r.tx_len = (uint16_t)(len < 60u ? 60u : len);  // BuildEthFrm pads to 60
        } while (0);
        results[i] = r;
        if (counts) ++counts[r.verdict];
    }
}

}  // namespace

extern "C" HALO_API int halo_switch_create(const halo_switch_config_t* cfg, halo_switch_t** out) {
    if (!cfg || !out) return HALO_E_INVAL;
    *out = nullptr;
    if (cfg->n_ports < 1 || cfg->n_ports > HALO_SW_MAX_PORTS || cfg->capacity == 0 || cfg->slots_log2 > 28 ||
        cfg->max_batch < 1 || cfg->max_batch > (1u << 24) || cfg->device < -1)
        return HALO_E_INVAL;
    uint64_t slots;
    if (cfg->slots_log2) {
        slots = 1ull << cfg->slots_log2;
    } else {
        slots = 2;
        while (slots < 2ull * cfg->capacity) slots <<= 1;
    }
    if (slots <= cfg->capacity || slots > (1ull << 28)) return HALO_E_INVAL;
    const DeviceOps* ops = nullptr;
    if (cfg->device >= 0) {
        ops = device_ops ? device_ops() : nullptr;
        if (!ops) return HALO_E_NODEV;
    }
    halo_switch* s = new (std::nothrow) halo_switch;
    if (!s) return HALO_E_NOMEM;
    s->cfg = *cfg;
    for (uint32_t q = cfg->n_ports; q < HALO_SW_MAX_PORTS; ++q) s->cfg.vlan_id[q] = 0;
    s->slots = (uint32_t)slots;
    for (uint32_t p = 0; p < HALO_SW_MAX_PORTS; ++p) {
        uint64_t m = 0;
        for (uint32_t q = 0; p < cfg->n_ports && q < cfg->n_ports; ++q)
            if (q != p && cfg->vlan_id[q] == cfg->vlan_id[p]) m |= 1ull << q;  // :104-112
        s->flood[p] = m;
    }
    s->ops = ops;
    if (ops) {
        const int rc = ops->create(s);
        if (rc) {
            delete s;
            return rc;
        }
    }
    *out = s;
    return HALO_OK;
}

extern "C" HALO_API int halo_switch_destroy(halo_switch_t* s) {
    if (!s) return HALO_E_INVAL;
    if (s->ops) s->ops->destroy(s);
    delete s;
    return HALO_OK;
}

extern "C" HALO_API int halo_switch_flood_mask(const halo_switch_t* s, uint32_t port, uint64_t* mask) {
    if (!s || !mask || port >= s->cfg.n_ports) return HALO_E_INVAL;
    *mask = s->flood[port];
    return HALO_OK;
}

extern "C" HALO_API int halo_switch_forward(halo_switch_t* s, uint32_t port, const uint8_t* bytes,
                                            const uint32_t* offsets_dw, const uint16_t* lens, uint32_t n, uint32_t now,
                                            halo_sw_result_t* results, uint32_t* counts, halo_stream_t stream) {
    if (!s || port >= s->cfg.n_ports) return HALO_E_INVAL;
    if (n > s->cfg.max_batch) return HALO_E_RANGE;
    if (n == 0) return HALO_OK;
    if (!bytes || !offsets_dw || !lens || !results) return HALO_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(bytes) | reinterpret_cast<uintptr_t>(offsets_dw) |
         reinterpret_cast<uintptr_t>(results) | reinterpret_cast<uintptr_t>(counts)) & 3u)
        return HALO_E_INVAL;
    if (reinterpret_cast<uintptr_t>(lens) & 1u) return HALO_E_INVAL;
    if (s->ops) return s->ops->forward(s, port, bytes, offsets_dw, lens, n, now, results, counts, stream);
    forward_host(s, port, bytes, offsets_dw, lens, n, now, results, counts);
    return HALO_OK;
}

extern "C" HALO_API int halo_switch_expire(halo_switch_t* s, uint32_t now, uint32_t* n_removed) {
    if (!s) return HALO_E_INVAL;
    if (n_removed) *n_removed = 0;
    if (s->ops) return s->ops->expire(s, now, n_removed);
    uint32_t removed = 0;
    for (auto it = s->table.begin(); it != s->table.end();) {
        if (expired(now, it->second.create_time)) {
            it = s->table.erase(it);
            ++removed;
        } else {
            ++it;
        }
    }
    if (n_removed) *n_removed = removed;
    return HALO_OK;
}

extern "C" HALO_API int halo_switch_list(halo_switch_t* s, halo_switch_entry_t* out, uint32_t cap, uint32_t* n) {
    if (!s || !n || (cap && !out)) return HALO_E_INVAL;
    uint32_t total = 0;
    if (s->ops) {
        std::vector<Slot> slots;
        const int rc = s->ops->snapshot(s, &slots);
        if (rc) return rc;
        for (const Slot& e : slots) {
            if (!e.key) continue;
            if (total < cap) store_entry(e.key & kMacMask, e.port, e.create_time, out + total);
            ++total;
        }
    } else {
        for (const auto& kv : s->table) {
            if (total < cap) store_entry(kv.first, kv.second.port, kv.second.create_time, out + total);
            ++total;
        }
    }
    *n = total;
    return HALO_OK;
}

extern "C" HALO_API int halo_switch_debug_set_epoch(halo_switch_t* s, uint32_t epoch) {
    if (!s || !s->ops) return HALO_E_INVAL;  // a host switch has no scratch set
    return s->ops->set_epoch(s, epoch);
}

extern "C" HALO_API int halo_switch_layout_stats(halo_switch_t* s, halo_switch_layout_stats_t* out) {
    if (!s || !out) return HALO_E_INVAL;
    memset(out, 0, sizeof *out);
    out->slots = s->slots;
    if (!s->ops) {
        out->entries = (uint32_t)s->table.size();
        return HALO_OK;
    }
    std::vector<Slot> slots;
    const int rc = s->ops->snapshot(s, &slots);
    if (rc) return rc;
    const uint32_t mask = s->slots - 1;
    for (uint32_t k = 0; k < slots.size(); ++k) {
        if (!slots[k].key) continue;
        const uint32_t home = mac_hash(slots[k].key & kMacMask) & mask;
        const uint32_t chain = ((k - home) & mask) + 1;
        ++out->entries;
        if (chain > out->longest_chain) out->longest_chain = chain;
        if (k < home) ++out->wrapped;
    }
    return HALO_OK;
}
