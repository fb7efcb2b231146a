// nat_table.cc — the host control plane of the NAT flow table (include/halo_rx.h, "NAT flow
// table"): NatAddFlow, NatGetFlowByHash / ByWan, CheckNatPortMapping, NatTableClear and ListNat of
// engine/ipv4_engine.go:524-759 restated over std containers, the slow path for device misses,
// and the compile of both indexes into the open-addressing image nat_lookup.hip uploads. The
// device side is reached through nat::DeviceOps. No HIP.
#include "nat_table.h"

#include <string.h>

#include <new>

using halo::flowkey::Key;
using namespace halo::nat;

namespace halo {
namespace nat {

uint32_t PortSet::take() {
    // wanPort := 32768; for used { wanPort++; if wanPort == 0 break } (:622-636)
    for (size_t w = 0; w < 512; ++w) {
        if (w >= bits.size()) bits.resize(w + 1, 0);
        const uint64_t free_bits = ~bits[w];
        if (!free_bits) continue;
        const uint32_t b = (uint32_t)__builtin_ctzll(free_bits);
        bits[w] |= 1ull << b;
        ++used;
        return 32768u + (uint32_t)w * 64u + b;
    }
    return 0;
}

void PortSet::release(uint32_t port) {
    if (port < 32768u || port > 65535u) return;
    const size_t w = (port - 32768u) / 64u;
    const uint64_t m = 1ull << ((port - 32768u) % 64u);
    if (w < bits.size() && (bits[w] & m)) {
        bits[w] &= ~m;
        --used;
    }
}

namespace {

// the normalisation of :525-537 / :555-567 / :588-599
Key norm_key(const halo_nat_table& t, uint32_t rip, uint32_t rport, uint32_t lip, uint32_t lport, uint32_t proto) {
    if (t.cfg.nat_type != HALO_NAT_SYMMETRIC) rip = 0, rport = 0;
    if (proto == 1u) rport = 0;
    return Key{rip, rport, lip, lport, proto};
}

const halo_nat_flow_t kNoFlow = {0, 0, 0, 0, 0, 0, 0, 0, 0, HALO_NAT_NO_FLOW};

void report(const Flow* f, halo_nat_flow_t* out, uint32_t* flow_id) {
    if (out) *out = f ? f->f : kNoFlow;
    if (flow_id) *flow_id = f ? f->f.id : HALO_NAT_NO_FLOW;
}

Flow* find(const std::unordered_map<Key, Flow*, KeyHash, KeyEq>& m, const Key& k) {
    auto it = m.find(k);
    return it == m.end() ? nullptr : it->second;
}

// NatAddFlow (:584-680); t.mu held
Flow* add_flow(halo_nat_table& t, uint32_t lan_ip, uint32_t remote_ip, uint32_t lan_port, uint32_t remote_port,
               uint32_t proto, uint32_t now) {
    if (lan_port == 0 || remote_port == 0) return nullptr;
    if (t.next_id == HALO_NAT_NO_FLOW) return nullptr;  // ids are never reused: the id space is spent
    const Key lk = norm_key(t, remote_ip, remote_port, lan_ip, lan_port, proto);
    PortSet& pa = t.ports[lk.rip];
    const uint32_t wan_port = pa.take();
    if (wan_port == 0) return nullptr;
    const uint32_t id = t.next_id++;
    Flow fl{};
    fl.f.remote_ip = lk.rip;
    fl.f.remote_port = (uint16_t)lk.rport;
    fl.f.wan_ip = t.cfg.wan_ip;
    fl.f.wan_port = (uint16_t)wan_port;
    fl.f.lan_ip = lan_ip;
    fl.f.lan_port = (uint16_t)lan_port;
    fl.f.proto = (uint8_t)proto;
    fl.f.last_alive = now;
    fl.f.id = id;
    fl.in_lan = true;
    Flow* p = &t.flows.emplace_hint(t.flows.end(), id, fl)->second;
    Flow*& slot = t.lan[lk];
    if (slot) {  // HashMap.Set on an existing key replaces the value: the old flow keeps its WAN key and port
        slot->in_lan = false;
        --t.n_lan;
    }
    slot = p;
    ++t.n_lan;
    t.wan[Key{lk.rip, lk.rport, t.cfg.wan_ip, wan_port, proto}] = p;
    return p;
}

// CheckNatPortMapping (:683-707): index of the first match, -1 for none
int check_mapping(const halo_nat_table& t, uint32_t dir, uint32_t ip, uint32_t port, uint32_t proto) {
    if (proto != 6u && proto != 17u) return -1;
    for (size_t k = 0; k < t.maps.size(); ++k) {
        const PortMapping& e = t.maps[k];
        if (dir == HALO_FLOW_NAT_WAN ? (e.wan_port == port && e.proto == proto)
                                     : (e.lan_ip == ip && e.lan_port == port && e.proto == proto))
            return (int)k;
    }
    return -1;
}

const DeviceOps* dev_ops(const halo_nat_table* t) {  // null: host-only build, or never synced
    return t->dev.load(std::memory_order_acquire) && device_ops ? device_ops() : nullptr;
}

}  // namespace

int compile(const halo_nat_table& t, Image* out, bool with_stamps) {
    std::lock_guard<std::mutex> g(t.mu);
    const uint32_t n_lan = t.n_lan, n_wan = (uint32_t)t.wan.size();
    const int rc = flowtab::capacity_slots(t.cfg.capacity_log2, n_lan > n_wan ? n_lan : n_wan, &out->slots);
    if (rc) return rc;
    const uint32_t mask = out->slots - 1;
    halo_nat_layout_stats_t st{};
    st.slots = out->slots;
    st.port_mappings = (uint32_t)t.maps.size();
    for (auto& v : out->index) v.assign(out->slots, Slot{});
    const auto put = [&](uint32_t dir, const Key& k, uint32_t x_ip, uint32_t x_port, uint32_t id) {
        Slot* idx = out->index[dir].data();
        const uint32_t s = flowtab::place(idx, mask, flowtab::home_slot(k, mask), &st.entries[dir], &st.longest_chain[dir],
                                          &st.wrapped[dir]);
        idx[s] = Slot{k.rip, k.lip, k.rport | k.lport << 16, kSlotUsed | k.proto, x_ip, x_port, id, 0};
    };
    for (const auto& kv : t.flows) {  // ascending id: the layout depends on the table's history only
        const halo_nat_flow_t& f = kv.second.f;
        if (kv.second.in_lan)
            put(HALO_FLOW_NAT_LAN, Key{f.remote_ip, f.remote_port, f.lan_ip, f.lan_port, f.proto}, f.wan_ip, f.wan_port, f.id);
        put(HALO_FLOW_NAT_WAN, Key{f.remote_ip, f.remote_port, f.wan_ip, f.wan_port, f.proto}, f.lan_ip, f.lan_port, f.id);
    }
    out->maps.clear();
    for (const PortMapping& e : t.maps)
        out->maps.push_back(MapWord{(uint32_t)e.wan_port | (uint32_t)e.lan_port << 16, e.lan_ip, e.proto});
    out->stamps.clear();
    if (with_stamps) {
        out->stamps.assign(t.next_id, 0u);
        for (const auto& kv : t.flows) out->stamps[kv.first] = kv.second.f.last_alive;
    }
    out->stats = st;
    return HALO_OK;
}

void merge_stamps(halo_nat_table& t, const uint32_t* dev, uint32_t n) {
    std::lock_guard<std::mutex> g(t.mu);
    flowtab::merge_stamps(t.flows, dev, n, [](Flow& fl) -> uint32_t& { return fl.f.last_alive; });
}

}  // namespace nat
}  // namespace halo

extern "C" HALO_API int halo_nat_table_create(const halo_nat_config_t* cfg, halo_nat_table_t** out) {
    if (!cfg || !out) return HALO_E_INVAL;
    if (cfg->capacity_log2 > 28) return HALO_E_RANGE;
    auto* t = new (std::nothrow) halo_nat_table;
    if (!t) return HALO_E_NOMEM;
    t->cfg = *cfg;
    *out = t;
    return HALO_OK;
}

extern "C" HALO_API int halo_nat_table_destroy(halo_nat_table_t* t) {
    if (!t) return HALO_E_INVAL;
    if (const DeviceOps* ops = dev_ops(t)) ops->destroy(t);
    delete t;
    return HALO_OK;
}

extern "C" HALO_API int halo_nat_port_mapping_add(halo_nat_table_t* t, uint16_t wan_port, uint32_t lan_ip,
                                                  uint16_t lan_port, uint8_t proto) {
    if (!t) return HALO_E_INVAL;
    std::lock_guard<std::mutex> g(t->mu);
    if (t->maps.size() >= HALO_NAT_MAX_PORT_MAPPINGS) return HALO_E_RANGE;
    t->maps.push_back(PortMapping{wan_port, lan_port, lan_ip, proto});
    return HALO_OK;
}

extern "C" HALO_API int halo_nat_add_flow(halo_nat_table_t* t, uint32_t lan_ip, uint32_t remote_ip, uint16_t lan_port,
                                          uint16_t remote_port, uint8_t proto, uint32_t now, halo_nat_flow_t* out,
                                          uint32_t* flow_id) {
    if (!t) return HALO_E_INVAL;
    std::lock_guard<std::mutex> g(t->mu);
    report(add_flow(*t, lan_ip, remote_ip, lan_port, remote_port, proto, now), out, flow_id);
    return HALO_OK;
}

extern "C" HALO_API int halo_nat_get_flow_lan(const halo_nat_table_t* t, uint32_t remote_ip, uint16_t remote_port,
                                              uint32_t lan_ip, uint16_t lan_port, uint8_t proto, halo_nat_flow_t* out,
                                              uint32_t* flow_id) {
    if (!t) return HALO_E_INVAL;
    std::lock_guard<std::mutex> g(t->mu);
    report(find(t->lan, norm_key(*t, remote_ip, remote_port, lan_ip, lan_port, proto)), out, flow_id);
    return HALO_OK;
}

extern "C" HALO_API int halo_nat_get_flow_wan(const halo_nat_table_t* t, uint32_t remote_ip, uint16_t remote_port,
                                              uint32_t wan_ip, uint16_t wan_port, uint8_t proto, halo_nat_flow_t* out,
                                              uint32_t* flow_id) {
    if (!t) return HALO_E_INVAL;
    std::lock_guard<std::mutex> g(t->mu);
    report(find(t->wan, norm_key(*t, remote_ip, remote_port, wan_ip, wan_port, proto)), out, flow_id);
    return HALO_OK;
}

namespace {

// One record of the miss slow path, t.mu held: CheckNatPortMapping, then the host flow lookup,
// then (LAN) NatAddFlow; nil is DROP (:214-217), a WAN miss stays MISS (:120-124), a hit stamps
// the flow. The one copy halo_nat_resolve_misses and halo_nat_resolve_items share.
halo_nat_answer_t resolve_one(halo_nat_table& t, bool wan, uint32_t proto, uint32_t src_ip, uint32_t dst_ip, uint32_t sport,
                              uint32_t dport, uint32_t now, uint32_t* added) {
    halo_nat_answer_t a{};
    a.ref = HALO_NAT_NO_FLOW;
    a.verdict = HALO_NAT_V_MISS;
    const int m = wan ? check_mapping(t, HALO_FLOW_NAT_WAN, 0, dport, proto) : check_mapping(t, HALO_FLOW_NAT_LAN, src_ip, sport, proto);
    if (m >= 0) {
        const PortMapping& e = t.maps[(size_t)m];
        a.ip = wan ? e.lan_ip : t.cfg.wan_ip;
        a.port = wan ? e.lan_port : e.wan_port;
        a.ref = (uint32_t)m;
        a.verdict = HALO_NAT_V_MAPPING;
        return a;
    }
    Flow* f;
    if (wan) {
        f = find(t.wan, norm_key(t, src_ip, sport, dst_ip, dport, proto));
        if (!f) return a;  // stays MISS: local delivery (:120-124)
    } else {
        f = find(t.lan, norm_key(t, dst_ip, dport, src_ip, sport, proto));
        if (!f) {
            f = add_flow(t, src_ip, dst_ip, sport, dport, proto, now);
            if (!f) {
                a.verdict = HALO_NAT_V_DROP;  // :214-217
                return a;
            }
            ++*added;
        }
    }
    f->f.last_alive = now;
    a.ip = wan ? f->f.lan_ip : f->f.wan_ip;
    a.port = wan ? f->f.lan_port : f->f.wan_port;
    a.ref = f->f.id;
    a.verdict = HALO_NAT_V_FLOW;
    return a;
}

}  // namespace

extern "C" HALO_API int halo_nat_resolve_misses(halo_nat_table_t* t, uint32_t dir, const halo_rx_result_t* records,
                                                const uint8_t* verdicts, uint32_t n, uint32_t now, halo_tx_op_t* ops,
                                                uint8_t* verdicts_out, uint32_t* n_added) {
    if (!t || (dir != HALO_FLOW_NAT_LAN && dir != HALO_FLOW_NAT_WAN)) return HALO_E_INVAL;
    if (n_added) *n_added = 0;
    if (n == 0) return HALO_OK;
    if (!records || !verdicts || !ops || !verdicts_out) return HALO_E_INVAL;
    const bool wan = dir == HALO_FLOW_NAT_WAN;
    uint32_t added = 0;
    std::lock_guard<std::mutex> g(t->mu);
    for (uint32_t i = 0; i < n; ++i) {  // ascending: NatAddFlow's port depends on packet order
        const uint8_t v = verdicts[i];
        verdicts_out[i] = v;
        if (v != HALO_NAT_V_MISS) continue;
        const halo_rx_result_t& r = records[i];
        const halo_nat_answer_t a = resolve_one(*t, wan, r.ip_proto, r.src_ip, r.dst_ip, r.sport, r.dport, now, &added);
        verdicts_out[i] = a.verdict;
        if (a.verdict != HALO_NAT_V_FLOW && a.verdict != HALO_NAT_V_MAPPING) continue;
        halo_tx_op_t& op = ops[i];
        if (wan) {
            op.steps |= HALO_TX_NAT_DST;
            op.dst_ip = a.ip;
            op.dst_port = a.port;
        } else {
            op.steps |= HALO_TX_NAT_SRC;
            op.src_ip = a.ip;
            op.src_port = a.port;
        }
    }
    if (n_added) *n_added = added;
    return HALO_OK;
}

extern "C" HALO_API int halo_nat_resolve_items(halo_nat_table_t* t, uint32_t dir, const halo_nat_miss_item_t* items,
                                               uint32_t k, uint32_t now, halo_nat_answer_t* answers, uint32_t* n_added) {
    if (!t || (dir != HALO_FLOW_NAT_LAN && dir != HALO_FLOW_NAT_WAN)) return HALO_E_INVAL;
    if (n_added) *n_added = 0;
    if (k == 0) return HALO_OK;
    if (!items || !answers) return HALO_E_INVAL;
    uint32_t added = 0;
    std::lock_guard<std::mutex> g(t->mu);
    for (uint32_t j = 0; j < k; ++j) {  // list order = ascending record index
        const halo_nat_miss_item_t& it = items[j];
        answers[j] = resolve_one(*t, dir == HALO_FLOW_NAT_WAN, it.proto, it.src_ip, it.dst_ip, it.sport, it.dport, now, &added);
    }
    if (n_added) *n_added = added;
    return HALO_OK;
}

// A LAN record no other record may answer for, and that answers for no other (include/halo_rx.h,
// "the miss path"): NatAddFlow refuses its raw remote port 0, yet its normalised key may be shared.
static bool miss_listed_alone(uint32_t dir, uint32_t sport, uint32_t dport) {
    return dir == HALO_FLOW_NAT_LAN && dport == 0 && sport != 0;
}

extern "C" HALO_API int halo_nat_collect_misses_host(const halo_nat_table_t* t, uint32_t dir,
                                                     const halo_rx_result_t* records, const uint8_t* verdict,
                                                     const uint8_t* select, uint32_t n, halo_nat_miss_item_t* items,
                                                     uint32_t cap, uint32_t* count, uint32_t* pos) {
    if (!t || (dir != HALO_FLOW_NAT_LAN && dir != HALO_FLOW_NAT_WAN) || !count || (cap && !items)) return HALO_E_INVAL;
    if (n && (!records || !verdict || !pos)) return HALO_E_INVAL;
    std::unordered_map<Key, uint32_t, KeyHash, KeyEq> first;  // normalised key -> list position
    uint32_t k = 0;
    for (uint32_t i = 0; i < n; ++i) {
        pos[i] = HALO_NAT_NO_FLOW;
        if (verdict[i] != HALO_NAT_V_MISS || (select && !select[i])) continue;
        const halo_rx_result_t& r = records[i];
        if (!miss_listed_alone(dir, r.sport, r.dport)) {
            const auto ins =
                first.emplace(halo::flowkey::nat_key(r.ip_proto, r.src_ip, r.dst_ip, r.sport, r.dport, dir, t->cfg.nat_type), k);
            if (!ins.second) {
                pos[i] = ins.first->second;
                continue;
            }
        }
        if (k < cap) {
            halo_nat_miss_item_t it{};
            it.index = i, it.src_ip = r.src_ip, it.dst_ip = r.dst_ip, it.sport = r.sport, it.dport = r.dport, it.proto = r.ip_proto;
            items[k] = it;
        }
        pos[i] = k++;
    }
    *count = k;
    return HALO_OK;
}

extern "C" HALO_API uint64_t halo_nat_miss_workspace(uint32_t n, uint32_t scratch_log2) {
    const uint64_t slots = miss_slots(n, scratch_log2);
    const uint64_t tiles = miss_tiles(n);
    return slots ? 4 * (slots + (tiles ? tiles : 1) + n) : 0;
}

// halo_nat_collect_misses_device and halo_nat_collect_misses_compact_device: the argument checks,
// then DeviceOps::collect / collect_compact.
#define HALO_NAT_COLLECT(NAME, RECORD, OP)                                                                              \
    extern "C" HALO_API int NAME(const halo_nat_table_t* t, uint32_t dir, const RECORD* d_records,                      \
                                 const uint8_t* d_verdict, const uint8_t* d_select, uint32_t n, uint32_t scratch_log2,  \
                                 halo_nat_miss_item_t* d_items, uint32_t cap, uint32_t* d_count, uint32_t* d_pos,       \
                                 void* d_workspace, uint64_t workspace_bytes, halo_stream_t stream) {                   \
        if (!t || (dir != HALO_FLOW_NAT_LAN && dir != HALO_FLOW_NAT_WAN) || !d_count || (cap && !d_items))              \
            return HALO_E_INVAL;                                                                                        \
        if (n && (!d_records || !d_verdict || !d_pos || !d_workspace)) return HALO_E_INVAL;                             \
        if (reinterpret_cast<uintptr_t>(d_records) & 15u) return HALO_E_INVAL;                                          \
        if ((reinterpret_cast<uintptr_t>(d_items) | reinterpret_cast<uintptr_t>(d_count) |                              \
             reinterpret_cast<uintptr_t>(d_pos) | reinterpret_cast<uintptr_t>(d_workspace)) & 3u)                       \
            return HALO_E_INVAL;                                                                                        \
        const uint32_t slots = miss_slots(n, scratch_log2);                                                             \
        if (slots <= n) return HALO_E_RANGE;                                                                            \
        if (n && workspace_bytes < halo_nat_miss_workspace(n, scratch_log2)) return HALO_E_INVAL;                       \
        if (!device_ops) return HALO_E_NODEV;                                                                           \
        return device_ops()->OP(t, dir, d_records, d_verdict, d_select, n, slots, d_items, cap, d_count, d_pos,         \
                                d_workspace, stream);                                                                   \
    }
HALO_NAT_COLLECT(halo_nat_collect_misses_device, halo_rx_result_t, collect)
HALO_NAT_COLLECT(halo_nat_collect_misses_compact_device, halo_rx_record16_t, collect_compact)
#undef HALO_NAT_COLLECT

extern "C" HALO_API int halo_nat_apply_answers_device(uint32_t dir, const uint32_t* d_pos, uint32_t n,
                                                      const halo_nat_answer_t* d_answers, uint32_t k, halo_tx_op_t* d_ops,
                                                      uint8_t* d_verdict, uint32_t* d_ref, uint32_t* d_counts,
                                                      halo_stream_t stream) {
    if (dir != HALO_FLOW_NAT_LAN && dir != HALO_FLOW_NAT_WAN) return HALO_E_INVAL;
    if (n && (!d_pos || !d_ops || !d_verdict || !d_ref || (k && !d_answers))) return HALO_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_answers) | reinterpret_cast<uintptr_t>(d_ops)) & 15u) return HALO_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_pos) | reinterpret_cast<uintptr_t>(d_ref) | reinterpret_cast<uintptr_t>(d_counts)) & 3u)
        return HALO_E_INVAL;
    if (!device_ops) return HALO_E_NODEV;
    return device_ops()->apply(dir, d_pos, n, d_answers, k, d_ops, d_verdict, d_ref, d_counts, stream);
}

extern "C" HALO_API int halo_nat_expire(halo_nat_table_t* t, uint32_t now, uint32_t* n_removed) {
    if (!t) return HALO_E_INVAL;
    if (n_removed) *n_removed = 0;
    std::lock_guard<std::mutex> sg(t->sync_mu);
    const DeviceOps* ops = dev_ops(t);
    int rc;
    if (ops && (rc = ops->fold(t))) return rc;
    uint32_t removed = 0;
    {
        std::lock_guard<std::mutex> g(t->mu);
        for (auto it = t->flows.begin(); it != t->flows.end();) {
            Flow& fl = it->second;
            if (!fl.in_lan || (uint32_t)(now - fl.f.last_alive) <= 60u) {  // NatFlowTable.For (:731-732)
                ++it;
                continue;
            }
            const halo_nat_flow_t& f = fl.f;
            t->lan.erase(Key{f.remote_ip, f.remote_port, f.lan_ip, f.lan_port, f.proto});
            t->wan.erase(Key{f.remote_ip, f.remote_port, f.wan_ip, f.wan_port, f.proto});
            --t->n_lan;
            auto pa = t->ports.find(f.remote_ip);
            if (pa != t->ports.end()) {
                pa->second.release(f.wan_port);
                if (pa->second.used == 0) t->ports.erase(pa);  // :748-752
            }
            it = t->flows.erase(it);
            ++removed;
        }
    }
    if (n_removed) *n_removed = removed;
    // the device must stop answering with the flows that left
    return removed && ops ? ops->publish(t) : HALO_OK;
}

extern "C" HALO_API int halo_nat_list(const halo_nat_table_t* t, halo_nat_flow_t* out, uint32_t cap, uint32_t* n) {
    if (!t || !n || (cap && !out)) return HALO_E_INVAL;
    std::lock_guard<std::mutex> g(t->mu);
    uint32_t k = 0;
    for (const auto& kv : t->flows) {
        if (!kv.second.in_lan) continue;
        if (k < cap) out[k] = kv.second.f;
        ++k;
    }
    *n = k;
    return HALO_OK;
}

extern "C" HALO_API int halo_nat_layout_stats(const halo_nat_table_t* t, halo_nat_layout_stats_t* out) {
    if (!t || !out) return HALO_E_INVAL;
    Image img;
    const int rc = compile(*t, &img, false);
    if (rc) return rc;
    *out = img.stats;
    return HALO_OK;
}

extern "C" HALO_API int halo_nat_sync_device(halo_nat_table_t* t, int device) {
    if (!t || device < 0) return HALO_E_INVAL;
    if (!device_ops) return HALO_E_NODEV;
    std::lock_guard<std::mutex> sg(t->sync_mu);
    return device_ops()->sync(t, device);
}

// halo_nat_lookup_wan_device, halo_nat_lookup_lan_device, halo_nat_lookup_wan_compact_device and
// halo_nat_lookup_lan_compact_device: halo_nat_lookup_<WHICH>_device over RECORD is DeviceOps::lookup_<WHICH>.
#define HALO_NAT_LOOKUP(WHICH, RECORD)                                                                                  \
    extern "C" HALO_API int halo_nat_lookup_##WHICH##_device(                                                           \
        const halo_nat_table_t* t, const RECORD* d_records, uint32_t n, uint32_t now, const uint8_t* d_skip,            \
        halo_tx_op_t* d_ops, uint8_t* d_verdict, uint32_t* d_ref, uint32_t* d_miss_count, halo_stream_t stream) {       \
        if (!t) return HALO_E_INVAL;                                                                                    \
        if (!device_ops) return HALO_E_NODEV;                                                                           \
        return device_ops()->lookup_##WHICH(t, d_records, n, now, d_skip, d_ops, d_verdict, d_ref, d_miss_count, stream); \
    }
HALO_NAT_LOOKUP(wan, halo_rx_result_t)
HALO_NAT_LOOKUP(lan, halo_rx_result_t)
HALO_NAT_LOOKUP(wan_compact, halo_rx_record16_t)
HALO_NAT_LOOKUP(lan_compact, halo_rx_record16_t)
#undef HALO_NAT_LOOKUP

extern "C" HALO_API int halo_nat_lookup_quote_device(const halo_nat_table_t* t, const halo_rx_result_t* d_quote_records,
                                                     uint32_t n, halo_tx_deep_nat_t* d_nat, halo_stream_t stream) {
    if (!t) return HALO_E_INVAL;
    return device_ops ? device_ops()->quote(t, d_quote_records, n, d_nat, stream) : HALO_E_NODEV;
}
