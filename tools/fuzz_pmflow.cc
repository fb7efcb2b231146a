// fuzz_pmflow.cc — the port-mapping return-flow table's host control plane
// (halo_amd/csrc/pmflow_table.cc, the file libhalo_rx.so links) under ASan/UBSan: a stand-alone
// program that makes random create / record / get / expire / list / layout_stats / dirty calls
// through the public C ABI — a small key universe so that tables fill up, `now` across the uint32
// wrap, item, dropped and list buffers of exactly the size the call needs — and checks each result
// against a map-based restatement. tests/test_sanitize_pmflow.py builds and runs it.
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ihalo_amd/csrc
//       halo_amd/csrc/pmflow_table.cc tools/fuzz_pmflow.cc -o fuzz_pmflow && ./fuzz_pmflow 200000 0x5EED
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <tuple>
#include <vector>

#include "halo_rx.h"

static uint64_t g_state;
static uint32_t rnd(uint32_t n) {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) % n);
}

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);    \
            return 1;                                                  \
        }                                                              \
    } while (0)

typedef std::tuple<uint32_t, uint16_t, uint32_t, uint16_t, uint8_t> Key;  // remote ip, port, lan ip, port, proto
struct Val {
    uint32_t wan_netif, wan_port, last_alive, id;
};
struct Tab {
    halo_pmflow_table_t* h = nullptr;
    halo_pmflow_config_t cfg{};
    std::map<Key, Val> model;
    uint32_t next_id = 0;
};

static int make(Tab* t) {
    if (t->h) CHECK(halo_pmflow_table_destroy(t->h) == HALO_OK);
    t->h = nullptr;
    t->model.clear();
    t->next_id = 0;
    memset(&t->cfg, 0, sizeof t->cfg);
    t->cfg.n_netifs = 1 + rnd(rnd(4) ? 3 : 64);
    for (uint32_t q = 0; q < t->cfg.n_netifs; ++q) {
        t->cfg.netif[q].ip = 0x0A000001u + (q << 8);
        t->cfg.netif[q].nat_enable = rnd(2);
        t->cfg.gateway[q] = rnd(3) ? 0x0A0000FEu + (q << 8) : 0;
    }
    t->cfg.capacity = 1 + rnd(rnd(3) ? 6 : 40);
    t->cfg.capacity_log2 = rnd(3) ? 0 : 4;  // 16 slots: a table of 16 or more flows is a RANGE error
    CHECK(halo_pmflow_table_create(&t->cfg, &t->h) == HALO_OK);
    return 0;
}

static Key random_key() {
    return Key{0x08080800u + rnd(5), (uint16_t)(1 + rnd(4)), 0xC0A80114u + rnd(2), (uint16_t)(rnd(2) ? 80 : 443),
               (uint8_t)(rnd(2) ? 6 : 17)};
}

int main(int argc, char** argv) {
    const long calls = argc > 1 ? strtol(argv[1], nullptr, 0) : 200000;
    g_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x5EED;
    Tab tabs[3];
    for (auto& t : tabs)
        if (make(&t)) return 1;
    uint32_t now = 0xFFFFF000u;  // crosses the uint32 wrap
    unsigned long creates = 3, items_total = 0, added_total = 0, dropped_total = 0, overwritten = 0, removed_total = 0;
    unsigned long lists = 0, get_hits = 0, get_misses = 0, ranges = 0, refused = 0;
    for (long c = 0; c < calls; ++c) {
        Tab& t = tabs[rnd(3)];
        const uint32_t nn = t.cfg.n_netifs;
        switch (rnd(12)) {
            case 0: {
                if (rnd(8) == 0) {
                    if (make(&t)) return 1;
                    ++creates;
                }
                break;
            }
            case 1: case 2: {
                now += rnd(30);
                break;
            }
            case 3: {
                uint32_t want = 0, removed = 0xDEAD;
                for (auto it = t.model.begin(); it != t.model.end();)
                    if ((uint32_t)(now - it->second.last_alive) > 60u) it = t.model.erase(it), ++want;
                    else ++it;
                const bool report = rnd(4) != 0;  // n_removed is optional
                CHECK(halo_pmflow_expire(t.h, now, report ? &removed : nullptr) == HALO_OK);  // no device copy: no fold, no publish
                CHECK(removed == (report ? want : 0xDEADu));
                removed_total += want;
                break;
            }
            case 4: {
                const uint32_t cap = rnd(3) ? rnd(5) : 64u;
                std::vector<halo_pmflow_entry_t> exact(cap);  // exactly `cap`: an overrun is ASan's to find
                uint32_t total = 0;
                CHECK(halo_pmflow_list(t.h, cap ? exact.data() : nullptr, cap, &total) == HALO_OK);
                CHECK(total == t.model.size());
                for (uint32_t i = 0; i < cap && i < total; ++i) {
                    const halo_pmflow_entry_t& e = exact[i];
                    const auto it = t.model.find(Key{e.remote_ip, e.remote_port, e.lan_ip, e.lan_port, e.proto});
                    CHECK(it != t.model.end() && it->second.wan_netif == e.wan_netif && it->second.wan_port == e.wan_port &&
                          it->second.last_alive == e.last_alive && it->second.id == e.id);
                    if (i) CHECK(exact[i - 1].id < e.id);  // ascending id
                }
                ++lists;
                break;
            }
            case 5: {
                halo_pmflow_layout_stats_t st;
                const int rc = halo_pmflow_layout_stats(t.h, &st);
                if (t.cfg.capacity_log2 && t.model.size() >= 16) {
                    CHECK(rc == HALO_E_RANGE);
                    ++ranges;
                } else {
                    CHECK(rc == HALO_OK);
                    CHECK((st.slots & (st.slots - 1)) == 0 && st.slots > t.model.size() && st.entries == t.model.size());
                    CHECK(st.slots >= 2 * st.entries || t.cfg.capacity_log2);
                    CHECK(st.longest_chain <= st.entries && (st.entries == 0) == (st.longest_chain == 0) && st.wrapped <= st.entries);
                }
                CHECK(halo_pmflow_dirty(t.h) == 1);  // no device copy in this build
                break;
            }
            case 6: case 7: {
                const Key k = random_key();
                halo_pmflow_entry_t e;
                memset(&e, 0xEE, sizeof e);
                uint32_t found = 99;
                const bool stamp = rnd(2) != 0;
                CHECK(halo_pmflow_get(t.h, std::get<0>(k), std::get<1>(k), std::get<2>(k), std::get<3>(k), std::get<4>(k),
                                      stamp ? &now : nullptr, rnd(4) ? &e : nullptr, &found) == HALO_OK);
                const auto it = t.model.find(k);
                CHECK(found == (it != t.model.end() ? 1u : 0u));
                if (it != t.model.end() && stamp) it->second.last_alive = now;
                ++(found ? get_hits : get_misses);
                break;
            }
            default: {
                const uint32_t n = rnd(7), nif = rnd(nn);
                std::vector<halo_pmflow_item_t> items(n);  // exactly n
                std::vector<uint8_t> got(n), want(n);
                for (uint32_t i = 0; i < n; ++i) {
                    const Key k = random_key();
                    items[i] = halo_pmflow_item_t{i, std::get<0>(k), std::get<2>(k), std::get<1>(k), std::get<3>(k),
                                                  (uint16_t)(8000 + rnd(3)), std::get<4>(k), 0};
                }
                if (n && rnd(16) == 0) {  // an item no NatPortMappingEntry can produce: nothing applied
                    items[n - 1].proto = 1;
                    CHECK(halo_pmflow_record(t.h, nif, items.data(), n, now, got.data(), nullptr) == HALO_E_INVAL);
                    CHECK(halo_pmflow_record(t.h, nn, items.data(), n, now, got.data(), nullptr) == HALO_E_RANGE);
                    uint32_t total = 0;
                    CHECK(halo_pmflow_list(t.h, nullptr, 0, &total) == HALO_OK && total == t.model.size());
                    ++refused;
                    break;
                }
                uint32_t want_added = 0;
                for (uint32_t i = 0; i < n; ++i) {
                    const halo_pmflow_item_t& it = items[i];
                    const Key k{it.remote_ip, it.remote_port, it.lan_ip, it.lan_port, it.proto};
                    auto f = t.model.find(k);
                    if (f == t.model.end()) {
                        if (t.model.size() >= t.cfg.capacity) {
                            want[i] = 1;
                            ++dropped_total;
                            continue;
                        }
                        f = t.model.emplace(k, Val{0, 0, 0, t.next_id++}).first;
                        ++want_added;
                    } else {
                        ++overwritten;
                    }
                    f->second.wan_netif = nif, f->second.wan_port = it.wan_port, f->second.last_alive = now;
                }
                uint32_t added = 0xDEAD;
                const bool report = rnd(4) != 0;
                CHECK(halo_pmflow_record(t.h, nif, n ? items.data() : nullptr, n, now, n ? got.data() : nullptr,
                                         report ? &added : nullptr) == HALO_OK);
                CHECK(got == want && added == (report ? want_added : 0xDEADu));
                items_total += n;
                added_total += want_added;
                break;
            }
        }
    }
    // this build has no device side
    uint32_t dummy = 0;
    CHECK(halo_pmflow_sync_device(tabs[0].h, nullptr, 0) == HALO_E_NODEV);
    CHECK(halo_pmflow_lookup_device(tabs[0].h, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ==
          HALO_E_NODEV);
    CHECK(halo_pmflow_record_device(tabs[0].h, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, &dummy, nullptr, 0,
                                    nullptr) == HALO_E_NODEV);
    CHECK(halo_arp_drop_device(nullptr, nullptr, 0, nullptr) == HALO_E_NODEV);
    CHECK(halo_pmflow_record_workspace(1000) == 16 + 1000);
    for (auto& t : tabs) CHECK(halo_pmflow_table_destroy(t.h) == HALO_OK);
    CHECK(halo_pmflow_table_destroy(nullptr) == HALO_E_INVAL);
    printf("pmflow fuzz: %ld calls, %lu tables, %lu items, %lu added, %lu dropped, %lu overwritten, %lu removed, %lu lists, "
           "%lu get hits, %lu get misses, %lu range, %lu refused\n",
           calls, creates, items_total, added_total, dropped_total, overwritten, removed_total, lists, get_hits, get_misses,
           ranges, refused);
    return 0;
}
