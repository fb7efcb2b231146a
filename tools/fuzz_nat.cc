// fuzz_nat.cc — the NAT flow table's host control plane (halo_amd/csrc/nat_table.cc, the file
// libhalo_rx.so links) under ASan/UBSan: a stand-alone program that drives random control-plane
// calls through the public C ABI — add, both gets, port mappings, the miss slow path, expire,
// list with a short cap, layout statistics at automatic and forced capacity — over a small key
// universe (so keys are replaced, ports run out of order and allocators empty) and checks the
// invariants a caller relies on, then that the sync and every device lookup of this host-only
// build answer HALO_E_NODEV. tests/test_sanitize_nat.py builds and runs it.
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ihalo_amd/csrc
//       halo_amd/csrc/nat_table.cc tools/fuzz_nat.cc -o fuzz_nat && ./fuzz_nat 300000 0x5EED
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

static const uint8_t kProtos[4] = {1, 6, 17, 47};

int main(int argc, char** argv) {
    const long calls = argc > 1 ? strtol(argv[1], nullptr, 0) : 300000;
    g_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x5EED;
    const uint32_t wan_ip = 0xCB007101u;
    halo_nat_table_t* tabs[4] = {};
    const halo_nat_config_t cfgs[4] = {{wan_ip, HALO_NAT_SYMMETRIC, 0, 0},
                                       {wan_ip, HALO_NAT_FULL_CONE, 0, 0},
                                       {wan_ip, HALO_NAT_SYMMETRIC, 5, 0},
                                       {wan_ip, 7, 4, 0}};  // an unknown nat_type behaves as full cone
    for (int k = 0; k < 4; ++k) CHECK(halo_nat_table_create(&cfgs[k], &tabs[k]) == HALO_OK);
    uint32_t now = 0xFFFFF000u;  // crosses the uint32 wrap
    unsigned long adds = 0, nils = 0, hits = 0, removed_total = 0, resolves = 0, range = 0, lists = 0;
    for (long c = 0; c < calls; ++c) {
        halo_nat_table_t* t = tabs[rnd(4)];
        const uint32_t lan_ip = 0xC0A80000u | rnd(6), remote_ip = 0x08080800u | rnd(4);
        const uint16_t lan_port = (uint16_t)(rnd(8) ? 1000 + rnd(40) : 0), remote_port = (uint16_t)(rnd(8) ? 50 + rnd(3) : 0);
        const uint8_t proto = kProtos[rnd(4)];
        switch (rnd(16)) {
            case 0: case 1: case 2: case 3: case 4: {
                halo_nat_flow_t f;
                uint32_t id = 0;
                CHECK(halo_nat_add_flow(t, lan_ip, remote_ip, lan_port, remote_port, proto, now, &f, &id) == HALO_OK);
                CHECK(f.id == id);
                if (id == HALO_NAT_NO_FLOW) {
                    ++nils;
                    break;
                }
                ++adds;
                CHECK(f.wan_port >= 32768 && f.wan_ip == wan_ip && f.lan_ip == lan_ip && f.last_alive == now);
                halo_nat_flow_t g;
                CHECK(halo_nat_get_flow_lan(t, remote_ip, remote_port, lan_ip, lan_port, proto, &g, nullptr) == HALO_OK);
                CHECK(g.id == id);
                CHECK(halo_nat_get_flow_wan(t, remote_ip, remote_port, wan_ip, f.wan_port, proto, &g, nullptr) == HALO_OK);
                CHECK(g.id == id);
                break;
            }
            case 5: case 6: {
                uint32_t id;
                CHECK(halo_nat_get_flow_lan(t, remote_ip, remote_port, lan_ip, lan_port, proto, nullptr, &id) == HALO_OK);
                hits += id != HALO_NAT_NO_FLOW;
                CHECK(halo_nat_get_flow_wan(t, remote_ip, remote_port, wan_ip, (uint16_t)(32768 + rnd(50)), proto, nullptr,
                                            &id) == HALO_OK);
                hits += id != HALO_NAT_NO_FLOW;
                break;
            }
            case 7: {
                const int rc = halo_nat_port_mapping_add(t, (uint16_t)(8000 + rnd(8)), lan_ip, lan_port, proto);
                CHECK(rc == HALO_OK || rc == HALO_E_RANGE);
                break;
            }
            case 8: case 9: case 10: {
                const uint32_t n = rnd(40), dir = rnd(2);
                std::vector<halo_rx_result_t> recs(n);
                std::vector<uint8_t> verd(n), out(n, 0xEE);
                std::vector<halo_tx_op_t> ops(n);
                if (n) memset(recs.data(), 0, n * sizeof(halo_rx_result_t)), memset(ops.data(), 0, n * sizeof(halo_tx_op_t));
                for (uint32_t i = 0; i < n; ++i) {
                    recs[i].ip_proto = rnd(10) ? kProtos[rnd(3)] : 0xFF;
                    recs[i].src_ip = dir == HALO_FLOW_NAT_LAN ? (0xC0A80000u | rnd(6)) : (0x08080800u | rnd(4));
                    recs[i].dst_ip = dir == HALO_FLOW_NAT_LAN ? (0x08080800u | rnd(4)) : wan_ip;
                    recs[i].sport = (uint16_t)(dir == HALO_FLOW_NAT_LAN ? 1000 + rnd(40) : 50 + rnd(3));
                    recs[i].dport = (uint16_t)(dir == HALO_FLOW_NAT_LAN ? 50 + rnd(3) : (rnd(4) ? 32768 + rnd(50) : 8000 + rnd(8)));
                    verd[i] = (uint8_t)(rnd(4) ? HALO_NAT_V_MISS : rnd(6));
                }
                uint32_t added = 0;
                CHECK(halo_nat_resolve_misses(t, dir, recs.data(), verd.data(), n, now, ops.data(), out.data(), &added) ==
                      HALO_OK);
                for (uint32_t i = 0; i < n; ++i) {
                    if (verd[i] != HALO_NAT_V_MISS) CHECK(out[i] == verd[i] && ops[i].steps == 0);
                    else CHECK(out[i] == HALO_NAT_V_MISS || out[i] == HALO_NAT_V_FLOW || out[i] == HALO_NAT_V_MAPPING ||
                               out[i] == HALO_NAT_V_DROP);
                    if (verd[i] == HALO_NAT_V_MISS && (out[i] == HALO_NAT_V_FLOW || out[i] == HALO_NAT_V_MAPPING))
                        CHECK(ops[i].steps == (dir == HALO_FLOW_NAT_LAN ? HALO_TX_NAT_SRC : HALO_TX_NAT_DST));
                }
                adds += added;
                ++resolves;
                break;
            }
            case 11: {
                now += rnd(40);
                break;
            }
            case 12: {
                uint32_t removed = 0, before = 0, after = 0;
                CHECK(halo_nat_list(t, nullptr, 0, &before) == HALO_OK);
                CHECK(halo_nat_expire(t, now, &removed) == HALO_OK);
                CHECK(halo_nat_list(t, nullptr, 0, &after) == HALO_OK);
                CHECK(before - removed == after);
                removed_total += removed;
                break;
            }
            case 13: case 14: {
                const uint32_t cap = rnd(3) ? rnd(8) : 64u;
                std::vector<halo_nat_flow_t> exact(cap);  // exactly `cap` entries: an overrun is ASan's to find
                uint32_t total = 0;
                CHECK(halo_nat_list(t, cap ? exact.data() : nullptr, cap, &total) == HALO_OK);
                for (uint32_t i = 0; i < cap && i < total; ++i) {
                    halo_nat_flow_t g;
                    // a listed flow is the value of its LAN key, and its WAN key finds it too
                    CHECK(halo_nat_get_flow_wan(t, exact[i].remote_ip, exact[i].remote_port, exact[i].wan_ip,
                                                exact[i].wan_port, exact[i].proto, &g, nullptr) == HALO_OK);
                    CHECK(g.id == exact[i].id);
                    CHECK(halo_nat_get_flow_lan(t, exact[i].remote_ip, exact[i].remote_port, exact[i].lan_ip,
                                                exact[i].lan_port, exact[i].proto, &g, nullptr) == HALO_OK);
                    CHECK(g.id == exact[i].id);
                }
                ++lists;
                break;
            }
            default: {
                halo_nat_layout_stats_t st;
                const int rc = halo_nat_layout_stats(t, &st);
                CHECK(rc == HALO_OK || rc == HALO_E_RANGE);
                if (rc == HALO_E_RANGE) {
                    ++range;
                    break;
                }
                CHECK((st.slots & (st.slots - 1)) == 0 && st.entries[0] < st.slots && st.entries[1] < st.slots);
                CHECK(st.entries[0] <= st.entries[1] && st.longest_chain[1] <= st.entries[1]);
                break;
            }
        }
    }
    // this build has no device side
    CHECK(halo_nat_sync_device(tabs[0], 0) == HALO_E_NODEV);
    CHECK(halo_nat_sync_device(tabs[0], -1) == HALO_E_INVAL && halo_nat_sync_device(nullptr, 0) == HALO_E_INVAL);
    CHECK(halo_nat_lookup_wan_device(tabs[0], nullptr, 0, now, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == HALO_E_NODEV);
    CHECK(halo_nat_lookup_lan_device(tabs[0], nullptr, 0, now, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == HALO_E_NODEV);
    CHECK(halo_nat_lookup_wan_compact_device(tabs[0], nullptr, 0, now, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ==
          HALO_E_NODEV);
    CHECK(halo_nat_lookup_lan_compact_device(tabs[0], nullptr, 0, now, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ==
          HALO_E_NODEV);
    CHECK(halo_nat_lookup_quote_device(tabs[0], nullptr, 0, nullptr, nullptr) == HALO_E_NODEV);
    CHECK(halo_nat_lookup_wan_device(nullptr, nullptr, 0, now, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == HALO_E_INVAL);
    for (auto* t : tabs) CHECK(halo_nat_table_destroy(t) == HALO_OK);
    CHECK(halo_nat_table_destroy(nullptr) == HALO_E_INVAL);
    printf("nat fuzz: %ld calls, %lu flows added, %lu nil, %lu get hits, %lu removed, %lu resolves, %lu lists, %lu range\n",
           calls, adds, nils, hits, removed_total, resolves, lists, range);
    return 0;
}
