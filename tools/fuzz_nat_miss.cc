// fuzz_nat_miss.cc — the host parts of the NAT miss path (halo_amd/csrc/nat_table.cc, the file
// libhalo_rx.so links) under ASan/UBSan: a stand-alone program that drives random batches with
// heavy key reuse, zero ports, protocols without ports, select masks and short caps, in both
// directions and NAT types, through halo_nat_collect_misses_host -> halo_nat_resolve_items -> the
// apply rule (restated here over host arrays) on one table and through halo_nat_resolve_misses on a
// twin table built by the same calls, and checks that ops, verdicts, the flow tables and n_added
// agree, that the list is the ascending first occurrences, and that every output array is written
// within its exact size. tests/test_sanitize_nat_miss.py builds and runs it.
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ihalo_amd/csrc
//       halo_amd/csrc/nat_table.cc tools/fuzz_nat_miss.cc -o fuzz_nat_miss && ./fuzz_nat_miss 4000 0x5EED
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
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
static const uint32_t kWanIp = 0xCB007101u;

static bool flows_equal(halo_nat_table_t* a, halo_nat_table_t* b, bool* ok) {
    uint32_t na = 0, nb = 0;
    if (halo_nat_list(a, nullptr, 0, &na) != HALO_OK || halo_nat_list(b, nullptr, 0, &nb) != HALO_OK) return *ok = false;
    if (na != nb) return *ok = false;
    std::vector<halo_nat_flow_t> fa(na), fb(nb);
    if (na && (halo_nat_list(a, fa.data(), na, &na) != HALO_OK || halo_nat_list(b, fb.data(), nb, &nb) != HALO_OK))
        return *ok = false;
    const auto by_id = [](const halo_nat_flow_t& x, const halo_nat_flow_t& y) { return x.id < y.id; };
    std::sort(fa.begin(), fa.end(), by_id);
    std::sort(fb.begin(), fb.end(), by_id);
    for (uint32_t i = 0; i < na; ++i) {
        const halo_nat_flow_t &x = fa[i], &y = fb[i];
        if (x.id != y.id || x.remote_ip != y.remote_ip || x.wan_ip != y.wan_ip || x.lan_ip != y.lan_ip ||
            x.last_alive != y.last_alive || x.remote_port != y.remote_port || x.wan_port != y.wan_port ||
            x.lan_port != y.lan_port || x.proto != y.proto)
            return *ok = false;
    }
    return *ok = true;
}

int main(int argc, char** argv) {
    const long batches = argc > 1 ? strtol(argv[1], nullptr, 0) : 4000;
    g_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x5EED;
    halo_nat_table_t* tabs[2][2] = {};  // [nat type][table, twin]
    for (uint32_t k = 0; k < 2; ++k)
        for (int w = 0; w < 2; ++w) {
            const halo_nat_config_t cfg = {kWanIp, k ? HALO_NAT_FULL_CONE : HALO_NAT_SYMMETRIC, 0, 0};
            CHECK(halo_nat_table_create(&cfg, &tabs[k][w]) == HALO_OK);
            CHECK(halo_nat_port_mapping_add(tabs[k][w], 8001, 0xC0A80003u, 1003, 17) == HALO_OK);
        }
    uint32_t now = 0xFFFFF000u;  // crosses the uint32 wrap
    unsigned long n_items = 0, n_dups = 0, n_alone = 0, n_sport0 = 0, n_short = 0, n_drop = 0, n_added = 0, n_wan = 0,
                  n_wan_flow = 0, n_deselected = 0, n_mapping = 0, n_removed = 0;
    for (long b = 0; b < batches; ++b) {
        const uint32_t type = rnd(2), dir = rnd(3) ? HALO_FLOW_NAT_LAN : HALO_FLOW_NAT_WAN;
        halo_nat_table_t *t = tabs[type][0], *twin = tabs[type][1];
        const uint32_t n = rnd(8) ? rnd(300) : 0;
        // exactly-sized arrays: an overrun is ASan's to find
        std::vector<halo_rx_result_t> recs(n);
        std::vector<uint8_t> verd(n), sel(n);
        std::vector<halo_tx_op_t> ops(n), ops2(n);
        if (n) memset(recs.data(), 0, n * sizeof(halo_rx_result_t)), memset(ops.data(), 0x5A, n * sizeof(halo_tx_op_t));
        const bool use_sel = rnd(3) == 0;
        const uint32_t hosts = 1 + rnd(6), ports = 1 + rnd(12);
        for (uint32_t i = 0; i < n; ++i) {
            halo_rx_result_t& r = recs[i];
            r.ip_proto = kProtos[rnd(4)];
            const uint16_t lport = (uint16_t)(r.ip_proto == 47 || !rnd(12) ? 0 : 1000 + rnd(ports));
            const uint16_t rport = (uint16_t)(r.ip_proto == 47 || !rnd(6) ? 0 : 50 + rnd(3));
            if (dir == HALO_FLOW_NAT_LAN) {
                r.src_ip = 0xC0A80000u | rnd(hosts), r.sport = lport, r.dst_ip = 0x08080800u | rnd(3), r.dport = rport;
            } else {
                r.src_ip = 0x08080800u | rnd(3), r.sport = rport, r.dst_ip = kWanIp;
                r.dport = (uint16_t)(rnd(8) ? 32768 + rnd(40) : 8001);
            }
            verd[i] = (uint8_t)(rnd(5) ? HALO_NAT_V_MISS : rnd(5));
            sel[i] = (uint8_t)(rnd(4) ? 1 + rnd(200) : 0);
        }
        ops2 = ops;
        const uint8_t* select = use_sel ? sel.data() : nullptr;

        // ---- the miss path on t ----
        const uint32_t cap = rnd(4) ? n : rnd(n + 1);
        std::vector<halo_nat_miss_item_t> items(cap);
        std::vector<uint32_t> pos(n);
        uint32_t count = 0xDEAD;
        CHECK(halo_nat_collect_misses_host(t, dir, recs.data(), verd.data(), select, n, items.data(), cap, &count,
                                           pos.data()) == HALO_OK);
        CHECK(count <= n);
        const uint32_t k = count < cap ? count : cap;
        n_short += count > cap;
        uint32_t next = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const bool selected = verd[i] == HALO_NAT_V_MISS && (!select || select[i]);
            n_deselected += verd[i] == HALO_NAT_V_MISS && !selected;
            if (!selected) {
                CHECK(pos[i] == HALO_NAT_NO_FLOW);
                continue;
            }
            CHECK(pos[i] <= next && pos[i] < count);
            if (pos[i] == next) {  // a representative: the next item, in ascending index
                if (next < k) {
                    const halo_nat_miss_item_t& it = items[next];
                    CHECK(it.index == i && it.src_ip == recs[i].src_ip && it.dst_ip == recs[i].dst_ip &&
                          it.sport == recs[i].sport && it.dport == recs[i].dport && it.proto == recs[i].ip_proto &&
                          !it.pad[0] && !it.pad[1] && !it.pad[2]);
                }
                ++next;
                n_alone += dir == HALO_FLOW_NAT_LAN && recs[i].dport == 0 && recs[i].sport != 0;
            } else {
                ++n_dups;
                CHECK(!(dir == HALO_FLOW_NAT_LAN && recs[i].dport == 0 && recs[i].sport != 0));
                n_sport0 += dir == HALO_FLOW_NAT_LAN && recs[i].sport == 0;
            }
        }
        CHECK(next == count);
        n_items += k;
        std::vector<halo_nat_answer_t> answers(k);
        uint32_t added = 0;
        CHECK(halo_nat_resolve_items(t, dir, items.data(), k, now, answers.data(), &added) == HALO_OK);
        std::vector<uint8_t> out(verd);
        for (uint32_t i = 0; i < n; ++i) {  // halo_nat_apply_answers_device's rule
            if (pos[i] >= k) continue;
            const halo_nat_answer_t& a = answers[pos[i]];
            if (a.verdict == HALO_NAT_V_FLOW || a.verdict == HALO_NAT_V_MAPPING) {
                if (dir == HALO_FLOW_NAT_WAN)
                    ops[i].steps |= HALO_TX_NAT_DST, ops[i].dst_ip = a.ip, ops[i].dst_port = a.port;
                else
                    ops[i].steps |= HALO_TX_NAT_SRC, ops[i].src_ip = a.ip, ops[i].src_port = a.port;
                out[i] = a.verdict;
                n_mapping += a.verdict == HALO_NAT_V_MAPPING;
                n_wan_flow += dir == HALO_FLOW_NAT_WAN && a.verdict == HALO_NAT_V_FLOW;
            } else if (a.verdict == HALO_NAT_V_DROP) {
                out[i] = HALO_NAT_V_DROP;
                CHECK(a.ref == HALO_NAT_NO_FLOW);
                ++n_drop;
            } else {
                CHECK(a.verdict == HALO_NAT_V_MISS && dir == HALO_FLOW_NAT_WAN && a.ref == HALO_NAT_NO_FLOW);
            }
        }
        // deselected misses are nobody's business in either path
        std::vector<uint8_t> masked(n);
        if (count > cap) {  // the cap cut the list: the rest goes through the old path, in order
            for (uint32_t i = 0; i < n; ++i)
                masked[i] = out[i] == HALO_NAT_V_MISS && select && !select[i] ? (uint8_t)HALO_NAT_V_SKIP : out[i];
            uint32_t more = 0;
            std::vector<uint8_t> rest(n);
            CHECK(halo_nat_resolve_misses(t, dir, recs.data(), masked.data(), n, now, ops.data(), rest.data(), &more) ==
                  HALO_OK);
            for (uint32_t i = 0; i < n; ++i)
                if (!(verd[i] == HALO_NAT_V_MISS && select && !select[i])) out[i] = rest[i];
            added += more;
        }
        // ---- the twin: the whole batch through halo_nat_resolve_misses ----
        for (uint32_t i = 0; i < n; ++i)
            masked[i] = verd[i] == HALO_NAT_V_MISS && select && !select[i] ? (uint8_t)HALO_NAT_V_SKIP : verd[i];
        std::vector<uint8_t> out2(n);
        uint32_t added2 = 0;
        CHECK(halo_nat_resolve_misses(twin, dir, recs.data(), masked.data(), n, now, ops2.data(), out2.data(), &added2) ==
              HALO_OK);
        for (uint32_t i = 0; i < n; ++i)
            if (verd[i] == HALO_NAT_V_MISS && select && !select[i]) out2[i] = HALO_NAT_V_MISS;
        CHECK(added == added2);
        CHECK(n == 0 || memcmp(ops.data(), ops2.data(), n * sizeof(halo_tx_op_t)) == 0);
        CHECK(out == out2);
        bool same;
        CHECK(flows_equal(t, twin, &same));
        n_added += added;
        n_wan += dir == HALO_FLOW_NAT_WAN;
        // time passes; both tables expire alike
        if (!rnd(3)) now += rnd(50);
        if (!rnd(6)) {
            uint32_t r1 = 0, r2 = 0;
            CHECK(halo_nat_expire(t, now, &r1) == HALO_OK && halo_nat_expire(twin, now, &r2) == HALO_OK && r1 == r2);
            n_removed += r1;
        }
    }
    // argument checks; this build has no device side
    halo_nat_table_t* t = tabs[0][0];
    uint32_t c = 0, p4[4] = {};
    alignas(16) uint8_t buf[64] = {};
    CHECK(halo_nat_collect_misses_host(nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, &c, nullptr) == HALO_E_INVAL);
    CHECK(halo_nat_collect_misses_host(t, 0, nullptr, nullptr, nullptr, 1, nullptr, 0, &c, p4) == HALO_E_INVAL);
    CHECK(halo_nat_resolve_items(t, 2, nullptr, 0, now, nullptr, nullptr) == HALO_E_INVAL);
    CHECK(halo_nat_collect_misses_device(t, 0, (const halo_rx_result_t*)buf, buf, nullptr, 1, 0, (halo_nat_miss_item_t*)buf, 1,
                                         &c, p4, buf, sizeof buf, nullptr) == HALO_E_INVAL);  // a short workspace
    CHECK(halo_nat_collect_misses_device(t, 0, (const halo_rx_result_t*)buf, buf, nullptr, 16, 4, (halo_nat_miss_item_t*)buf, 1,
                                         &c, p4, buf, 4096, nullptr) == HALO_E_RANGE);
    CHECK(halo_nat_collect_misses_device(t, 0, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, &c, nullptr, nullptr, 0, nullptr) ==
          HALO_E_NODEV);
    CHECK(halo_nat_collect_misses_compact_device(t, 0, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, &c, nullptr, nullptr, 0,
                                                 nullptr) == HALO_E_NODEV);
    CHECK(halo_nat_apply_answers_device(0, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == HALO_E_NODEV);
    CHECK(halo_nat_apply_answers_device(5, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == HALO_E_INVAL);
    for (auto& pair : tabs)
        for (auto* x : pair) CHECK(halo_nat_table_destroy(x) == HALO_OK);
    printf("nat miss fuzz: %ld batches, %lu items, %lu duplicates, %lu alone, %lu sport0 duplicates, %lu short caps, "
           "%lu drops, %lu added, %lu wan batches, %lu wan flow hits, %lu deselected, %lu mapping hits, %lu removed\n",
           batches, n_items, n_dups, n_alone, n_sport0, n_short, n_drop, n_added, n_wan, n_wan_flow, n_deselected, n_mapping,
           n_removed);
    return 0;
}
