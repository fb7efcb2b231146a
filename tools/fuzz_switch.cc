// fuzz_switch.cc — the L2 switch's host mode (halo_amd/csrc/switch_table.cc, the file
// libhalo_rx.so links) under ASan/UBSan: a stand-alone program that makes random create / forward /
// expire / list / flood-mask / layout calls through the public C ABI on host switches — frames of
// every drop class over a small MAC universe, tables that fill up, `now` across the uint32 wrap,
// list buffers of exactly `cap` entries, frame arrays of exactly the bytes the frames need — and
// checks each result against a map-based restatement of the sequential loop.
// tests/test_sanitize_switch.py builds and runs it.
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ihalo_amd/csrc
//       halo_amd/csrc/switch_table.cc tools/fuzz_switch.cc -o fuzz_switch && ./fuzz_switch 200000 0x5EED
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <utility>
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

struct Sw {
    halo_switch_t* h = nullptr;
    halo_switch_config_t cfg{};
    std::map<uint64_t, std::pair<uint32_t, uint32_t>> model;  // mac -> (port, create_time)
};

static void put_mac(uint8_t* p, uint32_t k, bool mcast) {
    p[0] = mcast ? 0x01 : 0x02;
    p[1] = 0x10;
    p[2] = p[3] = 0;
    p[4] = (uint8_t)(k >> 8);
    p[5] = (uint8_t)k;
}
static uint64_t mac_of(const uint8_t* p) {
    uint64_t m = 0;
    for (int k = 5; k >= 0; --k) m = m << 8 | p[k];
    return m;
}

static int make(Sw* s) {
    if (s->h) CHECK(halo_switch_destroy(s->h) == HALO_OK);
    s->h = nullptr;
    s->model.clear();
    memset(&s->cfg, 0, sizeof s->cfg);
    s->cfg.n_ports = 1 + rnd(rnd(4) ? 6 : 64);
    for (uint32_t q = 0; q < s->cfg.n_ports; ++q) s->cfg.vlan_id[q] = (uint16_t)(1 + rnd(3));
    s->cfg.capacity = 1 + rnd(rnd(3) ? 12 : 60);
    s->cfg.slots_log2 = rnd(3) ? 0 : 7;
    s->cfg.max_batch = 1 + rnd(64);
    s->cfg.device = -1;
    CHECK(halo_switch_create(&s->cfg, &s->h) == HALO_OK);
    return 0;
}

int main(int argc, char** argv) {
    const long calls = argc > 1 ? strtol(argv[1], nullptr, 0) : 200000;
    g_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x5EED;
    Sw sw[3];
    for (auto& s : sw)
        if (make(&s)) return 1;
    uint32_t now = 0xFFFFF800u;  // crosses the uint32 wrap
    unsigned long frames_total = 0, removed_total = 0, lists = 0, creates = 3, range = 0;
    unsigned long verdicts[HALO_SW_V_COUNT] = {};
    for (long c = 0; c < calls; ++c) {
        Sw& s = sw[rnd(3)];
        switch (rnd(16)) {
            case 0: {
                if (rnd(8) == 0) {
                    if (make(&s)) return 1;
                    ++creates;
                }
                break;
            }
            case 1: case 2: {
                now += rnd(120);
                break;
            }
            case 3: case 4: {
                uint32_t removed = 0, want = 0;
                for (auto it = s.model.begin(); it != s.model.end();)
                    if (now > (uint32_t)(it->second.second + 300u)) it = s.model.erase(it), ++want;
                    else ++it;
                const bool report = rnd(4) != 0;  // n_removed is optional
                removed = 0xDEAD;
                CHECK(halo_switch_expire(s.h, now, report ? &removed : nullptr) == HALO_OK);
                CHECK(removed == (report ? want : 0xDEADu));
                removed_total += want;
                break;
            }
            case 5: case 6: {
                const uint32_t cap = rnd(3) ? rnd(6) : 64u;
                std::vector<halo_switch_entry_t> exact(cap);  // exactly `cap` entries: an overrun is ASan's to find
                uint32_t total = 0;
                CHECK(halo_switch_list(s.h, cap ? exact.data() : nullptr, cap, &total) == HALO_OK);
                CHECK(total == s.model.size());
                for (uint32_t i = 0; i < cap && i < total; ++i) {
                    const auto it = s.model.find(mac_of(exact[i].mac));
                    CHECK(it != s.model.end() && it->second.first == exact[i].port && it->second.second == exact[i].create_time);
                }
                ++lists;
                break;
            }
            case 7: {
                halo_switch_layout_stats_t st;
                CHECK(halo_switch_layout_stats(s.h, &st) == HALO_OK);
                CHECK((st.slots & (st.slots - 1)) == 0 && st.slots > s.cfg.capacity && st.entries == s.model.size());
                const uint32_t p = rnd(s.cfg.n_ports);
                uint64_t mask = 0, want = 0;
                CHECK(halo_switch_flood_mask(s.h, p, &mask) == HALO_OK);
                for (uint32_t q = 0; q < s.cfg.n_ports; ++q)
                    if (q != p && s.cfg.vlan_id[q] == s.cfg.vlan_id[p]) want |= 1ull << q;
                CHECK(mask == want);
                CHECK(halo_switch_flood_mask(s.h, s.cfg.n_ports, &mask) == HALO_E_INVAL);
                break;
            }
            default: {
                const uint32_t n = rnd(s.cfg.max_batch + 2), port = rnd(s.cfg.n_ports);
                std::vector<uint32_t> offs(n);
                std::vector<uint16_t> lens(n);
                std::vector<uint8_t> bytes;  // exactly the frames, each padded to a dword: no slack behind the last
                for (uint32_t i = 0; i < n; ++i) {
                    static const uint16_t kLens[] = {0, 13, 41, 42, 59, 60, 61, 64, 1514, 1515, 65535};
                    const uint32_t len = rnd(4) ? 42 + rnd(40) : kLens[rnd(11)];
                    const uint32_t have = len > 1600 ? 16 : len;  // a bogus length need not be backed by bytes
                    offs[i] = (uint32_t)(bytes.size() / 4);
                    lens[i] = (uint16_t)len;
                    bytes.resize(bytes.size() + ((have + 3) & ~3u), 0xEE);
                    uint8_t* f = bytes.data() + 4 * offs[i];
                    uint8_t hdr[14];
                    put_mac(hdr, rnd(40), rnd(10) == 0);
                    if (rnd(12) == 0) memset(hdr, 0xFF, 6);
                    put_mac(hdr + 6, rnd(40), rnd(14) == 0);
                    static const uint16_t kTypes[] = {0x0800, 0x0806, 0x86DD, 0x05DC, 0x8100, 0x0000};
                    const uint16_t et = kTypes[rnd(10) ? rnd(4) : 4 + rnd(2)];
                    hdr[12] = (uint8_t)(et >> 8), hdr[13] = (uint8_t)et;
                    if (have) memcpy(f, hdr, have < 14 ? have : 14);
                }
                if (bytes.empty()) bytes.reserve(4);  // only zero-length frames: still a non-null array
                std::vector<halo_sw_result_t> res(n);
                uint32_t counts[HALO_SW_V_COUNT] = {5, 5, 5, 5, 5, 5};
                const int rc = halo_switch_forward(s.h, port, n ? bytes.data() : nullptr, offs.data(), lens.data(), n, now,
                                                   res.data(), rnd(3) ? counts : nullptr, nullptr);
                if (n > s.cfg.max_batch) {
                    CHECK(rc == HALO_E_RANGE);
                    ++range;
                    break;
                }
                CHECK(rc == HALO_OK);
                for (uint32_t i = 0; i < n; ++i) {  // the sequential loop, restated
                    const uint8_t* f = bytes.data() + 4 * offs[i];
                    const uint32_t len = lens[i];
                    uint32_t v, out = 0xFF;
                    if (len < 42 || len > 1514) {
                        v = HALO_SW_V_ETH_LEN;
                    } else {
                        const uint32_t et = (uint32_t)f[12] << 8 | f[13];
                        if (et != 0x0800 && et != 0x0806 && et != 0x86DD && et != 0x05DC) {
                            v = HALO_SW_V_ETH_TYPE;
                        } else if (f[6] & 1) {
                            v = HALO_SW_V_SRC_MCAST;
                        } else if (!s.model.count(mac_of(f + 6)) && s.model.size() >= s.cfg.capacity) {
                            v = HALO_SW_V_TABLE_FULL;
                        } else {
                            s.model[mac_of(f + 6)] = {port, now};
                            const auto d = s.model.find(mac_of(f));
                            v = d != s.model.end() ? HALO_SW_V_UNICAST : HALO_SW_V_FLOOD;
                            if (d != s.model.end()) out = d->second.first;
                        }
                    }
                    CHECK(res[i].verdict == v && res[i].out_port == out);
                    CHECK(res[i].tx_len == (v >= HALO_SW_V_UNICAST ? (len < 60 ? 60 : len) : 0));
                    ++verdicts[v];
                }
                frames_total += n;
                break;
            }
        }
    }
    for (auto& s : sw) CHECK(halo_switch_destroy(s.h) == HALO_OK);
    CHECK(halo_switch_destroy(nullptr) == HALO_E_INVAL);
    halo_switch_config_t dev_cfg = sw[0].cfg;
    dev_cfg.device = 0;  // this build has no device side
    halo_switch_t* h = nullptr;
    CHECK(halo_switch_create(&dev_cfg, &h) == HALO_E_NODEV && h == nullptr);
    CHECK(halo_switch_debug_set_epoch(nullptr, 1) == HALO_E_INVAL);
    printf("switch fuzz: %ld calls, %lu switches, %lu frames, %lu removed, %lu lists, %lu range, verdicts", calls, creates,
           frames_total, removed_total, lists, range);
    for (unsigned long v : verdicts) printf(" %lu", v);
    printf("\n");
    return 0;
}
