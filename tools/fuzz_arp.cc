// fuzz_arp.cc — the ARP neighbour cache's host control plane (halo_amd/csrc/arp_table.cc, the file
// libhalo_rx.so links) under ASan/UBSan: a stand-alone program that makes random create / set / get
// / handle_msgs / build_request / expire / refresh_list / list / layout_stats / dirty calls through
// the public C ABI — a small address universe so that tables fill up, `now` across the uint32
// wrap, message, verdict, reply and list buffers of exactly the size the call needs — and checks
// each result against a map-based restatement. tests/test_sanitize_arp.py builds and runs it.
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ihalo_amd/csrc
//       halo_amd/csrc/arp_table.cc tools/fuzz_arp.cc -o fuzz_arp && ./fuzz_arp 200000 0x5EED
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <array>
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

typedef std::array<uint8_t, 6> Mac;
struct Entry {
    Mac mac;
    uint32_t exp;
};
struct Tab {
    halo_arp_table_t* h = nullptr;
    halo_arp_config_t cfg{};
    std::map<std::pair<uint32_t, uint32_t>, Entry> model;  // (netif, ip)
};

static Mac mac_of(uint32_t k) { return Mac{(uint8_t)(k & 1 ? 0x01 : 0x02), 0x33, 0, 0, (uint8_t)(k >> 8), (uint8_t)k}; }
static uint32_t ip_of(const Tab& t, uint32_t netif, uint32_t host) { return (t.cfg.netif[netif].ip & 0xFFFFFF00u) | host; }
static void put_ip(uint8_t* p, uint32_t ip) {
    p[0] = (uint8_t)(ip >> 24), p[1] = (uint8_t)(ip >> 16), p[2] = (uint8_t)(ip >> 8), p[3] = (uint8_t)ip;
}

static int make(Tab* t) {
    if (t->h) CHECK(halo_arp_table_destroy(t->h) == HALO_OK);
    t->h = nullptr;
    t->model.clear();
    memset(&t->cfg, 0, sizeof t->cfg);
    t->cfg.n_netifs = 1 + rnd(rnd(4) ? 3 : 64);
    for (uint32_t q = 0; q < t->cfg.n_netifs; ++q) {
        const Mac m = mac_of(0x1000 + 2 * q);
        memcpy(t->cfg.netif[q].mac, m.data(), 6);
        t->cfg.netif[q].ip = 0x0A000001u + (q << 8);  // host 1 of its /24
        t->cfg.netif[q].nat_enable = rnd(2);
    }
    t->cfg.capacity = 1 + rnd(rnd(3) ? 6 : 40);
    t->cfg.slots_log2 = rnd(3) ? 0 : 6;
    CHECK(halo_arp_table_create(&t->cfg, &t->h) == HALO_OK);
    return 0;
}

// SetArpCache restated; false when the table was full
static bool model_set(Tab& t, uint32_t netif, uint32_t ip, const Mac& mac, uint32_t now, uint32_t* changed) {
    auto it = t.model.find({netif, ip});
    if (it == t.model.end()) {
        if (t.model.size() >= t.cfg.capacity) return false;
        it = t.model.emplace(std::make_pair(netif, ip), Entry{}).first;
        ++*changed;
    } else if (it->second.mac != mac) {
        ++*changed;
    }
    it->second = Entry{mac, (uint32_t)(now + 300u)};
    return true;
}

int main(int argc, char** argv) {
    const long calls = argc > 1 ? strtol(argv[1], nullptr, 0) : 200000;
    g_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x5EED;
    Tab tabs[3];
    for (auto& t : tabs)
        if (make(&t)) return 1;
    uint32_t now = 0xFFFFF000u;  // crosses the uint32 wrap
    unsigned long creates = 3, msgs_total = 0, replies_total = 0, removed_total = 0, refresh_total = 0, lists = 0, gets[3] = {};
    unsigned long verdicts[HALO_ARP_H_COUNT] = {}, not_learned = 0, full_replies = 0, dirty_seen = 0;
    for (long c = 0; c < calls; ++c) {
        Tab& t = tabs[rnd(3)];
        const uint32_t nn = t.cfg.n_netifs;
        switch (rnd(16)) {
            case 0: {
                if (rnd(8) == 0) {
                    if (make(&t)) return 1;
                    ++creates;
                }
                break;
            }
            case 1: case 2: {
                now += rnd(90);
                break;
            }
            case 3: {
                uint32_t want = 0, removed = 0xDEAD;
                for (auto it = t.model.begin(); it != t.model.end();)
                    if (now > it->second.exp) it = t.model.erase(it), ++want;
                    else ++it;
                const bool report = rnd(4) != 0;  // n_removed is optional
                CHECK(halo_arp_expire(t.h, now, report ? &removed : nullptr) == HALO_OK);  // no device copy: no publish
                CHECK(removed == (report ? want : 0xDEADu));
                removed_total += want;
                break;
            }
            case 4: {
                std::vector<std::pair<uint32_t, uint32_t>> want;
                for (const auto& kv : t.model)
                    if (now > (uint32_t)(kv.second.exp - 10u)) want.push_back(kv.first);
                const uint32_t cap = rnd(3) ? rnd(4) : 64u;
                std::vector<uint8_t> nifs(cap);  // exactly `cap`: an overrun is ASan's to find
                std::vector<uint32_t> ips(cap);
                uint32_t total = 0;
                CHECK(halo_arp_refresh_list(t.h, now, cap ? nifs.data() : nullptr, cap ? ips.data() : nullptr, cap, &total) == HALO_OK);
                CHECK(total == want.size());
                for (uint32_t i = 0; i < cap && i < total; ++i) {
                    bool found = false;
                    for (const auto& w : want) found |= w.first == nifs[i] && w.second == ips[i];
                    CHECK(found);
                }
                refresh_total += total;
                break;
            }
            case 5: {
                const uint32_t cap = rnd(3) ? rnd(5) : 64u;
                std::vector<halo_arp_entry_t> exact(cap);
                uint32_t total = 0;
                CHECK(halo_arp_list(t.h, cap ? exact.data() : nullptr, cap, &total) == HALO_OK);
                CHECK(total == t.model.size());
                for (uint32_t i = 0; i < cap && i < total; ++i) {
                    const auto it = t.model.find({exact[i].netif, exact[i].ip});
                    CHECK(it != t.model.end() && memcmp(it->second.mac.data(), exact[i].mac, 6) == 0 &&
                          it->second.exp == exact[i].exp_time && exact[i].pad == 0);
                }
                ++lists;
                break;
            }
            case 6: {
                halo_arp_layout_stats_t st;
                CHECK(halo_arp_layout_stats(t.h, &st) == HALO_OK);
                CHECK((st.slots & (st.slots - 1)) == 0 && st.slots > t.cfg.capacity && st.entries == t.model.size());
                CHECK(st.longest_chain <= st.entries && (st.entries == 0) == (st.longest_chain == 0) && st.wrapped <= st.entries);
                CHECK(halo_arp_dirty(t.h) == 1);  // no device copy in this build
                ++dirty_seen;
                uint8_t frame[60];  // exactly 60
                const uint32_t nif = rnd(nn), target = ip_of(t, nif, rnd(12));
                CHECK(halo_arp_build_request(t.h, nif, target, frame) == HALO_OK);
                uint8_t want[60] = {};
                memset(want, 0xFF, 6);
                memcpy(want + 6, t.cfg.netif[nif].mac, 6);
                const uint8_t fixed[10] = {0x08, 0x06, 0, 1, 8, 0, 6, 4, 0, 1};
                memcpy(want + 12, fixed, 10);
                memcpy(want + 22, t.cfg.netif[nif].mac, 6);
                put_ip(want + 28, t.cfg.netif[nif].ip);
                memset(want + 32, 0xFF, 6);
                put_ip(want + 38, target);
                CHECK(memcmp(frame, want, 60) == 0);
                CHECK(halo_arp_build_request(t.h, nn, target, frame) == HALO_E_RANGE);
                break;
            }
            case 7: case 8: {
                const uint32_t nif = rnd(nn), ip = ip_of(t, nif, rnd(12));
                const Mac m = mac_of(rnd(8));
                uint32_t changed = 0;
                CHECK(halo_arp_set(t.h, nif, ip, m.data(), now) == HALO_OK);
                (void)model_set(t, nif, ip, m, now, &changed);
                CHECK(halo_arp_set(t.h, nn, ip, m.data(), now) == HALO_E_RANGE);
                break;
            }
            case 9: case 10: {
                const uint32_t nif = rnd(nn), ip = ip_of(t, nif, rnd(12));
                halo_arp_entry_t e;
                memset(&e, 0xEE, sizeof e);
                uint32_t found = 99;
                CHECK(halo_arp_get(t.h, nif, ip, rnd(4) ? &e : nullptr, &found) == HALO_OK);
                const auto it = t.model.find({nif, ip});
                const uint32_t want = ip == t.cfg.netif[nif].ip ? HALO_ARP_GET_OWN_IP
                                      : it != t.model.end()     ? HALO_ARP_GET_FOUND
                                                                : HALO_ARP_GET_ABSENT;
                CHECK(found == want);
                ++gets[want];
                break;
            }
            default: {
                const uint32_t n = rnd(9);
                std::vector<halo_arp_msg_t> msgs(n);  // exactly n
                std::vector<Mac> srcs(n);
                for (uint32_t i = 0; i < n; ++i) {
                    halo_arp_msg_t& m = msgs[i];
                    memset(&m, 0, sizeof m);
                    m.index = i;
                    m.netif = (uint8_t)rnd(nn);
                    const Mac sha = mac_of(rnd(8));
                    srcs[i] = rnd(7) ? sha : mac_of(100);
                    memcpy(m.eth_src, srcs[i].data(), 6);
                    for (int k = 0; k < 6; ++k) m.arp[k] = (uint8_t)rnd(256);  // never looked at
                    static const uint16_t kOps[] = {1, 1, 1, 2, 2, 0, 3, 0x0100};
                    const uint16_t op = kOps[rnd(8)];
                    m.arp[6] = (uint8_t)(op >> 8), m.arp[7] = (uint8_t)op;
                    memcpy(m.arp + 8, sha.data(), 6);
                    put_ip(m.arp + 14, ip_of(t, m.netif, rnd(12)));
                    put_ip(m.arp + 24, ip_of(t, m.netif, rnd(3)));
                }
                // the model first: it tells how many replies the exactly-sized buffer must hold
                std::vector<uint8_t> want_v(n);
                std::vector<uint8_t> want_frames;
                uint32_t want_changed = 0;
                for (uint32_t i = 0; i < n; ++i) {
                    const halo_arp_msg_t& m = msgs[i];
                    const halo_rx_netif_t& nif = t.cfg.netif[m.netif];
                    const uint32_t op = (uint32_t)m.arp[6] << 8 | m.arp[7];
                    const uint32_t spa = (uint32_t)m.arp[14] << 24 | m.arp[15] << 16 | m.arp[16] << 8 | m.arp[17];
                    const uint32_t tpa = (uint32_t)m.arp[24] << 24 | m.arp[25] << 16 | m.arp[26] << 8 | m.arp[27];
                    Mac sha;
                    memcpy(sha.data(), m.arp + 8, 6);
                    uint8_t v;
                    if (op != 1 && op != 2) {
                        v = HALO_ARP_H_BAD_OP;
                    } else if (sha != srcs[i]) {
                        v = HALO_ARP_H_SRC_MISMATCH;
                    } else if (spa == nif.ip) {
                        v = HALO_ARP_H_CONFLICT;
                    } else {
                        v = HALO_ARP_H_ACCEPTED;
                        if (!model_set(t, m.netif, spa, sha, now, &want_changed)) v |= HALO_ARP_H_F_NOT_LEARNED, ++not_learned;
                        if (op == 1 && tpa == nif.ip) {
                            uint8_t f[60] = {};
                            memcpy(f, sha.data(), 6);
                            memcpy(f + 6, nif.mac, 6);
                            const uint8_t fixed[10] = {0x08, 0x06, 0, 1, 8, 0, 6, 4, 0, 2};
                            memcpy(f + 12, fixed, 10);
                            memcpy(f + 22, nif.mac, 6);
                            put_ip(f + 28, nif.ip);
                            memcpy(f + 32, sha.data(), 6);
                            put_ip(f + 38, spa);
                            want_frames.insert(want_frames.end(), f, f + 60);
                            if (v & HALO_ARP_H_F_NOT_LEARNED) ++full_replies;
                            v |= HALO_ARP_H_F_REPLY;
                        }
                    }
                    want_v[i] = v;
                    ++verdicts[v & HALO_ARP_H_MASK];
                }
                const bool frames = rnd(4) != 0, counts = rnd(4) != 0;
                std::vector<uint8_t> got_v(n), got_frames(want_frames.size());  // exactly the replies
                uint32_t n_replies = 0xDEAD, n_changed = 0xDEAD;
                CHECK(halo_arp_handle_msgs(t.h, n ? msgs.data() : nullptr, n, now, n ? got_v.data() : nullptr,
                                           frames && !got_frames.empty() ? got_frames.data() : nullptr,
                                           counts ? &n_replies : nullptr, counts ? &n_changed : nullptr) == HALO_OK);
                CHECK(got_v == want_v);
                if (frames) CHECK(got_frames == want_frames);
                if (counts) CHECK(n_replies == want_frames.size() / 60 && n_changed == want_changed);
                msgs_total += n;
                replies_total += want_frames.size() / 60;
                if (n && rnd(16) == 0) {  // a NetIf the table does not have: nothing applied
                    msgs[n - 1].netif = (uint8_t)nn;
                    CHECK(halo_arp_handle_msgs(t.h, msgs.data(), n, now, got_v.data(), nullptr, nullptr, nullptr) == HALO_E_RANGE);
                    uint32_t total = 0;
                    CHECK(halo_arp_list(t.h, nullptr, 0, &total) == HALO_OK && total == t.model.size());
                }
                break;
            }
        }
    }
    // this build has no device side
    CHECK(halo_arp_sync_device(tabs[0].h, nullptr, 0) == HALO_E_NODEV);
    uint32_t dummy = 0;
    CHECK(halo_arp_lookup_device(tabs[0].h, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr) == HALO_E_NODEV);
    CHECK(halo_arp_encap_device(tabs[0].h, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) ==
          HALO_E_NODEV);
    CHECK(halo_arp_gather_device(nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, &dummy, nullptr, 0, nullptr) == HALO_E_NODEV);
    CHECK(halo_arp_gather_workspace(1000) == 16);
    for (auto& t : tabs) CHECK(halo_arp_table_destroy(t.h) == HALO_OK);
    CHECK(halo_arp_table_destroy(nullptr) == HALO_E_INVAL);
    printf("arp fuzz: %ld calls, %lu tables, %lu msgs, %lu replies, %lu removed, %lu refresh, %lu lists, %lu dirty, gets %lu %lu %lu, "
           "not_learned %lu, full_replies %lu, verdicts",
           calls, creates, msgs_total, replies_total, removed_total, refresh_total, lists, dirty_seen, gets[0], gets[1], gets[2],
           not_learned, full_replies);
    for (unsigned long v : verdicts) printf(" %lu", v);
    printf("\n");
    return 0;
}
