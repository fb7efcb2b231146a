// fuzz_lo.cc — the loopback gather's host side (halo_amd/csrc/lo_gather_host.cc, the file
// libhalo_rx.so links) under ASan/UBSan: a stand-alone program that makes random halo_lo_gather_host
// calls in both modes — the batch in a heap buffer that ends with the last frame's last byte, every
// region, summary and per-packet array of exactly the size the call needs, so a read or a write one
// byte out is the sanitizer's to find — and checks each against a restatement with std::vector
// streams. tests/test_sanitize_lo.py builds and runs it.
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ihalo_amd/csrc
//       halo_amd/csrc/lo_gather_host.cc tools/fuzz_lo.cc -o fuzz_lo && ./fuzz_lo 3000 0x10C4A
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

static const uint32_t kLens[] = {0, 17, 33, 34, 35, 36, 37, 38, 60, 64, 100, 1514, 1515, 9014, 9015};

int main(int argc, char** argv) {
    const long calls = argc > 1 ? strtol(argv[1], nullptr, 0) : 3000;
    g_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x10C4A;
    unsigned long modes[2] = {}, cuts = 0, skips = 0, packets = 0, beyond = 0;
    for (long c = 0; c < calls; ++c) {
        const bool tx = rnd(2), jumbo = rnd(4) == 0;
        const uint32_t n = rnd(40), n_netifs = rnd(3) ? 1 + rnd(4) : 1 + rnd(64);
        // the batch: frames at 4-byte boundaries with gaps, in a buffer that ends with the last byte of the frame that ends last
        std::vector<uint32_t> offs(n);
        std::vector<uint16_t> lens(n);
        uint64_t pos = 0, end = 0;
        for (uint32_t i = 0; i < n; ++i) {
            lens[i] = (uint16_t)(rnd(3) ? kLens[rnd(12)] : kLens[rnd(15)]);
            pos += 4 * rnd(3);
            offs[i] = (uint32_t)(pos / 4);
            if (pos + lens[i] > end) end = pos + lens[i];
            pos += (lens[i] + 3u) & ~3u;
        }
        uint8_t* bytes = (uint8_t*)malloc(end ? end : 1);  // exactly
        CHECK(bytes);
        for (uint64_t k = 0; k < end; ++k) bytes[k] = (uint8_t)rnd(256);
        std::vector<halo_arp_result_t> res(n);
        for (uint32_t i = 0; i < n; ++i) {
            res[i].verdict = (uint8_t)(rnd(3) ? HALO_ARP_V_LOOPBACK : rnd(HALO_ARP_V_COUNT + 2));
            res[i].out_netif = (uint8_t)(rnd(5) ? rnd(n_netifs) : (rnd(2) ? n_netifs : 0xFF));
            res[i].tx_len = (uint16_t)rnd(1u << 16);
            res[i].target_ip = rnd(0xFFFFFFFFu);
            if (tx && lens[i] >= 18) {  // totalLen below, equal to and above len - 14; under 20
                const uint32_t room = lens[i] - 14u, k = rnd(8);
                const uint32_t t = k < 3 ? room : k == 3 ? (room > 4 ? room - 1 - rnd(4) : 0)
                                   : k == 4 ? room + 1 + rnd(3) : k == 5 ? rnd(20) : k == 6 ? 20 : rnd(1u << 16);
                bytes[4ull * offs[i] + 16] = (uint8_t)(t >> 8);
                bytes[4ull * offs[i] + 17] = (uint8_t)t;
            }
        }
        // the restatement, with no region
        std::vector<std::vector<uint8_t>> streams(n_netifs);
        std::vector<std::vector<uint32_t>> idx(n_netifs), ends(n_netifs), plens(n_netifs);
        uint32_t want_skipped = 0;
        for (uint32_t i = 0; i < n; ++i) {
            if (res[i].verdict != HALO_ARP_V_LOOPBACK || res[i].out_netif >= n_netifs) continue;
            const uint8_t* f = bytes + 4ull * offs[i];
            uint32_t plen = 0;
            bool ok;
            if (tx) {
                ok = lens[i] >= 34;
                if (ok) plen = (uint32_t)f[16] << 8 | f[17], ok = plen >= 20 && plen + 14 <= lens[i];
            } else {
                ok = lens[i] >= 34 && lens[i] <= (jumbo ? 9014u : 1514u);
                plen = lens[i] - 14u;
            }
            if (!ok) {
                ++want_skipped;
                continue;
            }
            std::vector<uint8_t>& s = streams[res[i].out_netif];
            s.insert(s.end(), f + 14, f + 14 + plen);
            s.resize((s.size() + 3) & ~(size_t)3, 0);
            idx[res[i].out_netif].push_back(i);
            ends[res[i].out_netif].push_back((uint32_t)s.size());
            plens[res[i].out_netif].push_back(plen);
        }
        skips += want_skipped;
        // a region that cuts some NetIfs, any byte count (the host loop asks no alignment)
        uint64_t longest = 0;
        for (const auto& s : streams) longest = s.size() > longest ? s.size() : longest;
        const uint64_t region = rnd(3) == 0 ? longest + rnd(8) : (longest ? rnd((uint32_t)longest + 1) : 0);
        const uint32_t index_cap = rnd(3) ? rnd(8) : n;
        halo_lo_config_t cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.n_netifs = n_netifs, cfg.flags = (jumbo ? HALO_RX_JUMBO_EXT : 0) | (tx ? HALO_LO_TX : 0);
        cfg.region_bytes = region, cfg.index_cap = index_cap;
        // one heap block per NetIf would not be one `out`: the regions lie back to back, and the
        // block ends with the last region, so the last NetIf's overrun is caught at once and any
        // other's by the 0xA5 check below
        std::vector<uint8_t> out(n_netifs * region, 0xA5);  // exactly
        std::vector<halo_egress_port_t> ports(n_netifs);
        memset(ports.data(), 0xA5, n_netifs * sizeof(halo_egress_port_t));
        const size_t cells = (size_t)n_netifs * index_cap;
        std::vector<uint32_t> pkt_off(cells, 0xA5A5A5A5u), index(cells, 0xA5A5A5A5u);
        std::vector<uint16_t> pkt_len(cells, 0xA5A5u);
        uint32_t skipped = 5;
        uint8_t* before = (uint8_t*)malloc(end ? end : 1);
        CHECK(before);
        memcpy(before, bytes, end);
        CHECK(halo_lo_gather_host(&cfg, n ? bytes : nullptr, n ? offs.data() : nullptr, n ? lens.data() : nullptr, n,
                                  n ? res.data() : nullptr, out.empty() ? nullptr : out.data(), ports.data(),
                                  index_cap ? pkt_off.data() : nullptr, index_cap ? pkt_len.data() : nullptr,
                                  index_cap ? index.data() : nullptr, rnd(4) ? &skipped : nullptr) == HALO_OK);
        CHECK(memcmp(before, bytes, end) == 0);
        CHECK(skipped == 5 || skipped == 5 + want_skipped);
        ++modes[tx];
        for (uint32_t p = 0; p < n_netifs; ++p) {
            uint32_t written = 0;
            while (written < ends[p].size() && ends[p][written] <= region) ++written;
            const uint64_t wbytes = written ? ends[p][written - 1] : 0;
            CHECK(ports[p].frames == idx[p].size() && ports[p].bytes == streams[p].size());
            CHECK(ports[p].frames_written == written && ports[p].bytes_written == wbytes);
            if (written < idx[p].size()) ++cuts;
            packets += written;
            CHECK(wbytes == 0 || memcmp(out.data() + p * region, streams[p].data(), wbytes) == 0);
            for (uint64_t k = wbytes; k < region; ++k) CHECK(out[p * region + k] == 0xA5);
            for (uint32_t k = 0; k < index_cap; ++k) {
                const size_t at = (size_t)p * index_cap + k;
                if (k >= idx[p].size()) {
                    CHECK(index[at] == 0xA5A5A5A5u && pkt_off[at] == 0xA5A5A5A5u && pkt_len[at] == 0xA5A5u);
                    continue;
                }
                CHECK(index[at] == idx[p][k] && pkt_len[at] == plens[p][k]);
                CHECK(pkt_off[at] == (k < written ? (k ? ends[p][k - 1] : 0) / 4 : 0xFFFFFFFFu));
                if (k >= written) ++beyond;
            }
        }
        free(before);
        free(bytes);
    }
    // argument errors, and a build without the device side
    halo_lo_config_t cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.n_netifs = 2, cfg.region_bytes = 64;
    alignas(16) static uint8_t buf[256];
    halo_egress_port_t ports[2];
    CHECK(halo_lo_gather_device(&cfg, nullptr, nullptr, nullptr, 0, nullptr, buf, ports, nullptr, nullptr, nullptr, nullptr, nullptr,
                                0, nullptr) == HALO_E_NODEV);
    CHECK(halo_lo_gather_device(&cfg, nullptr, nullptr, nullptr, 0, nullptr, buf + 8, ports, nullptr, nullptr, nullptr, nullptr,
                                nullptr, 0, nullptr) == HALO_E_INVAL);
    CHECK(halo_lo_gather_host(&cfg, nullptr, nullptr, nullptr, 1, nullptr, buf, ports, nullptr, nullptr, nullptr, nullptr) ==
          HALO_E_INVAL);
    cfg.flags = 0x1;
    CHECK(halo_lo_gather_host(&cfg, nullptr, nullptr, nullptr, 0, nullptr, buf, ports, nullptr, nullptr, nullptr, nullptr) ==
          HALO_E_INVAL);
    CHECK(halo_lo_gather_workspace(1000, 3) == 16 * 4 * 3 && halo_lo_gather_workspace(5, 65) == 0);
    printf("lo fuzz: %ld calls, modes %lu %lu, cuts %lu, skips %lu, packets %lu, beyond %lu\n", calls, modes[0], modes[1], cuts,
           skips, packets, beyond);
    return 0;
}
