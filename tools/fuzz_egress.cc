// fuzz_egress.cc — the egress step's host side (halo_amd/csrc/tx_egress_host.cc and
// halo_ring_write_span in halo_amd/csrc/host_logic.cc, the files libhalo_rx.so links) under
// ASan/UBSan: a stand-alone program that makes random halo_tx_egress_host calls of all three kinds —
// frame, selector, output, summary and index buffers of exactly the size the call needs, so an
// overrun is the sanitizer's to find — checks each against a restatement with std::vector streams,
// and publishes every port's stream into a small ring with halo_ring_write_span, reading it back
// record by record. tests/test_sanitize_egress.py builds and runs it.
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ihalo_amd/csrc
//       halo_amd/csrc/tx_egress_host.cc halo_amd/csrc/host_logic.cc tools/fuzz_egress.cc -o fuzz_egress
//       && ./fuzz_egress 3000 0x5EED
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

static const uint32_t kLens[] = {0, 13, 14, 41, 42, 59, 60, 61, 62, 63, 64, 65, 100, 1514, 1515, 9014, 9015};

int main(int argc, char** argv) {
    const long calls = argc > 1 ? strtol(argv[1], nullptr, 0) : 3000;
    g_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x5EED;
    unsigned long kinds[3] = {}, cuts = 0, skips = 0, records = 0, ring_records = 0, ring_short = 0, ring_bad = 0;
    for (long c = 0; c < calls; ++c) {
        const uint32_t kind = rnd(3), n = rnd(40), n_ports = rnd(3) ? 1 + rnd(4) : 1 + rnd(64);
        const bool jumbo = rnd(4) == 0;
        // the batch: frames at 4-byte boundaries with gaps, in a buffer that ends with the last frame's last word
        std::vector<uint32_t> offs(n);
        std::vector<uint16_t> lens(n);
        uint64_t pos = 0;
        for (uint32_t i = 0; i < n; ++i) {
            lens[i] = (uint16_t)(rnd(3) ? kLens[rnd(13)] : kLens[rnd(17)]);
            pos += 4 * rnd(3);
            offs[i] = (uint32_t)(pos / 4);
            pos += (lens[i] + 3u) & ~3u;
        }
        std::vector<uint8_t> bytes(pos ? pos : 4);  // never null: a batch of empty frames still has an address
        for (auto& b : bytes) b = (uint8_t)rnd(256);
        // selectors and the port mask each decodes to
        const uint64_t valid = n_ports == 64 ? ~0ull : (1ull << n_ports) - 1;
        const uint64_t flood = ((uint64_t)rnd(1u << 16) | (uint64_t)rnd(1u << 16) << 48 | 1ull << (n_ports - 1));
        std::vector<uint64_t> masks(n), want_mask(n);
        std::vector<halo_arp_result_t> arp(n);
        std::vector<halo_sw_result_t> sw(n);
        for (uint32_t i = 0; i < n; ++i) {
            const uint8_t port = (uint8_t)(rnd(4) ? rnd(n_ports) : (rnd(2) ? n_ports : 0xFF));
            if (kind == HALO_EGRESS_KIND_MASKS) {
                masks[i] = rnd(4) == 0 ? 0 : (rnd(4) == 0 ? ~0ull : 1ull << rnd(64)) | (rnd(2) ? 1ull << rnd(n_ports) : 0);
                want_mask[i] = masks[i];
            } else if (kind == HALO_EGRESS_KIND_ARP) {
                arp[i].verdict = (uint8_t)(rnd(2) ? HALO_ARP_V_HIT : rnd(HALO_ARP_V_COUNT));
                arp[i].out_netif = port;
                arp[i].tx_len = (uint16_t)rnd(1u << 16);
                arp[i].target_ip = rnd(0xFFFFFFFFu);
                want_mask[i] = arp[i].verdict == HALO_ARP_V_HIT && port < 64 ? 1ull << port : 0;
            } else {
                sw[i].verdict = (uint8_t)(rnd(2) ? (rnd(2) ? HALO_SW_V_UNICAST : HALO_SW_V_FLOOD) : rnd(HALO_SW_V_COUNT));
                sw[i].out_port = port;
                sw[i].tx_len = (uint16_t)rnd(1u << 16);
                want_mask[i] = sw[i].verdict == HALO_SW_V_FLOOD ? flood
                               : sw[i].verdict == HALO_SW_V_UNICAST && port < 64 ? 1ull << port : 0;
            }
            want_mask[i] &= valid;
        }
        // the restatement, with no region
        std::vector<std::vector<uint8_t>> streams(n_ports);
        std::vector<std::vector<uint32_t>> idx(n_ports), ends(n_ports);
        uint32_t want_skipped = 0;
        const uint32_t cap_len = jumbo ? 9014 : 1514;
        for (uint32_t i = 0; i < n; ++i) {
            if (!want_mask[i]) continue;
            if (lens[i] < 14 || lens[i] > cap_len) {
                ++want_skipped;
                continue;
            }
            const uint32_t tx = lens[i] < 60 ? 60 : lens[i], rec = (4 + tx + 3) & ~3u;
            std::vector<uint8_t> r(rec, 0);
            memcpy(r.data(), &tx, 4);
            memcpy(r.data() + 4, bytes.data() + 4ull * offs[i], lens[i]);
            for (uint32_t p = 0; p < n_ports; ++p)
                if (want_mask[i] >> p & 1) {
                    streams[p].insert(streams[p].end(), r.begin(), r.end());
                    idx[p].push_back(i);
                    ends[p].push_back((uint32_t)streams[p].size());
                }
        }
        skips += want_skipped;
        // a region that cuts some ports, any byte count (the host loop asks no alignment)
        uint64_t longest = 0;
        for (const auto& s : streams) longest = s.size() > longest ? s.size() : longest;
        const uint64_t region = rnd(3) == 0 ? longest + rnd(8) : (longest ? rnd((uint32_t)longest + 1) : 0);
        const uint32_t index_cap = rnd(3) ? rnd(8) : n;
        halo_egress_config_t cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.n_ports = n_ports, cfg.flags = jumbo ? HALO_RX_JUMBO_EXT : 0, cfg.region_bytes = region, cfg.index_cap = index_cap;
        std::vector<uint8_t> out(n_ports * region, 0xA5);  // exactly
        std::vector<halo_egress_port_t> ports(n_ports);
        memset(ports.data(), 0xA5, n_ports * sizeof(halo_egress_port_t));
        std::vector<uint32_t> index((size_t)n_ports * index_cap, 0xA5A5A5A5u);
        uint32_t skipped = 5;
        const void* sel = kind == HALO_EGRESS_KIND_MASKS ? (const void*)masks.data()
                          : kind == HALO_EGRESS_KIND_ARP ? (const void*)arp.data()
                                                         : (const void*)sw.data();
        const std::vector<uint8_t> bytes_before = bytes;
        CHECK(halo_tx_egress_host(&cfg, kind, n ? bytes.data() : nullptr, n ? offs.data() : nullptr, n ? lens.data() : nullptr, n,
                                  n ? sel : nullptr, flood, out.empty() ? nullptr : out.data(), ports.data(),
                                  index_cap ? index.data() : nullptr, rnd(4) ? &skipped : nullptr) == HALO_OK);
        CHECK(bytes == bytes_before);
        CHECK(skipped == 5 || skipped == 5 + want_skipped);
        ++kinds[kind];
        for (uint32_t p = 0; p < n_ports; ++p) {
            uint32_t written = 0;
            while (written < ends[p].size() && ends[p][written] <= region) ++written;
            const uint64_t wbytes = written ? ends[p][written - 1] : 0;
            CHECK(ports[p].frames == idx[p].size() && ports[p].bytes == streams[p].size());
            CHECK(ports[p].frames_written == written && ports[p].bytes_written == wbytes);
            if (written < idx[p].size()) ++cuts;
            records += written;
            CHECK(wbytes == 0 || memcmp(out.data() + p * region, streams[p].data(), wbytes) == 0);
            for (uint64_t k = wbytes; k < region; ++k) CHECK(out[p * region + k] == 0xA5);
            for (uint32_t k = 0; k < index_cap; ++k)
                CHECK(index[(size_t)p * index_cap + k] == (k < idx[p].size() ? idx[p][k] : 0xA5A5A5A5u));
            // the stream into a ring that may be too small for all of it, then read back
            if (!wbytes || rnd(3)) continue;
            const uint64_t size = 1ull << (7 + rnd(12));  // 128 B .. 256 KiB
            void* mem = nullptr;
            CHECK(posix_memalign(&mem, 64, 128 + size) == 0);
            CHECK(halo_ring_create(mem, 128 + size) == HALO_OK);
            const uint64_t start = 4ull * rnd((uint32_t)(size / 4)) + size * rnd(3);  // head == tail: empty, anywhere
            memcpy(mem, &start, 8);
            memcpy((uint8_t*)mem + 64, &start, 8);
            std::vector<uint8_t> span(out.begin() + p * region, out.begin() + p * region + wbytes);  // exactly
            uint32_t took = 0xDEAD;
            uint64_t took_bytes = 0xDEAD;
            const int rc = halo_ring_write_span(mem, span.data(), span.size(), &took, &took_bytes);
            bool overlong = false;
            for (uint32_t k = 0; k < written; ++k) {
                uint32_t len;
                memcpy(&len, span.data() + (k ? ends[p][k - 1] : 0), 4);
                overlong |= len > size / 2;
            }
            uint64_t head;
            memcpy(&head, mem, 8);
            if (overlong) {
                CHECK(rc == HALO_E_INVAL && head == start && took == 0xDEAD);
                ++ring_bad;
            } else {
                CHECK(rc == HALO_OK);
                uint32_t fit = 0;
                while (fit < written && ends[p][fit] <= size) ++fit;
                CHECK(took == fit && took_bytes == (fit ? ends[p][fit - 1] : 0) && head == start + took_bytes);
                if (fit < written) ++ring_short;
                const uint8_t* data = (const uint8_t*)mem + 128;
                for (uint64_t k = 0; k < took_bytes; ++k) CHECK(data[(start + k) & (size - 1)] == span[k]);
                ring_records += took;
                // a truncated span: nothing is written
                if (span.size() > 4) {
                    uint32_t t2 = 7;
                    CHECK(halo_ring_write_span(mem, span.data(), span.size() - 1 - rnd(3), &t2, nullptr) == HALO_E_INVAL);
                    uint64_t h2;
                    memcpy(&h2, mem, 8);
                    CHECK(h2 == head && t2 == 7);
                }
            }
            free(mem);
        }
    }
    // argument errors, and a build without the device side
    halo_egress_config_t cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.n_ports = 2, cfg.region_bytes = 64;
    alignas(16) static uint8_t buf[256];
    halo_egress_port_t ports[2];
    CHECK(halo_tx_egress_masks_device(&cfg, nullptr, nullptr, nullptr, 0, nullptr, buf, ports, nullptr, nullptr, nullptr, 0, nullptr) ==
          HALO_E_NODEV);
    CHECK(halo_tx_egress_arp_device(&cfg, nullptr, nullptr, nullptr, 0, nullptr, buf + 8, ports, nullptr, nullptr, nullptr, 0,
                                    nullptr) == HALO_E_INVAL);
    CHECK(halo_tx_egress_switch_device(&cfg, nullptr, nullptr, nullptr, 1, nullptr, 0, buf, ports, nullptr, nullptr, nullptr, 0,
                                       nullptr) == HALO_E_INVAL);
    CHECK(halo_tx_egress_host(&cfg, 3, nullptr, nullptr, nullptr, 0, nullptr, 0, buf, ports, nullptr, nullptr) == HALO_E_INVAL);
    CHECK(halo_tx_egress_workspace(1000, 3) == 16 * 4 * 3 && halo_tx_egress_workspace(5, 65) == 0);
    CHECK(halo_ring_write_span(nullptr, buf, 0, nullptr, nullptr) == HALO_E_INVAL);
    printf("egress fuzz: %ld calls, kinds %lu %lu %lu, cuts %lu, skips %lu, records %lu, ring records %lu, ring short %lu, "
           "ring refused %lu\n",
           calls, kinds[0], kinds[1], kinds[2], cuts, skips, records, ring_records, ring_short, ring_bad);
    return 0;
}
