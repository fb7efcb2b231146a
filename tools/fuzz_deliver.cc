// fuzz_deliver.cc — local delivery's host side (halo_amd/csrc/rx_deliver_host.cc over rx_deliver.h
// and rx_dispatch.h, and halo_rx_dispatch in halo_amd/csrc/host_logic.cc, the files libhalo_rx.so
// links) under ASan/UBSan: a stand-alone program that makes random halo_rx_deliver_host calls —
// the batch bytes ending with the last frame's last byte, records, offsets, lengths, the two port
// maps and every output in heap buffers of exactly the size the call needs, so an overrun is the
// sanitizer's to find — with each optional input present or absent, the region below, at and above
// the total, records whose payload overruns their frame, and LoChan batches, and checks each
// against a restatement written field by field on the record struct over halo_rx_dispatch /
// halo_rx_dispatch_loopback; the dword arithmetic the kernels share with the host side (rx_deliver.h's
// needs_upper / funnel / tail_mask) is checked against the same bytes. tests/test_sanitize_deliver.py
// builds and runs it.
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ihalo_amd/csrc
//       halo_amd/csrc/rx_deliver_host.cc halo_amd/csrc/host_logic.cc tools/fuzz_deliver.cc -o fuzz_deliver
//       && ./fuzz_deliver 3000 0x5EED
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "halo_rx.h"
#include "rx_deliver.h"

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

static void put32(std::vector<uint8_t>& v, uint32_t x) {
    for (int k = 0; k < 4; ++k) v.push_back((uint8_t)(x >> 8 * k));
}
static void put16(std::vector<uint8_t>& v, uint32_t x) { v.push_back((uint8_t)x), v.push_back((uint8_t)(x >> 8)); }

int main(int argc, char** argv) {
    const long calls = argc > 1 ? strtol(argv[1], nullptr, 0) : 3000;
    g_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x5EED;
    unsigned long kinds[HALO_DELIVER_KIND_COUNT] = {}, absent[3] = {}, align[4] = {}, cut = 0, l3_calls = 0, records = 0, skipped = 0;
    static const uint16_t kTypes[] = {0x0800, 0x0800, 0x0800, 0x0800, 0x0800, 0x0800, 0x0806, 0x86DD, 0xFFFF};
    static const uint8_t kProtos[] = {6, 17, 17, 6, 1, 0xFF};
    static const uint16_t kPorts[] = {0, 53, 67, 68, 80, 65535, 4000, 8080};
    for (long c = 0; c < calls; ++c) {
        const uint32_t n = rnd(60);
        const bool l3 = rnd(4) == 0, have_udp = rnd(4) != 0, have_tcp = rnd(4) != 0, dhcp = rnd(3) != 0;
        halo_rx_netif_t nif;
        memset(&nif, 0, sizeof nif);
        nif.ip = 0xC0A86464u;
        nif.nat_enable = rnd(8) == 0;
        std::vector<uint32_t> udp_map(2048), tcp_map(2048);
        for (uint32_t k = 0; k < 8; ++k) {
            if (rnd(4)) udp_map[kPorts[k] >> 5] |= 1u << (kPorts[k] & 31);
            if (rnd(4)) tcp_map[kPorts[k] >> 5] |= 1u << (kPorts[k] & 31);
        }
        // the batch: frames at 4-byte boundaries with gaps; the buffer ends with the last frame
        std::vector<halo_rx_result_t> recs(n);
        std::vector<uint32_t> offs(n);
        std::vector<uint16_t> lens(n);
        uint64_t pos = 0, end = 0;
        for (uint32_t i = 0; i < n; ++i) {
            pos += 4 * rnd(3);
            offs[i] = (uint32_t)(pos / 4);
            lens[i] = (uint16_t)(rnd(8) ? 34 + rnd(120) : rnd(4) ? rnd(34) : 1000 + rnd(600));
            end = pos + lens[i];
            pos = (end + 3) & ~3ull;
        }
        std::vector<uint8_t> bytes(end ? end : 1);  // a non-null address for a batch of empty frames
        for (uint8_t& b : bytes) b = (uint8_t)rnd(256);
        for (uint32_t i = 0; i < n; ++i) {
            halo_rx_result_t& r = recs[i];
            memset(&r, 0, sizeof r);
            r.status = (uint8_t)(rnd(8) ? 0 : rnd(HALO_RX_STATUS_COUNT));
            r.flags = (uint8_t)(rnd(8) ? (1 | (rnd(8) ? 4 : 0) | (rnd(3) ? 0 : 2)) : rnd(8));
            r.ethertype = kTypes[rnd(9)];
            r.ip_proto = kProtos[rnd(6)];
            r.l4_aux = (uint8_t)rnd(256);
            r.src_ip = rnd(0xFFFFFFFFu), r.dst_ip = rnd(0xFFFFFFFFu);
            r.sport = (uint16_t)rnd(65536), r.dport = rnd(8) ? kPorts[rnd(8)] : (uint16_t)rnd(65536);
            r.l4_seq = rnd(0xFFFFFFFFu), r.l4_ack = rnd(0xFFFFFFFFu);
            const uint32_t len = lens[i];
            if (rnd(10)) {  // inside the frame, at every alignment and up to the last byte
                r.payload_off = (uint16_t)rnd(len + 1);
                r.payload_len = (uint16_t)(rnd(3) ? len - r.payload_off : rnd(len - r.payload_off + 1));
            } else {  // not this frame's record
                r.payload_off = (uint16_t)rnd(2000), r.payload_len = (uint16_t)(rnd(2) ? rnd(65536) : len + 1 - (r.payload_off < len ? r.payload_off : len));
            }
        }
        // the restatement
        std::vector<uint8_t> act(n);
        if (n) CHECK((l3 ? halo_rx_dispatch_loopback : halo_rx_dispatch)(recs.data(), n, &nif, act.data(), nullptr) == HALO_OK);
        std::vector<std::vector<uint8_t>> want;
        std::vector<uint32_t> want_frame;
        uint32_t per_kind[HALO_DELIVER_KIND_COUNT] = {}, want_skipped = 0;
        uint64_t total = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const halo_rx_result_t& r = recs[i];
            uint32_t kind = 0xFF;
            if (act[i] == HALO_RX_ACT_LOCAL_UDP && have_udp && (udp_map[r.dport >> 5] >> (r.dport & 31) & 1)) kind = HALO_DELIVER_UDP;
            if (act[i] == HALO_RX_ACT_LOCAL_TCP && have_tcp && (tcp_map[r.dport >> 5] >> (r.dport & 31) & 1)) kind = HALO_DELIVER_TCP;
            if (act[i] == HALO_RX_ACT_BCAST_UDP && dhcp && (r.dport == 67 || r.dport == 68)) kind = HALO_DELIVER_DHCP;
            if (kind == 0xFF) continue;
            if ((uint32_t)r.payload_off + r.payload_len > lens[i]) {
                ++want_skipped;
                continue;
            }
            std::vector<uint8_t> w;
            put32(w, i);
            w.push_back((uint8_t)kind), w.push_back(r.l4_aux);
            put16(w, r.payload_len);
            put32(w, r.src_ip);
            put16(w, r.sport), put16(w, r.dport);
            put32(w, r.l4_seq), put32(w, r.l4_ack);
            const uint8_t* p = bytes.data() + 4ull * offs[i] + r.payload_off;
            w.insert(w.end(), p, p + r.payload_len);
            while (w.size() & 3) w.push_back(0);
            // the kernels' way to the same bytes (rx_deliver.h): destination dword j out of the frame's
            // dwords s + j and s + j + 1, none of them beyond the word that holds the frame's last byte
            const uint32_t poff = r.payload_off, plen = r.payload_len;
            for (uint32_t j = 0; j < halo::deliver::payload_dwords(plen); ++j) {
                uint32_t word[2] = {0, 0};
                for (uint32_t h = 0; h < 2; ++h) {
                    if (h && !halo::deliver::needs_upper(poff, plen, j)) break;
                    const uint32_t at = (poff >> 2) + j + h;
                    CHECK(at <= (lens[i] - 1u) >> 2);
                    for (uint32_t b = 0; b < 4 && 4ull * offs[i] + 4 * at + b < bytes.size(); ++b)
                        word[h] |= (uint32_t)bytes[4ull * offs[i] + 4 * at + b] << 8 * b;
                }
                const uint32_t v = halo::deliver::funnel(word[0], word[1], poff & 3) & halo::deliver::tail_mask(plen, j);
                uint32_t have;
                memcpy(&have, w.data() + 24 + 4 * j, 4);
                CHECK(v == have);
            }
            total += w.size();
            ++per_kind[kind];
            if (r.payload_len) ++align[r.payload_off & 3];
            want.push_back(w), want_frame.push_back(i);
        }
        const uint32_t count = (uint32_t)want.size();
        const uint64_t region = rnd(3) == 0 ? (total ? rnd((uint32_t)total) : 0) : rnd(2) ? total : total + rnd(64);
        const uint32_t index_cap = rnd(4) == 0 ? 0 : rnd(3) == 0 ? (count ? rnd(count) : 0) : count + rnd(3);
        // outputs, exactly sized
        std::vector<uint8_t> out(region, 0xA5), index(8ull * index_cap, 0xA5), summary(sizeof(halo_deliver_summary_t), 0xA5);
        halo_deliver_config_t cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.flags = (l3 ? HALO_RX_L3_START : 0u) | (dhcp ? HALO_DELIVER_DHCP : 0u);
        cfg.index_cap = index_cap, cfg.region_bytes = region;
        CHECK(halo_rx_deliver_host(&cfg, n ? bytes.data() : nullptr, n ? offs.data() : nullptr, n ? lens.data() : nullptr,
                                   n ? recs.data() : nullptr, n, &nif, have_udp ? udp_map.data() : nullptr,
                                   have_tcp ? tcp_map.data() : nullptr, region ? out.data() : nullptr,
                                   reinterpret_cast<halo_deliver_summary_t*>(summary.data()),
                                   index_cap ? reinterpret_cast<halo_deliver_index_t*>(index.data()) : nullptr) == HALO_OK);
        halo_deliver_summary_t s;
        memcpy(&s, summary.data(), sizeof s);
        uint64_t at = 0;
        uint32_t written = 0;
        bool stopped = false;
        for (uint32_t k = 0; k < count; ++k) {
            uint32_t where = 0xFFFFFFFFu;
            if (!stopped && at + want[k].size() <= region) {
                CHECK(memcmp(out.data() + at, want[k].data(), want[k].size()) == 0);
                where = (uint32_t)at;
                at += want[k].size();
                ++written;
            } else {
                stopped = true;
            }
            if (k < index_cap) {
                uint32_t e[2];
                memcpy(e, index.data() + 8ull * k, 8);
                CHECK(e[0] == want_frame[k] && e[1] == where);
            }
        }
        for (uint64_t b = at; b < region; ++b) CHECK(out[b] == 0xA5);
        for (uint64_t b = 8ull * (count < index_cap ? count : index_cap); b < index.size(); ++b) CHECK(index[b] == 0xA5);
        CHECK(s.records == count && s.records_written == written && s.bytes == total && s.bytes_written == at);
        CHECK(s.skipped == want_skipped);
        for (uint32_t k = 0; k < HALO_DELIVER_KIND_COUNT; ++k) {
            CHECK(s.kind_counts[k] == per_kind[k]);
            kinds[k] += per_kind[k];
        }
        records += count, skipped += want_skipped, cut += written < count, l3_calls += l3;
        absent[0] += !have_udp, absent[1] += !have_tcp, absent[2] += !index_cap;
    }
    // argument errors, and a build without the device side
    alignas(16) static uint8_t buf[1024];
    halo_rx_netif_t nif;
    memset(&nif, 0, sizeof nif);
    auto dev = [&](uint32_t flags, uint64_t region, uint32_t index_cap, void* index, uint64_t wsb, const halo_rx_netif_t* netif) {
        halo_deliver_config_t cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.flags = flags, cfg.region_bytes = region, cfg.index_cap = index_cap;
        return halo_rx_deliver_device(&cfg, buf, reinterpret_cast<uint32_t*>(buf), reinterpret_cast<uint16_t*>(buf),
                                      reinterpret_cast<halo_rx_result_t*>(buf), 1, netif, nullptr, nullptr, buf,
                                      reinterpret_cast<halo_deliver_summary_t*>(buf), static_cast<halo_deliver_index_t*>(index), buf,
                                      wsb, nullptr);
    };
    CHECK(dev(0, 64, 1, buf, 24, &nif) == HALO_E_NODEV);
    CHECK(dev(HALO_RX_L3_START | HALO_DELIVER_DHCP, (1ull << 32) - 16, 0, nullptr, 24, &nif) == HALO_E_NODEV);
    CHECK(dev(HALO_RX_CSUM_ENABLE, 64, 1, buf, 24, &nif) == HALO_E_INVAL);
    CHECK(dev(0, 72, 1, buf, 24, &nif) == HALO_E_INVAL);
    CHECK(dev(0, 1ull << 32, 1, buf, 24, &nif) == HALO_E_INVAL);
    CHECK(dev(0, 64, 1, nullptr, 24, &nif) == HALO_E_INVAL);
    CHECK(dev(0, 64, 1, buf + 4, 24, &nif) == HALO_E_INVAL);
    CHECK(dev(0, 64, 1, buf, 23, &nif) == HALO_E_INVAL);
    CHECK(dev(0, 64, 1, buf, 24, nullptr) == HALO_E_INVAL);
    CHECK(halo_rx_deliver_workspace(0) == 24 && halo_rx_deliver_workspace(256) == 24 && halo_rx_deliver_workspace(257) == 40);
    printf("deliver fuzz: %ld calls, kinds %lu %lu %lu, records %lu, skipped %lu, cut %lu, l3 %lu, absent %lu %lu %lu, "
           "align %lu %lu %lu %lu\n",
           calls, kinds[0], kinds[1], kinds[2], records, skipped, cut, l3_calls, absent[0], absent[1], absent[2], align[0], align[1],
           align[2], align[3]);
    return 0;
}
