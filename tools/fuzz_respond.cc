// fuzz_respond.cc — the local responders' host side (halo_amd/csrc/tx_respond_host.cc over
// tx_respond.h and rx_dispatch.h, and halo_rx_dispatch in halo_amd/csrc/host_logic.cc, the files
// libhalo_rx.so links) under ASan/UBSan: a stand-alone program that makes random
// halo_tx_respond_host calls — records, offsets, lengths, verdict / op / result arrays, the port
// map and every output in heap buffers of exactly the size the call needs, so an overrun is the
// sanitizer's to find — with each optional input present or absent and `cap` below, at and above
// the count, and checks each against a restatement written field by field on the record struct,
// d_actions against halo_rx_dispatch / halo_rx_dispatch_loopback. tests/test_sanitize_respond.py
// builds and runs it.
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ihalo_amd/csrc
//       halo_amd/csrc/tx_respond_host.cc halo_amd/csrc/host_logic.cc tools/fuzz_respond.cc -o fuzz_respond
//       && ./fuzz_respond 3000 0x5EED
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

struct Want {
    uint32_t index, kind;
    halo_tx_build_desc_t d;
};

int main(int argc, char** argv) {
    const long calls = argc > 1 ? strtol(argv[1], nullptr, 0) : 3000;
    g_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x5EED;
    unsigned long kinds[HALO_RESPOND_KIND_COUNT] = {}, absent[4] = {}, cut = 0, l3_calls = 0, replies = 0;
    static const uint16_t kTypes[] = {0x0800, 0x0800, 0x0800, 0x0800, 0x0800, 0x0800, 0x0806, 0x86DD, 0xFFFF};
    static const uint8_t kProtos[] = {1, 6, 17, 0xFF};
    for (long c = 0; c < calls; ++c) {
        const uint32_t n = rnd(60);
        const bool l3 = rnd(4) == 0, have_nat = rnd(3) != 0, have_fix = rnd(3) != 0, have_ports = rnd(3) != 0;
        halo_rx_netif_t nif;
        memset(&nif, 0, sizeof nif);
        nif.ip = 0xC0A86464u;
        nif.nat_enable = rnd(2);
        std::vector<halo_rx_result_t> recs(n);
        std::vector<uint32_t> offs(n);
        std::vector<uint16_t> lens(n);
        std::vector<uint8_t> nat(n), result(n);
        std::vector<halo_tx_op_t> ops(n);
        std::vector<uint32_t> ports(2048);
        for (uint32_t k = 0; k < 64; ++k) {
            const uint32_t p = rnd(4) ? rnd(16) : rnd(65536);
            ports[p >> 5] |= 1u << (p & 31);
        }
        for (uint32_t i = 0; i < n; ++i) {
            halo_rx_result_t& r = recs[i];
            memset(&r, 0, sizeof r);
            r.status = (uint8_t)(rnd(4) ? 0 : rnd(HALO_RX_STATUS_COUNT));
            r.flags = (uint8_t)(rnd(8) ? (1 | (rnd(2) ? 4 : 0) | (rnd(16) ? 0 : 2)) : rnd(8));
            r.ethertype = kTypes[rnd(9)];
            r.ip_proto = kProtos[rnd(4)];
            r.l4_aux = (uint8_t)(rnd(2) ? (r.ip_proto == 1 ? (rnd(2) ? 8 : 0) : (rnd(2) ? 0x02 : 0x12)) : rnd(256));
            r.src_ip = rnd(0xFFFFFFFFu);
            r.sport = (uint16_t)rnd(65536), r.dport = (uint16_t)(rnd(2) ? rnd(16) : rnd(65536));
            r.payload_off = (uint16_t)rnd(65536), r.payload_len = (uint16_t)rnd(65536);
            r.l4_seq = rnd(8) ? rnd(0xFFFFFFFFu) : 0xFFFFFFFFu;
            offs[i] = rnd(4) ? rnd(1u << 20) : 0xFFFFFFFFu - rnd(4);  // payload_off needs 64 bits
            lens[i] = (uint16_t)(rnd(4) ? 42 + rnd(1500) : rnd(65536));
            nat[i] = (uint8_t)(rnd(3) ? HALO_NAT_V_MISS : rnd(6));
            memset(&ops[i], 0xEE, sizeof ops[i]);
            ops[i].steps = (uint8_t)rnd(32);
            result[i] = (uint8_t)rnd(8);
        }
        // the restatement
        std::vector<uint8_t> want_act(n);
        if (n) CHECK((l3 ? halo_rx_dispatch_loopback : halo_rx_dispatch)(recs.data(), n, &nif, want_act.data(), nullptr) == HALO_OK);
        std::vector<Want> want;
        for (uint32_t i = 0; i < n; ++i) {
            const halo_rx_result_t& r = recs[i];
            const uint8_t a = want_act[i];
            Want w;
            memset(&w, 0, sizeof w);
            w.index = i, w.kind = 0xFF;
            w.d.src_ip = nif.ip, w.d.dst_ip = r.src_ip, w.d.payload_off = 4ull * offs[i];
            const bool fwd = !l3 && a == HALO_RX_ACT_FORWARD, miss = fwd && have_nat && nat[i] == HALO_NAT_V_MISS;
            if ((a == HALO_RX_ACT_LOCAL_ICMP && r.l4_aux == 8) || (miss && r.ip_proto == 1 && r.status == HALO_RX_OK && r.l4_aux == 8)) {
                w.kind = HALO_RESPOND_ECHO;
                w.d.proto = 1, w.d.src_port = (uint16_t)(r.l4_seq >> 16), w.d.dst_port = (uint16_t)r.l4_seq;
                w.d.payload_off += r.payload_off, w.d.payload_len = r.payload_len;
            } else if (miss) {
            } else if (fwd && have_fix && (ops[i].steps & HALO_TX_TTL) && !(result[i] & HALO_TX_R_TTL_ALIVE)) {
                w.kind = HALO_RESPOND_TTL;
                w.d.proto = 1, w.d.aux = 11, w.d.payload_off += 14;
                const uint32_t rest = lens[i] > 14 ? lens[i] - 14u : 0u;
                w.d.payload_len = (uint16_t)(rest < 28 ? rest : 28);
            } else if (a == HALO_RX_ACT_LOCAL_TCP && have_ports && (ports[r.dport >> 5] >> (r.dport & 31) & 1) && (r.l4_aux & 2)) {
                const bool ack = r.l4_aux & 0x10;
                w.kind = ack ? HALO_RESPOND_TCP_SYNACK : HALO_RESPOND_TCP_SYN;
                w.d.proto = 6, w.d.aux = ack ? 0x10 : 0x12, w.d.src_port = r.dport, w.d.dst_port = r.sport;
                w.d.seq = ack ? 1234567891u : 1234567890u, w.d.ack = r.l4_seq + 1u;
            }
            if (w.kind != 0xFF) want.push_back(w);
        }
        const uint32_t count = (uint32_t)want.size();
        const uint32_t cap = rnd(3) == 0 ? (count ? rnd(count) : 0) : rnd(2) ? count : count + rnd(5);
        const uint32_t w_n = count < cap ? count : cap;
        if (cap < count) ++cut;
        // outputs, exactly sized
        std::vector<halo_tx_build_desc_t> desc(cap);
        std::vector<halo_respond_src_t> src(cap);
        std::vector<uint32_t> dst_ip(cap, 0xA5A5A5A5u);
        std::vector<uint8_t> actions(n, 0xA5);
        if (cap) memset(desc.data(), 0xA5, cap * sizeof desc[0]), memset(src.data(), 0xA5, cap * sizeof src[0]);
        uint32_t got_count = 0xA5A5A5A5u, kind_counts[HALO_RESPOND_KIND_COUNT] = {7, 7, 7, 7};
        const bool with_dst = rnd(4) != 0, with_kinds = rnd(4) != 0, with_actions = rnd(4) != 0;
        CHECK(halo_tx_respond_host(n ? offs.data() : nullptr, n ? lens.data() : nullptr, n ? recs.data() : nullptr, n,
                                   l3 ? HALO_RX_L3_START : 0, &nif, have_nat && n ? nat.data() : nullptr,
                                   have_fix && n ? ops.data() : nullptr, have_fix && n ? result.data() : nullptr,
                                   have_ports ? ports.data() : nullptr, cap ? desc.data() : nullptr, cap ? src.data() : nullptr,
                                   with_dst && cap ? dst_ip.data() : nullptr, cap, &got_count, with_kinds ? kind_counts : nullptr,
                                   with_actions && n ? actions.data() : nullptr) == HALO_OK);
        CHECK(got_count == count);
        for (uint32_t k = 0; k < cap; ++k) {
            if (k < w_n) {
                CHECK(memcmp(&desc[k], &want[k].d, sizeof desc[k]) == 0);
                CHECK(src[k].index == want[k].index && src[k].kind == want[k].kind && !src[k].pad[0] && !src[k].pad[1] && !src[k].pad[2]);
                CHECK(dst_ip[k] == (with_dst ? want[k].d.dst_ip : 0xA5A5A5A5u));
            } else {
                const uint8_t* p = reinterpret_cast<const uint8_t*>(&desc[k]);
                for (size_t b = 0; b < sizeof desc[k]; ++b) CHECK(p[b] == 0xA5);
                CHECK(src[k].index == 0xA5A5A5A5u && dst_ip[k] == 0xA5A5A5A5u);
            }
        }
        uint32_t per_kind[HALO_RESPOND_KIND_COUNT] = {};
        for (const Want& w : want) ++per_kind[w.kind];
        for (uint32_t k = 0; k < HALO_RESPOND_KIND_COUNT; ++k) {
            CHECK(kind_counts[k] == 7 + (with_kinds ? per_kind[k] : 0));
            kinds[k] += per_kind[k];
        }
        for (uint32_t i = 0; i < n; ++i) CHECK(actions[i] == (with_actions ? want_act[i] : 0xA5));
        replies += count;
        absent[0] += !have_nat, absent[1] += !have_fix, absent[2] += !have_ports, absent[3] += !with_dst;
        l3_calls += l3;
    }
    // argument errors, and a build without the device side
    alignas(16) static uint8_t buf[1024];
    halo_rx_netif_t nif;
    memset(&nif, 0, sizeof nif);
    uint32_t* u32 = reinterpret_cast<uint32_t*>(buf);
    auto dev = [&](const halo_tx_op_t* ops, const uint8_t* res, uint32_t flags, uint64_t wsb) {
        return halo_tx_respond_device(u32, reinterpret_cast<uint16_t*>(buf), reinterpret_cast<halo_rx_result_t*>(buf), 1, flags, &nif,
                                      nullptr, ops, res, nullptr, reinterpret_cast<halo_tx_build_desc_t*>(buf),
                                      reinterpret_cast<halo_respond_src_t*>(buf), nullptr, 1, u32, nullptr, nullptr, buf, wsb, nullptr);
    };
    CHECK(dev(nullptr, nullptr, 0, 4) == HALO_E_NODEV);
    CHECK(dev(reinterpret_cast<halo_tx_op_t*>(buf), nullptr, 0, 4) == HALO_E_INVAL);
    CHECK(dev(nullptr, buf, 0, 4) == HALO_E_INVAL);
    CHECK(dev(nullptr, nullptr, HALO_RX_CSUM_ENABLE, 4) == HALO_E_INVAL);
    CHECK(dev(nullptr, nullptr, 0, 3) == HALO_E_INVAL);
    CHECK(halo_tx_respond_host(nullptr, nullptr, nullptr, 0, 0, &nif, nullptr, nullptr, buf, nullptr, nullptr, nullptr, nullptr, 0, u32,
                               nullptr, nullptr) == HALO_E_INVAL);
    CHECK(halo_tx_respond_host(nullptr, nullptr, nullptr, 0, 0, &nif, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1,
                               u32, nullptr, nullptr) == HALO_E_INVAL);
    CHECK(halo_tx_respond_workspace(0) == 4 && halo_tx_respond_workspace(256) == 4 && halo_tx_respond_workspace(257) == 8);
    printf("respond fuzz: %ld calls, kinds %lu %lu %lu %lu, replies %lu, cut %lu, l3 %lu, absent %lu %lu %lu %lu\n", calls, kinds[0],
           kinds[1], kinds[2], kinds[3], replies, cut, l3_calls, absent[0], absent[1], absent[2], absent[3]);
    return 0;
}
