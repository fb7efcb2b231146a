// fuzz_kcp.cc — KCP ingest's host side (halo_amd/csrc/rx_kcp_host.cc over rx_kcp.h, the files
// libhalo_rx.so links) under ASan/UBSan: a stand-alone program that makes random
// halo_kcp_ingest_host calls — a delivery stream that ends with its last record's last byte, its
// summary and index, and every output in heap buffers of exactly the size the call needs, so an
// overrun is the sanitizer's to find — over datagrams of random segments (good ones, each kind of
// structural failure, wrong hash fields, ENet packets and near misses, short payloads, other
// kinds and ports, unwritten records), in every byte-check mode, with capacities and index_cap
// below, at and above what the delivery needs, and checks each against a restatement written
// field by field on the structs with a table-driven CRC-32. (XXH3 mode: the restatement knows the
// hash of the empty string only; for other PUSH segments it takes the call's own check byte and
// holds n_segs / ret / the counters to it — tests/test_kcp_host.py holds the host XXH3 against the
// oracle.) The arithmetic the kernels share with the host side — rx_kcp.h's lane ranges, bit
// steps, multiplication mod the polynomial and fixed powers, over dwords funnelled as
// rx_deliver.h does — is run in the lane decomposition and checked against the same table. It is
// the plain form of that arithmetic, not the kernel's code: the kernel's two shortcuts (no
// multiplication before the first pass, and none at fold levels below a short segment's occupied
// lanes) are not restated here; tests/test_gpu_kcp.py checks them on the device.
// tests/test_sanitize_kcp.py builds and runs it.
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ihalo_amd/csrc
//       halo_amd/csrc/rx_kcp_host.cc tools/fuzz_kcp.cc -o fuzz_kcp && ./fuzz_kcp 3000 0x5EED
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "halo_rx.h"
#include "rx_kcp.h"

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

typedef std::vector<uint8_t> Bytes;
static void put32(Bytes& v, uint32_t x) {
    for (int k = 0; k < 4; ++k) v.push_back((uint8_t)(x >> 8 * k));
}
static void put16(Bytes& v, uint32_t x) { v.push_back((uint8_t)x), v.push_back((uint8_t)(x >> 8)); }
static uint32_t get32(const uint8_t* p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }
static uint32_t get32be(const uint8_t* p) { return p[3] | p[2] << 8 | p[1] << 16 | (uint32_t)p[0] << 24; }

static uint32_t g_table[256];
static uint32_t crc_table(const uint8_t* d, size_t n) {  // the classic table-driven CRC-32
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = g_table[(c ^ d[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}

static const uint64_t kConv = 0x0102030405060708ull;
static const uint32_t kEmptyXxh3 = 0x38D394C2u;  // the low 32 bits of XXH3-64 of no bytes
static const uint8_t kMagic[4][8] = {{0, 0, 0, 0xff, 0xff, 0xff, 0xff, 0xff}, {0, 0, 1, 0x45, 0x14, 0x51, 0x45, 0x45},
                                     {0, 0, 1, 0x94, 0x19, 0x41, 0x94, 0x94}, {0, 0, 2, 0x27, 0x22, 0x72, 0x27, 0x27}};

static void put_seg(Bytes& v, int mode, uint64_t conv, uint32_t cmd, uint32_t length, const Bytes& data, bool wrong_hash) {
    put32(v, (uint32_t)conv), put32(v, (uint32_t)(conv >> 32));
    v.push_back((uint8_t)cmd), v.push_back((uint8_t)rnd(4));
    put16(v, rnd(65536)), put32(v, rnd(1u << 31)), put32(v, rnd(1u << 31)), put32(v, rnd(1u << 31)), put32(v, length);
    if (mode != -1) {
        uint32_t f = 0;
        if (cmd == 81) f = mode == 1 ? crc_table(data.data(), data.size()) : mode == 2 ? (data.empty() ? kEmptyXxh3 : rnd(1u << 31)) : 0u;
        else if (rnd(3) == 0) f = rnd(1u << 31);  // a non-PUSH field is never looked at
        if (wrong_hash) f ^= 1u << rnd(32);
        put32(v, f);
    }
    v.insert(v.end(), data.begin(), data.end());
}

// rx_kcp.h's lane decomposition of one segment's CRC, run lane by lane on the host over the
// stream's aligned dwords (dw holds ceil((a + len) / 4) dwords: no read may pass it); without the
// kernel's shortcuts for zero operands
static uint32_t crc_as_lanes(const std::vector<uint32_t>& dw, uint32_t a, uint32_t len) {
    using namespace halo;
    auto bytes_at = [&](uint32_t at, uint32_t n) {  // n = 1..4 data bytes
        const uint32_t s = at & 3u, lo = dw.at(at >> 2), hi = s + n > 4u ? dw.at((at >> 2) + 1) : 0u;
        return deliver::funnel(lo, hi, s) & (n == 4u ? 0xFFFFFFFFu : (1u << 8u * n) - 1u);
    };
    uint32_t v[kcp::kCrcLanes] = {};
    const uint32_t P = kcp::crc_passes(len);
    for (uint32_t g = 0; g < kcp::kCrcLanes; ++g)
        for (uint32_t p = 0; p < P; ++p) {
            uint32_t b0, b1;
            bool first;
            kcp::crc_lane_range(len, P, p, g, &b0, &b1, &first);
            v[g] = kcp::crc_mulmod(v[g], kcp::kCrcXStride);
            if (b1 <= b0) continue;
            uint32_t c = first ? 0xFFFFFFFFu : 0u;
            const uint32_t head = (b1 - b0) & 3u;
            if (head) c = kcp::crc_steps(c ^ bytes_at(a + b0, head), 8 * head), b0 += head;
            for (; b0 < b1; b0 += 4) c = kcp::crc_steps(c ^ bytes_at(a + b0, 4), 32);
            v[g] ^= c;
        }
    for (uint32_t l = 0; l < kcp::kCrcLevels; ++l)
        for (uint32_t g = 0; g < kcp::kCrcLanes; g += 2u << l) v[g] = kcp::crc_mulmod(v[g], kcp::crc_xlevel(l)) ^ v[g + (1u << l)];
    return len ? ~v[0] : 0u;
}

int main(int argc, char** argv) {
    const long calls = argc > 1 ? strtol(argv[1], nullptr, 0) : 3000;
    g_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x5EED;
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        g_table[i] = c;
    }
    unsigned long modes[4] = {}, rets[5] = {}, enets[4] = {}, kcps = 0, ignored = 0, cut = 0, passed = 0, failed = 0, unwritten = 0,
                  others = 0, capped = 0, lanes = 0, align[4] = {}, segs_total = 0;
    for (long c = 0; c < calls; ++c) {
        // ---- the shared arithmetic, as a lane group runs it ----
        {
            const uint32_t a = rnd(64), len = rnd(8) == 0 ? rnd(5000) : rnd(2) ? rnd(80) : halo::kcp::kCrcStride - 2 + rnd(5);
            Bytes raw(((a + len + 3) & ~3u), 0);
            for (auto& b : raw) b = (uint8_t)rnd(256);
            std::vector<uint32_t> dw(raw.size() / 4);
            if (!dw.empty()) memcpy(dw.data(), raw.data(), raw.size());
            CHECK(crc_as_lanes(dw, a, len) == crc_table(raw.data() + a, len));
            ++lanes, ++align[a & 3];
        }
        // ---- one call ----
        const int mode = (int)rnd(4) - 1;
        const uint32_t H = mode == -1 ? 28 : 32, port = rnd(2) ? 22102 : rnd(65536);
        ++modes[mode + 1];
        const uint32_t n = rnd(40);
        Bytes stream;
        std::vector<uint32_t> index;  // {frame, offset} pairs
        struct Item { uint32_t off, kind, lport; Bytes payload; };
        std::vector<Item> items;
        for (uint32_t i = 0; i < n; ++i) {
            Bytes p;
            const uint32_t what = rnd(12);
            if (what == 0) {  // ENet or a near miss
                const uint32_t t = rnd(4);
                p.insert(p.end(), kMagic[t], kMagic[t] + 4);
                for (int k = 0; k < 12; ++k) p.push_back((uint8_t)rnd(256));
                const uint32_t tt = rnd(6) ? t : rnd(4);  // sometimes another type's tail
                p.insert(p.end(), kMagic[tt] + 4, kMagic[tt] + 8);
            } else if (what == 1) {  // short or random bytes
                p.resize(rnd(3) ? rnd(H + 2) : 20);
                for (auto& b : p) b = (uint8_t)rnd(256);
            } else {
                const uint32_t nseg = 1 + rnd(6);
                const uint64_t conv = kConv + rnd(3);
                for (uint32_t s = 0; s < nseg; ++s) {
                    Bytes data(rnd(4) ? rnd(40) : rnd(1500));
                    for (auto& b : data) b = (uint8_t)rnd(256);
                    const uint32_t flaw = rnd(24);
                    const uint32_t cmd = flaw == 0 ? (rnd(2) ? 80 : 85 + rnd(170)) : 81 + rnd(4);
                    put_seg(p, mode, flaw == 1 ? conv ^ (1ull << rnd(64)) : conv, cmd, flaw == 2 ? (uint32_t)data.size() + 1 + rnd(3) * 0x7FFFFFFFu
                                                                                                 : (uint32_t)data.size(), data, flaw == 3 || flaw == 4);
                }
                if (rnd(4) == 0) p.resize(p.size() + rnd(H));  // a tail shorter than a header
                if (p.size() > 65507) p.resize(65507);
            }
            Item it{(uint32_t)stream.size(), rnd(8) ? 0u : 1u + rnd(2), rnd(8) ? port : port ^ 1u, p};
            put32(stream, i), stream.push_back((uint8_t)it.kind), stream.push_back(0), put16(stream, (uint32_t)p.size());
            put32(stream, rnd(1u << 31)), put16(stream, rnd(65536)), put16(stream, it.lport), put32(stream, 0), put32(stream, 0);
            stream.insert(stream.end(), p.begin(), p.end());
            if (i + 1 < n) stream.resize((stream.size() + 3) & ~3u);  // the buffer ends with the last payload byte
            items.push_back(it);
        }
        const uint32_t extra = rnd(4) ? 0 : rnd(5);  // records beyond the region
        unwritten += extra;
        const uint32_t records = n + extra;
        const uint32_t index_cap = rnd(3) ? records : rnd(records + 3);
        if (index_cap < records) ++capped;
        uint32_t* idx = index_cap ? (uint32_t*)malloc(8ull * index_cap) : nullptr;
        for (uint32_t k = 0; k < index_cap; ++k) idx[2 * k] = k, idx[2 * k + 1] = k < n ? items[k].off : 0xFFFFFFFFu;
        uint8_t* sbytes = (uint8_t*)malloc(stream.empty() ? 1 : stream.size());  // an empty stream still has an address
        if (!stream.empty()) memcpy(sbytes, stream.data(), stream.size());
        halo_deliver_summary_t* dsum = (halo_deliver_summary_t*)malloc(sizeof *dsum);
        memset(dsum, 0, sizeof *dsum);
        dsum->records = records, dsum->records_written = n;
        // what the delivery needs
        uint32_t need_d = 0, need_s = 0;
        halo_kcp_config_t cfg = {mode, port, 0, 0};
        {
            halo_kcp_summary_t s0;
            CHECK(halo_kcp_ingest_host(&cfg, sbytes, dsum, (halo_deliver_index_t*)idx, index_cap, nullptr, nullptr, &s0) == HALO_OK);
            need_d = s0.dgrams, need_s = s0.segs;
            CHECK(s0.dgrams_written == 0 && s0.segs_written == 0);
        }
        cfg.dgram_cap = rnd(3) ? need_d : rnd(need_d + 2);
        cfg.seg_cap = rnd(3) ? need_s : rnd(need_s + 2);
        halo_kcp_dgram_t* dg = cfg.dgram_cap ? (halo_kcp_dgram_t*)malloc(sizeof(halo_kcp_dgram_t) * cfg.dgram_cap) : nullptr;
        halo_kcp_seg_t* sg = cfg.seg_cap ? (halo_kcp_seg_t*)malloc(sizeof(halo_kcp_seg_t) * cfg.seg_cap) : nullptr;
        halo_kcp_summary_t* sum = (halo_kcp_summary_t*)malloc(sizeof *sum);
        CHECK(halo_kcp_ingest_host(&cfg, sbytes, dsum, (halo_deliver_index_t*)idx, index_cap, dg, sg, sum) == HALO_OK);
        // ---- the restatement ----
        halo_kcp_summary_t w;
        memset(&w, 0, sizeof w);
        bool stop = false;
        for (uint32_t k = 0; k < (index_cap < n ? index_cap : n); ++k) {
            const Item& it = items[k];
            if (it.kind != HALO_DELIVER_UDP || it.lport != port) { ++others; continue; }
            const uint8_t* p = it.payload.data();
            const uint32_t L = (uint32_t)it.payload.size();
            halo_kcp_dgram_t e;
            memset(&e, 0, sizeof e);
            e.index = k, e.payload_len = L;
            std::vector<halo_kcp_seg_t> ws;
            if (L == 20) {
                int t = -1;
                for (int m = 0; m < 4; ++m)
                    if (!memcmp(p, kMagic[m], 4) && !memcmp(p + 16, kMagic[m] + 4, 4)) { t = m; break; }
                if (t < 0) { ++w.ignored; continue; }
                e.kind = HALO_KCP_DGRAM_ENET, e.conn_type = (uint8_t)t;
                e.session_id = get32be(p + 4), e.conv = get32be(p + 8), e.enet_type = get32be(p + 12);
                e.conv0 = get32(p + 4) | (uint64_t)get32(p + 8) << 32;
            } else if (L >= H) {
                e.kind = HALO_KCP_DGRAM_KCP;
                e.conv0 = get32(p) | (uint64_t)get32(p + 4) << 32;
                uint32_t pos = 0;
                while (L - pos >= H) {
                    const uint8_t* h = p + pos;
                    const uint64_t conv = get32(h) | (uint64_t)get32(h + 4) << 32;
                    const uint32_t length = get32(h + 24), field = H == 32 ? get32(h + 28) : 0;
                    pos += H;
                    if (conv != e.conv0) { e.ret = -1; break; }
                    if (length > L - pos) { e.ret = -2; break; }
                    if (h[8] < 81 || h[8] > 84) { e.ret = -3; break; }
                    halo_kcp_seg_t x;
                    memset(&x, 0, sizeof x);
                    x.cmd = h[8], x.frg = h[9], x.wnd = (uint16_t)(h[10] | h[11] << 8), x.ts = get32(h + 12), x.sn = get32(h + 16);
                    x.una = get32(h + 20), x.len = length, x.data_off = it.off + 24 + pos;
                    if (mode != -1 && x.cmd == 81) {
                        if (mode == 0) x.check = field == 0 ? 1 : 2;
                        else if (mode == 1) x.check = field == crc_table(p + pos, length) ? 1 : 2;
                        else x.check = length == 0 ? (field == kEmptyXxh3 ? 1 : 2) : 0xFF;  // 0xFF: the call's own
                    }
                    ws.push_back(x);
                    pos += length;
                }
            } else { ++w.ignored; continue; }
            const uint32_t nw = (uint32_t)ws.size();
            if (!stop && w.dgrams < cfg.dgram_cap && w.segs + nw <= cfg.seg_cap) {
                const uint32_t j = w.dgrams_written, first = w.segs_written;
                uint32_t n_segs = nw;
                for (uint32_t i = 0; i < nw; ++i) {
                    ws[i].dgram = j;
                    if (ws[i].check == 0xFF) {
                        ws[i].check = sg[first + i].check;
                        CHECK(ws[i].check == 1 || ws[i].check == 2);
                    }
                    CHECK(!memcmp(&ws[i], &sg[first + i], sizeof(halo_kcp_seg_t)));
                    if (ws[i].check == 2 && n_segs == nw) n_segs = i;
                    if (ws[i].check == 1) ++passed;
                    if (ws[i].check == 2) ++failed;
                    if (ws[i].cmd == 81 && mode > 0) w.bytes_hashed += ws[i].len;
                    ++align[ws[i].data_off & 3];
                }
                segs_total += nw;
                if (n_segs < nw) e.ret = -4;
                e.n_segs = (uint16_t)n_segs, e.n_walked = (uint16_t)nw, e.first_seg = first;
                CHECK(!memcmp(&e, &dg[j], sizeof e));
                if (e.kind == HALO_KCP_DGRAM_KCP) {
                    ++w.ret_counts[-e.ret], ++w.in_pkts, w.in_bytes += L, ++rets[-e.ret], ++kcps;
                    if (e.ret) ++w.in_errs;
                    else w.in_segs += n_segs;
                } else {
                    ++w.enet_counts[e.conn_type], ++enets[e.conn_type];
                }
                ++w.dgrams_written, w.segs_written += nw;
            } else {
                if (!stop) ++cut;
                stop = true;
            }
            ++w.dgrams, w.segs += nw;
        }
        CHECK(!memcmp(&w, sum, sizeof w));
        ignored += w.ignored;
        free(idx), free(sbytes), free(dsum), free(dg), free(sg), free(sum);
    }
    printf("kcp fuzz: %ld calls, modes %lu %lu %lu %lu, kcp %lu, rets %lu %lu %lu %lu %lu, enet %lu %lu %lu %lu, ignored %lu, "
           "segs %lu, passed %lu, failed %lu, cut %lu, unwritten %lu, others %lu, capped %lu, lanes %lu, align %lu %lu %lu %lu\n",
           calls, modes[0], modes[1], modes[2], modes[3], kcps, rets[0], rets[1], rets[2], rets[3], rets[4], enets[0], enets[1], enets[2],
           enets[3], ignored, segs_total, passed, failed, cut, unwritten, others, capped, lanes, align[0], align[1], align[2], align[3]);
    return 0;
}
