// fuzz_kcp_emit.cc — KCP emit's host side (halo_amd/csrc/tx_kcp_host.cc over tx_kcp.h, the files
// libhalo_rx.so links) under ASan/UBSan: a stand-alone program that makes random halo_kcp_emit_host
// calls — entries, descriptors and a payload that ends with its last data byte, and every output in
// heap buffers of exactly the size the call needs, so an overrun is the sanitizer's to find — over
// sessions of random segments at random mtus, ENet entries, every non-OK status (ranges past the
// list and into the previous entry, data past the payload, bad mtus, segments longer than the mtu,
// bad ENet entries), gaps between ranges, in every byte-check mode, with dgram_cap and stream_cap
// below, at and above what the batch needs, and checks each against a restatement that builds the
// datagrams byte by byte with a table-driven CRC-32. (XXH3 mode: the restatement knows the hash of
// the empty string only; for other PUSH segments it takes the field the call wrote —
// tests/test_kcp_emit_host.py holds the host XXH3 against the oracle.)
// tests/test_sanitize_kcp_emit.py builds and runs it.
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ihalo_amd/csrc
//       halo_amd/csrc/tx_kcp_host.cc tools/fuzz_kcp_emit.cc -o fuzz_kcp_emit && ./fuzz_kcp_emit 3000 0x5EED
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

typedef std::vector<uint8_t> Bytes;
static void put32(Bytes& v, uint32_t x) {
    for (int k = 0; k < 4; ++k) v.push_back((uint8_t)(x >> 8 * k));
}
static void put32be(Bytes& v, uint32_t x) {
    for (int k = 3; k >= 0; --k) v.push_back((uint8_t)(x >> 8 * k));
}

static uint32_t g_table[256];
static uint32_t crc_table(const uint8_t* d, size_t n) {  // the classic table-driven CRC-32
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = g_table[(c ^ d[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}
static const uint32_t kEmptyXxh3 = 0x38D394C2u;  // the low 32 bits of XXH3-64 of no bytes
static const uint8_t kMagic[4][8] = {{0, 0, 0, 0xff, 0xff, 0xff, 0xff, 0xff}, {0, 0, 1, 0x45, 0x14, 0x51, 0x45, 0x45},
                                     {0, 0, 1, 0x94, 0x19, 0x41, 0x94, 0x94}, {0, 0, 2, 0x27, 0x22, 0x72, 0x27, 0x27}};

struct Counters {
    uint64_t modes[4], status[4], cut_dgram, cut_stream, enet, dgrams, segs, dst_align[4], gaps, empty;
};

// a heap copy of exactly n bytes (one byte when n == 0, never handed to the call then)
template <typename T>
static T* exact(const std::vector<T>& v) {
    T* p = (T*)malloc(v.empty() ? 1 : v.size() * sizeof(T));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

static int one_call(Counters& c) {
    const int mode = (int)rnd(4) - 1;
    const uint32_t H = mode == -1 ? 28 : 32;
    ++c.modes[mode + 1];
    std::vector<halo_kcp_out_session_t> ss;
    std::vector<halo_kcp_seg_t> segs;
    Bytes payload;
    const uint32_t n_sessions = rnd(8) == 0 ? 0 : 1 + rnd(24);
    const uint32_t bad_rate = rnd(3) ? 8 : 2;
    for (uint32_t k = 0; k < n_sessions; ++k) {
        halo_kcp_out_session_t e;
        memset(&e, 0, sizeof e);
        e.conv = ((uint64_t)rnd(1u << 31) << 32) | rnd(1u << 31);
        e.dst_ip = rnd(1u << 31), e.dst_port = (uint16_t)rnd(65536);
        if (rnd(10) == 0) {
            for (uint32_t g = 1 + rnd(2); g; --g) segs.push_back(halo_kcp_seg_t{}), ++c.gaps;
        }
        e.first_seg = (uint32_t)segs.size();
        const uint32_t what = rnd(bad_rate) == 0 ? 1 + rnd(8) : 0;
        if (rnd(6) == 0 || what == 7 || what == 8) {
            e.kind = HALO_KCP_DGRAM_ENET, e.conn_type = (uint8_t)rnd(4);
            e.session_id = rnd(1u << 31), e.enet_conv = rnd(1u << 31), e.enet_type = rnd(1u << 31);
            if (what == 7) e.conn_type = (uint8_t)(4 + rnd(252));
            if (what == 8 && !segs.empty()) e.first_seg = (uint32_t)segs.size() - 1, e.n_segs = 1;  // overlaps or not: BAD_RANGE
            ss.push_back(e);
            continue;
        }
        const uint32_t mtus[5] = {H + 1, 100, 300, 1400, 1472};
        e.mtu = (uint16_t)mtus[rnd(5)];
        const uint32_t n = rnd(5) == 0 ? 0 : 1 + rnd(6);
        for (uint32_t i = 0; i < n; ++i) {
            halo_kcp_seg_t s;
            memset(&s, 0xEE, sizeof s);  // dgram, check and reserved are ignored
            const uint32_t cmds[5] = {81, 81, 82, 83, 84};
            s.cmd = (uint8_t)cmds[rnd(5)], s.frg = (uint8_t)rnd(256), s.wnd = (uint16_t)rnd(65536);
            s.ts = rnd(1u << 31), s.sn = rnd(1u << 31), s.una = rnd(1u << 31);
            const uint32_t room = e.mtu - H;
            s.len = rnd(3) == 0 ? 0 : rnd(room + 1 < 200 ? room + 1 : (rnd(4) ? 200 : room + 1));
            payload.resize(payload.size() + rnd(4), 0xC3);  // any source alignment
            s.data_off = (uint32_t)payload.size();
            for (uint32_t b = 0; b < s.len; ++b) payload.push_back((uint8_t)rnd(256));
            segs.push_back(s);
        }
        e.n_segs = n;
        switch (what) {
            case 1: e.mtu = (uint16_t)(rnd(2) ? rnd(H + 1) : 1473 + rnd(60000)); break;
            case 2:  // too long; half of them past the payload as well, which is BAD_RANGE first
                if (n) {
                    segs.back().len = e.mtu - H + 1 + rnd(50);
                    if (rnd(2)) payload.resize(segs.back().data_off + segs.back().len, 0x5A);
                }
                break;
            case 3: e.n_segs = n + 1 + rnd(1000); break;                                 // may reach past the list
            case 4: if (n) segs[e.first_seg + rnd(n)].data_off = 0xFFFFFFF0u + rnd(16); break;
            case 5: if (e.first_seg) e.first_seg -= 1 + rnd(e.first_seg < 3 ? e.first_seg : 3); break;  // into the previous entry, or a gap
            case 6: e.kind = (uint8_t)(2 + rnd(254)); break;
            default: break;
        }
        ss.push_back(e);
    }
    const uint32_t n_segs = (uint32_t)segs.size();

    // ---- the restatement: every entry's status and datagrams, byte by byte --------------------
    struct Dg { Bytes bytes; uint32_t n_segs, session, first_seg; };
    std::vector<uint8_t> want_status(ss.size());
    std::vector<std::vector<Dg>> made(ss.size());
    std::vector<std::vector<size_t>> hash_at(ss.size());  // XXH3: where a datagram's unknown fields lie (dgram index, offset) flattened
    uint64_t prev_end = 0;
    for (size_t k = 0; k < ss.size(); ++k) {
        const halo_kcp_out_session_t& e = ss[k];
        uint32_t st = HALO_KCP_EMIT_OK;
        const uint64_t end = (uint64_t)e.first_seg + e.n_segs;
        if (end > n_segs || e.first_seg < prev_end) st = HALO_KCP_EMIT_BAD_RANGE;
        else if (e.kind == HALO_KCP_DGRAM_ENET) {
            if (e.conn_type > 3 || e.n_segs) st = HALO_KCP_EMIT_BAD_RANGE;
            else {
                Dg d{{}, 0, (uint32_t)k, e.first_seg};
                d.bytes.insert(d.bytes.end(), kMagic[e.conn_type], kMagic[e.conn_type] + 4);
                put32be(d.bytes, e.session_id), put32be(d.bytes, e.enet_conv), put32be(d.bytes, e.enet_type);
                d.bytes.insert(d.bytes.end(), kMagic[e.conn_type] + 4, kMagic[e.conn_type] + 8);
                made[k].push_back(d);
            }
        } else if (e.kind != HALO_KCP_DGRAM_KCP) st = HALO_KCP_EMIT_BAD_RANGE;
        else if (e.mtu <= H || e.mtu > 1472) st = HALO_KCP_EMIT_BAD_MTU;
        else {
            Dg cur{{}, 0, (uint32_t)k, e.first_seg};
            for (uint32_t i = 0; i < e.n_segs && st == HALO_KCP_EMIT_OK; ++i) {
                const halo_kcp_seg_t& s = segs[e.first_seg + i];
                if ((uint64_t)s.data_off + s.len > payload.size()) { st = HALO_KCP_EMIT_BAD_RANGE; break; }
                if ((uint64_t)H + s.len > e.mtu) { st = HALO_KCP_EMIT_SEG_TOO_LONG; break; }
                if (cur.bytes.size() + H + s.len > e.mtu) {
                    made[k].push_back(cur);
                    cur = Dg{{}, 0, (uint32_t)k, e.first_seg + i};
                }
                Bytes& v = cur.bytes;
                put32(v, (uint32_t)e.conv), put32(v, (uint32_t)(e.conv >> 32));
                v.push_back(s.cmd), v.push_back(s.frg), v.push_back((uint8_t)s.wnd), v.push_back((uint8_t)(s.wnd >> 8));
                put32(v, s.ts), put32(v, s.sn), put32(v, s.una), put32(v, s.len);
                if (H == 32) {
                    uint32_t f = 0;
                    if (s.cmd == 81 && mode == 1) f = crc_table(payload.data() + s.data_off, s.len);
                    if (s.cmd == 81 && mode == 2) {
                        f = kEmptyXxh3;
                        if (s.len) hash_at[k].push_back(made[k].size() << 16 | v.size());
                    }
                    put32(v, f);
                }
                v.insert(v.end(), payload.begin() + s.data_off, payload.begin() + s.data_off + s.len);
                ++cur.n_segs;
                ++c.dst_align[v.size() & 3];
            }
            if (st == HALO_KCP_EMIT_OK && !cur.bytes.empty()) made[k].push_back(cur);
            if (st != HALO_KCP_EMIT_OK) made[k].clear(), hash_at[k].clear();
        }
        prev_end = end;
        want_status[k] = (uint8_t)st;
    }
    uint64_t all_dg = 0, all_bytes = 0;
    for (size_t k = 0; k < ss.size(); ++k)
        for (const Dg& d : made[k]) ++all_dg, all_bytes += (d.bytes.size() + 3) & ~(size_t)3;
    // capacities below, at and above the need
    uint32_t dgram_cap = (uint32_t)all_dg + 2, stream_cap = (uint32_t)all_bytes + 5;
    switch (rnd(6)) {
        case 0: dgram_cap = all_dg ? rnd((uint32_t)all_dg) : 0; break;
        case 1: stream_cap = all_bytes ? rnd((uint32_t)all_bytes) : 0; break;
        case 2: dgram_cap = (uint32_t)all_dg, stream_cap = (uint32_t)all_bytes; break;
        case 3: dgram_cap = all_dg ? rnd((uint32_t)all_dg + 1) : 0, stream_cap = all_bytes ? rnd((uint32_t)all_bytes + 1) : 0; break;
        default: break;
    }

    halo_kcp_emit_summary_t want;
    memset(&want, 0, sizeof want);
    Bytes want_stream;
    std::vector<halo_kcp_out_dgram_t> want_dg;
    std::vector<uint32_t> dg_session;
    std::vector<std::pair<size_t, size_t>> unknown;  // stream offsets of XXH3 fields the restatement cannot know
    bool cut = false;
    uint64_t dg_before = 0, bytes_before = 0, segs_before = 0;
    for (size_t k = 0; k < ss.size(); ++k) {
        ++want.status_counts[want_status[k]];
        ++c.status[want_status[k]];
        if (want_status[k] != HALO_KCP_EMIT_OK) continue;
        uint64_t bytes = 0;
        for (const Dg& d : made[k]) bytes += (d.bytes.size() + 3) & ~(size_t)3;
        const bool fits_dg = dg_before + made[k].size() <= dgram_cap, fits_bytes = bytes_before + bytes <= stream_cap;
        const bool fits_segs = segs_before + ss[k].n_segs <= n_segs;  // the third capacity: only overlapping ranges reach it
        if (!cut && fits_dg && fits_bytes && fits_segs) {
            const size_t base_dg = want_dg.size();
            for (const Dg& d : made[k]) {
                halo_kcp_out_dgram_t r;
                r.offset = (uint32_t)want_stream.size(), r.len = (uint16_t)d.bytes.size(), r.n_segs = (uint16_t)d.n_segs;
                r.session = d.session, r.first_seg = d.first_seg;
                want_dg.push_back(r);
                want_stream.insert(want_stream.end(), d.bytes.begin(), d.bytes.end());
                want_stream.resize((want_stream.size() + 3) & ~(size_t)3, 0);
                want.out_bytes += d.bytes.size();
                want.segs_written += d.n_segs;
                for (uint32_t i = 0; i < d.n_segs; ++i) {
                    const halo_kcp_seg_t& s = segs[d.first_seg + i];
                    if (s.cmd == 81 && mode >= 1) want.bytes_hashed += s.len;
                }
            }
            for (size_t h : hash_at[k]) unknown.push_back({want_dg[base_dg + (h >> 16)].offset + (h & 0xFFFF), 0});
            ++want.sessions_written;
            want.dgrams_written += (uint32_t)made[k].size();
            want.bytes_written += bytes;
            if (ss[k].kind == HALO_KCP_DGRAM_ENET) ++c.enet;
            if (made[k].empty()) ++c.empty;
        } else if (!cut) {
            cut = true;
            if (!fits_dg) ++c.cut_dgram;
            if (!fits_bytes) ++c.cut_stream;
        }
        ++want.sessions;
        dg_before += made[k].size(), bytes_before += bytes, segs_before += ss[k].n_segs;
        want.dgrams += (uint32_t)made[k].size(), want.bytes += bytes, want.segs += ss[k].n_segs;
    }
    want.out_segs = want.segs_written, want.out_pkts = want.dgrams_written;
    c.dgrams += want.dgrams_written, c.segs += want.segs_written;

    // ---- the call, over exactly-sized heap buffers --------------------------------------------
    halo_kcp_out_session_t* h_ss = exact(ss);
    halo_kcp_seg_t* h_segs = exact(segs);
    uint8_t* h_payload = exact(payload);
    uint8_t* h_stream = (uint8_t*)malloc(stream_cap ? stream_cap : 1);
    halo_kcp_out_dgram_t* h_dg = (halo_kcp_out_dgram_t*)malloc(dgram_cap ? 16 * (size_t)dgram_cap : 1);
    halo_tx_build_desc_t* h_desc = (halo_tx_build_desc_t*)malloc(dgram_cap ? 40 * (size_t)dgram_cap : 1);
    uint8_t* h_status = (uint8_t*)malloc(ss.empty() ? 1 : ss.size());
    halo_kcp_emit_summary_t* h_sum = (halo_kcp_emit_summary_t*)malloc(sizeof(halo_kcp_emit_summary_t));
    memset(h_stream, 0xA5, stream_cap ? stream_cap : 1);
    if (dgram_cap) memset(h_dg, 0xA5, 16 * (size_t)dgram_cap), memset(h_desc, 0xA5, 40 * (size_t)dgram_cap);
    halo_kcp_emit_config_t cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.byte_check_mode = mode, cfg.src_ip = 0x0A000001u, cfg.src_port = 22102, cfg.dgram_cap = dgram_cap, cfg.stream_cap = stream_cap;
    const int rc = halo_kcp_emit_host(&cfg, ss.empty() ? nullptr : h_ss, (uint32_t)ss.size(), segs.empty() ? nullptr : h_segs, n_segs,
                                      payload.empty() ? nullptr : h_payload, payload.size(), stream_cap ? h_stream : nullptr,
                                      dgram_cap ? h_dg : nullptr, dgram_cap ? h_desc : nullptr, ss.empty() ? nullptr : h_status, h_sum);
    CHECK(rc == HALO_OK);
    for (size_t k = 0; k < ss.size(); ++k) CHECK(h_status[k] == want_status[k]);
    for (auto& u : unknown) memcpy(&want_stream[u.first], h_stream + u.first, 4);  // XXH3: the call's own field
    CHECK(memcmp(h_sum, &want, sizeof want) == 0);
    CHECK(want_stream.size() == want.bytes_written && want.bytes_written <= stream_cap && want_dg.size() <= dgram_cap);
    CHECK(want_stream.empty() || memcmp(h_stream, want_stream.data(), want_stream.size()) == 0);
    for (size_t b = want_stream.size(); b < stream_cap; ++b) CHECK(h_stream[b] == 0xA5);
    for (size_t j = 0; j < want_dg.size(); ++j) {
        CHECK(memcmp(&h_dg[j], &want_dg[j], 16) == 0);
        const halo_tx_build_desc_t& d = h_desc[j];
        const halo_kcp_out_session_t& e = ss[want_dg[j].session];
        halo_tx_build_desc_t w;
        memset(&w, 0, sizeof w);
        w.payload_off = want_dg[j].offset, w.payload_len = want_dg[j].len, w.proto = 17, w.src_port = 22102, w.dst_port = e.dst_port;
        w.src_ip = 0x0A000001u, w.dst_ip = e.dst_ip, w.mode = HALO_TX_BUILD_ETH;
        CHECK(memcmp(&d, &w, sizeof w) == 0);
    }
    for (size_t b = 16 * want_dg.size(); b < 16 * (size_t)dgram_cap; ++b) CHECK(((uint8_t*)h_dg)[b] == 0xA5);
    for (size_t b = 40 * want_dg.size(); b < 40 * (size_t)dgram_cap; ++b) CHECK(((uint8_t*)h_desc)[b] == 0xA5);
    free(h_ss), free(h_segs), free(h_payload), free(h_stream), free(h_dg), free(h_desc), free(h_status), free(h_sum);
    return 0;
}

int main(int argc, char** argv) {
    const int calls = argc > 1 ? atoi(argv[1]) : 3000;
    g_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x5EED;
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
        g_table[i] = c;
    }
    Counters c;
    memset(&c, 0, sizeof c);
    for (int i = 0; i < calls; ++i)
        if (one_call(c)) {
            fprintf(stderr, "call %d failed\n", i);
            return 1;
        }
    printf("kcp emit fuzz: %d calls, modes %llu %llu %llu %llu, status %llu %llu %llu %llu, cut_dgram %llu, cut_stream %llu, "
           "enet %llu, dgrams %llu, segs %llu, empty %llu, gaps %llu, align %llu %llu %llu %llu\n",
           calls, (unsigned long long)c.modes[0], (unsigned long long)c.modes[1], (unsigned long long)c.modes[2],
           (unsigned long long)c.modes[3], (unsigned long long)c.status[0], (unsigned long long)c.status[1],
           (unsigned long long)c.status[2], (unsigned long long)c.status[3], (unsigned long long)c.cut_dgram,
           (unsigned long long)c.cut_stream, (unsigned long long)c.enet, (unsigned long long)c.dgrams, (unsigned long long)c.segs,
           (unsigned long long)c.empty, (unsigned long long)c.gaps, (unsigned long long)c.dst_align[0],
           (unsigned long long)c.dst_align[1], (unsigned long long)c.dst_align[2], (unsigned long long)c.dst_align[3]);
    return 0;
}
