// fuzz_dhcp.cc — a stand-alone driver for the DHCP service's host side (rx_dhcp_host.cc,
// tx_dhcp_host.cc, dhcp_table.cc), built with them alone under -fsanitize=address,undefined
// (tests/test_sanitize_dhcp.py). Seeded runs: a random delivery stream in a heap buffer sized
// exactly to it (a read past a payload's last byte is an ASan error), halo_dhcp_decode_host into
// exactly-sized outputs, the messages through halo_dhcp_handle_msgs of a server that lives across
// calls, the replies through halo_dhcp_reply_build_host, and the built payloads decoded again —
// each step compared with the restatement below, which shares no code with the files under test:
// it parses byte by byte into a struct, keeps its leases in a plain vector and appends a reply's
// bytes one option after the other.
//   usage: fuzz_dhcp <calls> <seed>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/halo_rx.h"

namespace {

uint64_t g_state;
uint32_t rnd() {  // xorshift64*
    g_state ^= g_state >> 12, g_state ^= g_state << 25, g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}
uint32_t below(uint32_t n) { return rnd() % n; }
bool chance(uint32_t percent) { return below(100) < percent; }

[[noreturn]] void fail(const char* what, long a = 0, long b = 0) {
    printf("dhcp fuzz: MISMATCH %s (%ld, %ld)\n", what, a, b);
    exit(1);
}

typedef std::vector<uint8_t> Bytes;
void put32le(Bytes& b, uint32_t v) { for (int i = 0; i < 4; ++i) b.push_back((uint8_t)(v >> 8 * i)); }
void put16le(Bytes& b, uint32_t v) { b.push_back((uint8_t)v), b.push_back((uint8_t)(v >> 8)); }
void put32be(Bytes& b, uint32_t v) { for (int i = 3; i >= 0; --i) b.push_back((uint8_t)(v >> 8 * i)); }
uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// ---- the restatement: decode ----------------------------------------------------------------------
struct RefMsg {
    uint32_t index = 0, status = 0, dir = 0, msg_type = 0, options = 0, yiaddr = 0, payload_len = 0, remote_ip = 0, req_ip = 0;
    uint8_t xid[4] = {0}, chaddr[6] = {0}, mask[4] = {0}, gateway[4] = {0}, dns[4] = {0}, hostname[64] = {0};
    uint32_t mask_n = 0, gateway_n = 0;
    Bytes bytes() const {
        Bytes b;
        put32le(b, index);
        b.push_back((uint8_t)status), b.push_back((uint8_t)dir), b.push_back((uint8_t)msg_type), b.push_back(0);
        put32le(b, options);
        b.insert(b.end(), xid, xid + 4);
        put32le(b, yiaddr);
        b.insert(b.end(), chaddr, chaddr + 6);
        put16le(b, payload_len);
        put32le(b, remote_ip), put32le(b, req_ip);
        b.insert(b.end(), mask, mask + 4), b.insert(b.end(), gateway, gateway + 4), b.insert(b.end(), dns, dns + 4);
        b.push_back((uint8_t)mask_n), b.push_back((uint8_t)gateway_n);
        b.resize(64, 0);
        b.insert(b.end(), hostname, hostname + 64);
        return b;
    }
};

RefMsg ref_decode(uint32_t k, uint32_t remote_ip, uint32_t rport, uint32_t lport, const Bytes& p) {
    RefMsg m;
    m.index = k, m.remote_ip = remote_ip, m.payload_len = (uint32_t)p.size();
    if (rport == 68 && lport == 67) m.dir = HALO_DHCP_TO_SERVER;
    else if (rport == 67 && lport == 68) m.dir = HALO_DHCP_TO_CLIENT;
    else { m.dir = HALO_DHCP_DIR_NONE, m.status = HALO_DHCP_PORTS; return m; }
    if (p.size() < 240) { m.status = HALO_DHCP_SHORT; return m; }
    if (p[236] != 0x63 || p[237] != 0x82 || p[238] != 0x53 || p[239] != 0x63) { m.status = HALO_DHCP_COOKIE; return m; }
    memcpy(m.xid, &p[4], 4), memcpy(m.chaddr, &p[28], 6);
    m.yiaddr = be32(&p[16]);
    // the kept options, last one wins: a (present, data) pair per code
    struct Kept { bool have = false; Bytes data; } k1, k3, k6, k12, k50, k53;
    const Bytes o(p.begin() + 240, p.end());
    size_t i = 0;
    for (;;) {
        if (i >= o.size()) { m.status = HALO_DHCP_REF_PANIC; return m; }
        if (o[i] == 0xFF) break;
        if (i + 1 >= o.size()) break;
        const uint32_t code = o[i], len = o[i + 1];
        if (i + 2 + len > o.size()) break;
        Bytes data(o.begin() + i + 2, o.begin() + i + 2 + len);
        Kept* kp = code == 1 ? &k1 : code == 3 ? &k3 : code == 6 ? &k6 : code == 12 ? &k12 : code == 50 ? &k50 : code == 53 ? &k53 : nullptr;
        if (code == 53 && len == 0) { m.status = HALO_DHCP_REF_PANIC; return m; }
        if (kp) kp->have = true, kp->data = data;
        i += 2 + len;
    }
    if (k53.have) m.options |= HALO_DHCP_OPT_MSG_TYPE, m.msg_type = k53.data[0];
    if (k50.have) m.options |= HALO_DHCP_OPT_REQ_IP, m.req_ip = k50.data.size() == 4 ? be32(k50.data.data()) : 0;
    if (k1.have) {
        m.options |= HALO_DHCP_OPT_MASK, m.mask_n = k1.data.size() < 4 ? (uint32_t)k1.data.size() : 4;
        for (uint32_t x = 0; x < m.mask_n; ++x) m.mask[x] = k1.data[x];
    }
    if (k3.have) {
        m.options |= HALO_DHCP_OPT_ROUTER, m.gateway_n = k3.data.size() < 4 ? (uint32_t)k3.data.size() : 4;
        for (uint32_t x = 0; x < m.gateway_n; ++x) m.gateway[x] = k3.data[x];
    }
    if (k6.have) {
        if (k6.data.size() >= 4) m.options |= HALO_DHCP_OPT_DNS, memcpy(m.dns, k6.data.data(), 4);
        else m.options |= HALO_DHCP_OPT_DNS_SHORT;
    }
    if (k12.have) {
        m.options |= HALO_DHCP_OPT_HOSTNAME;
        const size_t n = k12.data.size() < 63 ? k12.data.size() : 63;
        for (size_t x = 0; x < n; ++x) m.hostname[x] = k12.data[x];
        m.hostname[63] = (uint8_t)n;
    }
    return m;
}

// ---- the restatement: the state machine ----------------------------------------------------------
struct RefLease { uint32_t ip; uint8_t mac[6]; uint32_t exp; uint8_t name[64]; };
struct RefReply { uint32_t kind; uint8_t xid[4]; uint32_t yiaddr; uint8_t chaddr[6]; uint32_t req_ip, server_id; };
struct RefServer {
    halo_dhcp_config_t cfg;
    std::vector<RefLease> leases;
    bool xid_set = false;
    uint8_t xid[4];
    int find(uint32_t ip) const {
        for (size_t i = 0; i < leases.size(); ++i) if (leases[i].ip == ip) return (int)i;
        return -1;
    }
};
RefReply mk(uint32_t kind, const uint8_t* xid, uint32_t yi, const uint8_t* mac, uint32_t req = 0, uint32_t sid = 0) {
    RefReply r{};
    r.kind = kind, r.yiaddr = yi, r.req_ip = req, r.server_id = sid;
    memcpy(r.xid, xid, 4), memcpy(r.chaddr, mac, 6);
    return r;
}
uint32_t popcount(uint32_t v) { uint32_t c = 0; for (; v; v &= v - 1) ++c; return c; }

uint8_t ref_handle(RefServer& s, const RefMsg& m, uint64_t now, std::vector<RefReply>& out, uint32_t& n_events) {
    if (m.status != HALO_DHCP_OK) return HALO_DHCP_H_NONE;
    if (m.dir == HALO_DHCP_TO_SERVER) {
        if (!s.cfg.server_enable || !(m.options & HALO_DHCP_OPT_MSG_TYPE)) return HALO_DHCP_H_NONE;
        if (m.msg_type == HALO_DHCP_DISCOVER) {
            uint32_t client = 0;
            uint8_t flags = 0;
            if (m.options & HALO_DHCP_OPT_REQ_IP) {
                const int at = s.find(m.req_ip);
                if (at >= 0 && !memcmp(s.leases[at].mac, m.chaddr, 6) && m.req_ip) client = m.req_ip, flags = HALO_DHCP_H_F_REUSED;
            }
            if (!client) {
                const uint32_t net = s.cfg.ip & s.cfg.network_mask, bits = 32 - popcount(net);
                if (bits < 32)
                    for (uint64_t ii = 0; ii < (1ull << bits) && !client; ++ii) {
                        const uint32_t a = net + (uint32_t)ii;
                        if ((a & 255) == 0 || (a & 255) == 255 || a == s.cfg.ip || s.find(a) >= 0) continue;
                        client = a;
                    }
            }
            if (!client) return HALO_DHCP_H_NO_ADDR;
            out.push_back(mk(HALO_DHCP_OFFER, m.xid, client, m.chaddr));
            return HALO_DHCP_H_OFFER | flags | HALO_DHCP_H_F_REPLY;
        }
        if (m.msg_type == HALO_DHCP_REQUEST) {
            if (!(m.options & HALO_DHCP_OPT_REQ_IP)) return HALO_DHCP_H_NO_REQ_IP;
            const int at = s.find(m.req_ip);
            uint8_t code = HALO_DHCP_H_ACK_NAK, flags = 0;
            if (m.req_ip == 0) code = HALO_DHCP_H_NAK_ZERO;
            else if ((s.cfg.ip ^ m.req_ip) & s.cfg.network_mask) code = HALO_DHCP_H_NAK_SUBNET;
            else if (at >= 0 && memcmp(s.leases[at].mac, m.chaddr, 6)) code = HALO_DHCP_H_NAK_OTHER_MAC;
            else if (at < 0 && s.leases.size() >= s.cfg.capacity) code = HALO_DHCP_H_NAK_FULL;
            if (code == HALO_DHCP_H_ACK_NAK) {
                const uint32_t hn = (m.options & HALO_DHCP_OPT_HOSTNAME) ? m.hostname[63] : 0;
                if (!hn) return HALO_DHCP_H_REF_PANIC;
                if (at < 0) {
                    RefLease l{};
                    s.leases.push_back(l);
                } else {
                    flags = HALO_DHCP_H_F_REUSED;
                }
                RefLease& l = at < 0 ? s.leases.back() : s.leases[at];
                l.ip = m.req_ip, l.exp = (uint32_t)(now + 3600);
                memcpy(l.mac, m.chaddr, 6);
                for (uint32_t x = 0; x < hn; ++x) l.name[x] = m.hostname[x];
                l.name[63] = (uint8_t)hn;
                out.push_back(mk(HALO_DHCP_ACK, m.xid, m.req_ip, m.chaddr));
            }
            out.push_back(mk(HALO_DHCP_NAK, m.xid, 0, m.chaddr));
            return code | flags | HALO_DHCP_H_F_REPLY;
        }
        if (m.msg_type == HALO_DHCP_RELEASE) {
            const int at = s.find(m.remote_ip);
            if (at < 0) return HALO_DHCP_H_RELEASE_ABSENT;
            s.leases.erase(s.leases.begin() + at);
            return HALO_DHCP_H_RELEASED;
        }
        return HALO_DHCP_H_NONE;
    }
    if (m.dir != HALO_DHCP_TO_CLIENT || !s.cfg.client_enable || s.cfg.ip != 0) return HALO_DHCP_H_NONE;
    if (!s.xid_set || memcmp(s.xid, m.xid, 4) || !(m.options & HALO_DHCP_OPT_MSG_TYPE)) return HALO_DHCP_H_NONE;
    if (m.msg_type == HALO_DHCP_OFFER) {
        out.push_back(mk(HALO_DHCP_REQUEST, m.xid, 0, s.cfg.mac, m.yiaddr, m.remote_ip));
        return HALO_DHCP_H_CLIENT_REQUEST | HALO_DHCP_H_F_REPLY;
    }
    if (m.msg_type == HALO_DHCP_ACK) {
        ++n_events;
        return HALO_DHCP_H_CLIENT_ACK;
    }
    return HALO_DHCP_H_NONE;
}

// ---- the restatement: the builder -----------------------------------------------------------------
void opt4(Bytes& b, uint8_t code, uint32_t v) { b.push_back(code), b.push_back(4), put32be(b, v); }
Bytes ref_build(const RefReply& r, const halo_dhcp_config_t& c) {
    const bool server = r.kind == HALO_DHCP_OFFER || r.kind == HALO_DHCP_ACK || r.kind == HALO_DHCP_NAK;
    Bytes b = {(uint8_t)(server ? 2 : 1), 1, 6, 0};
    b.insert(b.end(), r.xid, r.xid + 4);
    b.insert(b.end(), {0, 0, 0x80, 0, 0, 0, 0, 0});
    put32be(b, r.yiaddr);
    b.resize(28, 0);
    b.insert(b.end(), r.chaddr, r.chaddr + 6);
    b.resize(236, 0);
    b.insert(b.end(), {0x63, 0x82, 0x53, 0x63});
    b.insert(b.end(), {53, 1, (uint8_t)r.kind});
    if (r.kind == HALO_DHCP_OFFER || r.kind == HALO_DHCP_ACK) {
        opt4(b, 1, c.network_mask), opt4(b, 3, c.ip), opt4(b, 6, c.dns), opt4(b, 51, 3600), opt4(b, 59, 3150), opt4(b, 58, 1800);
        opt4(b, 54, c.ip);
    } else if (r.kind == HALO_DHCP_NAK) {
        opt4(b, 54, c.ip);
    } else {
        b.insert(b.end(), {61, 7, 1});
        b.insert(b.end(), r.chaddr, r.chaddr + 6);
        if (r.kind == HALO_DHCP_REQUEST) opt4(b, 50, r.req_ip), opt4(b, 54, r.server_id);
        b.insert(b.end(), {55, 3, 1, 3, 6});
    }
    b.push_back(0xFF);
    return b;
}

// ---- random messages ----------------------------------------------------------------------------
const uint32_t kNet = 0xC0A80100u;
uint64_t g_align[4];

void tlv(Bytes& b, uint8_t code, const Bytes& data) {
    b.push_back(code), b.push_back((uint8_t)data.size());
    b.insert(b.end(), data.begin(), data.end());
}
Bytes rbytes(uint32_t n) {
    Bytes b(n);
    for (auto& x : b) x = (uint8_t)rnd();
    return b;
}
Bytes ip_bytes(uint32_t v) { Bytes b; put32be(b, v); return b; }

Bytes random_payload(const uint8_t* client_xid) {
    const uint32_t shape = below(100);
    if (shape < 4) return rbytes(below(240));
    Bytes p(240, 0);
    p[0] = 1, p[1] = 1, p[2] = 6;
    for (int i = 0; i < 4; ++i) p[4 + i] = chance(50) ? client_xid[i] : (uint8_t)rnd();
    if (chance(50)) memcpy(&p[4], client_xid, 4);
    Bytes yi = ip_bytes(kNet + below(256));
    memcpy(&p[16], yi.data(), 4);
    p[28] = 2, p[33] = (uint8_t)below(6);  // six clients
    p[236] = 0x63, p[237] = 0x82, p[238] = 0x53, p[239] = 0x63;
    if (shape < 8) p[236 + below(4)] ^= (uint8_t)(1u << below(8));
    const uint32_t n_opts = below(8);
    const uint8_t types[] = {1, 1, 3, 3, 3, 7, 2, 5, 5, 0, 4, 8, 200};
    for (uint32_t i = 0; i < n_opts; ++i) {
        const uint32_t what = below(100);
        if (what < 30) tlv(p, 53, chance(3) ? Bytes() : Bytes{types[below(sizeof types)]});
        else if (what < 50) tlv(p, 50, chance(85) ? ip_bytes(chance(10) ? 0 : (chance(10) ? kNet + 512 : kNet) + below(12)) : rbytes(below(7)));
        else if (what < 70) {
            const uint32_t n = chance(10) ? 0 : chance(10) ? 60 + below(196) : 1 + below(12);
            g_align[(p.size() + 2) & 3]++;
            tlv(p, 12, rbytes(n));
        } else if (what < 76) tlv(p, 1, rbytes(below(7)));
        else if (what < 82) tlv(p, 3, rbytes(below(7)));
        else if (what < 90) tlv(p, 6, rbytes(below(10)));
        else tlv(p, (uint8_t)below(255), rbytes(below(6)));  // code 0 included; 0xff never as a code here
    }
    const uint32_t end = below(100);
    if (end < 70) p.push_back(0xFF);
    else if (end < 78) {}                                    // ends exactly at the end: the panic (or the empty area)
    else if (end < 86) p.push_back((uint8_t)below(255));     // one byte remains
    else if (end < 94) p.push_back(12), p.push_back((uint8_t)(1 + below(255)));  // a length that overruns
    else { p.push_back(0xFF); Bytes t = rbytes(below(40)); p.insert(p.end(), t.begin(), t.end()); }
    return p;
}

struct Rec { uint32_t kind, rport, lport, rip; Bytes payload; bool written; };

}  // namespace

int main(int argc, char** argv) {
    const long calls = argc > 1 ? strtol(argv[1], nullptr, 0) : 1000;
    g_state = (argc > 2 ? strtoull(argv[2], nullptr, 0) : 1) | 1;
    uint64_t status_n[5] = {0}, verdict_n[14] = {0}, kinds_n[9] = {0}, msgs_n = 0, cut_n = 0, unwritten_n = 0, others_n = 0, capped_n = 0,
             events_n = 0, built_n = 0, reused_n = 0;
    halo_dhcp_server_t* srv = nullptr;
    RefServer ref;
    uint8_t client_xid[4] = {0xAB, 0xCD, 0xEF, 0x01};
    uint64_t now = 1000;
    for (long c = 0; c < calls; ++c) {
        if (c % 50 == 0) {  // a new server: a LAN server with a small table, or a WAN client
            halo_dhcp_server_destroy(srv);
            halo_dhcp_config_t cfg;
            memset(&cfg, 0, sizeof cfg);
            const bool client = (c / 50) % 4 == 3;
            cfg.ip = client ? 0 : kNet + 1, cfg.network_mask = (c / 50) % 4 == 2 ? 0u : 0xFFFFFF00u,  // mask 0: hostBits == 32
             cfg.dns = rnd(), cfg.capacity = 1 + below(8);
            cfg.mac[0] = 2, cfg.mac[5] = (uint8_t)rnd(), cfg.server_enable = !client || chance(50), cfg.client_enable = client || chance(20);
            if (halo_dhcp_server_create(&cfg, &srv) != HALO_OK) fail("create");
            ref = RefServer();
            ref.cfg = cfg;
            if (client) {
                halo_dhcp_reply_t d;
                if (halo_dhcp_discover(srv, client_xid, &d) != HALO_OK || d.kind != HALO_DHCP_DISCOVER || memcmp(d.chaddr, cfg.mac, 6)) fail("discover");
                ref.xid_set = true, memcpy(ref.xid, client_xid, 4);
                uint8_t slot[288];
                halo_tx_build_desc_t desc;
                Bytes b = ref_build(mk(HALO_DHCP_DISCOVER, client_xid, 0, cfg.mac), cfg);
                b.resize(288, 0);
                if (halo_dhcp_reply_build_host(&cfg, &d, 1, slot, &desc) != HALO_OK || memcmp(slot, b.data(), 288) || desc.payload_len != 258 ||
                    desc.src_port != 68 || desc.dst_port != 67)
                    fail("discover build");
                ++kinds_n[HALO_DHCP_DISCOVER];
            }
        }
        // the delivery
        std::vector<Rec> recs(below(40));
        const uint32_t n_unwritten = chance(20) ? below(4) : 0;
        Bytes stream;
        std::vector<uint32_t> index;
        for (auto& r : recs) {
            r.kind = chance(75) ? HALO_DELIVER_DHCP : below(2);
            const uint32_t pp = below(100);
            r.rport = pp < 60 ? 68 : pp < 90 ? 67 : pp < 95 ? 68 : below(65536);
            r.lport = pp < 60 ? 67 : pp < 90 ? 68 : pp < 95 ? 68 : below(65536);
            r.rip = kNet + below(12);
            r.payload = random_payload(client_xid);
            index.push_back(rnd()), index.push_back((uint32_t)stream.size());
            put32le(stream, rnd());
            stream.push_back((uint8_t)r.kind), stream.push_back(0), put16le(stream, (uint32_t)r.payload.size());
            put32le(stream, r.rip), put16le(stream, r.rport), put16le(stream, r.lport), put32le(stream, 0), put32le(stream, 0);
            stream.insert(stream.end(), r.payload.begin(), r.payload.end());
            while (stream.size() & 3) stream.push_back(0);
        }
        for (uint32_t u = 0; u < n_unwritten; ++u) index.push_back(rnd()), index.push_back(0xFFFFFFFFu);
        unwritten_n += n_unwritten;
        const uint32_t total = (uint32_t)recs.size() + n_unwritten;
        uint32_t index_cap = total;
        if (chance(15) && total) index_cap = below(total + 1), ++capped_n;
        // the restatement's messages
        std::vector<RefMsg> want;
        uint32_t want_total = 0;
        for (uint32_t k = 0; k < recs.size() && k < index_cap; ++k) {
            if (recs[k].kind != HALO_DELIVER_DHCP) { ++others_n; continue; }
            ++want_total;
            want.push_back(ref_decode(k, recs[k].rip, recs[k].rport, recs[k].lport, recs[k].payload));
        }
        uint32_t msg_cap = want_total + below(3);
        if (chance(20) && want_total) msg_cap = below(want_total), ++cut_n;
        if (want.size() > msg_cap) want.resize(msg_cap);
        // exactly-sized heap buffers
        uint8_t* h_stream = (uint8_t*)malloc(stream.size() ? stream.size() : 1);
        if (!stream.empty()) memcpy(h_stream, stream.data(), stream.size());
        uint32_t* h_index = (uint32_t*)malloc(index_cap ? 8ull * index_cap : 1);
        if (index_cap) memcpy(h_index, index.data(), 8ull * index_cap);
        halo_deliver_summary_t dsum;
        memset(&dsum, 0, sizeof dsum);
        dsum.records = total, dsum.records_written = (uint32_t)recs.size();
        uint8_t* h_msgs = (uint8_t*)malloc(msg_cap ? 128ull * msg_cap : 1);
        memset(h_msgs, 0xA5, msg_cap ? 128ull * msg_cap : 1);
        halo_dhcp_summary_t sum;
        if (halo_dhcp_decode_host(h_stream, &dsum, (halo_deliver_index_t*)h_index, index_cap, msg_cap ? (halo_dhcp_msg_t*)h_msgs : nullptr,
                                  msg_cap, &sum) != HALO_OK)
            fail("decode rc");
        if (sum.msgs != want_total || sum.msgs_written != want.size()) fail("counts", sum.msgs, want_total);
        uint32_t st[5] = {0}, ty[9] = {0};
        for (size_t j = 0; j < want.size(); ++j) {
            const Bytes b = want[j].bytes();
            if (b.size() != 128 || memcmp(b.data(), h_msgs + 128 * j, 128)) fail("msg", c, (long)j);
            ++st[want[j].status], ++status_n[want[j].status];
            if (want[j].status == HALO_DHCP_OK) ++ty[(want[j].options & HALO_DHCP_OPT_MSG_TYPE) && want[j].msg_type < 9 ? want[j].msg_type : 0];
        }
        if (memcmp(st, sum.status_counts, sizeof st) || memcmp(ty, sum.type_counts, sizeof ty)) fail("summary counts", c);
        for (size_t x = 128 * want.size(); x < 128ull * msg_cap; ++x) if (h_msgs[x] != 0xA5) fail("written beyond the prefix", c);
        msgs_n += want.size();
        // the state machine
        const uint32_t n = (uint32_t)want.size();
        halo_dhcp_reply_t* replies = (halo_dhcp_reply_t*)malloc(n ? 64ull * n : 1);
        halo_dhcp_client_event_t* events = (halo_dhcp_client_event_t*)malloc(n ? 24ull * n : 1);
        uint8_t* verdicts = (uint8_t*)malloc(n ? n : 1);
        uint32_t n_replies = 0, n_events = 0;
        now += below(900);
        if (halo_dhcp_handle_msgs(srv, (halo_dhcp_msg_t*)h_msgs, n, now, replies, 2 * n, verdicts, &n_replies, events, n, &n_events) != HALO_OK)
            fail("handle rc");
        std::vector<RefReply> rr;
        uint32_t ref_events = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const uint8_t v = ref_handle(ref, want[i], now, rr, ref_events);
            if (v != verdicts[i]) fail("verdict", v, verdicts[i]);
            ++verdict_n[v & HALO_DHCP_H_MASK];
            if (v & HALO_DHCP_H_F_REUSED) ++reused_n;
        }
        if (rr.size() != n_replies || ref_events != n_events) fail("reply count", (long)rr.size(), n_replies);
        events_n += n_events;
        for (uint32_t i = 0; i < n_replies; ++i) {
            const halo_dhcp_reply_t& g = replies[i];
            if (g.kind != rr[i].kind || memcmp(g.xid, rr[i].xid, 4) || g.yiaddr != rr[i].yiaddr || memcmp(g.chaddr, rr[i].chaddr, 6) ||
                g.req_ip != rr[i].req_ip || g.server_id != rr[i].server_id || g.reserved1 || g.reserved2)
                fail("reply", c, i);
        }
        if (chance(30)) {
            const uint32_t gone = halo_dhcp_clear(srv, now);
            uint32_t ref_gone = 0;
            for (size_t i = ref.leases.size(); i-- > 0;)
                if ((uint32_t)now > ref.leases[i].exp) ref.leases.erase(ref.leases.begin() + i), ++ref_gone;
            if (gone != ref_gone) fail("clear", gone, ref_gone);
        }
        {
            const uint32_t have = halo_dhcp_list(srv, nullptr, 0);
            if (have != ref.leases.size()) fail("lease count", have, (long)ref.leases.size());
            halo_dhcp_lease_t* l = (halo_dhcp_lease_t*)malloc(have ? 80ull * have : 1);
            halo_dhcp_list(srv, l, have);
            for (uint32_t i = 0; i < have; ++i) {
                const int at = ref.find(l[i].ip);
                if (at < 0 || memcmp(l[i].mac, ref.leases[at].mac, 6) || l[i].exp_time != ref.leases[at].exp ||
                    memcmp(l[i].hostname, ref.leases[at].name, 64) || (i && l[i - 1].ip >= l[i].ip))
                    fail("lease", c, i);
            }
            free(l);
        }
        // the reply build, and the built payloads decoded again
        if (n_replies) {
            uint8_t* slots = (uint8_t*)malloc(288ull * n_replies);
            halo_tx_build_desc_t* descs = (halo_tx_build_desc_t*)malloc(40ull * n_replies);
            memset(slots, 0xA5, 288ull * n_replies);
            if (halo_dhcp_reply_build_host(&ref.cfg, replies, n_replies, slots, descs) != HALO_OK) fail("build rc");
            for (uint32_t i = 0; i < n_replies; ++i) {
                Bytes b = ref_build(rr[i], ref.cfg);
                const uint32_t len = (uint32_t)b.size();
                b.resize(288, 0);
                if (memcmp(b.data(), slots + 288ull * i, 288)) fail("built bytes", c, i);
                const halo_tx_build_desc_t& d = descs[i];
                const bool server = rr[i].kind == HALO_DHCP_OFFER || rr[i].kind == HALO_DHCP_ACK || rr[i].kind == HALO_DHCP_NAK;
                const uint8_t ff[6] = {255, 255, 255, 255, 255, 255};
                if (d.payload_off != 288ull * i || d.payload_len != len || d.proto != 17 || d.aux || d.src_port != (server ? 67 : 68) ||
                    d.dst_port != (server ? 68 : 67) || d.src_ip != ref.cfg.ip || d.dst_ip != 0xFFFFFFFFu || d.seq || d.ack ||
                    memcmp(d.dst_mac, ff, 6) || d.mode != HALO_TX_BUILD_ETH || d.pad)
                    fail("desc", c, i);
                const RefMsg back = ref_decode(0, 0, d.src_port, d.dst_port, Bytes(slots + 288ull * i, slots + 288ull * i + len));
                if (back.status != HALO_DHCP_OK || back.msg_type != rr[i].kind || back.yiaddr != rr[i].yiaddr) fail("round trip", c, i);
                ++kinds_n[rr[i].kind], ++built_n;
            }
            free(slots), free(descs);
        }
        free(replies), free(events), free(verdicts), free(h_msgs), free(h_index), free(h_stream);
    }
    halo_dhcp_server_destroy(srv);
    printf("dhcp fuzz: %ld calls, msgs %llu, status", calls, (unsigned long long)msgs_n);
    for (uint64_t v : status_n) printf(" %llu", (unsigned long long)v);
    printf(", verdicts");
    for (uint64_t v : verdict_n) printf(" %llu", (unsigned long long)v);
    printf(", reused %llu, events %llu, built %llu, kinds %llu %llu %llu %llu %llu, cut %llu, unwritten %llu, others %llu, capped %llu, align %llu %llu %llu %llu\n",
           (unsigned long long)reused_n, (unsigned long long)events_n, (unsigned long long)built_n, (unsigned long long)kinds_n[HALO_DHCP_OFFER],
           (unsigned long long)kinds_n[HALO_DHCP_ACK], (unsigned long long)kinds_n[HALO_DHCP_NAK], (unsigned long long)kinds_n[HALO_DHCP_REQUEST],
           (unsigned long long)kinds_n[HALO_DHCP_DISCOVER], (unsigned long long)cut_n, (unsigned long long)unwritten_n,
           (unsigned long long)others_n, (unsigned long long)capped_n, (unsigned long long)g_align[0], (unsigned long long)g_align[1],
           (unsigned long long)g_align[2], (unsigned long long)g_align[3]);
    return 0;
}
